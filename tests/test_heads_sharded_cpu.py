"""The float64 restatement of the three-term loss (tests/heads_ref.py) on data-parallel shards, without a GPU: the rank-local
losses sum to the full-batch loss and their gradients to its gradient, for every world size tests/test_heads_sharded_gpu.py
uses - the reference is checked here before it judges the kernels - and the world sizes hold the shards they are meant to."""
import numpy as np
import pytest
import torch

import heads_ref as H
import rnnt_ref as R
import synth


@pytest.fixture(scope="module")
def case():
    p = H.leaves(H.tiny_net())
    xs, ilens, ys = H.batch()
    full_loss, full_grads, parts = H.loss_and_grads(p, synth.TINY, xs, ilens, ys)
    return dict(p=p, xs=xs, ilens=ilens, ys=ys, loss=full_loss, grads=full_grads, part=parts[0])


def test_the_model_has_both_heads(case):
    assert set(case["p"]) >= {"ctc_lo.weight", "ctc_lo.bias"} | {"rnnt." + k for k in R.HEAD_KEYS}
    assert all(v.dtype == torch.float64 for v in case["p"].values())
    part = case["part"]
    assert float(part["att"]) > 0 and float(part["rnnt_nll"].min()) > 0 and float(part["ctc_nll"].max()) > 0
    for n, g in case["grads"].items():
        assert float(g.abs().max()) > 0, n


@pytest.mark.parametrize("world", H.WORLDS)
def test_float64_shards_sum_to_the_full_batch(case, world):
    total, grads, parts = H.loss_and_grads(case["p"], synth.TINY, case["xs"], case["ilens"], case["ys"], world)
    want = float(case["loss"])
    assert abs(float(total) - want) <= 1e-12 * abs(want), (world, float(total), want)
    for n, g in grads.items():
        top = float(case["grads"][n].abs().max())
        err = float((g - case["grads"][n]).abs().max())
        assert err <= 1e-10 * top, (world, n, err, top)
    # a rank's per-utterance terms are the full batch's rows
    for rank, part in enumerate(parts):
        rows = H.shard_rows(len(case["ilens"]), rank, world)
        assert (part is None) == (not rows)
        if part is None:
            continue
        for k in ("ctc_nll", "rnnt_nll"):
            assert float((part[k] - case["part"][k][rows]).abs().max()) <= 1e-12 * float(case["part"][k].abs().max())


def test_float32_restatement_runs(case):
    """The yardstick a derived gate would come from: the same restatement on float32 leaves stays close to float64."""
    p32 = H.leaves(H.tiny_net(), torch.float32)
    total, grads, _ = H.loss_and_grads(p32, synth.TINY, case["xs"], case["ilens"], case["ys"], 3)
    assert total.dtype == torch.float32 and abs(float(total) - float(case["loss"])) <= 1e-5 * abs(float(case["loss"]))
    for n, g in grads.items():
        assert float((g.double() - case["grads"][n]).abs().max()) <= 1e-3 * float(case["grads"][n].abs().max()), n


def test_the_world_sizes_hold_the_shards_the_kernels_have_not_met(case):
    import parallel
    ilens, ys = case["ilens"], case["ys"]
    enc_lens, t_out = case["part"]["enc_lens"], case["part"]["t_out"]
    assert max(enc_lens) == t_out and len(set(enc_lens)) > 1
    u_global = max(len(y) for y in ys)
    seen = set()
    for world in H.WORLDS:
        for rank in range(world):
            rows = H.shard_rows(len(ilens), rank, world)
            assert rows == parallel.shard_indices(len(ilens), rank, world)
            if not rows:
                seen.add("empty")
                continue
            if len(rows) == 1:
                seen.add("one utterance")
            if max(enc_lens[i] for i in rows) < t_out:
                seen.add("every T_b below T'")
            if max(len(ys[i]) for i in rows) < u_global:
                seen.add("local U below the global one")
    assert seen >= {"empty", "one utterance", "every T_b below T'", "local U below the global one"}, seen
    assert np.all(np.diff(ilens) <= 0)
