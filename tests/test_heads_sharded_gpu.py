"""The three-term training step - attention, CTC and transducer loss - on data-parallel shards, on the GPU, against the float64
restatement of tests/heads_ref.py (which tests/test_heads_sharded_cpu.py checks first: its rank-local losses and gradients
sum to the full batch's).

A rank's call is not the single-process call on fewer rows: the encoder is padded to the global T_max, so ctc_nll,
TransducerHead.project_enc, ops.rnnt_joint, ops.ctc_loss and ops.rnnt_loss run over frames that belong to no utterance of the
call; U is the shard's own longest transcript while the decoder runs the global olength; and parallel.joint_loss rescales the
two head terms to the global batch size.  The ranks run one after another in this process through parallel.sup_local_loss, the
route Solver takes, and their gradients accumulate in .grad as an all-reduce would sum them.

Gates, all the project's own: the loss against float64 within test_deterministic_gpu.LOSS_GATE; every gradient against float64
within 1e-3 of the tensor's largest element (test_head_gradients_against_float64); the summed shards against the full batch
within test_sharded_equals_full_batch_on_gpu's _close(rtol=1e-4, atol=1e-6); a rank's per-utterance nll against the full
batch's rows within test_rnnt_gpu._allowance of that vector (4 x the float32 restatement's error, floor 8 x 2^-24 x its
largest).  Every test prints `heads-sharded` lines: the measured error / gate per tensor (profiles/heads_sharded_parity.txt
keeps one run)."""
import functools

import numpy as np
import pytest
import torch

import heads_ref as H
import rnnt_ref as R
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_RTOL = 1e-3                                   # worst element / the tensor's largest, and the largest > 0
SHARD_GATE = dict(rtol=1e-4, atol=1e-6)            # test_sharded_equals_full_batch_on_gpu


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _cfg(hidden):
    return synth.TINY if hidden == synth.TINY["enc_hidden_dim"] else dict(synth.TINY, enc_hidden_dim=hidden)


@functools.lru_cache(maxsize=None)
def _reference(hidden=synth.TINY["enc_hidden_dim"]):
    """The float64 full-batch loss, gradients and per-utterance nll vectors, and the float32 restatement's nll vectors (the
    yardstick of _allowance); computed once per model width and left unchanged."""
    cfg = _cfg(hidden)
    xs, ilens, ys = H.batch(cfg)
    net = H.tiny_net(cfg)
    loss, grads, parts = H.loss_and_grads(H.leaves(net), cfg, xs, ilens, ys)
    _, part32 = H.loss(H.leaves(net, torch.float32), cfg, xs, ilens, ys)
    return dict(loss=float(loss), grads=grads, part=parts[0], part32=part32)


def _model(hidden=synth.TINY["enc_hidden_dim"]):
    cfg = _cfg(hidden)
    xs, ilens, ys = H.batch(cfg)
    return H.tiny_net(cfg).to(DEV), cfg, torch.from_numpy(xs).to(DEV), ilens, [torch.from_numpy(y).to(DEV) for y in ys]


def _grads(net):
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def _full_step(net, xs, ilens, ys):
    """One net(...) + parallel.local_loss on the whole batch -> (loss, gradients, the log-probs with the head terms)."""
    import parallel
    np.random.seed(4)
    _, lp, _, _ = net(xs, ilens, ys, tf_rate=1.0, loss_norm=len(ilens))
    loss = parallel.local_loss(lp, dict(b_global=len(ilens)))
    net.zero_grad()
    loss.backward()
    return float(loss.detach()), _grads(net), lp


def _sharded_step(hb, net, cfg, xs, ilens, ys, world):
    """The ranks of one step, one after another -> (sum of the rank-local losses, summed gradients, per rank the log-probs -
    None for an empty shard)."""
    import parallel
    seen = []
    hook = net.register_forward_hook(lambda mod, args, out: seen.append(out[1]))
    net.zero_grad()
    total, lps = 0.0, []
    try:
        for rank in range(world):
            rows = parallel.shard_indices(len(ilens), rank, world)
            before = dict(hb.LAUNCHES)
            np.random.seed(4)
            loss = parallel.sup_local_loss(net, xs, ilens, ys, 1.0, rank, world, cfg["enc_n_layers"], cfg["subsample"])
            ran = {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
            if not rows:
                assert loss is None and not seen, "rank %d of %d owns no utterance" % (rank, world)
                assert not any(k.startswith(("rnnt", "ctc")) for k in ran), ran
                lps.append(None)
                continue
            for k in ("ctc_loss", "rnnt_joint", "rnnt_loss"):
                assert ran.get(k) == 1, (k, ran)
            lps.append(seen.pop())
            loss.backward()                              # accumulates into .grad
            total += float(loss.detach())
    finally:
        hook.remove()
    return total, _grads(net), lps


def _ratio(got, want, rtol, atol=0.0):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    top = float(want.abs().max())
    return float((got - want).abs().max()) / max(atol + rtol * top, 1e-300), top


def _check_against_float64(what, loss, grads, ref):
    import test_deterministic_gpu as TD
    rtol, atol = TD.LOSS_GATE
    r = abs(loss - ref["loss"]) / (atol + rtol * abs(ref["loss"]))
    print("heads-sharded %-26s loss %.7f  float64 %.7f  error / gate %.3g" % (what, loss, ref["loss"], r))
    TD._close(torch.tensor(loss, dtype=torch.float64), torch.tensor(ref["loss"], dtype=torch.float64), rtol, atol, what + " loss")
    assert set(grads) == set(ref["grads"]) and {"ctc_lo.weight", "ctc_lo.bias"} | {"rnnt." + k for k in R.HEAD_KEYS} <= set(grads)
    worst = {}
    for n, g in grads.items():
        worst[n], top = _ratio(g, ref["grads"][n], GRAD_RTOL)
        assert top > 0, n
    print("heads-sharded %-26s gradient vs float64, error / gate: worst %.3g (%s)  heads %s" % (
        what, max(worst.values()), max(worst, key=worst.get),
        "  ".join("%s %.2g" % (n, r) for n, r in worst.items() if n.startswith(("ctc_lo.", "rnnt.")))))
    for n, r in worst.items():
        assert r <= 1.0, "%s: gradient of %s is %.3f of its gate against float64" % (what, n, r)


def _check_sharded_against_full(what, total, grads, full_loss, full_grads):
    import test_hip_parity as THP
    worst = {n: _ratio(g, full_grads[n], **SHARD_GATE)[0] for n, g in grads.items()}
    print("heads-sharded %-26s summed shards vs full batch, error / gate: loss %.3g  worst %.3g (%s)  heads %s" % (
        what, abs(total - full_loss) / (1e-5 * abs(full_loss)), max(worst.values()), max(worst, key=worst.get),
        "  ".join("%s %.2g" % (n, r) for n, r in worst.items() if n.startswith(("ctc_lo.", "rnnt.")))))
    assert abs(total - full_loss) < 1e-5 * abs(full_loss)
    for n, g in grads.items():
        THP._close(g, full_grads[n], what="%s: sharded grad %s" % (what, n), **SHARD_GATE)


def _check_rank_terms(what, lps, full_lp, ref, ilens, world):
    """Every rank's norms are the global batch size; its per-utterance nll vectors are the full batch's rows."""
    import parallel
    from test_rnnt_gpu import _allowance
    worst = dict(ctc_nll=0.0, rnnt_nll=0.0)
    for rank, lp in enumerate(lps):
        if lp is None:
            continue
        rows = parallel.shard_indices(len(ilens), rank, world)
        assert lp.ctc_norm == lp.rnnt_norm == float(len(ilens)), (rank, lp.ctc_norm, lp.rnnt_norm)
        for k in worst:
            allow = _allowance(ref["part32"][k].numpy(), ref["part"][k].numpy())
            got, want = getattr(lp, k).detach().double().cpu(), getattr(full_lp, k).detach().double().cpu()[rows]
            assert tuple(got.shape) == (len(rows),)
            worst[k] = max(worst[k], float((got - want).abs().max()) / allow)
    print("heads-sharded %-26s rank nll vs the full batch's rows, error / allowance: ctc %.3g  rnnt %.3g" % (
        what, worst["ctc_nll"], worst["rnnt_nll"]))
    for k, r in worst.items():
        assert r <= 1.0, "%s: a rank's %s is %.3f of its allowance off the full batch's rows" % (what, k, r)


@pytest.fixture(scope="module")
def tiny(hb):
    net, cfg, xs, ilens, ys = _model()
    full_loss, full_grads, full_lp = _full_step(net, xs, ilens, ys)
    _check_against_float64("full batch", full_loss, full_grads, _reference())
    return dict(net=net, cfg=cfg, xs=xs, ilens=ilens, ys=ys, loss=full_loss, grads=full_grads, lp=full_lp)


@pytest.mark.parametrize("world", H.WORLDS)
def test_sharded_step_against_float64(hb, tiny, world):
    """World sizes 1, 2, 3, 4 and 7 (ranks 6.. are empty) on ilens 11 .. 3: a shard of one utterance (world 4), shards whose
    every T_b is below the padded T' and whose longest transcript is below the global one (world 2, rank 1), an empty shard."""
    t, ref, what = tiny, _reference(), "world %d" % world
    total, grads, lps = _sharded_step(hb, t["net"], t["cfg"], t["xs"], t["ilens"], t["ys"], world)
    assert [lp is None for lp in lps] == [rank >= len(t["ilens"]) for rank in range(world)]
    _check_against_float64(what, total, grads, ref)
    _check_sharded_against_full(what, total, grads, t["loss"], t["grads"])
    _check_rank_terms(what, lps, t["lp"], ref, t["ilens"], world)


@pytest.mark.parametrize("rows,hidden", [("padded", 16), ("packed", 128)])
def test_sharded_step_on_the_other_encoder_paths(hb, monkeypatch, rows, hidden):
    """The world-2 comparison where enc_h behind a length comes from other code: the time-major padded encoder (the default
    is packed rows: there the frames behind an utterance are rows_unpack's fill), and H = 128, the smallest width the
    persistent LSTM kernels serve (asserted on the launch counters)."""
    monkeypatch.setattr(hb, "USE_PACKED_ROWS", rows == "packed")
    net, cfg, xs, ilens, ys = _model(hidden)
    ref, what = _reference(hidden), "world 2 %s H=%d" % (rows, hidden)
    hb.persist_clear_abort(torch.device(DEV))
    before = dict(hb.LAUNCHES)
    full_loss, full_grads, full_lp = _full_step(net, xs, ilens, ys)
    total, grads, lps = _sharded_step(hb, net, cfg, xs, ilens, ys, 2)
    ran = {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
    assert not hb.persist_aborted(torch.device(DEV))
    # three forwards (the full batch, two ranks) of two encoder layers and of the head's prediction network, whose width
    # (dec_hidden_dim = 16) stays on the per-step kernels
    if hidden >= 128:
        if not hb.USE_PERSIST:
            pytest.fail("the persistent kernels are switched off in this process")
        assert ran.get("lstm_fwd_persist") == 6 and ran.get("lstm_bwd_persist", 0) >= 6, ran
        assert ran.get("lstm_fwd_step") == 3 and ran.get("lstm_bwd_step") == 3, ran
    else:
        assert ran.get("lstm_fwd_step") == 9 and ran.get("lstm_bwd_step") == 9, ran
        assert "lstm_fwd_persist" not in ran and "lstm_bwd_persist" not in ran, ran
    assert (getattr(net.encoder.enc2, "last_layout", None) is not None) == (rows == "packed")
    _check_against_float64(what + " full", full_loss, full_grads, ref)
    _check_against_float64(what, total, grads, ref)
    _check_sharded_against_full(what, total, grads, full_loss, full_grads)
    _check_rank_terms(what, lps, full_lp, ref, ilens, 2)


def test_sharded_step_is_bit_reproducible_in_deterministic_mode(hb, tiny):
    """The world-3 sequence twice from the same state under hb.deterministic(): the same bits in every .grad."""
    t = tiny
    with hb.deterministic():
        first = _sharded_step(hb, t["net"], t["cfg"], t["xs"], t["ilens"], t["ys"], 3)
        second = _sharded_step(hb, t["net"], t["cfg"], t["xs"], t["ilens"], t["ys"], 3)
    assert first[0] == second[0]
    for n in first[1]:
        assert torch.equal(first[1][n], second[1][n]), n
    _check_against_float64("world 3 deterministic", first[0], first[1], _reference())
    print("heads-sharded %-26s two runs: the same bits in %d gradients" % ("world 3 deterministic", len(first[1])))
