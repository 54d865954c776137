"""Shallow-fusion beam search without a GPU: the float64 restatement (tests/beam_lm_ref.py) against beam_ref at
lm_weight = 0 and on hand-built logit sequences where the LM decides, and the C-ABI of the three new entries."""
import os
import re

import numpy as np
import torch

import beam_lm_ref
import beam_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2
NEG = -1e9           # a logit that is never chosen, but finite


def _scripted(asr_rows, lm_rows):
    def step(t, parents, toks):
        return np.asarray(asr_rows[t], dtype=np.float64), np.asarray(lm_rows[t], dtype=np.float64)
    return step


def _logp(p):
    return np.log(np.asarray(p, dtype=np.float64))


def test_lm_weight_zero_is_beam_ref(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "tiny_e2e.npz")))
    sd = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    lm_cfg = dict(synth.TINY_LM, output_dim=synth.TINY["output_dim"])
    lm_sd = {k: torch.from_numpy(v) for k, v in synth.lm_weights(lm_cfg, 5).items()}
    enc, lens = torch.from_numpy(g["enc_h"]), g["enc_lens"].tolist()
    for K in (1, 3):
        for alpha in (0.0, 0.7):
            want = beam_ref.decode(sd, enc, lens, 5, K, alpha)
            got = beam_lm_ref.decode(sd, lm_sd, enc, lens, 5, K, 0.0, alpha)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a["hyps"] == b["hyps"] and a["margins"] == b["margins"] and a["steps"] == b["steps"]
                assert a["rank_margin"] == b["rank_margin"]
    # and with a weight the LM is in the scores: the best key is log p_asr + 0.5 log p_lm of its tokens
    fused = beam_lm_ref.decode(sd, lm_sd, enc, lens, 5, 3, 0.5)
    plain = beam_ref.decode(sd, enc, lens, 5, 3)
    assert any(a["hyps"][0][1] != b["hyps"][0][1] for a, b in zip(fused, plain))


def test_lm_step_is_the_stacked_cell():
    lm_sd = {k: torch.from_numpy(v).double() for k, v in synth.lm_weights(synth.TINY_LM, 5).items()}
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randn(3, 16))
    h, c = torch.from_numpy(rs.randn(2, 3, 16) * 0.5), torch.from_numpy(rs.randn(2, 3, 16) * 0.5)
    logits, h1, c1 = beam_lm_ref.lm_step(lm_sd, x, h, c)
    lstm = torch.nn.LSTM(16, 16, num_layers=2).double()
    lstm.load_state_dict({k[5:]: v for k, v in lm_sd.items() if k.startswith("LSTM.")})
    with torch.no_grad():
        y, (h2, c2) = lstm(x[None], (h, c))
    assert torch.allclose(h1, h2, atol=1e-12) and torch.allclose(c1, c2, atol=1e-12)
    want = y[0] @ lm_sd["output_layer.weight"].t() + lm_sd["output_layer.bias"]
    assert torch.allclose(logits, want, atol=1e-12)


def test_the_lm_changes_the_winner():
    # K = 1 (fused greedy), V = 4: the recogniser prefers token 1 (0.5 vs 0.4), the LM token 3 (0.9 vs 0.05)
    V, K = 4, 1
    a0 = _logp([1e-30, 0.5, 0.1, 0.4])
    l0 = _logp([1e-30, 0.05, 0.05, 0.9])
    end = _logp([1e-30, 0.05, 0.9, 0.05])
    asr, lm = [[a0], [end]], [[l0], [end]]
    plain = beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 0.0)
    fused = beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 1.0)
    assert plain["hyps"][0][0] == [1, EOS] and fused["hyps"][0][0] == [3, EOS]
    want = (a0[3] + 1.0 * l0[3]) + (end[EOS] + 1.0 * end[EOS])
    assert np.isclose(fused["hyps"][0][1], want)
    # below the weight where 0.4 * 0.9^w overtakes 0.5 * 0.05^w the recogniser still wins
    w_flip = np.log(0.5 / 0.4) / np.log(0.9 / 0.05)
    assert beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 0.9 * w_flip)["hyps"][0][0] == [1, EOS]
    assert beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 1.1 * w_flip)["hyps"][0][0] == [3, EOS]


def test_the_lm_changes_which_eos_finishes():
    # K = 2, V = 4.  Step 0 leaves beams [1] and [3] live.  Step 1: the recogniser alone ranks ([1], <EOS>) first and
    # ([3], <EOS>) third (rank >= K: skipped); the LM dislikes <EOS> after 1 and likes it after 3, so fused the <EOS> of
    # beam 1 is the one that finishes at rank < K
    V, K = 4, 2
    s0 = _logp([1e-30, 0.5, 1e-6, 0.5 - 1e-6])
    a1 = np.stack([_logp([1e-30, 0.30, 0.60, 0.10]), _logp([1e-30, 0.45, 0.35, 0.20])])
    l1 = np.stack([_logp([1e-30, 0.80, 0.01, 0.19]), _logp([1e-30, 0.05, 0.90, 0.05])])
    flat = _logp([1e-30, 1 / 3., 1 / 3., 1 / 3.])
    asr = [np.stack([s0, s0]), a1]
    lm = [np.stack([flat, flat]), l1]
    plain = beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 0.0)
    fused = beam_lm_ref.search(_scripted(asr, lm), K, V, 2, EOS, 1.0)
    ended = lambda r: [h[0] for h in r["hyps"] if h[0][-1] == EOS]      # noqa: E731
    assert ended(plain) == [[1, EOS]]
    assert ended(fused) == [[3, EOS]]


def test_a_tie_in_the_fused_score_goes_to_the_lower_flat_index():
    # the recogniser separates tokens 1 and 3 by exactly what the LM gives back: asr (2, 1) + 1.0 * lm (1, 2) tie at 3
    K, V = 2, 5
    a = np.array([0.0, 2.0, -3.0, 1.0, -5.0])
    l = np.array([0.0, 1.0, -3.0, 2.0, -5.0])
    # log_softmax shifts both rows by constants: the fused values of tokens 1 and 3 stay equal
    fa, fl = beam_ref.log_softmax(a), beam_ref.log_softmax(l)
    assert fa[1] + fl[1] == fa[3] + fl[3]
    sel = beam_ref.select(np.array([-1.0, -1.0]), np.stack([fa + 1.0 * fl] * 2), EOS)
    # candidates (beam 0, tok 1), (0, 3), (1, 1), (1, 3) tie: the first two by flat index live
    assert sel["tok"].tolist() == [1, 3] and sel["bp"].tolist() == [0, 0] and sel["margin"] == 0.0
    res = beam_lm_ref.search(_scripted([np.stack([a, a])] * 2, [np.stack([l, l])] * 2), K, V, 2, EOS, 1.0)
    # step 0 keeps tokens 1 and 3 (equal scores, beams 0 and 1); at step 1 the four continuations tie and both survivors
    # descend from beam 0, the lower flat index
    assert res["margins"][1] == 0.0 and [h[0] for h in res["hyps"]] == [[1, 1], [1, 3]]


def test_lm_exports_and_abi_version():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    lib = hb.load()
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_lm_step_f32", "asr_beam_select_lm_f32", "asr_beam_reorder_lm_f32"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in hb.EXPORTS and hasattr(lib, name), name
    assert lib.asr_abi_version() == 8 == hb.ABI_VERSION
    assert "additive" in header
    assert "#define ASR_LM_MAX_LAYERS 4" in header and "#define ASR_LM_MAX_ROWS 512" in header
    assert (hb.LM_MAX_LAYERS, hb.LM_MAX_ROWS) == (4, 512)
