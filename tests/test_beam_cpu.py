"""Beam search without a GPU: the CPU restatement (tests/beam_ref.py) against the reference's own greedy decode and on
hand-built logit sequences that reach every rule of DESIGN 4.8, and the C-ABI of the beam kernels."""
import os
import re

import numpy as np
import torch

import beam_ref
import synth
from oracle import asr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2
NEG = -1e9           # a logit that is never chosen, but finite


def _scripted(rows):
    """A step function that ignores the state and returns rows[t] ([K, V] or [V] for every beam)."""
    def step(t, parents, toks):
        return rows[t]
    return step


def _lp(row):
    return beam_ref.log_softmax(np.asarray(row, dtype=np.float64))


def test_k1_reproduces_the_reference_greedy_decode(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "tiny_e2e.npz")))
    sd = O.make_leaf_state(synth.e2e_weights(synth.TINY, 11))
    res = beam_ref.decode(sd, torch.from_numpy(g["enc_h"]), g["enc_lens"].tolist(), 5, 1)
    for b, r in enumerate(res):
        want = g["gr_pred"][b].tolist()
        if EOS in want:
            want = want[:want.index(EOS) + 1]
        assert r["hyps"][0][0] == want, (b, r["hyps"][0], g["gr_pred"][b])


def test_eos_at_rank_k_or_later_is_skipped():
    # K = 2, V = 4.  Step 0 (one live beam): ranks 1 (tok 1), 2 (<EOS>), 3 (tok 3), ... -> <EOS> at rank 1 < K finishes.
    # Step 1: the two live beams' candidates put an <EOS> at rank 2 >= K: skipped, the non-<EOS> fill the slots.
    V = 4
    s0 = np.array([[NEG, 5.0, 4.0, 3.0]] * 2)
    s1 = np.array([[NEG, 1.0, 6.5, 9.0], [NEG, 9.0, 0.5, 1.0]])
    sel0 = beam_ref.select(np.array([0.0, -np.inf]), _lp(s0), EOS)
    assert sel0["tok"].tolist() == [1, 3] and sel0["bp"].tolist() == [0, 0] and [k for k, _ in sel0["finished"]] == [0]
    sel1 = beam_ref.select(sel0["scores"], _lp(s1), EOS)
    cand, order = beam_ref.rank(sel0["scores"], _lp(s1))
    assert [divmod(int(i), V) for i in order[:3]] == [(0, 3), (1, 1), (0, EOS)]
    assert sel1["finished"] == [] and sel1["nlive"] == 2 and EOS not in sel1["tok"].tolist()


def test_ties_go_to_the_lower_flat_index():
    K, V = 2, 5
    row = np.array([0.0, 1.0, -3.0, 1.0, 1.0])          # tokens 1, 3, 4 tie
    sel = beam_ref.select(np.array([-1.0, -1.0]), _lp(np.stack([row, row])), EOS)
    # candidates (beam 0, tok 1), (0, 3), (0, 4), (1, 1), ... tie: the first two by flat index live
    assert sel["tok"].tolist() == [1, 3] and sel["bp"].tolist() == [0, 0]
    assert sel["margin"] == 0.0                           # the tie is reported as a zero margin


def test_v_smaller_than_2k_leaves_beams_dead():
    # K = 4, V = 3: at step 0 only one beam is live, so at most 2 non-<EOS> candidates exist
    K, V = 4, 3
    sel = beam_ref.select(np.array([0.0] + [-np.inf] * (K - 1)), _lp(np.array([[1.0, 2.0, 0.5]] * K)), EOS)
    assert sel["nlive"] == 2 and sel["tok"].tolist() == [1, 0, EOS, EOS]
    assert np.isneginf(sel["scores"][2:]).all() and [k for k, _ in sel["finished"]] == [0]
    res = beam_ref.search(_scripted([np.array([[1.0, 2.0, 0.5]] * K)] * 6), K, V, 6, EOS)
    assert 1 <= len(res["hyps"]) <= K and all(np.isfinite(h[1]) for h in res["hyps"])


def test_max_dec_timesteps_finishes_the_live_beams():
    K, V, L = 2, 4, 3
    row = np.array([[0.0, 3.0, NEG, 2.0]] * K)              # <EOS> never wins
    res = beam_ref.search(_scripted([row] * L), K, V, L, EOS)
    assert res["steps"] == L and len(res["hyps"]) == K
    assert [h[2] for h in res["hyps"]] == [L, L] and all(EOS not in h[0] for h in res["hyps"])
    assert res["hyps"][0][0] == [1, 1, 1]
    assert np.isclose(res["hyps"][0][1], 3 * _lp(row[0])[1])


def test_length_penalty_reranks():
    # K = 2, V = 4: <EOS> at rank 1 finishes at step 0 (a short hypothesis, log 0.3 = -1.2); [1, <EOS>] finishes at
    # step 1 with a lower sum (log 0.6 + log 0.2 = -2.1) but a higher per-token average
    K, V = 2, 4
    s0 = np.log(np.array([1e-30, 0.6, 0.3, 0.1]))
    a = np.log(np.array([1e-30, 0.75, 0.2, 0.05]))
    e = np.log(np.array([1e-30, 0.05, 0.9, 0.05]))
    rows = [np.stack([s0, s0]), np.stack([a, a]), np.stack([e, e])]
    raw = beam_ref.search(_scripted(rows), K, V, 3, EOS, 0.0)
    norm = beam_ref.search(_scripted(rows), K, V, 3, EOS, 1.0)
    assert raw["hyps"][0][0] == [EOS]
    assert norm["hyps"][0][0] == [1, EOS]
    by_tokens = {tuple(h[0]): h for h in raw["hyps"]}
    for toks, key, n in norm["hyps"]:
        assert np.isclose(key, by_tokens[tuple(toks)][1] / n)
    keys = [h[1] for h in raw["hyps"]]
    assert keys == sorted(keys, reverse=True)


def test_beam_exports_and_abi_version():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    lib = hb.load()
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_beam_select_f32", "asr_beam_reorder_f32", "asr_beam_backtrack"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in hb.EXPORTS and hasattr(lib, name), name
    assert lib.asr_abi_version() == 8 == hb.ABI_VERSION
    assert "#define ASR_BEAM_KMAX 16" in header and "#define ASR_BEAM_FCAP 48" in header
    assert (hb.BEAM_KMAX, hb.BEAM_FCAP) == (16, 48)
