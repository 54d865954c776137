"""The restatement of joint CTC-attention beam search (tests/beam_ctc_ref.py) pinned without a GPU: the prefix recurrences
against an enumeration of every frame path, psi(g <EOS>) against torch's CTC loss, the search at ctc_weight = 0 against
beam_ref / beam_lm_ref, and the refusals of the Python surface that need no launch."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import beam_ctc_ref as R
import beam_lm_ref
import beam_ref
import synth


def _collapse(path):
    out, prev = [], 0
    for v in path:
        if v != 0 and v != prev:
            out.append(v)
        prev = v
    return tuple(out)


def _enumerate(x):
    """{collapsed label string: probability} over all V^T frame paths of log-probabilities x [T, V]."""
    T, V = x.shape
    probs = {}
    for path in itertools.product(range(V), repeat=T):
        key = _collapse(path)
        probs[key] = probs.get(key, 0.0) + float(np.exp(sum(x[t, v] for t, v in enumerate(path))))
    return probs


# Bound of the enumeration check, in probability: every compared number is at most 1; the enumeration adds at most
# V^T <= 1 024 products of at most 6 factors, the recurrences run at most 2 T logaddexp per value - about 1 100 roundings of
# 2^-53 relative each, 1.2e-13, taken twice.
ENUM_BOUND = 2.5e-13


@pytest.mark.parametrize("T,V", [(1, 3), (2, 3), (4, 3), (6, 3), (5, 4)])
def test_prefix_recurrences_against_path_enumeration(T, V):
    """exp(psi(h)) = P(the collapsed path starts with h), exp(psi(g <EOS>)) = P(it equals g), for every prefix up to length
    T + 1 (repeated labels included; longer than the frames allow: exactly -inf).  The slot of <EOS> holds the end score, so
    every state is scored under two choices of <EOS> and each label is read from the call in which it is an ordinary one."""
    rs = np.random.RandomState(10 * T + V)
    x = R.log_probs(rs.randn(T, V) * 2.0)
    probs = _enumerate(x)
    assert abs(sum(probs.values()) - 1.0) < ENUM_BOUND
    starts = lambda h: sum(p for s, p in probs.items() if s[:len(h)] == h)       # noqa: E731
    worst, seen = 0.0, 0
    stack = [((), R.prefix_init(x))]
    while stack:
        g, st = stack.pop()
        psi_a, psi_b = R.prefix_scores(st, x, eos=2), R.prefix_scores(st, x, eos=1)
        assert np.isneginf(psi_a[0]) and np.isneginf(psi_b[0])
        worst = max(worst, abs(np.exp(psi_a[2]) - probs.get(g, 0.0)), abs(np.exp(psi_b[1]) - probs.get(g, 0.0)))
        if g:
            assert abs(np.exp(st["psi_prev"]) - starts(g)) <= ENUM_BOUND
        for c in range(1, V):
            psi = psi_b if c == 2 else psi_a
            want = starts(g + (c,))
            worst = max(worst, abs(np.exp(psi[c]) - want))
            if want == 0.0:
                assert np.isneginf(psi[c]), (g, c)
            seen += 1
            if len(g) < T + 1:
                stack.append((g + (c,), R.prefix_advance(st, x, c, psi)))
    print("prefix recurrences T=%d V=%d: %d extensions, worst |exp(psi) - enumeration| %.2e" % (T, V, seen, worst))
    assert worst <= ENUM_BOUND, worst
    assert not any(np.isnan(v).any() for v in (psi_a, psi_b, st["r_n"], st["r_b"]))


def test_end_score_is_the_ctc_likelihood():
    """-psi(g <EOS>) of a prefix reached by prefix_advance against torch.nn.functional.ctc_loss, float64, random g (repeats
    included, one g without an alignment)."""
    T, V, eos = 12, 6, 2
    rs = np.random.RandomState(5)
    x = R.log_probs(rs.randn(T, V) * 3.0)
    lp = torch.from_numpy(x).unsqueeze(1)
    for g in ([], [3], [3, 3], [1, 4, 4, 5, 1], [int(v) for v in rs.randint(1, V, size=7)], [4] * 7):
        st = R.prefix_init(x)
        for c in g:
            st = R.prefix_advance(st, x, c, R.prefix_scores(st, x, eos))
        got = -R.prefix_scores(st, x, eos)[eos]
        want = float(F.ctc_loss(lp, torch.tensor([g], dtype=torch.long), torch.tensor([T]), torch.tensor([len(g)]), blank=0,
                                reduction="none", zero_infinity=False)) if g else -float(x[:, 0].sum())
        if np.isinf(want):
            assert np.isposinf(got), g
        else:
            np.testing.assert_allclose(got, want, rtol=1e-12, err_msg=str(g))
    assert np.isposinf(-R.prefix_scores(st, x, eos)[eos])                  # [4] * 7 needs 13 frames


def test_weight_zero_is_the_search_without_ctc(golden_dir):
    K, V, L, eos = 4, 11, 9, 2
    rs = np.random.RandomState(2)
    table, lm_table = rs.randn(L, K, V) * 2, rs.randn(L, K, V) * 2
    table[3:, :, eos] += 3.0
    x = R.log_probs(rs.randn(7, V))
    plain = beam_ref.search(lambda t, p, k: table[t], K, V, L, eos)
    fused = beam_lm_ref.search(lambda t, p, k: (table[t], lm_table[t]), K, V, L, eos, 0.4)
    assert R.search(lambda t, p, k: table[t], K, V, L, eos, x, 0.0) == plain
    assert R.search(lambda t, p, k: (table[t], lm_table[t]), K, V, L, eos, x, 0.0, lm_weight=0.4) == fused
    joint = R.search(lambda t, p, k: table[t], K, V, L, eos, x, 0.5)
    assert all(0 not in h[0] and len(h[0]) <= 7 + 1 for h in joint["hyps"])          # no blank, no more labels than frames
    # and over the decoder of the tiny fixture
    g = dict(np.load(os.path.join(golden_dir, "tiny_e2e.npz")))
    sd = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    w, b = rs.randn(synth.TINY["output_dim"], synth.TINY["enc_hidden_dim"]), rs.randn(synth.TINY["output_dim"])
    enc, lens = torch.from_numpy(g["enc_h"]), g["enc_lens"].tolist()
    a = R.decode(sd, w, b, enc, lens, 5, 2, 0.0)
    want = beam_ref.decode(sd, enc, lens, 5, 2)
    assert [r["hyps"] for r in a] == [r["hyps"] for r in want]


def test_refusals_that_need_no_gpu():
    import model as M
    xs = torch.zeros(2, 12, synth.TINY["input_dim"])
    ld = synth.labeldist(synth.TINY["output_dim"], 12)
    bare = M.E2E(labeldist=ld, **synth.TINY)
    with pytest.raises(ValueError, match="CTC head"):                      # no head, before the encoder runs
        bare.recognize_beams(xs, [12, 9], 5, 2, ctc_decode_weight=0.3)
    head = M.E2E(labeldist=ld, ctc_weight=0.3, **synth.TINY)
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            head.recognize_beams(xs, [12, 9], 5, 2, ctc_decode_weight=w)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            head.decoder.recognize_beams(torch.zeros(2, 3, 16), [3, 2], 5, 2, ctc_decode_weight=w)
    with pytest.raises(ValueError, match="ctc_logits"):
        head.decoder.recognize_beams(torch.zeros(2, 3, 16), [3, 2], 5, 2, ctc_decode_weight=0.3)
