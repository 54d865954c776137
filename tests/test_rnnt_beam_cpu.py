"""The transducer beam search's restatement (tests/rnnt_beam_ref.py) against the head's own loss and greedy decoder, and the
conditions the GPU tests lean on: no GPU needed."""
import functools

import numpy as np
import pytest

import rnnt_beam_ref as BR
import rnnt_ref as R


def seq_logp(p, enc_h, bos, seq):
    """log P(seq | enc_h) of the head in float64: -rnnt_ref.loss_and_grad on the sequence's own lattice."""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    pe = np.asarray(enc_h, np.float64) @ p["lin_enc.weight"].T + p["lin_enc.bias"]
    h = c = np.zeros(p["lstm.weight_hh_l0"].shape[1])
    pps = []
    for tok in (bos,) + tuple(seq):
        h, c = R._cell(p, tok, h, c, np)
        pps.append(p["lin_pred.weight"] @ h)
    z = R.joint(pe, np.stack(pps))
    return -float(R.loss_and_grad(z @ p["lin_out.weight"].T + p["lin_out.bias"], list(seq))[0])


def exhaustive_case(T, seed=31):
    p, enc_h = BR.grid_case(3, 8, T, seed)
    return dict(p=p, enc_h=enc_h, bos=1, K=16, L=3)


@functools.lru_cache(maxsize=None)
def small_lm(V):
    import ngram
    rs = np.random.RandomState(V)
    seqs = [[int(t) for t in rs.randint(3, V, rs.randint(1, 6))] for _ in range(40)]
    return ngram.NgramLM.estimate(seqs, 3, V, 1, 2)


@pytest.mark.parametrize("T", (1, 2, 4))
def test_exhaustive_beam_equals_the_loss(T):
    """V = 3, L = 3, K = 16: all 15 sequences stay in the beam, so the merged masses ARE the loss's alpha - this proves the
    merge rule.  The case is decisive (the GPU test compares every final)."""
    case = exhaustive_case(T)
    out = BR.search(case["p"], case["enc_h"], 1, 16, 3)
    assert len(out["finals"]) == 15 and len(set(f["tokens"] for f in out["finals"])) == 15
    for f in out["finals"]:
        assert abs(float(f["tot"]) - seq_logp(case["p"], case["enc_h"], 1, f["tokens"])) <= 1e-12, f["tokens"]
    assert BR.judge(case)["decisive"]


@pytest.mark.parametrize("name", sorted(R.DECODE_CASES))
def test_beam_one_is_greedy(name):
    """K = 1 walks greedy's path (max_symbols = max_len): greedy's hypothesis is among the finals with greedy's score as the
    sum of its label terms.  It is the BEST final wherever the blank wins before the last frame ends the utterance: at the
    last frame every prefix of the path finalises (the blank there is a final, and the one entry goes on with its best
    label), so a shorter prefix can outrank it - both cases have such a row, and a row where greedy's hypothesis is the best."""
    p, enc_h, lens, _, max_len = R.decode_case(name)
    best = 0
    for b, t in enumerate(lens):
        want = R.greedy(p, enc_h[b, :t], 1, max_len, max_len)
        got = BR.search(p, enc_h[b, :t], 1, 1, max_len)["finals"]
        same = [f for f in got if list(f["tokens"]) == want["tokens"]]
        assert len(same) == 1 and abs(float(same[0]["label_lp"]) - want["score"]) <= 1e-12
        assert all(f["tokens"] == same[0]["tokens"][:len(f["tokens"])] or same[0]["tokens"] == f["tokens"][:len(same[0]["tokens"])]
                   for f in got)                                     # one path: every final is a prefix or an extension
        best += got[0] is same[0]
    print("rnnt-beam K = 1 vs greedy, %s: greedy's hypothesis is the best final in %d of %d rows" % (name, best, len(lens)))
    assert best >= 1


def test_finals_are_below_the_sequence_probability_and_unique():
    """The beam's mass of a sequence is a subset of its paths: tot <= log P(y | x); a sequence finalises once."""
    for V, K, J, lens, L, seed in BR.GRID:
        p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
        for enc_h in utts:
            out = BR.search(p, enc_h, 1, K, L)
            assert len(out["finalised"]) == len(set(out["finalised"])) >= 1
            for f in out["finals"][:K]:
                if enc_h.shape[0]:
                    assert float(f["tot"]) <= seq_logp(p, enc_h, 1, f["tokens"]) + 1e-12
                else:
                    assert f["tokens"] == () and float(f["tot"]) == 0.0


def test_ngram_weights():
    """Zero weights: the plain search.  With weights: lm is the LM's score of the hypothesis, with and without </s>."""
    lm = small_lm(34)
    table = lm.compile()
    p, enc_h = BR.grid_case(34, 32, 7, 6)
    plain = BR.search(p, enc_h, 1, 4, 4)["finals"][:4]
    zero = BR.search(p, enc_h, 1, 4, 4, table=table)["finals"][:4]
    assert [(f["tokens"], float(f["tot"]), float(f["rank"])) for f in plain] == \
        [(f["tokens"], float(f["tot"]), float(f["rank"])) for f in zero]
    for eos_term in (True, False):
        got = BR.search(p, enc_h, 1, 4, 4, table=table, alpha=0.7, beta=0.3, eos_term=eos_term)["finals"][:4]
        for f in got:
            want = lm.score(list(f["tokens"]), eos_term=eos_term)
            assert abs(float(f["lm"]) - want) <= 1e-5 * max(1.0, abs(want)), (f["tokens"], float(f["lm"]), want)
            assert abs(float(f["rank"]) - ((float(f["tot"]) + 0.7 * float(f["lm"])) + 0.3 * len(f["tokens"]))) <= 1e-12
    fused = BR.search(p, enc_h, 1, 4, 4, table=table, alpha=0.7, beta=0.3)["finals"][:4]
    assert [f["tokens"] for f in fused] != [f["tokens"] for f in plain]      # (the weights do change this search)


def test_the_grid_is_decisive():
    """At most 10 % of the grid's utterances are undecided between the float64 and the float32 restatement (the GPU test
    compares hypotheses and order only where judge() is decisive); the exhaustive cases are all decisive."""
    total = undecided = 0
    for V, K, J, lens, L, seed in BR.GRID:
        p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
        for enc_h in utts:
            total += 1
            undecided += not BR.judge(dict(p=p, enc_h=enc_h, bos=1, K=K, L=L))["decisive"]
    print("rnnt-beam grid: %d of %d utterances undecided" % (undecided, total))
    assert undecided <= 0.1 * total
    lm = small_lm(34).compile()
    for V, K, J, lens, L, seed in BR.GRID:
        if V == 34:
            p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
            for enc_h in utts:
                total += 1
                undecided += not BR.judge(dict(p=p, enc_h=enc_h, bos=1, K=K, L=L, table=lm, alpha=0.7, beta=0.3))["decisive"]
    assert undecided <= 0.1 * total


def test_workspace_size_and_refusals_need_no_gpu():
    """asr_transducer_beam_ws_bytes runs on plain integers: the refusals (K outside 1 .. 16, J not a multiple of 4, V < 2,
    the LDS bound K (J + V) * 4 <= 56 KB) as UnsupportedShape, an accepted shape as its documented size, the C entries
    declared in the header and exported by the library."""
    import os
    import re
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    for B, T, J, V, K, L in ((3, 8, 32, 34, 0, 4), (3, 8, 32, 34, 17, 4), (3, 8, 30, 34, 4, 4), (3, 8, 32, 1, 4, 4),
                             (3, 8, 1024, 34, 16, 4), (1, 8, 868, 32, 16, 4), (1, 8, 3584, 4, 4, 4)):
        with pytest.raises(hb.UnsupportedShape):
            hb.rnnt_beam_ws_bytes(B, T, J, V, K, L, 16, 16)
    assert hb.RNNT_BEAM_LDS_BYTES == 56 * 1024
    assert hb.rnnt_beam_ws_bytes(1, 8, 864, 32, 16, 4, 16, 16) > 0       # 16 (864 + 32) * 4 = 57 344: the bound itself is inside
    with pytest.raises(RuntimeError):
        hb.rnnt_beam_ws_bytes(0, 8, 32, 34, 4, 4, 16, 16)               # (an argument error, not a shape)
    r64 = lambda n: (n + 63) // 64 * 64                                  # noqa: E731
    B, T, J, V, K, L, P = 3, 8, 260, 65, 16, 40, 16
    bk = r64(B * K)
    want = 8 * (2 * bk + r64((T + L) * B * K)) + 4 * (17 * bk + 3 * r64(B) + r64(B * K * P))
    assert hb.rnnt_beam_ws_bytes(B, T, J, V, K, L, 16, P) == want
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_transducer_beam_\w+)\s*\(", header, flags=re.M))
    assert len(declared) == 5 and declared <= set(hb.EXPORTS) and all(hasattr(hb.load(), n) for n in declared)


@pytest.mark.parametrize("K", (1, 2, 4, 16))
def test_tie_rule_blank_against_labels(K):
    """Two frames, L = 1: the blank ties with both labels at iteration 0 and wins (flat index 0); the merged candidates tie
    at iteration 1 and keep their slot order."""
    p = BR.tie_params(3, 4, 3)
    got = [f["tokens"] for f in BR.search(p, np.ones((2, 16), np.float32), 1, K, 1)["finals"][:K]]
    assert got == {1: [()], 2: [(), (1,)]}.get(K, [(), (1,), (2,)])


@pytest.mark.parametrize("K", (1, 2, 4, 16))
def test_tie_rule(K):
    """lin_out zero and one frame: no candidate merges, every candidate of one length ties, and the order is the rule's -
    the lower flat index (parent V + token) in the beam, the earlier iteration and then the lower slot among the finals."""
    p = BR.tie_params(3, 4, 3)
    enc_h = np.ones((1, 16), np.float32)
    got = [f["tokens"] for f in BR.search(p, enc_h, 1, K, 3)["finals"][:K]]
    want = [(), (1,), (2,), (1, 1), (1, 2), (2, 1), (2, 2), (1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (2, 1, 1), (2, 1, 2),
            (2, 2, 1), (2, 2, 2)]
    kept, out = [()], []
    for _ in range(4):                                               # the beam by the rule: K lowest flat indices per iteration
        out += kept
        kept = [s + (k,) for s in kept for k in (1, 2) if len(s) < 3][:K]
    assert got == out[:K] and (K < 16 or got == want)
