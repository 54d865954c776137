"""The word-level LM and lexicon on the GPU (csrc/word_lm.hip, csrc/ctc_beam.hip with a word LM, ops.word_lm_score,
ops.ctc_beam(word_lm=...), E2E.recognize_two_pass(word_lm=...), Solver.test with `word_lm`) against the
restatements of tests/word_lm_ref.py.  The allowance of every comparison is the restatement's own: 4 x the float32
restatement's error against float64, at least 8 fp32 ulps of the quantity's greatest magnitude.  Each case prints its worst
error / allowance with the `word-lm-parity` tag (`pytest -s`; profiles/word_lm_parity.txt holds one run)."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as R
import wer_ref
import word_lm_ref as WR

pytestmark = pytest.mark.gpu
EOS = 2


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


# ----------------------------------------------------------------------------------------------- asr_word_lm_score_f32
def _score_rows(V, L, n_seq, rs, wlm):
    """Ragged rows of tokens 1 .. V-1 with every shape of spacing: leading, double and trailing spaces, words outside the
    lexicon, lexicon words, one word of L tokens; the lengths 0, 1, L and -1 all occur."""
    space = V - 1
    lens = rs.randint(0, L + 1, size=n_seq)
    lens[:4] = [L, 0, 1, -1]
    ids = np.full((n_seq, L + 3), 10 ** 6, dtype=np.int32)               # (ld = L + 3; nothing behind a length is read)
    pool = [t for t in range(1, V)] + [space] * max(1, V // 4)
    for i, n in enumerate(lens):
        n = max(int(n), 0)
        row = [int(pool[rs.randint(len(pool))]) for _ in range(n)]
        if i % 5 == 1 and n >= 3:                                         # lexicon words between spaces
            row = []
            while len(row) < n:
                row += list(wlm.lexicon.spellings[rs.randint(len(wlm.lexicon))]) + [space] * rs.randint(1, 3)
            row = row[:n]
        if i % 5 == 2 and n >= 2:
            row[0] = row[-1] = space                                      # leading and trailing spaces
        if i % 5 == 3 and n >= 4:
            row[1] = row[2] = space                                       # a double space
        ids[i, :n] = row
    ids[0, :L] = 1                                                        # one word of L tokens
    return ids, lens


@pytest.mark.parametrize("V", [4, 34])
@pytest.mark.parametrize("order", [1, 3])
def test_word_lm_score_against_float64(hb, V, order):
    import ops
    wlm = WR.random_word_lm(V, order, 17 * V + order)
    table = wlm.compile()
    worst = 0.0
    for L in (1, 7, 100):
        n_seq = 200
        rs = np.random.RandomState(n_seq * 1000 + L)
        ids, lens = _score_rows(V, L, n_seq, rs, wlm)
        ids_dev = torch.from_numpy(ids).cuda()[:, :L]
        lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
        for eos_term in (True, False):
            hb.LAUNCHES.clear()
            score, n_words, terms = ops.word_lm_score(wlm, ids_dev, lens_dev, eos_term=eos_term, per_word=True)
            assert hb.LAUNCHES["word_lm_score"] == 1 and sum(hb.LAUNCHES.values()) == 1
            again = ops.word_lm_score(wlm, ids_dev, lens_dev, eos_term=eos_term)
            assert torch.equal(score, again[0]) and torch.equal(n_words, again[1])
            score, n_words, terms = score.cpu().numpy(), n_words.cpu().numpy(), terms.cpu().numpy()
            ref = [WR.walk(table, ids[i, :n], np.float64, eos_term) if n >= 0 else None for i, n in enumerate(lens)]
            r32 = [WR.walk(table, ids[i, :n], np.float32, eos_term) if n >= 0 else None for i, n in enumerate(lens)]
            mag = max([abs(float(r[0])) for r in ref if r] + [0.0])
            for i, n in enumerate(lens):
                if n < 0:
                    assert np.isneginf(score[i]) and n_words[i] == 0 and (terms[i] == 0).all()
                    continue
                want_words = wer_ref.words(ids[i, :n], V - 1)
                assert n_words[i] == len(want_words) == ref[i][2]
                allow = max(4 * abs(float(r32[i][0]) - float(ref[i][0])), 8 * R.ulp32(mag))
                err = abs(float(score[i]) - float(ref[i][0]))
                worst = max(worst, err / allow)
                assert err <= allow, (L, i, score[i], ref[i][0], allow)
                k = len(want_words)
                # (a term is acc + value in fp32, operation for operation: the float32 walk's bits)
                assert np.array_equal(terms[i, :k], np.array(r32[i][1], dtype=np.float32)) and (terms[i, k:] == 0).all()
            if L >= 7:                                                 # an id outside 0 .. V-1: NaN for that row only
                rows = [i for i, n in enumerate(lens) if n >= 1][:2]
                bad = ids.copy()
                bad[rows[0], lens[rows[0]] - 1] = V
                bad[rows[-1], 0] = -1
                got = ops.word_lm_score(wlm, torch.from_numpy(bad).cuda()[:, :L], lens_dev, eos_term=eos_term)[0].cpu().numpy()
                assert np.isnan(got[rows]).all()
                keep = np.ones(n_seq, dtype=bool)
                keep[rows] = False
                assert np.array_equal(got[keep], score[keep])
    print("word-lm-parity score V=%d order=%d: worst error / allowance %.3f" % (V, order, worst))


def test_argument_errors(hb):
    import ops
    wlm = WR.random_word_lm(5, 2, 3)
    ng_V = 5
    z = torch.zeros(1, 3, 5, device="cuda")
    lens = hb.to_device_i32([3], "cuda")
    import ngram_ref as N
    with pytest.raises(ValueError, match="ngram and word_lm"):
        ops.ctc_beam(z, lens, 2, ngram=N.random_lm(ng_V, 2, 3), word_lm=wlm)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(z, lens, 2, word_lm=WR.random_word_lm(6, 2, 3))
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(z, lens, 17, word_lm=wlm)
    t = hb._word_lm_table(wlm.to("cuda"), "test")
    import ctypes
    ids = torch.ones(2, 4, dtype=torch.int32, device="cuda")
    f = torch.zeros(4, device="cuda")
    lib = hb.load()
    assert lib.asr_word_lm_score_f32(0, 4, ctypes.byref(t), 1, hb.ptr(ids), 4, hb.ptr(ids), hb.ptr(f), hb.ptr(ids), None, hb.stream()) == -1
    assert lib.asr_word_lm_score_f32(2, 4, None, 1, hb.ptr(ids), 4, hb.ptr(ids), hb.ptr(f), hb.ptr(ids), None, hb.stream()) == -1
    t.eos = t.W
    assert lib.asr_word_lm_score_f32(2, 4, ctypes.byref(t), 1, hb.ptr(ids), 4, hb.ptr(ids), hb.ptr(f), hb.ptr(ids), None, hb.stream()) == -2
    t.eos = 2
    rc = lib.asr_ctc_beam_wlm_f32(1, 3, 5, 2, hb.ptr(z), 5, hb.ptr(lens), ctypes.byref(t), float("nan"), 0.0, 1, 0, hb.ptr(ids),
                                  hb.ptr(ids), hb.ptr(f), hb.ptr(f), hb.ptr(f), hb.ptr(ids), hb.ptr(f), hb.stream())
    assert rc == -1


# ------------------------------------------------------------------------------------------------- the fused search
def _fused(z, lens, V, K, wlm, alpha, beta, eos_term=True, lexicon_only=False):
    import hip_backend as hb
    import ops
    view = torch.from_numpy(z).cuda()[:, :, :V]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    out = ops.ctc_beam(view, lens_dev, K, word_lm=wlm, word_lm_weight=alpha, word_bonus=beta, eos_term=eos_term,
                       lexicon_only=lexicon_only)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], view, lens_dev


def _check_case(case, worst):
    V, K, T, scale, order, alpha, beta, lexicon_only = case
    z, lens, wlm = WR.grid_case(*case)
    (hyp, hyp_len, score, ctc, lms, nws), _, _ = _fused(z, lens, V, K, wlm, alpha, beta, lexicon_only=lexicon_only)
    verdict = WR.judge(case)
    for b in range(3):
        rows = []
        for k in range(K):
            n = int(hyp_len[b, k])
            if n < 0:                                                # an unused slot: behind every used one, -inf, all padding
                assert np.isneginf([score[b, k], ctc[b, k], lms[b, k]]).all() and (hyp[b, k] == -1).all() and nws[b, k] == -1
                assert (hyp_len[b, k:] == -1).all()
                continue
            h = tuple(int(c) for c in hyp[b, k, :n])
            assert n <= lens[b] and all(1 <= c < V for c in h) and (hyp[b, k, n:] == -1).all(), (b, k, h)
            assert np.isfinite([score[b, k], ctc[b, k], lms[b, k]]).all()
            assert nws[b, k] == len(wer_ref.words(h, V - 1)), (b, k, h)
            if lexicon_only:
                assert all(w in wlm.lexicon.index for w in wer_ref.words(h, V - 1)), (case, b, h)
            rows.append((h, dict(score=float(score[b, k]), ctc=float(ctc[b, k]), lm=float(lms[b, k]))))
        assert len({h for h, _ in rows}) == len(rows), "a hypothesis twice"
        assert all(a[1]["score"] >= c[1]["score"] for a, c in zip(rows, rows[1:])), "scores not descending"
        ref, allow = verdict[b]["ref"], verdict[b]["allowance"]
        at = {h: i for i, h in enumerate(ref["hyps"])}
        if verdict[b]["decisive"]:
            assert [h for h, _ in rows] == ref["hyps"], (case, b)
        else:
            assert lexicon_only or len(rows) >= 1
        for h, got in rows:                                          # undecided: only the scores of the shared hypotheses
            if h not in at:
                continue
            for q in WR.QUANTITIES:
                err = abs(got[q] - float(ref[q][at[h]]))
                worst[0] = max(worst[0], err / allow[q])
                assert err <= allow[q], "%r utterance %d %r: %s error %.3g above %.3g" % (case, b, h, q, err, allow[q])
    assert hyp_len[2].tolist() == [0] + [-1] * (K - 1) and ctc[2, 0] == 0.0 and nws[2, 0] == 0     # no frames: the empty hypothesis


@pytest.mark.parametrize("V", WR.GRID_V)
@pytest.mark.parametrize("K", WR.GRID_K)
def test_grid_against_the_restatement(hb, V, K):
    worst = [0.0]
    cases = [c for c in WR.grid()[0] if c[0] == V and c[1] == K]
    assert len(cases) == 8
    for case in cases:
        _check_case(case, worst)
    print("word-lm-parity search V=%d K=%d: worst error / allowance %.3f" % (V, K, worst[0]))


@pytest.mark.parametrize("case", WR.grid()[1], ids=lambda c: "V%d-K%d-T%d-x%g-o%d-a%g-b%g-l%d" % c)
def test_either_side_of_the_switches(hb, case):
    worst = [0.0]
    _check_case(case, worst)
    print("word-lm-parity search %r: worst error / allowance %.3f" % (case, worst[0]))


@pytest.mark.parametrize("V,K,T,scale", [(5, 4, 7, 1.0), (34, 4, 100, 1.0), (34, 16, 100, 50.0), (257, 16, 7, 1.0), (1030, 2, 3, 1.0),
                                         (5, 16, 257, 50.0)])
def test_zero_weights_are_the_plain_search_bit_for_bit(hb, V, K, T, scale):
    """alpha = beta = 0, no end term, lexicon_only off: hyp, hyp_len and ctc_score are ops.ctc_beam's bits on the same
    logits; lm_score and n_words are asr_word_lm_score_f32's over each hypothesis."""
    import ops
    z, lens, wlm = WR.grid_case(V, K, T, scale, 2, 0.0, 0.0, False)
    (hyp, hyp_len, score, ctc, lms, nws), view, lens_dev = _fused(z, lens, V, K, wlm, 0.0, 0.0, eos_term=False)
    p_hyp, p_len, p_score = [o.cpu().numpy() for o in ops.ctc_beam(view, lens_dev, K)]
    assert np.array_equal(hyp, p_hyp) and np.array_equal(hyp_len, p_len)
    assert np.array_equal(ctc.view(np.int32), p_score.view(np.int32))
    assert np.array_equal(score, p_score)                            # (tot + 0 lm) + 0 n_words = tot
    again, n_again = ops.word_lm_score(wlm, torch.from_numpy(hyp).cuda().view(3 * K, T), torch.from_numpy(hyp_len).cuda().view(-1),
                                       eos_term=False)
    assert np.array_equal(again.cpu().numpy().reshape(3, K).view(np.int32), lms.view(np.int32))
    live = hyp_len >= 0
    assert np.array_equal(n_again.cpu().numpy().reshape(3, K)[live], nws[live])


def test_launches_and_types(hb):
    import ops
    z, lens, wlm = WR.grid_case(34, 4, 100, 1.0, 3, 2.0, 1.5, False)
    zd = torch.from_numpy(z).cuda()[:, :, :34]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4)
    assert len(out) == 3 and dict(hb.LAUNCHES) == {"ctc_beam": 1, "ctc_beam_launch": 2}
    hb.LAUNCHES.clear()
    a = ops.ctc_beam(zd, lens_dev, 4, word_lm=wlm, word_lm_weight=2.0, word_bonus=1.5)
    assert len(a) == 6 and dict(hb.LAUNCHES) == {"ctc_beam_wlm": 1, "ctc_beam_wlm_launch": 2}
    with hb.deterministic(True):
        b = ops.ctc_beam(zd, lens_dev, 4, word_lm=wlm, word_lm_weight=2.0, word_bonus=1.5)
    for x, y in zip(a, b):                                           # two runs give the same bits
        assert torch.equal(x, y)
    assert [t.dtype for t in a] == [torch.int32, torch.int32] + [torch.float32] * 3 + [torch.int32]


def _one_frame_lm(eos_probs):
    """V = 5 (blank, a, b, c, <space>): the words a and b with equal unigrams and the given p(</s> | word)."""
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM
    ln = np.log
    lex = Lexicon([(1,), (2,)], None, 4, V=5)
    lm = NgramLM(2, 6, 1, 2, {(2,): ln(0.1), (4,): ln(0.45), (5,): ln(0.45), (4, 2): ln(eos_probs[0]), (5, 2): ln(eos_probs[1])},
                 {(4,): 0.0, (5,): 0.0})
    return WordLM(lm, lex)


def test_the_end_term_reorders(hb):
    """Two one-word labellings of one frame whose order the end-of-sentence term turns over."""
    wlm = _one_frame_lm((0.01, 0.9))
    z = np.full((1, 1, 5 + 3), np.nan, dtype=np.float32)
    z[0, 0, :5] = np.log(np.array([0.02, 0.5, 0.46, 0.01, 0.01]))
    (hyp, hyp_len, score, ctc, lms, nws), _, _ = _fused(z, [1], 5, 2, wlm, 1.0, 0.0, eos_term=False)
    assert hyp[0, :, 0].tolist() == [1, 2] and nws[0].tolist() == [1, 1]
    (hyp, hyp_len, score, ctc, lms, nws), _, _ = _fused(z, [1], 5, 2, wlm, 1.0, 0.0, eos_term=True)
    assert hyp[0, :, 0].tolist() == [2, 1] and score[0, 0] > score[0, 1] and ctc[0, 0] < ctc[0, 1]
    f = np.float32
    assert np.array_equal(score[0], ((ctc[0] + f(1.0) * lms[0]).astype(f) + f(0.0) * f(1.0)).astype(f))


def test_lexicon_only_lists_hold_lexicon_words(hb):
    """One frame whose best token c is in no word: without lexicon_only it leads as <unk> (oov_logp), with it it is gone and
    the list holds the lexicon's words, the empty hypothesis and the lone <space>."""
    wlm = _one_frame_lm((0.5, 0.5))
    z = np.full((2, 1, 5 + 3), np.nan, dtype=np.float32)
    z[0, 0, :5] = np.log(np.array([0.02, 0.2, 0.1, 0.67, 0.01]))
    z[1, 0, :5] = z[0, 0, :5]
    (hyp, hyp_len, score, ctc, lms, nws), _, _ = _fused(z, [1, 1], 5, 4, wlm, 0.01, 0.0, lexicon_only=False)
    assert hyp[0, 0, 0] == 3 and lms[0, 0] == np.float32(np.float32(-30.0) + np.float32(wlm.compile().uni_logp[2]))
    (hyp, hyp_len, score, ctc, lms, nws), _, _ = _fused(z, [1, 1], 5, 4, wlm, 0.01, 0.0, lexicon_only=True)
    for b in range(2):
        got = [tuple(hyp[b, k, :hyp_len[b, k]]) for k in range(4) if hyp_len[b, k] >= 0]
        assert got[:2] == [(1,), (2,)] and all(h in ((1,), (2,), (), (4,)) for h in got) and (3,) not in got


# ------------------------------------------------------------------------------------------------- the model and solver
@pytest.fixture(scope="module")
def tiny(hb):
    import test_beam_ctc_gpu as tb
    net, lm, xs, ilens, _ = tb._modules((0, 0.0, 14))
    return net, lm, xs, ilens


def _tiny_word_lm(V, seed=3, order=3, space=3):
    from word_lm import WordLM
    rs = np.random.RandomState(seed)
    letters = [c for c in range(4, V)]
    words = [tuple(int(letters[rs.randint(len(letters))]) for _ in range(rs.randint(1, 3))) for _ in range(12)]
    text = []
    for _ in range(40):
        row = []
        for _ in range(rs.randint(1, 5)):
            row += list(words[rs.randint(len(words))]) + [space]
        text.append(row[:-1])
    return WordLM.estimate(text, space, order, V=V, bos=1, eos=EOS)


@pytest.mark.parametrize("w,lmw,wlw,bonus,alpha", [(0.4, 0.0, 0.5, 0.0, 0.0), (0.3, 0.5, 0.7, 1.5, 0.0), (0.3, 0.5, 2.0, -1.0, 0.5)])
def test_two_pass_with_the_word_lm(hb, tiny, w, lmw, wlw, bonus, alpha):
    """The scores are ((1 - w) att + w ctc + lm_weight lm + word_lm_weight lm_word + word_bonus n_words) / (len + 1)**alpha
    recomputed in fp32 from last_two_pass's parts, bit for bit; the first pass is the fused search; lm_word and n_words are
    what asr_word_lm_score_f32 gives the returned hypotheses; without the LM the call is the old one."""
    import synth
    net, lm, xs, ilens = tiny
    K = 4
    wl = _tiny_word_lm(synth.TINY["output_dim"])
    hb.LAUNCHES.clear()
    tokens, scores = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, length_penalty=alpha, nbest=True, lm=lm if lmw else None,
                                            lm_weight=lmw, word_lm=wl, word_lm_weight=wlw, word_bonus=bonus)
    assert hb.LAUNCHES["ctc_beam_wlm"] == 1 and hb.LAUNCHES.get("ctc_beam", 0) == 0 and hb.LAUNCHES.get("ctc_beam_lm", 0) == 0
    p = {k: (None if v is None else v.cpu().numpy()) for k, v in net.last_two_pass.items()}
    f = np.float32
    live = p["hyp_len"] >= 0
    with np.errstate(invalid="ignore"):
        total = (p["att"].astype(f) * f(f(1.0) - f(w))).astype(f) + (p["ctc"].astype(f) * f(w)).astype(f)
        if lmw:
            total = (total + (p["lm"].astype(f) * f(lmw)).astype(f)).astype(f)
        total = (total + (p["word_lm"].astype(f) * f(wlw)).astype(f)).astype(f)
        total = (total + (np.maximum(p["n_words"], 0).astype(f) * f(bonus)).astype(f)).astype(f)
        if alpha:
            total = total / np.power((np.maximum(p["hyp_len"], 0) + 1).astype(f), f(alpha))
    total = np.where(live, total, -np.inf).astype(f)
    order = np.argsort(-total.astype(np.float64), axis=1, kind="stable")
    want = np.take_along_axis(total, order, axis=1)
    got = scores.cpu().numpy()
    if alpha:                                                        # (the power is the device's: an ulp of it may differ)
        np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=4 * np.finfo(f).eps)
    else:
        assert np.array_equal(got, want) and np.array_equal(p["order"], order)
    rank = ((p["ctc"] + (f(wlw) * p["word_lm"]).astype(f)).astype(f) + (f(bonus) * np.maximum(p["n_words"], 0).astype(f)).astype(f)).astype(f)
    assert np.array_equal(rank[live], p["rank"][live])
    rows = [[int(c) for c in p["hyp"][b, k, :max(int(p["hyp_len"][b, k]), 0)]] for b in range(got.shape[0]) for k in range(K)]
    again, n_again = net.word_lm_score(wl, rows)
    assert np.array_equal(again.cpu().numpy().reshape(-1, K)[live], p["word_lm"][live])
    assert np.array_equal(n_again.cpu().numpy().reshape(-1, K)[live], p["n_words"][live])
    assert [len(wer_ref.words(r, 3)) for r in rows] == [int(n) for n in n_again.cpu().numpy()]
    rescored, _ = net.word_lm_score(wl, tokens)                       # (a row counts up to its first <EOS>)
    assert rescored.shape == tokens.shape[:2]
    # without the LM: the existing call, launch for launch
    hb.LAUNCHES.clear()
    a = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True)
    n_plain = dict(hb.LAUNCHES)
    hb.LAUNCHES.clear()
    b = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True, word_lm=None, word_lm_weight=wlw, word_bonus=bonus)
    assert dict(hb.LAUNCHES) == n_plain and n_plain["ctc_beam"] == 1 and "ctc_beam_wlm" not in n_plain
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and "word_lm" not in net.last_two_pass


def test_refusals(hb, tiny):
    import synth
    import test_ngram_gpu as tn
    net, lm, xs, ilens = tiny
    V = synth.TINY["output_dim"]
    wl = _tiny_word_lm(V)
    hb.LAUNCHES.clear()
    for bad, kw in ((_tiny_word_lm(V + 1), {}), (wl, dict(ngram=tn._tiny_ngram(V)))):
        for call in (lambda: net.recognize_two_pass(xs, ilens, 4, word_lm=bad, word_lm_weight=0.5, **kw),
                     lambda: net.recognize_ctc_beams(xs, ilens, 4, word_lm=bad, word_lm_weight=0.5, **kw)):
            with pytest.raises(ValueError, match="word LM|word_lm"):
                call()
    with pytest.raises(ValueError, match="word LM"):
        net.word_lm_score(_tiny_word_lm(V + 1), [[4, 5]])
    assert sum(hb.LAUNCHES.values()) == 0
    ids, sc = net.recognize_ctc_beams(xs, ilens, 4, nbest=True, word_lm=wl, word_lm_weight=0.5, word_bonus=0.5)
    assert len(net.last_ctc_beams) == 6 and all(len(u) >= 1 and all(a >= b for a, b in zip(s, s[1:])) for u, s in zip(ids, sc))
    listed, n = net.word_lm_score(wl, [u[0] for u in ids])
    assert np.array_equal(listed.cpu().numpy(), net.last_ctc_beams[4][:, 0].cpu().numpy())
    assert np.array_equal(n.cpu().numpy(), net.last_ctc_beams[5][:, 0].cpu().numpy())
    ids, _ = net.recognize_ctc_beams(xs, ilens, 4, nbest=True, word_lm=wl, word_lm_weight=0.5, lexicon_only=True)
    assert all(w in wl.lexicon.index for u in ids for h in u for w in wer_ref.words(h, 3))


def test_solver_test_with_word_lm(hb, tmp_path, monkeypatch):
    """`word_lm` puts the ARPA file's word LM inside ctc_beam_decode and two_pass_decode; the lines are the direct calls';
    with the keys absent the launches are what they were; a misplaced key raises."""
    import test_ctc_gpu as tc
    from dataloader import get_data_loader
    from word_lm import WordLM, W_UNK
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    assert not any(k in cfg for k in ("word_lm", "lexicon", "word_lm_weight", "word_bonus", "lexicon_only"))
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    plain = sorted(i for s, i in solver.vocab.items() if not s.startswith("<"))
    assert len(plain) <= len(letters) and "<space>" in solver.vocab
    # the fixture's symbols are s0, s1, ...: a character model has one-character symbols, so they are renamed (same ids)
    solver.vocab = {(letters[plain.index(i)] if i in plain else s): i for s, i in solver.vocab.items()}
    vocab = solver.vocab
    space = vocab["<space>"]
    special = {vocab["<PAD>"], vocab["<BOS>"], vocab["<EOS>"], vocab["<NOISE>"]}        # (<NOISE> is no character of a word)
    sym = {i: s for s, i in vocab.items()}
    loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    text = [[int(c) for c in y if int(c) not in special] for batch in solver._feed(loader, sharded=False) for y in batch.ys_host]
    lm = WordLM.estimate(text, space, 3, V=len(vocab), bos=vocab["<BOS>"], eos=vocab["<EOS>"])
    names = {wid: "".join(sym[c] for c in sp) for sp, wid in zip(lm.lexicon.spellings, lm.word_ids)}
    names[W_UNK] = "<unk>"
    arpa = os.path.join(root, "words.arpa")
    with open(arpa, "w") as f:
        f.write(lm.lm.to_arpa(names))

    def run(**extra):
        solver.config = dict(cfg, **extra)
        hb.LAUNCHES.clear()
        solver.test(state_dict=sd)
        with open(os.path.join(root, "dev.txt")) as f:
            return f.read().splitlines(), dict(hb.LAUNCHES)

    def direct(fn):
        loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
        solver.model.eval()
        preds, refs = [], []
        for batch in solver._feed(loader, sharded=False):
            xs, ilens, _ = batch
            preds += fn(xs, ilens)
            refs += batch.ys_host
        solver.model.train()
        return solver.ind2sent(preds, refs)[1]

    run()
    absent, n_absent = run()
    assert not any(k.startswith(("ctc_beam", "word_lm")) for k in n_absent)
    back = solver.load_word_lm(arpa)
    assert sorted(back.lexicon.spellings) == sorted(lm.lexicon.spellings)
    lines, n = run(ctc_beam_decode=True, beam_size=4, word_lm=arpa, word_lm_weight=0.8, word_bonus=0.5)
    assert n["ctc_beam_wlm"] == 4 and n["ctc_beam_wlm_launch"] == 8 and "ctc_beam" not in n and "ctc_beam_lm" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_ctc_beams(xs, ilens, 4, word_lm=back, word_lm_weight=0.8,
                                                                              word_bonus=0.5)[0])
    lines, n = run(two_pass_decode=True, beam_size=4, ctc_decode_weight=0.4, word_lm=arpa, word_lm_weight=0.8, word_bonus=0.5,
                   lexicon_only=True)
    assert n["ctc_beam_wlm"] == 4 and "ctc_beam" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_two_pass(
        xs, ilens, 4, ctc_weight=0.4, word_lm=back, word_lm_weight=0.8, word_bonus=0.5,
        lexicon_only=True)[0].cpu().numpy().tolist())
    lex = os.path.join(root, "lexicon.txt")
    with open(lex, "w") as f:
        f.write("\n".join(list(names.values())[:3]) + "\n")
    run(ctc_beam_decode=True, beam_size=4, word_lm=arpa, lexicon=lex, word_lm_weight=0.8)
    for bad in (dict(word_lm=arpa, beam_size=4), dict(word_lm=arpa, ctc_greedy_decode=True), dict(word_lm_weight=0.5, beam_size=4),
                dict(ctc_beam_decode=True, word_lm=arpa, ngram_lm=arpa)):
        solver.config = dict(cfg, **bad)
        with pytest.raises(ValueError):
            solver.test(state_dict=sd)
