"""Contextual biasing on the GPU (csrc/context.hip, csrc/ctc_beam.hip with a context, ops.context_score,
ops.ctc_beam(context=...), E2E.recognize_two_pass(context=...), Solver.test with `context_bias`) against the
restatements of tests/context_ref.py.  The allowance of every comparison is the restatement's own: 4 x the float32
restatement's error against float64, at least 8 fp32 ulps of the quantity's greatest magnitude.  Utterances whose float64
selection margin lies inside the allowance are left undecided (only the scores of the shared hypotheses are checked);
tests/test_context_cpu.py asserts that at most 1 in 10 of a parametrisation are.  Each case prints its worst error / allowance
with the `ctx-parity` tag (`pytest -s`; profiles/context_parity.txt holds one run: the worst over the grid and the switches
0.38 of the allowance, the scorer 0.14)."""
import os

import numpy as np
import pytest
import torch

import context_ref as C
import ctc_beam_ref as R
import poison as P

from context import ContextBatch, ContextGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _i32(hb, values):
    return hb.to_device_i32([int(v) for v in values], "cuda")


# ------------------------------------------------------------------------------------------------- asr_context_score_f32
@pytest.mark.parametrize("V", [5, 34])
def test_context_score_against_float64(hb, V):
    import ops
    space = V - 1 if V > 5 else None
    graphs = [ContextGraph(*C.random_phrases(V, 6 if V <= 5 else 30, 11 + V), V=V),
              ContextGraph(*C.random_phrases(V, 4 if V <= 5 else 20, 12 + V, space), V=V, word_start_only=space)]
    worst = 0.0
    for L in (1, 40):
        rs = np.random.RandomState(100 * V + L)
        n_seq = 67
        lens = rs.randint(0, L + 1, size=n_seq)
        lens[:4] = [L, 0, 1 if L >= 1 else 0, -1]                      # the lengths 0, 1, L and -1 all occur
        graph_of = rs.randint(-1, 2, size=n_seq)
        graph_of[:6] = [0, 1, -1, 0, 1, -1]
        ids = np.full((n_seq, L + 3), 10 ** 6, dtype=np.int32)         # (ld = L + 3; nothing behind a length is read)
        for i, n in enumerate(lens):
            ids[i, :max(n, 0)] = rs.randint(1, V, size=max(n, 0))
        batch = ContextBatch(graphs, graph_of)
        table = batch.compile()
        nxt = C.dense(table)
        ids_dev = torch.from_numpy(ids).cuda()[:, :L]
        lens_dev = _i32(hb, lens)
        hb.LAUNCHES.clear()
        score, tok = ops.context_score(batch, ids_dev, lens_dev, per_token=True)
        assert hb.LAUNCHES["context_score"] == 1 and sum(hb.LAUNCHES.values()) == 1
        assert torch.equal(score, ops.context_score(batch, ids_dev, lens_dev))
        assert torch.equal(score, ops.context_score(batch, ids_dev, lens_dev, graph_of=_i32(hb, graph_of)))
        for pattern in P.PATTERNS:                                     # nothing of the outputs is left to the allocation
            with P.poisoned(pattern):
                s2, t2 = ops.context_score(batch, ids_dev, lens_dev, per_token=True)
            assert torch.equal(s2.view(torch.int32), score.view(torch.int32)) and torch.equal(t2.view(torch.int32), tok.view(torch.int32))
        score, tok = score.cpu().numpy(), tok.cpu().numpy()
        roots = [int(table.root[g]) if g >= 0 else -1 for g in graph_of]
        ref = [C.walk(table, roots[i], ids[i, :n], np.float64, nxt) if n >= 0 else None for i, n in enumerate(lens)]
        r32 = [C.walk(table, roots[i], ids[i, :n], np.float32, nxt) if n >= 0 else None for i, n in enumerate(lens)]
        mag = max([abs(float(r[0])) for r in ref if r] + [0.0])
        for i, n in enumerate(lens):
            if n < 0:
                assert np.isneginf(score[i]) and (tok[i] == 0).all()
                continue
            allow = max(4 * abs(float(r32[i][0]) - float(ref[i][0])), 8 * R.ulp32(mag))
            err = abs(float(score[i]) - float(ref[i][0]))
            worst = max(worst, err / allow)
            assert err <= allow, (L, i, score[i], ref[i][0], allow)
            assert np.array_equal(tok[i, :n], np.array(ref[i][1][:n], dtype=np.float32)) and (tok[i, n:] == 0).all()
            assert graph_of[i] >= 0 or (score[i] == 0 and (tok[i] == 0).all())
            assert abs(float(score[i]) - batch.score(i, ids[i, :n])) <= 1e-4 * max(1.0, mag)      # the graph's own float64
        rows = [i for i, n in enumerate(lens) if n >= 1][:2]             # an id outside 1 .. V-1: NaN for that row only
        bad = ids.copy()
        bad[rows[0], lens[rows[0]] - 1] = V
        bad[rows[-1], 0] = 0
        got = ops.context_score(batch, torch.from_numpy(bad).cuda()[:, :L], lens_dev).cpu().numpy()
        assert np.isnan(got[rows]).all()
        keep = np.ones(n_seq, dtype=bool)
        keep[rows] = False
        assert np.array_equal(got[keep], score[keep])
    print("ctx-parity score V=%d: worst error / allowance %.3f" % (V, worst))


# ------------------------------------------------------------------------------------------------- the fused search
def _search(z, lens, V, K, context, weight, lm=None, alpha=0.0, beta=0.0, eos_term=True):
    import hip_backend as hb
    import ops
    view = torch.from_numpy(z).cuda()[:, :, :V]
    lens_dev = _i32(hb, lens)
    out = ops.ctc_beam(view, lens_dev, K, ngram=lm, ngram_weight=alpha, ngram_bonus=beta, eos_term=eos_term, context=context,
                       ctx_weight=weight)
    torch.cuda.synchronize()
    return out, view, lens_dev


def _named(out, with_lm):
    names = ("hyp", "hyp_len", "score", "ctc") + (("lm",) if with_lm else ()) + ("ctx",)
    assert len(out) == len(names)
    return {k: v.cpu().numpy() for k, v in zip(names, out)}


def _check_case(case, worst):
    import ops
    V, K, T, scale, with_lm, weight, variant = case
    z, lens, batch, lm = C.grid_case(case)
    out, view, lens_dev = _search(z, lens, V, K, batch, weight, lm, *C.LM_WEIGHTS)
    for pattern in P.PATTERNS:                                       # the same bits whatever the allocations held
        with P.poisoned(pattern):
            again, _, _ = _search(z, lens, V, K, batch, weight, lm, *C.LM_WEIGHTS)
        for a, b in zip(out, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (case, pattern)
    # ctx_score is the scoring kernel's output for each hypothesis, bit for bit
    graph_rows = torch.from_numpy(np.repeat(batch.graph_of, K).astype(np.int32)).cuda()
    rescored = ops.context_score(batch, out[0].view(3 * K, T), out[1].view(-1), graph_of=graph_rows).view(3, K)
    assert torch.equal(rescored.view(torch.int32), out[-1].view(torch.int32)), case
    got = _named(out, with_lm)
    verdict = C.judge(case)
    qs = C.quantities(case)
    for b in range(3):
        rows = []
        for k in range(K):
            n = int(got["hyp_len"][b, k])
            if n < 0:                                                # an unused slot: behind every used one, -inf, all padding
                assert all(np.isneginf(got[q][b, k]) for q in qs) and (got["hyp"][b, k] == -1).all()
                assert (got["hyp_len"][b, k:] == -1).all()
                continue
            h = tuple(int(c) for c in got["hyp"][b, k, :n])
            assert n <= lens[b] and all(1 <= c < V for c in h) and (got["hyp"][b, k, n:] == -1).all(), (b, k, h)
            assert all(np.isfinite(got[q][b, k]) for q in qs)
            rows.append((h, {q: float(got[q][b, k]) for q in qs}))
        assert len({h for h, _ in rows}) == len(rows) >= 1, "a hypothesis twice, or none"
        assert all(a[1]["score"] >= c[1]["score"] for a, c in zip(rows, rows[1:])), "scores not descending"
        if batch.graph_of[b] < 0:
            assert all(r["ctx"] == 0.0 for _, r in rows)
        ref, allow = verdict[b]["ref"], verdict[b]["allowance"]
        at = {h: i for i, h in enumerate(ref["hyps"])}
        if verdict[b]["decisive"]:
            assert [h for h, _ in rows] == ref["hyps"], (case, b)
        for h, r in rows:                                            # undecided: only the scores of the shared hypotheses
            if h not in at:
                continue
            for q in qs:
                err = abs(r[q] - float(ref[q][at[h]]))
                worst[0] = max(worst[0], err / allow[q])
                assert err <= allow[q], "%r utterance %d %r: %s error %.3g above %.3g" % (case, b, h, q, err, allow[q])
    assert got["hyp_len"][2].tolist() == [0] + [-1] * (K - 1)         # no frames: the empty hypothesis, final(root) = 0
    assert got["ctc"][2, 0] == 0.0 and got["ctx"][2, 0] == 0.0


@pytest.mark.parametrize("V", C.GRID_V)
@pytest.mark.parametrize("K", C.GRID_K)
def test_grid_against_the_restatement(hb, V, K):
    worst = [0.0]
    cases = [c for c in C.grid()[0] if c[0] == V and c[1] == K]
    assert len(cases) == 6
    for case in cases:
        _check_case(case, worst)
    print("ctx-parity search V=%d K=%d: worst error / allowance %.3f" % (V, K, worst[0]))


@pytest.mark.parametrize("case", C.grid()[1], ids=lambda c: "V%d-K%d-T%d-x%g-lm%d-w%g-g%d" % c)
def test_either_side_of_the_switches(hb, case):
    worst = [0.0]
    _check_case(case, worst)
    print("ctx-parity search %r: worst error / allowance %.3f" % (case, worst[0]))


@pytest.mark.parametrize("V,K,T,with_lm", [(5, 4, 7, False), (34, 4, 40, True), (34, 16, 40, False), (65, 16, 7, True),
                                           (5, 16, 257, False), (5, 16, 257, True)])
def test_zero_weight_and_no_graph_are_the_search_without_a_context(hb, V, K, T, with_lm):
    """ctx_weight = 0, and graph_of = -1 everywhere, each give the plain (with an LM: the n-gram) search bit for bit; with
    the weight at 0 ctx_score still is the scorer's sum over each hypothesis."""
    import ops
    case = (V, K, T, 1.0, with_lm, 1.0, 0)
    z, lens, batch, lm = C.grid_case(case)
    a, bt = C.LM_WEIGHTS
    view = torch.from_numpy(z).cuda()[:, :, :V]
    lens_dev = _i32(hb, lens)
    plain = ops.ctc_beam(view, lens_dev, K, ngram=lm, ngram_weight=a, ngram_bonus=bt) if with_lm else ops.ctc_beam(view, lens_dev, K)
    plain = tuple(plain) if with_lm else tuple(plain) + (plain[2],)                      # (plain: the score IS tot)
    zero, _, _ = _search(z, lens, V, K, batch, 0.0, lm, a, bt)
    none, _, _ = _search(z, lens, V, K, ContextBatch(batch.graphs, [-1, -1, -1]), 1.0, lm, a, bt)
    for got in (zero, none):
        for x, y in zip(plain, got[:len(plain)]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert (none[-1][none[1] >= 0] == 0).all() and torch.isneginf(none[-1][none[1] < 0]).all()
    rows = torch.from_numpy(np.repeat(batch.graph_of, K).astype(np.int32)).cuda()
    again = ops.context_score(batch, zero[0].view(3 * K, T), zero[1].view(-1), graph_of=rows).view(3, K)
    assert torch.equal(again.view(torch.int32), zero[-1].view(torch.int32)) and (zero[-1][:2].abs() > 0).any()


def test_without_a_context_nothing_changes(hb):
    import ops
    case = (34, 4, 40, 1.0, True, 1.0, 0)
    z, lens, batch, lm = C.grid_case(case)
    zd = torch.from_numpy(z).cuda()[:, :, :34]
    lens_dev = _i32(hb, lens)
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4)
    assert len(out) == 3 and dict(hb.LAUNCHES) == {"ctc_beam": 1, "ctc_beam_launch": 2}
    hb.LAUNCHES.clear()
    out_none = ops.ctc_beam(zd, lens_dev, 4, context=None, ctx_weight=3.0)
    assert dict(hb.LAUNCHES) == {"ctc_beam": 1, "ctc_beam_launch": 2} and all(torch.equal(a, b) for a, b in zip(out, out_none))
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4, ngram=lm, ngram_weight=0.5, context=None)
    assert len(out) == 5 and dict(hb.LAUNCHES) == {"ctc_beam_lm": 1, "ctc_beam_lm_launch": 2}
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4, context=batch)
    assert len(out) == 5 and dict(hb.LAUNCHES) == {"ctc_beam_ctx": 1, "ctc_beam_ctx_launch": 2}
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4, ngram=lm, ngram_weight=0.5, context=batch.graphs[0], ctx_weight=0.5)
    assert len(out) == 6 and hb.LAUNCHES["ctc_beam_ctx"] == 1 and hb.LAUNCHES["ctc_beam_ctx_launch"] == 2
    assert [t.dtype for t in out] == [torch.int32, torch.int32] + [torch.float32] * 4


def test_two_runs_give_the_same_bits(hb):
    case = (34, 4, 40, 4.0, True, 2.5, 1)
    z, lens, batch, lm = C.grid_case(case)
    a, _, _ = _search(z, lens, 34, 4, batch, 2.5, lm, *C.LM_WEIGHTS)
    with hb.deterministic(True):
        b, _, _ = _search(z, lens, 34, 4, batch, 2.5, lm, *C.LM_WEIGHTS)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _frames(rows, V):
    """One utterance whose frames have the given probabilities over the tokens 0 .. V-1 (ld = V + 3, NaN in the padding)."""
    z = np.full((1, len(rows), V + 3), np.nan, dtype=np.float32)
    z[0, :, :V] = np.log(np.array(rows, dtype=np.float64))
    return z


def test_a_phrase_turns_the_ranking_over(hb):
    """Two labellings the plain search ranks one way; the phrase of the second turns them over, and every score says why."""
    import ops
    V = 5
    z = _frames([[0.02, 0.5, 0.4, 0.04, 0.04], [0.02, 0.03, 0.03, 0.55, 0.37]], V)     # (1 3) 0.275, (2 3) 0.22, (2 4) 0.148
    view = torch.from_numpy(z).cuda()[:, :, :V]
    lens_dev = _i32(hb, [2])
    hyp, hyp_len, score = ops.ctc_beam(view, lens_dev, 2)
    assert hyp[0].tolist() == [[1, 3], [2, 3]] and hyp_len[0].tolist() == [2, 2]
    g = ContextGraph([[2, 4]], boost=1.5, V=V)
    hyp, hyp_len, score, ctc, ctx = ops.ctc_beam(view, lens_dev, 2, context=g)
    assert hyp[0].tolist() == [[2, 4], [1, 3]] and ctx[0].tolist() == [3.0, 0.0] and ctc[0, 0] < ctc[0, 1]
    f = np.float32
    assert np.array_equal(score[0].cpu().numpy(), (ctc[0].cpu().numpy() + f(1.0) * ctx[0].cpu().numpy()).astype(f))
    assert abs(float(ctc[0, 0]) - np.log(0.148)) < 1e-5 and abs(float(ctc[0, 1]) - np.log(0.275)) < 1e-5
    # a small weight leaves the order alone
    hyp, hyp_len, score, ctc, ctx = ops.ctc_beam(view, lens_dev, 2, context=g, ctx_weight=0.05)
    assert hyp[0].tolist() == [[1, 3], [2, 3]] and ctx[0].tolist() == [0.0, 0.0]


def test_a_failed_phrase_gives_its_boost_back(hb):
    """K = 2: the first token of a phrase is boosted into the beam, past a labelling the plain search keeps there; the phrase
    does not go on, a later frame takes the boost back - and the final list is the plain search's, scores included."""
    import ops
    V = 5
    z = _frames([[0.02, 0.50, 0.30, 0.12, 0.06], [0.90, 0.03, 0.03, 0.02, 0.02], [0.04, 0.02, 0.40, 0.04, 0.50]], V)
    view = torch.from_numpy(z).cuda()[:, :, :V]
    p_hyp, p_len, p_score = ops.ctc_beam(view, _i32(hb, [3]), 2)
    assert p_hyp[0, :, :2].tolist() == [[1, 4], [1, 2]]
    g = ContextGraph([[3, 1, 1]], boost=2.0, V=V)                      # token 3 opens the phrase; nothing continues it
    # after two frames token 3 sits in the beam (as a hypothesis its credit is back: ctx 0, ranked behind) where the plain
    # search holds token 2
    two, _, _, two_ctc, two_ctx = ops.ctc_beam(view[:, :2], _i32(hb, [2]), 2, context=g)
    assert two[0, :, 0].tolist() == [1, 3] and two_ctx[0].tolist() == [0.0, 0.0]
    assert ops.ctc_beam(view[:, :2], _i32(hb, [2]), 2)[0][0, :, 0].tolist() == [1, 2]
    hyp, hyp_len, score, ctc, ctx = ops.ctc_beam(view, _i32(hb, [3]), 2, context=g)
    assert hyp[0].tolist() == p_hyp[0].tolist() and hyp_len[0].tolist() == p_len[0].tolist() and ctx[0].tolist() == [0.0, 0.0]
    ref = C.search_ctx(z[0, :, :V].astype(np.float64), 2, g.compile(), 0, 1.0)
    assert [[c for c in h if c >= 0] for h in hyp[0].tolist()] == [list(h) for h in ref["hyps"]]
    allow = 8 * R.ulp32(float(np.abs(ref["score"]).max()))
    assert np.abs(score[0].cpu().numpy() - p_score[0].cpu().numpy()).max() <= allow
    assert np.abs(ctc[0].cpu().numpy() - p_score[0].cpu().numpy()).max() <= allow
    assert np.abs(score[0].cpu().numpy().astype(np.float64) - ref["score"]).max() <= allow


# ------------------------------------------------------------------------------------------------- the model and solver
@pytest.fixture(scope="module")
def tiny(hb):
    import test_beam_ctc_gpu as tb
    net, lm, xs, ilens, _ = tb._modules((0, 0.0, 14))
    return net, lm, xs, ilens


def _tiny_context(V, seed=5):
    rs = np.random.RandomState(seed)
    return ContextGraph([[int(c) for c in rs.randint(3, V, size=rs.randint(1, 4))] for _ in range(12)], boost=1.5, V=V)


@pytest.mark.parametrize("w,ngw,cw", [(0.4, 0.0, 1.0), (0.3, 0.7, 0.5)])
def test_two_pass_with_a_context(hb, tiny, w, ngw, cw):
    """The scores are ((1 - w) att + w ctc [+ ngram_weight lm_ngram + ngram_bonus len] + ctx_weight ctx) recomputed in fp32 from
    last_two_pass's parts, bit for bit; the first pass is the search with the context inside; ctx is what
    asr_context_score_f32 gives the returned hypotheses; without a context the call is the old one."""
    import synth
    import test_ngram_gpu as tn
    net, lm, xs, ilens = tiny
    K, V = 4, synth.TINY["output_dim"]
    ng = tn._tiny_ngram(V) if ngw else None
    ctx = _tiny_context(V)
    hb.LAUNCHES.clear()
    tokens, scores = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True, ngram=ng, ngram_weight=ngw, ngram_bonus=0.5,
                                            context=ctx, ctx_weight=cw)
    assert hb.LAUNCHES["ctc_beam_ctx"] == 1 and hb.LAUNCHES.get("ctc_beam", 0) == 0 and hb.LAUNCHES.get("ctc_beam_lm", 0) == 0
    p = {k: (None if v is None else v.cpu().numpy()) for k, v in net.last_two_pass.items()}
    f = np.float32
    live = p["hyp_len"] >= 0
    with np.errstate(invalid="ignore"):
        total = (p["att"].astype(f) * f(f(1.0) - f(w))).astype(f) + (p["ctc"].astype(f) * f(w)).astype(f)
        if ngw:
            total = (total + (p["ngram"].astype(f) * f(ngw)).astype(f)).astype(f)
            total = (total + (np.maximum(p["hyp_len"], 0).astype(f) * f(0.5)).astype(f)).astype(f)
        total = (total + (p["context"].astype(f) * f(cw)).astype(f)).astype(f)
    total = np.where(live, total, -np.inf).astype(f)
    order = np.argsort(-total.astype(np.float64), axis=1, kind="stable")
    assert np.array_equal(scores.cpu().numpy(), np.take_along_axis(total, order, axis=1)) and np.array_equal(p["order"], order)
    rows = [[int(c) for c in p["hyp"][b, k, :max(int(p["hyp_len"][b, k]), 0)]] for b in range(p["hyp"].shape[0]) for k in range(K)]
    again = net.context_score(ctx, rows).cpu().numpy().reshape(-1, K)
    assert np.array_equal(again[live], p["context"][live]) and np.abs(p["context"][live]).max() > 0
    hb.LAUNCHES.clear()
    a = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True)
    n_plain = dict(hb.LAUNCHES)
    hb.LAUNCHES.clear()
    b = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True, context=None, ctx_weight=cw)
    assert dict(hb.LAUNCHES) == n_plain and "ctc_beam_ctx" not in n_plain and "context" not in net.last_two_pass
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals(hb, tiny):
    import ops
    import synth
    net, lm, xs, ilens = tiny
    V = synth.TINY["output_dim"]
    hb.LAUNCHES.clear()
    bad = _tiny_context(V + 1)
    for call in (lambda: net.recognize_two_pass(xs, ilens, 4, context=bad), lambda: net.recognize_ctc_beams(xs, ilens, 4, context=bad),
                 lambda: net.context_score(bad, [[4, 5]]),
                 lambda: net.recognize_ctc_beams(xs, ilens, 4, context=_tiny_context(V), word_lm=object())):
        with pytest.raises(ValueError):
            call()
    z = torch.zeros(2, 3, 5, device="cuda")
    lens = _i32(hb, [3, 2])
    g = ContextGraph([[1, 2]], V=5)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(z, lens, 2, context=ContextGraph([[1, 2]], V=6))
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(z, lens, 17, context=g)
    with pytest.raises(ValueError, match="utterances"):
        ops.ctc_beam(z, lens, 2, context=ContextBatch([g], [0, 0, -1]))
    assert sum(hb.LAUNCHES.values()) == 0
    # the C entry: null pointers and a weight that is not finite are ASR_E_ARG, sizes that do not fit ASR_E_SHAPE
    lib = hb.load()
    t, rows = hb._context_table(g.to("cuda"), 2, "test")
    import ctypes
    ints = torch.zeros(2 * 2 * 3, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, device="cuda")
    ws = torch.zeros(256, device="cuda")

    def call(**kw):
        tab = kw.get("table", t)
        return lib.asr_ctc_beam_ctx_f32(2, 3, kw.get("V", 5), 2, hb.ptr(z), 5, hb.ptr(lens), ctypes.byref(tab) if tab is not None else None,
                                        kw.get("rows", hb.ptr(rows)), kw.get("weight", 1.0), kw.get("S", 0), None, None, 0, -1, 0.0,
                                        0.0, hb.ptr(ints), hb.ptr(ints), hb.ptr(f), hb.ptr(f), None, kw.get("ctx", hb.ptr(f)),
                                        hb.ptr(ws), hb.stream())
    assert call(weight=float("nan")) == -1 and call(weight=float("inf")) == -1 and call(rows=None) == -1 and call(ctx=None) == -1
    assert call(table=None) == -1 and call(S=3) == -1 and call(S=-1) == -1
    wrong_v = hb.ContextTable.from_buffer_copy(t)
    wrong_v.V = 6
    assert call(table=wrong_v) == -2
    for field, value in (("N", 0), ("G", 0), ("R", 0), ("A", -1), ("V", 1)):
        broken = hb.ContextTable.from_buffer_copy(t)
        setattr(broken, field, value)
        assert call(table=broken) == -2, field
        assert lib.asr_context_score_f32(2, 3, ctypes.byref(broken), hb.ptr(rows), hb.ptr(ints), 3, hb.ptr(lens), hb.ptr(f), None,
                                         hb.stream()) == -2
    assert lib.asr_context_score_f32(0, 3, ctypes.byref(t), hb.ptr(rows), hb.ptr(ints), 3, hb.ptr(lens), hb.ptr(f), None, hb.stream()) == -1
    assert lib.asr_context_score_f32(2, 3, ctypes.byref(t), None, hb.ptr(ints), 3, hb.ptr(lens), hb.ptr(f), None, hb.stream()) == -1
    torch.cuda.synchronize()
    ids, sc = net.recognize_ctc_beams(xs, ilens, 4, nbest=True, context=_tiny_context(V), ctx_weight=0.8)
    assert len(net.last_ctc_beams) == 5 and all(len(u) >= 1 and all(a >= b for a, b in zip(s, s[1:])) for u, s in zip(ids, sc))
    listed = net.context_score(_tiny_context(V), [u[0] for u in ids]).cpu().numpy()
    assert np.array_equal(listed, net.last_ctc_beams[4][:, 0].cpu().numpy())


def test_solver_test_with_context_bias(hb, tmp_path, monkeypatch):
    """`context_bias` puts the phrase file's list inside ctc_beam_decode and two_pass_decode (alone and beside ngram_lm); the
    lines are the direct calls'; with the key absent the launches are what they were; a misplaced key raises."""
    import test_ctc_gpu as tc
    from dataloader import get_data_loader
    from ngram import NgramLM
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    assert "context_bias" not in cfg
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    vocab = solver.vocab
    special = {vocab["<PAD>"], vocab["<BOS>"], vocab["<EOS>"]}
    symbols = {i: s for s, i in vocab.items() if i not in special}
    loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    text = [[int(c) for c in y if int(c) not in special] for batch in solver._feed(loader, sharded=False) for y in batch.ys_host]
    phrases = os.path.join(root, "phrases.txt")
    with open(phrases, "w") as f:
        for row in text[:3]:
            f.write(" ".join(symbols[c] for c in row[:3]) + " 2.5\n")
        f.write(" ".join(symbols[c] for c in text[-1][:2]) + "\n")
    arpa = os.path.join(root, "lm.arpa")
    with open(arpa, "w") as f:
        f.write(NgramLM.estimate(text, 3, len(vocab), vocab["<BOS>"], vocab["<EOS>"]).to_arpa(symbols))
    back = NgramLM.from_arpa(arpa, vocab, vocab["<BOS>"], vocab["<EOS>"], V=len(vocab))
    sub = dict(phrases=phrases, boost=1.5, weight=0.8)
    graph = solver.load_context(sub)
    assert graph.boosts == [2.5] * 3 + [1.5] and graph.V == len(vocab)

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
    assert not any(k.startswith(("ctc_beam", "context")) for k in n_absent)
    plain, n_plain = run(ctc_beam_decode=True, beam_size=4)
    assert n_plain["ctc_beam"] == 4 and "ctc_beam_ctx" not in n_plain
    lines, n = run(ctc_beam_decode=True, beam_size=4, context_bias=sub)
    assert n["ctc_beam_ctx"] == 4 and n["ctc_beam_ctx_launch"] == 8 and "ctc_beam" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_ctc_beams(xs, ilens, 4, context=graph, ctx_weight=0.8)[0])
    lines, n = run(ctc_beam_decode=True, beam_size=4, context_bias=sub, ngram_lm=arpa, ngram_weight=0.8, ngram_bonus=0.5)
    assert n["ctc_beam_ctx"] == 4 and "ctc_beam_lm" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_ctc_beams(xs, ilens, 4, ngram=back, ngram_weight=0.8, ngram_bonus=0.5,
                                                                              context=graph, ctx_weight=0.8)[0])
    lines, n = run(two_pass_decode=True, beam_size=4, ctc_decode_weight=0.4, context_bias=sub)
    assert n["ctc_beam_ctx"] == 4 and "ctc_beam" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_two_pass(
        xs, ilens, 4, ctc_weight=0.4, context=graph, ctx_weight=0.8)[0].cpu().numpy().tolist())
    for bad in (dict(context_bias=sub, beam_size=4), dict(context_bias=sub, ctc_greedy_decode=True),
                dict(context_bias=dict(weight=1.0), ctc_beam_decode=True), dict(context_bias=dict(sub, bonus=1), ctc_beam_decode=True)):
        solver.config = dict(cfg, **bad)
        with pytest.raises(ValueError, match="context_bias"):
            solver.test(state_dict=sd)
