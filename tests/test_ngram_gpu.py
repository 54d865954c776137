"""The n-gram LM on the GPU (csrc/ngram.hip, csrc/ctc_beam.hip with an LM, ops.ngram_score, ops.ctc_beam(ngram=...),
E2E.recognize_two_pass(ngram=...), Solver.test with `ctc_beam_decode` / `ngram_lm`) against the restatements
of tests/ngram_ref.py.  The allowance of every comparison is the restatement's own: 4 x the float32 restatement's error
against float64, at least 8 fp32 ulps of the quantity's greatest magnitude.  Each case prints its worst error / allowance
with the `ngram_parity` tag (`pytest -s`; profiles/ngram_parity.txt holds one run)."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as R
import ngram_ref as N

pytestmark = pytest.mark.gpu
EOS = 2


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


# ------------------------------------------------------------------------------------------------- asr_ngram_score_f32
@pytest.mark.parametrize("V", [3, 257])
@pytest.mark.parametrize("order", [1, 4])
def test_ngram_score_against_float64(hb, V, order):
    import ops
    lm = N.random_lm(V, order, 17 * V + order)
    table = lm.compile()
    worst = 0.0
    for n_seq, L, only in [(65, L, None) for L in (1, 7, 100)] + [(1, L, n) for L in (1, 7, 100) for n in (L, 0, 1, -1)]:
        rs = np.random.RandomState(n_seq * 1000 + L)
        lens = rs.randint(0, L + 1, size=n_seq)
        lens[:4] = [L, 0, 1, -1] if n_seq > 1 else [only]               # the lengths 0, 1, L and -1 all occur
        ids = np.full((n_seq, L + 3), 10 ** 6, dtype=np.int32)           # (ld = L + 3; nothing behind a length is read)
        for i, n in enumerate(lens):
            ids[i, :max(n, 0)] = rs.randint(1, V, size=max(n, 0))
        ids_dev = torch.from_numpy(ids).cuda()[:, :L]
        lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
        for eos_term in (True, False):
            hb.LAUNCHES.clear()
            score, tok = ops.ngram_score(lm, ids_dev, lens_dev, eos_term=eos_term, per_token=True)
            assert hb.LAUNCHES["ngram_score"] == 1 and sum(hb.LAUNCHES.values()) == 1
            assert torch.equal(score, ops.ngram_score(lm, ids_dev, lens_dev, eos_term=eos_term))
            score, tok = score.cpu().numpy(), tok.cpu().numpy()
            ref = [N.walk(table, ids[i, :n], np.float64, eos_term) if n >= 0 else None for i, n in enumerate(lens)]
            r32 = [N.walk(table, ids[i, :n], np.float32, eos_term) if n >= 0 else None for i, n in enumerate(lens)]
            mag = max([abs(float(r[0])) for r in ref if r] + [0.0])
            for i, n in enumerate(lens):
                if n < 0:
                    assert np.isneginf(score[i]) and (tok[i] == 0).all()
                    continue
                allow = max(4 * abs(float(r32[i][0]) - float(ref[i][0])), 8 * R.ulp32(mag))
                err = abs(float(score[i]) - float(ref[i][0]))
                worst = max(worst, err / allow)
                assert err <= allow, (n_seq, L, i, score[i], ref[i][0], allow)
                assert np.array_equal(tok[i, :n], np.array(ref[i][1][:n], dtype=np.float32)) and (tok[i, n:] == 0).all()
            if lens.max() >= 1 and n_seq > 1:                      # an id outside 0 .. V-1: NaN for that row only
                rows = [i for i, n in enumerate(lens) if n >= 1][:2]
                bad = ids.copy()
                bad[rows[0], lens[rows[0]] - 1] = V
                bad[rows[-1], 0] = -1
                got = ops.ngram_score(lm, torch.from_numpy(bad).cuda()[:, :L], lens_dev, eos_term=eos_term).cpu().numpy()
                assert np.isnan(got[rows]).all()
                keep = np.ones(n_seq, dtype=bool)
                keep[rows] = False
                assert np.array_equal(got[keep], score[keep])
    print("ngram_parity score V=%d order=%d: worst error / allowance %.3f" % (V, order, worst))


def test_ngram_score_argument_errors(hb):
    import ops
    lm = N.random_lm(5, 2, 3)
    ids = torch.ones(2, 4, dtype=torch.int32, device="cuda")
    lens = hb.to_device_i32([4, 2], "cuda")
    t = lm.to("cuda")
    lib = hb.load()
    args = lambda **kw: [kw.get("N", 2), 4, kw.get("S", t.S), kw.get("V", 5), hb.ptr(t.logp), hb.ptr(t.nxt), kw.get("start", t.start),  # noqa: E731
                         kw.get("eos", 2), hb.ptr(ids), 4, hb.ptr(lens), hb.ptr(ids), None, hb.stream()]
    assert lib.asr_ngram_score_f32(*args(N=0)) == -1
    assert lib.asr_ngram_score_f32(*args(start=t.S)) == -2 and lib.asr_ngram_score_f32(*args(eos=5)) == -2
    assert lib.asr_ngram_score_f32(*args(V=1)) == -2
    other = N.random_lm(6, 2, 3)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(torch.zeros(1, 3, 5, device="cuda"), hb.to_device_i32([3], "cuda"), 2, ngram=other)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(torch.zeros(1, 3, 5, device="cuda"), hb.to_device_i32([3], "cuda"), 17, ngram=lm)
    z = torch.zeros(1, 3, 5, device="cuda")
    f = torch.zeros(4, device="cuda")
    rc = lib.asr_ctc_beam_lm_f32(1, 3, 5, 2, hb.ptr(z), 5, hb.ptr(lens), t.S, hb.ptr(t.logp), hb.ptr(t.nxt), t.start, 2,
                                 float("nan"), 0.0, hb.ptr(ids), hb.ptr(ids), hb.ptr(f), hb.ptr(f), hb.ptr(f), hb.ptr(f), hb.stream())
    assert rc == -1


# ------------------------------------------------------------------------------------------------- the fused search
def _fused(z, lens, V, K, lm, alpha, beta, eos_term=True):
    import hip_backend as hb
    import ops
    view = torch.from_numpy(z).cuda()[:, :, :V]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    out = ops.ctc_beam(view, lens_dev, K, ngram=lm, ngram_weight=alpha, ngram_bonus=beta, eos_term=eos_term)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], view, lens_dev


def _check_case(case, worst):
    V, K, T, scale, order, alpha, beta = case
    z, lens, lm = N.grid_case(*case)
    (hyp, hyp_len, score, ctc, lms), _, _ = _fused(z, lens, V, K, lm, alpha, beta)
    verdict = N.judge(case)
    for b in range(3):
        rows = []
        for k in range(K):
            n = int(hyp_len[b, k])
            if n < 0:                                                # an unused slot: behind every used one, -inf, all padding
                assert np.isneginf([score[b, k], ctc[b, k], lms[b, k]]).all() and (hyp[b, k] == -1).all()
                assert (hyp_len[b, k:] == -1).all()
                continue
            h = tuple(int(c) for c in hyp[b, k, :n])
            assert n <= lens[b] and all(1 <= c < V for c in h) and (hyp[b, k, n:] == -1).all(), (b, k, h)
            assert np.isfinite([score[b, k], ctc[b, k], lms[b, k]]).all()
            rows.append((h, dict(score=float(score[b, k]), ctc=float(ctc[b, k]), lm=float(lms[b, k]))))
        assert len({h for h, _ in rows}) == len(rows) >= 1, "a hypothesis twice, or none"
        assert all(a[1]["score"] >= c[1]["score"] for a, c in zip(rows, rows[1:])), "scores not descending"
        ref, allow = verdict[b]["ref"], verdict[b]["allowance"]
        at = {h: i for i, h in enumerate(ref["hyps"])}
        if verdict[b]["decisive"]:
            assert [h for h, _ in rows] == ref["hyps"], (case, b)
        for h, got in rows:                                          # undecided: only the scores of the shared hypotheses
            if h not in at:
                continue
            for q in N.QUANTITIES:
                err = abs(got[q] - float(ref[q][at[h]]))
                worst[0] = max(worst[0], err / allow[q])
                assert err <= allow[q], "%r utterance %d %r: %s error %.3g above %.3g" % (case, b, h, q, err, allow[q])
    assert hyp_len[2].tolist() == [0] + [-1] * (K - 1) and ctc[2, 0] == 0.0       # no frames: the empty hypothesis


@pytest.mark.parametrize("V", N.GRID_V)
@pytest.mark.parametrize("K", N.GRID_K)
def test_grid_against_the_restatement(hb, V, K):
    worst = [0.0]
    cases = [c for c in N.grid()[0] if c[0] == V and c[1] == K]
    assert len(cases) == 8
    for case in cases:
        _check_case(case, worst)
    print("ngram_parity search V=%d K=%d: worst error / allowance %.3f" % (V, K, worst[0]))


@pytest.mark.parametrize("case", N.grid()[1], ids=lambda c: "V%d-K%d-T%d-x%g-o%d-a%g-b%g" % c)
def test_either_side_of_the_switches(hb, case):
    worst = [0.0]
    _check_case(case, worst)
    print("ngram_parity search %r: worst error / allowance %.3f" % (case, worst[0]))


@pytest.mark.parametrize("V,K,T,scale", [(5, 4, 7, 1.0), (34, 4, 100, 1.0), (34, 16, 100, 50.0), (257, 16, 7, 1.0), (1030, 2, 3, 1.0),
                                         (5, 16, 257, 50.0)])
def test_zero_weights_are_the_plain_search_bit_for_bit(hb, V, K, T, scale):
    """alpha = beta = 0, no end term: hyp, hyp_len and ctc_score are ops.ctc_beam's bits on the same logits, and lm_score
    is the LM's fp32 sum over each hypothesis (asr_ngram_score_f32's bits)."""
    import ops
    z, lens, lm = N.grid_case(V, K, T, scale, 2, 0.0, 0.0)
    (hyp, hyp_len, score, ctc, lms), view, lens_dev = _fused(z, lens, V, K, lm, 0.0, 0.0, eos_term=False)
    p_hyp, p_len, p_score = [o.cpu().numpy() for o in ops.ctc_beam(view, lens_dev, K)]
    assert np.array_equal(hyp, p_hyp) and np.array_equal(hyp_len, p_len)
    assert np.array_equal(ctc.view(np.int32), p_score.view(np.int32))
    assert np.array_equal(score, p_score)                            # (tot + 0 lm) + 0 len = tot
    again = ops.ngram_score(lm, torch.from_numpy(hyp).cuda().view(3 * K, T), torch.from_numpy(hyp_len).cuda().view(-1),
                            eos_term=False).cpu().numpy().reshape(3, K)
    assert np.array_equal(again.view(np.int32), lms.view(np.int32))


def test_without_an_lm_nothing_changes(hb):
    import ops
    z, lens = R.grid_case(34, 4, 100, 1.0)
    zd = torch.from_numpy(z).cuda()[:, :, :34]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4)
    assert len(out) == 3 and dict(hb.LAUNCHES) == {"ctc_beam": 1, "ctc_beam_launch": 2}
    hb.LAUNCHES.clear()
    out = ops.ctc_beam(zd, lens_dev, 4, ngram=N.random_lm(34, 2, 1), ngram_weight=0.5)
    assert len(out) == 5 and dict(hb.LAUNCHES) == {"ctc_beam_lm": 1, "ctc_beam_lm_launch": 2}


def test_two_runs_give_the_same_bits(hb):
    import ops
    case = (34, 4, 100, 1.0, 4, 2.0, 1.5)
    z, lens, lm = N.grid_case(*case)
    zd = torch.from_numpy(z).cuda()[:, :, :34]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    a = ops.ctc_beam(zd, lens_dev, 4, ngram=lm, ngram_weight=2.0, ngram_bonus=1.5)
    with hb.deterministic(True):
        b = ops.ctc_beam(zd, lens_dev, 4, ngram=lm, ngram_weight=2.0, ngram_bonus=1.5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert [t.dtype for t in a] == [torch.int32, torch.int32] + [torch.float32] * 3


def test_the_end_term_reorders(hb):
    """Two labellings of one frame whose order the end-of-sentence term turns over; ties go to the search's order."""
    from ngram import NgramLM
    ln = np.log
    lm = NgramLM(2, 5, 1, 2, {(2,): ln(0.1), (3,): ln(0.45), (4,): ln(0.45), (3, 2): ln(0.01), (4, 2): ln(0.9)},
                 {(3,): 0.0, (4,): 0.0})
    z = np.full((1, 1, 5 + 3), np.nan, dtype=np.float32)
    z[0, 0, :5] = ln(np.array([0.02, 0.01, 0.01, 0.5, 0.46]))
    (hyp, hyp_len, score, ctc, lms), _, _ = _fused(z, [1], 5, 2, lm, 1.0, 0.0, eos_term=False)
    assert hyp[0, :, 0].tolist() == [3, 4]
    (hyp, hyp_len, score, ctc, lms), _, _ = _fused(z, [1], 5, 2, lm, 1.0, 0.0, eos_term=True)
    assert hyp[0, :, 0].tolist() == [4, 3] and score[0, 0] > score[0, 1] and ctc[0, 0] < ctc[0, 1]
    f = np.float32
    assert np.array_equal(score[0], ((ctc[0] + f(1.0) * lms[0]).astype(f) + f(0.0) * f(1.0)).astype(f))


# ------------------------------------------------------------------------------------------------- the model and solver
@pytest.fixture(scope="module")
def tiny(hb):
    import test_beam_ctc_gpu as tb
    net, lm, xs, ilens, _ = tb._modules((0, 0.0, 14))
    return net, lm, xs, ilens


def _tiny_ngram(V, seed=3, order=3):
    from ngram import NgramLM
    rs = np.random.RandomState(seed)
    text = [[int(c) for c in rs.randint(3, V, size=rs.randint(1, 9))] for _ in range(40)]
    return NgramLM.estimate(text, order, V, 1, EOS)


@pytest.mark.parametrize("w,lmw,ngw,bonus,alpha", [(0.4, 0.0, 0.5, 0.0, 0.0), (0.3, 0.5, 0.7, 1.5, 0.0), (0.3, 0.5, 2.0, -1.0, 0.5)])
def test_two_pass_with_the_ngram_lm(hb, tiny, w, lmw, ngw, bonus, alpha):
    """The scores are ((1 - w) att + w ctc + lm_weight lm + ngram_weight lm_ngram + ngram_bonus len) / (len + 1)**alpha
    recomputed in fp32 from last_two_pass's parts, bit for bit; the ranking follows them; the first pass is the fused
    search; lm_ngram is what asr_ngram_score_f32 gives the returned hypotheses; without the LM the call is the old one."""
    import synth
    net, lm, xs, ilens = tiny
    K = 4
    ng = _tiny_ngram(synth.TINY["output_dim"])
    hb.LAUNCHES.clear()
    tokens, scores = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, length_penalty=alpha, nbest=True, lm=lm if lmw else None,
                                            lm_weight=lmw, ngram=ng, ngram_weight=ngw, ngram_bonus=bonus)
    assert hb.LAUNCHES["ctc_beam_lm"] == 1 and hb.LAUNCHES.get("ctc_beam", 0) == 0
    p = {k: (None if v is None else v.cpu().numpy()) for k, v in net.last_two_pass.items()}
    f = np.float32
    live = p["hyp_len"] >= 0
    with np.errstate(invalid="ignore"):
        total = (p["att"].astype(f) * f(f(1.0) - f(w))).astype(f) + (p["ctc"].astype(f) * f(w)).astype(f)
        if lmw:
            total = (total + (p["lm"].astype(f) * f(lmw)).astype(f)).astype(f)
        total = (total + (p["ngram"].astype(f) * f(ngw)).astype(f)).astype(f)
        total = (total + (np.maximum(p["hyp_len"], 0).astype(f) * f(bonus)).astype(f)).astype(f)
        if alpha:
            total = total / np.power((np.maximum(p["hyp_len"], 0) + 1).astype(f), f(alpha))
    total = np.where(live, total, -np.inf).astype(f)
    order = np.argsort(-total.astype(np.float64), axis=1, kind="stable")
    want = np.take_along_axis(total, order, axis=1)
    got = scores.cpu().numpy()
    if alpha:                                                        # (the power is the device's: an ulp of it may differ)
        np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=4 * np.finfo(f).eps)
        order = p["order"]
    else:
        assert np.array_equal(got, want) and np.array_equal(p["order"], order)
    assert (np.diff(got, axis=1)[np.isfinite(got[:, 1:])] <= 0).all()
    tok = tokens.cpu().numpy()
    for b in range(tok.shape[0]):
        for r in range(K):
            k = int(order[b, r])
            n = int(p["hyp_len"][b, k])
            h = [] if n < 0 else [int(c) for c in p["hyp"][b, k, :n]]
            assert tok[b, r].tolist() == h + [EOS] * (tok.shape[2] - len(h))
    # the parts are the fused search's, and lm_ngram is the scoring kernel's sum of the returned rows
    rank = ((p["ctc"] + (f(ngw) * p["ngram"]).astype(f)).astype(f) + (f(bonus) * np.maximum(p["hyp_len"], 0).astype(f)).astype(f)).astype(f)
    assert np.array_equal(rank[live], p["rank"][live])
    rescored = net.ngram_score(ng, tokens).cpu().numpy()                # (a row counts up to its first <EOS>)
    again = net.ngram_score(ng, [[int(c) for c in p["hyp"][b, k, :max(int(p["hyp_len"][b, k]), 0)]]
                                 for b in range(tok.shape[0]) for k in range(K)]).cpu().numpy().reshape(-1, K)
    assert np.array_equal(again[live], p["ngram"][live])
    for b in range(tok.shape[0]):
        for r in range(K):
            k = int(order[b, r])
            if live[b, k] and EOS not in p["hyp"][b, k, :p["hyp_len"][b, k]]:
                assert rescored[b, r] == p["ngram"][b, k]
    # without the LM: the existing call, launch for launch
    hb.LAUNCHES.clear()
    a = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True)
    n_plain = dict(hb.LAUNCHES)
    hb.LAUNCHES.clear()
    b = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, nbest=True, ngram=None, ngram_weight=ngw, ngram_bonus=bonus)
    assert dict(hb.LAUNCHES) == n_plain and n_plain["ctc_beam"] == 1 and "ctc_beam_lm" not in n_plain
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and "ngram" not in net.last_two_pass


def test_refusals(hb, tiny):
    import synth
    from ngram import NgramLM
    net, lm, xs, ilens = tiny
    V = synth.TINY["output_dim"]
    hb.LAUNCHES.clear()
    for bad in (_tiny_ngram(V + 1), NgramLM.estimate([[4, 5]], 2, V, 1, 3), NgramLM.estimate([[4, 5]], 2, V, 3, EOS)):
        for call in (lambda: net.recognize_two_pass(xs, ilens, 4, ngram=bad, ngram_weight=0.5),
                     lambda: net.recognize_ctc_beams(xs, ilens, 4, ngram=bad, ngram_weight=0.5),
                     lambda: net.ngram_score(bad, [[4, 5]])):
            with pytest.raises(ValueError, match="n-gram"):
                call()
    assert sum(hb.LAUNCHES.values()) == 0
    ids, sc = net.recognize_ctc_beams(xs, ilens, 4, nbest=True, ngram=_tiny_ngram(V), ngram_weight=0.5, ngram_bonus=0.5)
    assert len(net.last_ctc_beams) == 5 and all(len(u) >= 1 and all(a >= b for a, b in zip(s, s[1:])) for u, s in zip(ids, sc))
    listed = net.ngram_score(_tiny_ngram(V), [u[0] for u in ids]).cpu().numpy()
    assert np.array_equal(listed, net.last_ctc_beams[4][:, 0].cpu().numpy())


def test_solver_test_with_ctc_beam_decode_and_ngram_lm(hb, tmp_path, monkeypatch):
    """`ctc_beam_decode` decodes with recognize_ctc_beams alone, `ngram_lm` puts the ARPA file's LM inside it (and inside
    two_pass_decode); the lines are the direct calls'; with the keys absent the launches are what they were; a misplaced
    key raises."""
    import test_ctc_gpu as tc
    from dataloader import get_data_loader
    from ngram import NgramLM
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    assert not any(k in cfg for k in ("ctc_beam_decode", "ngram_lm", "ngram_weight", "ngram_bonus"))
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    vocab = solver.vocab
    special = {vocab["<PAD>"], vocab["<BOS>"], vocab["<EOS>"]}
    symbols = {i: s for s, i in vocab.items() if i not in special}
    assert all(len(s.split()) == 1 for s in symbols.values())
    loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    text = [[int(c) for c in y if int(c) not in special] for batch in solver._feed(loader, sharded=False) for y in batch.ys_host]
    lm = NgramLM.estimate(text, 3, len(vocab), vocab["<BOS>"], vocab["<EOS>"])
    arpa = os.path.join(root, "lm.arpa")
    with open(arpa, "w") as f:
        f.write(lm.to_arpa(symbols))

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
    off, n_off = run(ctc_beam_decode=False)
    assert off == absent and n_off == n_absent and not any(k.startswith(("ctc_beam", "ngram")) for k in n_absent)
    back = NgramLM.from_arpa(arpa, vocab, vocab["<BOS>"], vocab["<EOS>"], V=len(vocab))
    lines, n = run(ctc_beam_decode=True, beam_size=4)
    assert n["ctc_beam"] == 4 and "ctc_beam_lm" not in n and n.get("beam_step", 0) == 0
    assert lines == direct(lambda xs, ilens: solver.model.recognize_ctc_beams(xs, ilens, 4)[0])
    lines, n = run(ctc_beam_decode=True, beam_size=4, ngram_lm=arpa, ngram_weight=0.8, ngram_bonus=0.5)
    assert n["ctc_beam_lm"] == 4 and n["ctc_beam_lm_launch"] == 8 and "ctc_beam" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_ctc_beams(xs, ilens, 4, ngram=back, ngram_weight=0.8,
                                                                              ngram_bonus=0.5)[0])
    run(ctc_beam_decode=True, beam_size=4, ngram_lm=arpa, ngram_weight=0.8, cer_on_gpu=True)
    assert solver.last_test["best_of_k_cer"] is not None and solver.last_test["best_of_k_cer"] <= solver.last_test["cer"]
    lines, n = run(two_pass_decode=True, beam_size=4, ctc_decode_weight=0.4, ngram_lm=arpa, ngram_weight=0.8, ngram_bonus=0.5)
    assert n["ctc_beam_lm"] == 4 and "ctc_beam" not in n
    assert lines == direct(lambda xs, ilens: solver.model.recognize_two_pass(
        xs, ilens, 4, ctc_weight=0.4, ngram=back, ngram_weight=0.8, ngram_bonus=0.5)[0].cpu().numpy().tolist())
    for bad in (dict(ngram_lm=arpa, beam_size=4), dict(ngram_lm=arpa, ctc_greedy_decode=True), dict(ngram_weight=0.5, beam_size=4),
                dict(ctc_beam_decode=True, two_pass_decode=True), dict(ctc_beam_decode=True, lm_weight=0.5)):
        solver.config = dict(cfg, **bad)
        with pytest.raises(ValueError):
            solver.test(state_dict=sd)
    plain, _ = tc._solver(os.path.join(root, "plain"), monkeypatch)
    plain.config = dict(plain.config, ctc_beam_decode=True)
    with pytest.raises(ValueError, match="CTC head"):
        plain.test(state_dict={k: v.clone() for k, v in plain.model.state_dict().items()})
