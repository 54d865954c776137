"""CTC forced alignment and best-path decoding on the GPU (csrc/ctc_align.hip, ops.ctc_align / ops.ctc_greedy, E2E.align /
E2E.recognize_ctc, Solver.align, Solver.test with ctc_greedy_decode) against the numpy restatement tests/ctc_align_ref.py.

Per feasible utterance of an alignment case:
  1. the device path is VALID: monotone over the extended labels, collapses to the labels, first / last agree with it, -1
     behind T_b;
  2. it is OPTIMAL: its score, recomputed in float64 along the DEVICE path, and the reported score are within the allowance
     of the float64 optimum;
  3. token_logp is within the allowance of float64 sums over the device's spans;
  4. the path EQUALS the float64 path whenever the utterance is decisive: runner-up gap > 2 x allowance.
Allowance: none is written down here.  Every case also runs the restatement in float32 on the same inputs; the kernel's worst
absolute error may be at most 4 x that float32 error, with a floor of 8 fp32 ulps of the tensor's largest magnitude (per case:
the scores of its feasible utterances are one tensor, their token sums another).  -inf and -1 must match exactly.  Each case
prints its ratios (error / allowance; profiles/ctc_align_parity.txt keeps the worst).
The exemption in (4) is capped over the restatement alone (test_exemption_cap): at most 1 in 8 of the feasible utterances of
the random cases may be non-decisive, none of those with T' <= 64.  The all-equal-logits case has no exemption at all: every
path ties exactly, in fp32 too, and the device path must be the restatement's - the tie rule on the device."""
import os

import numpy as np
import pytest
import torch

import ctc_align_ref as R
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

VOCABS = (2, 5, 34, 257)
# label counts per kernel path (tests/test_ctc_gpu.py): 2L + 1 straddles the wave at L = 31 / 32, the workgroup at 127 / 128
GROUPS = dict(wave=(31,), block=(32, 127), strided=(128, 200))
SEED = {}                              # (V, group, scale) -> seed offset, where the default draw misses the cap (none does)


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _labels(rs, V, n, equal=False):
    if equal or V == 2:
        return [int(rs.randint(1, V))] * n
    return [int(v) for v in rs.randint(1, V, size=n)]


def _utterances(V, group, seed):
    """(frames, labels): T' = 1 with L in {0, 1}; L = 0; repeated labels; an infeasible row; all-equal labels; a label
    outside [1, V); the group's label counts at T' = 2L + 3; a tight row (all labels equal: T' = L + repeats, one path)."""
    rs = np.random.RandomState(seed)
    a = int(rs.randint(1, V))
    b = a % (V - 1) + 1 if V > 2 else a
    utts = [(1, []), (1, [a]), (17, []), (3, [a, a]), (2, [a, b] if b != a else [a]),
            (5, [a, a, a, b]),                                # infeasible: 4 labels + 2 repeats (3 where b == a) need > 5
            (29, _labels(rs, V, 13, equal=True)),
            (7, [a, V]), (6, [0, a])]                         # labels outside [1, V): infeasible
    for L in GROUPS[group]:
        utts.append((2 * L + 3, _labels(rs, V, L)))
    L0 = GROUPS[group][0]
    utts.append((2 * L0 - 1, _labels(rs, V, L0, equal=True)))
    return utts


def _allow(f32, ref):
    f32, ref = np.asarray(f32, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err32 = float(np.abs(f32 - ref).max()) if ref.size else 0.0
    floor = 8.0 * float(np.spacing(np.float32(np.abs(ref).max()))) if ref.size else 0.0
    return max(4.0 * err32, floor)


def _restated(z, utts):
    """The CPU side of a case: per utterance the float64 and the float32 restatement, the two allowances, the census."""
    r64 = [R.align(z[i, :t].astype(np.float64), y) for i, (t, y) in enumerate(utts)]
    r32 = [R.align(z[i, :t], y, with_gap=False) for i, (t, y) in enumerate(utts)]
    feas = [i for i, r in enumerate(r64) if r["feasible"]]
    assert [i for i, r in enumerate(r32) if r["feasible"]] == feas
    allow_s = _allow([r32[i]["score"] for i in feas], [r64[i]["score"] for i in feas])
    cat = lambda rs: np.concatenate([np.asarray(rs[i]["token_logp"], dtype=np.float64) for i in feas] + [np.zeros(0)])   # noqa: E731
    allow_t = _allow(cat(r32), cat(r64))
    decisive = {i: r64[i]["gap"] > 2.0 * allow_s for i in feas}
    return dict(r64=r64, r32=r32, feasible=feas, allow_s=allow_s, allow_t=allow_t, decisive=decisive)


_CASES = {}


def _case(V, group, scale):
    key = (V, group, scale)
    if key in _CASES:
        return _CASES[key]
    utts = _utterances(V, group, 100 + V)
    rs = np.random.RandomState(7 * V + len(group) + SEED.get(key, 0))
    B, T = len(utts), max(t for t, _ in utts)
    z = (scale * rs.normal(0, 1, size=(B, T, V))).astype(np.float32)
    out = dict(z=z, utts=utts, V=V, **_restated(z, utts))
    assert len(out["feasible"]) == B - 3
    _CASES[key] = out
    return out


def _overflow_case(hb):
    """One utterance of the smallest T' at L = 200 whose back-pointers exceed the LDS budget: T' ceil(401 / 64) 16 bytes."""
    key = "overflow"
    if key not in _CASES:
        L, V = 200, 5
        W = (2 * L + 1 + 63) // 64
        T = hb.CTC_ALIGN_LDS_BYTES // (16 * W) + 1
        rs = np.random.RandomState(4242)
        utts = [(T, _labels(rs, V, L))]
        z = rs.normal(0, 1, size=(1, T, V)).astype(np.float32)
        _CASES[key] = dict(z=z, utts=utts, V=V, **_restated(z, utts))
    return _CASES[key]


ALIGN_GRID = [(V, g, 1.0) for V in VOCABS for g in sorted(GROUPS)] + [(34, g, 50.0) for g in sorted(GROUPS)]


def _run(hb, c, extra=0):
    """ops.ctc_align on the case: the logits are a [B, T, V] view of a [B, T, V + 3] buffer (ld = V + 3) whose padding - the
    frames behind every length and the three extra columns - is NaN.  extra: that many frames more than the longest
    utterance has (NaN too)."""
    import ops
    z, utts, V = c["z"], c["utts"], c["V"]
    B, T = z.shape[0], z.shape[1] + extra
    buf = np.full((B, T, V + 3), np.nan, dtype=np.float32)
    for i, (t, _) in enumerate(utts):
        buf[i, :t, :V] = z[i, :t]
    dev = torch.from_numpy(buf).to(DEV).requires_grad_()        # (forward only: accepted, nothing recorded)
    ys = torch.tensor([v for _, y in utts for v in y], dtype=torch.long, device=DEV)
    res = ops.ctc_align(dev[:, :, :V], hb.to_device_i32([t for t, _ in utts], DEV), ys, [len(y) for _, y in utts])
    assert not res.score.requires_grad and res.score.grad_fn is None
    return res


_WORST = {}


def _check(c, res, what):
    z, utts = c["z"], c["utts"]
    path, score = res.path.cpu().numpy(), res.score.cpu().numpy()
    first, last, tlp = res.first.cpu().numpy(), res.last.cpu().numpy(), res.token_logp.cpu().numpy()
    offs = np.concatenate([[0], np.cumsum([len(y) for _, y in utts])])
    assert res.offsets.cpu().tolist() == offs.tolist()
    worst = dict(path_score=0.0, score=0.0, token_logp=0.0)
    exact = 0
    for i, (t, y) in enumerate(utts):
        r, sl = c["r64"][i], slice(offs[i], offs[i + 1])
        assert (path[i, t:] == -1).all(), "%s: utterance %d has a path behind its %d frames" % (what, i, t)
        if not r["feasible"]:
            assert np.isneginf(score[i]) and (path[i] == -1).all() and (first[sl] == -1).all() and (last[sl] == -1).all()
            assert np.isneginf(tlp[sl]).all()
            continue
        p = path[i, :t]
        # 1. valid
        assert R.collapse(p) == y and ((p == 0) | np.isin(p, y)).all(), (what, i)
        L = len(y)
        runs = [(k, s, e) for k, s, e in _runs(p) if k != 0]
        assert [k for k, _, _ in runs] == y, "%s: utterance %d is not monotone over its labels" % (what, i)
        assert first[sl].tolist() == [s for _, s, _ in runs] and last[sl].tolist() == [e for _, _, e in runs]
        # 2. optimal
        x = R.log_probs(z[i, :t].astype(np.float64))
        opt = float(r["score"])
        along = float(R.path_score(x, p))
        assert np.isfinite(score[i])
        worst["path_score"] = max(worst["path_score"], abs(along - opt) / c["allow_s"])
        worst["score"] = max(worst["score"], abs(float(score[i]) - opt) / c["allow_s"])
        assert along <= opt + c["allow_s"]
        # 3. token sums over the device's spans
        if L:
            want = R.token_sums(x, y, first[sl], last[sl])
            worst["token_logp"] = max(worst["token_logp"], float(np.abs(tlp[sl].astype(np.float64) - want).max()) / c["allow_t"])
        # 4. the float64 path where the utterance is decisive
        if c["decisive"][i]:
            exact += 1
            assert p.tolist() == r["path"].tolist(), "%s: utterance %d (gap %.3g, allowance %.3g)" % (what, i, r["gap"], c["allow_s"])
    print("ctc_align_parity %s: path score %.3f  score %.3f  token_logp %.3f  (error / allowance; allowances %.3g, %.3g); "
          "%d of %d feasible utterances decisive, smallest gap %.3g"
          % (what, worst["path_score"], worst["score"], worst["token_logp"], c["allow_s"], c["allow_t"], exact, len(c["feasible"]),
             min(c["r64"][i]["gap"] for i in c["feasible"])))
    _WORST[what] = worst
    assert worst["path_score"] <= 1.0 and worst["score"] <= 1.0 and worst["token_logp"] <= 1.0, (what, worst)


def _runs(p):
    out, s = [], 0
    for t in range(1, len(p) + 1):
        if t == len(p) or p[t] != p[s]:
            out.append((int(p[s]), s, t - 1))
            s = t
    return out


@pytest.mark.parametrize("case", ALIGN_GRID, ids=lambda c: "V%d-%s-x%g" % c)
def test_align_against_float64(hb, case):
    c = _case(*case)
    _check(c, _run(hb, c), "V=%d %s x%g" % case)


def test_align_time_axis_past_every_utterance(hb):
    """The smallest ragged case on a time axis five frames longer than its longest utterance (a rank of a data-parallel
    step): the checks above, -1 on the extra frames, and paths, first / last frames, scores and token sums exactly those of
    the run at T = max(t)."""
    case = (VOCABS[0], sorted(GROUPS)[-1], 1.0)
    assert case == (2, "wave", 1.0)
    c = _case(*case)
    T = c["z"].shape[1]
    long, short = _run(hb, c, extra=5), _run(hb, c)
    assert tuple(long.path.shape) == (len(c["utts"]), T + 5)
    _check(c, long, "V=%d %s x%g T+5" % case)
    assert torch.equal(long.path[:, :T], short.path) and bool((long.path[:, T:] == -1).all())
    for name in ("score", "first", "last", "token_logp", "offsets"):
        assert torch.equal(getattr(long, name), getattr(short, name)), name


def test_exemption_cap():
    """Over the restatement alone: at most 1 in 8 of the feasible utterances of the random cases non-decisive, none of those
    with T' <= 64."""
    total = loose = 0
    for case in ALIGN_GRID:
        c = _case(*case)
        for i in c["feasible"]:
            total += 1
            if not c["decisive"][i]:
                loose += 1
                assert c["utts"][i][0] > 64, (case, i, c["r64"][i]["gap"], c["allow_s"])
    print("ctc_align_parity census: %d feasible utterances, %d non-decisive" % (total, loose))
    assert total >= 8 * len(ALIGN_GRID) and 8 * loose <= total


def test_back_pointers_in_the_workspace(hb):
    c = _overflow_case(hb)
    T, L = c["utts"][0][0], len(c["utts"][0][1])
    assert hb.ctc_align_ws_bytes(1, T, c["V"], L) > 8 * ((T + 63) // 64 * 64) == hb.ctc_align_ws_bytes(1, T - 1, c["V"], L)
    assert c["decisive"][0]
    _check(c, _run(hb, c), "V=5 L=200 T'=%d workspace" % T)


def test_tie_rule_on_the_device(hb):
    """All-equal logits: every path ties exactly, in fp32 too.  The device path must be the restatement's on every kernel
    path (and with the back-pointers in the workspace): stay, then s-1, then s-2; S-1 at the end."""
    import ops
    rs = np.random.RandomState(5)
    for V, T, counts in ((4, 70, (0, 1, 5, 17, 31)), (9, 300, (32, 100, 127)), (9, 420, (128, 200)),
                         (3, hb.CTC_ALIGN_LDS_BYTES // (16 * 7) + 40, (200,))):
        utts = [(T - j, _labels(rs, V, n)) for j, n in enumerate(counts)]
        z = np.full((len(utts), T, V), 0.25, dtype=np.float32)
        ys = torch.tensor([v for _, y in utts for v in y], dtype=torch.long, device=DEV)
        res = ops.ctc_align(torch.from_numpy(z).to(DEV), hb.to_device_i32([t for t, _ in utts], DEV), ys, [len(y) for _, y in utts])
        path, first = res.path.cpu().numpy(), res.first.cpu().numpy()
        o = 0
        for i, (t, y) in enumerate(utts):
            r = R.align(z[i, :t], y, with_gap=False)
            assert r["feasible"] and path[i, :t].tolist() == r["path"].tolist(), (V, T, i)
            assert first[o:o + len(y)].tolist() == r["first"].tolist()
            o += len(y)


@pytest.mark.parametrize("det", [False, True])
def test_same_bits_in_every_run(hb, det):
    c = _case(257, "strided", 1.0)
    with hb.deterministic(det):
        a, b = _run(hb, c), _run(hb, c)
    for name in ("path", "first", "last"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.score.view(torch.int32), b.score.view(torch.int32))
    assert torch.equal(a.token_logp.view(torch.int32), b.token_logp.view(torch.int32))


def test_launches_and_refused_shapes(hb):
    import ops
    c = _case(5, "wave", 1.0)
    hb.LAUNCHES.clear()
    _run(hb, c)
    assert dict(hb.LAUNCHES) == {"ctc_align": 1}
    z = torch.zeros(1, 4, 1, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_align(z, hb.to_device_i32([4], DEV), torch.zeros(0, dtype=torch.long, device=DEV), [0])
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_greedy(z, hb.to_device_i32([4], DEV))
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_align(torch.zeros(1, 4, 5, device=DEV), hb.to_device_i32([4], DEV),
                      torch.ones(hb.CTC_MAX_LABELS + 1, dtype=torch.long, device=DEV), [hb.CTC_MAX_LABELS + 1])


# ------------------------------------------------------------------------------------------------ best path
@pytest.mark.parametrize("T", [1, 2, 64, 65, 100])
@pytest.mark.parametrize("V", VOCABS)
def test_best_path_is_exact(hb, V, T):
    """Ragged lengths, NaN behind T_b and in the pad columns (ld = V + 3), tied maxima (the lowest index wins; a tie with the
    blank is a blank), an all-blank utterance, a run of equal tokens split by a blank, a NaN among the logits."""
    import ops
    rs = np.random.RandomState(31 * V + T)
    lens = [T, max(1, (2 * T) // 3), 1, max(1, T - 1), T, T]
    B = len(lens)
    z = rs.normal(0, 1, size=(B, T, V)).astype(np.float32)
    a = int(rs.randint(1, V))
    for t in range(0, T, 3):                                   # tied maxima
        k1, k2 = sorted(int(k) for k in rs.randint(0, V, size=2))
        z[0, t, k1] = z[0, t, k2] = 9.0
    z[1, ::2, V - 1] = np.nan                                  # NaN never wins
    z[4, :, 0] += 100.0                                        # all blank
    z[5, :, :] = 0.0                                           # a a blank a a ...: a run split by a blank
    for t in range(T):
        z[5, t, 0 if t % 3 == 2 else a] = 5.0
    buf = np.full((B, T, V + 3), np.nan, dtype=np.float32)
    for i, n in enumerate(lens):
        buf[i, :n, :V] = z[i, :n]
    hb.LAUNCHES.clear()
    ids, n, frame_tok = ops.ctc_greedy(torch.from_numpy(buf).to(DEV)[:, :, :V], hb.to_device_i32(lens, DEV))
    assert dict(hb.LAUNCHES) == {"ctc_greedy": 1}
    ids, n, frame_tok = ids.cpu().numpy(), n.cpu().numpy(), frame_tok.cpu().numpy()
    for i, t in enumerate(lens):
        ft, want = R.best_path(z[i, :t])
        assert frame_tok[i, :t].tolist() == ft.tolist() and (frame_tok[i, t:] == -1).all(), (V, T, i)
        assert int(n[i]) == len(want) and ids[i, :len(want)].tolist() == want and (ids[i, len(want):] == -1).all(), (V, T, i)
    assert int(n[4]) == 0
    if T >= 5:
        assert ids[5, :int(n[5])].tolist() == [a] * ((T + 2) // 3)


# ------------------------------------------------------------------------------------------------ model and solver
CAND = (0, 0.0, 14)                    # tests/test_beam_ctc_gpu.py: the tiny model with a seeded CTC head, B = 3 ragged


def _tiny_model():
    import test_beam_ctc_gpu as tbc
    net, _, xs, ilens, _ = tbc._modules(CAND)
    rs = np.random.RandomState(9)
    V = synth.TINY["output_dim"]
    ys = [torch.from_numpy(rs.randint(3, V, size=n)).to(DEV) for n in (5, 4, 3)]
    return net, xs, ilens, ys


def test_model_align_and_recognize_ctc(hb):
    net, xs, ilens, ys = _tiny_model()
    out = net.align(xs, ilens, ys)
    res = net.last_alignment
    again = net.align(xs, ilens, ys)
    res2 = net.last_alignment
    assert again == out                                                     # two calls: the same bits
    for name in ("path", "first", "last"):
        assert torch.equal(getattr(res, name), getattr(res2, name))
    assert torch.equal(res.score.view(torch.int32), res2.score.view(torch.int32))
    assert torch.equal(res.token_logp.view(torch.int32), res2.token_logp.view(torch.int32))
    # the time reduction: read from the layers, against ilens and the encoder's own output lengths
    r = net.time_reduction
    assert isinstance(r, int) and r == 4
    enc_lens = net.encoder.enc2.last_lens_dev.cpu().tolist()
    assert enc_lens == [-(-n // r) for n in ilens] == [o["frames"] for o in out]
    # the restatement on the logits the model itself produced
    with torch.no_grad():
        logits, _, _ = net._ctc_logits(xs, ilens, "test")
    z = logits.cpu().numpy()
    utts = [(enc_lens[b], ys[b].cpu().tolist()) for b in range(len(ilens))]
    c = dict(z=z, utts=utts, V=z.shape[2], **_restated(z, utts))
    assert len(c["feasible"]) == len(utts) and all(c["decisive"].values()), [c["r64"][i]["gap"] for i in c["feasible"]]
    _check(c, res, "tiny model")
    for b, o in enumerate(out):
        r64 = c["r64"][b]
        assert o["tokens"] == utts[b][1] and o["first"] == r64["first"].tolist() and o["last"] == r64["last"].tolist()
        span = r64["last"] - r64["first"] + 1
        np.testing.assert_allclose(o["confidence"], np.exp(r64["token_logp"] / span), rtol=1e-4)
        assert all(0.0 < v <= 1.0 for v in o["confidence"])
        np.testing.assert_allclose(o["score"], float(r64["score"]), rtol=1e-5)
    hb.LAUNCHES.clear()
    hyps = net.recognize_ctc(xs, ilens)
    assert hb.LAUNCHES["ctc_greedy"] == 1 and hb.LAUNCHES["ctc_align"] == 0
    assert hyps == [R.best_path(z[b, :enc_lens[b]])[1] for b in range(len(ilens))]
    assert hyps == net.recognize_ctc(xs, ilens) and any(hyps)
    ft = net.last_frame_tokens.cpu().numpy()
    assert all(ft[b, :enc_lens[b]].tolist() == R.best_path(z[b, :enc_lens[b]])[0].tolist() for b in range(len(ilens)))
    # a transcript that does not fit its frames
    long = [torch.full((enc_lens[2] + 1,), 4, dtype=torch.long, device=DEV)]
    bad = net.align(xs, ilens, ys[:2] + long)[2]
    assert bad["score"] == -np.inf and set(bad["first"]) == {-1} and set(bad["confidence"]) == {0.0}


def test_model_without_the_head(hb):
    import test_ctc_gpu as tc
    net, xs, ilens, ys = tc._tiny(None)
    net.eval()
    hb.LAUNCHES.clear()
    with pytest.raises(ValueError, match="CTC head"):
        net.align(xs, ilens, ys)
    with pytest.raises(ValueError, match="CTC head"):
        net.recognize_ctc(xs, ilens)
    assert not hb.LAUNCHES                                                   # before any launch
    assert net.time_reduction == 4


def test_solver_align_and_ctc_greedy_decode(hb, tmp_path, monkeypatch):
    import test_ctc_gpu as tc
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    records = solver.align()
    assert len(records) == 4 and solver.model.training                       # one record per dev utterance
    symbols = set(solver.vocab)
    for rec in records:
        assert set(rec) == {"tokens", "first", "last", "confidence", "score", "frames"}
        assert set(rec["tokens"]) <= symbols and len(rec["tokens"]) == len(rec["first"]) == len(rec["last"]) == len(rec["confidence"])
        if np.isfinite(rec["score"]):
            assert all(0 <= f <= l < rec["frames"] for f, l in zip(rec["first"], rec["last"]))
            assert rec["first"] == sorted(rec["first"]) and all(0.0 < v <= 1.0 for v in rec["confidence"])

    def run(**extra):
        solver.config = dict(cfg, **extra)
        hb.LAUNCHES.clear()
        cer = solver.test(state_dict=sd)
        with open(os.path.join(root, "dev.txt")) as f:
            return cer, f.read().splitlines(), dict(hb.LAUNCHES)

    cer0, lines0, launches0 = run()
    assert not any(k.startswith("ctc_") for k in launches0)                  # the key absent: the launches without the feature
    cer1, lines1, launches1 = run(ctc_greedy_decode=False)
    assert (cer1, lines1, launches1) == (cer0, lines0, launches0)
    cer, lines, launches = run(ctc_greedy_decode=True)
    assert isinstance(cer, float) and np.isfinite(cer) and cer >= 0 and len(lines) == 4
    assert launches["ctc_greedy"] == 4 and not any(k.startswith("dec_") or k.startswith("beam") for k in launches)
    for extra in (dict(beam_size=2), dict(lm_weight=0.5), dict(ctc_decode_weight=0.3)):
        solver.config = dict(cfg, ctc_greedy_decode=True, **extra)
        with pytest.raises(ValueError, match="ctc_greedy_decode"):
            solver.test(state_dict=sd)
    assert solver.judge.training
    solver.config = cfg
    solver.model.train()
