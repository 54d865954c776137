"""CTC segmentation on the GPU (csrc/ctc_segment.hip, ops.ctc_segment, E2E.segment, Solver.segment) against the numpy
restatement tests/ctc_segment_ref.py, by the method of tests/test_ctc_align_gpu.py with float64 as the checker.

Per feasible recording of a case (tests/ctc_segment_cases.py):
  1. the device path is VALID: monotone over the extended labels, collapses to the text, first / last agree with it, -2 only
     before the first and after the last label (free ends), -1 behind T_b; the utterance spans are its labels' spans;
  2. it is OPTIMAL: its score, recomputed in float64 along the DEVICE path with the call's emissions, and the reported score
     are within the allowance of the float64 optimum;
  3. token_logp, utt_logp and utt_conf are within their allowances of float64 sums over the device's spans;
  4. the path EQUALS the float64 path whenever the recording is decisive: runner-up gap > 2 x allowance.
Allowance: max(4 x the float32 restatement's error, 8 fp32 ulps of the tensor's largest magnitude), per case and tensor.
-inf, -1 and -2 must match exactly.  Each case prints its ratios (error / allowance; profiles/ctc_segment_parity.txt keeps
them).  The exemption in (4) is capped over the restatement alone (tests/test_ctc_segment_cpu.py::test_exemption_cap)."""
import numpy as np
import pytest
import torch

import ctc_align_ref as R
import ctc_segment_cases as C
import ctc_segment_ref as SR
import poison as P
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("path", "score", "first", "last", "token_logp", "utt_begin", "utt_end", "utt_logp", "utt_conf")


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _device_inputs(hb, z, recs, V, extra=0):
    """The logits as a [B, T, V] view of a [B, T, V + 3] buffer (ld = V + 3) whose padding - the frames behind every length
    and the three extra columns - is NaN; extra: that many frames more than the longest recording has (NaN too)."""
    B, T = z.shape[0], z.shape[1] + extra
    buf = np.full((B, T, V + 3), np.nan, dtype=np.float32)
    for i, (t, _) in enumerate(recs):
        buf[i, :t, :V] = z[i, :t]
    dev = torch.from_numpy(buf).to(DEV).requires_grad_()        # (forward only: accepted, nothing recorded)
    ys = torch.tensor([v for _, us in recs for u in us for v in u], dtype=torch.long, device=DEV)
    return dev[:, :, :V], hb.to_device_i32([t for t, _ in recs], DEV), ys


def _run(hb, c, extra=0):
    import ops
    logits, lens, ys = _device_inputs(hb, c["z"], c["recs"], c["V"], extra)
    res = ops.ctc_segment(logits, lens, ys, [[len(u) for u in us] for _, us in c["recs"]], free_ends=bool(c["free_ends"]),
                          window=c["window"])
    assert not res.score.requires_grad and res.score.grad_fn is None
    return res


def _runs(p):
    out, s = [], 0
    for t in range(1, len(p) + 1):
        if t == len(p) or p[t] != p[s]:
            out.append((int(p[s]), s, t - 1))
            s = t
    return out


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS + ("offsets", "utt_offsets", "rec_utts")}


def _check(c, res, what, exact_paths=True):
    z, recs, free = c["z"], c["recs"], c["free_ends"]
    h = _host(res)
    offs = np.concatenate([[0], np.cumsum([sum(len(u) for u in us) for _, us in recs])])
    uoffs = np.concatenate([[0], np.cumsum([len(u) for _, us in recs for u in us])])
    ru = np.concatenate([[0], np.cumsum([len(us) for _, us in recs])])
    assert h["offsets"].tolist() == offs.tolist() and h["utt_offsets"].tolist() == uoffs.tolist() and h["rec_utts"].tolist() == ru.tolist()
    worst = dict(path_score=0.0, score=0.0, token_logp=0.0, utt_logp=0.0, utt_conf=0.0)
    al = c["allows"]
    exact = 0
    for i, (t, us) in enumerate(recs):
        r, sl, usl = c["r64"][i], slice(offs[i], offs[i + 1]), slice(ru[i], ru[i + 1])
        y = [k for u in us for k in u]
        path = h["path"][i]
        assert (path[t:] == -1).all(), "%s: recording %d has a path behind its %d frames" % (what, i, t)
        if not r["feasible"]:
            assert np.isneginf(h["score"][i]) and (path == -1).all() and (h["first"][sl] == -1).all() and (h["last"][sl] == -1).all()
            assert np.isneginf(h["token_logp"][sl]).all() and (h["utt_begin"][usl] == -1).all() and (h["utt_end"][usl] == -1).all()
            assert np.isneginf(h["utt_logp"][usl]).all() and np.isneginf(h["utt_conf"][usl]).all()
            continue
        p = path[:t]
        # 1. valid
        inside = np.nonzero(p != SR.OUTSIDE)[0]
        if free:
            assert (len(inside) == 0) == (len(y) == 0), (what, i)
            if len(inside):
                assert inside.tolist() == list(range(inside[0], inside[-1] + 1)) and p[inside[0]] > 0 and p[inside[-1]] > 0
        else:
            assert len(inside) == t
        tok = np.where(p == SR.OUTSIDE, 0, p)
        assert (p >= -2).all() and R.collapse(tok) == y, (what, i)
        runs = [(k, s, e) for k, s, e in _runs(p) if k > 0]
        assert [k for k, _, _ in runs] == y, "%s: recording %d is not monotone over its labels" % (what, i)
        first, last = h["first"][sl], h["last"][sl]
        assert first.tolist() == [s for _, s, _ in runs] and last.tolist() == [e for _, _, e in runs]
        # 2. optimal: the path's score with the call's emissions (outside frames cost nothing)
        x = R.log_probs(z[i, :t].astype(np.float64))
        fx = x[np.arange(t), tok]
        along = float(R.path_score(np.where((p == SR.OUTSIDE)[:, None], 0.0, x), tok))
        opt = float(r["score"])
        assert np.isfinite(h["score"][i])
        worst["path_score"] = max(worst["path_score"], abs(along - opt) / al["score"] if al["score"] else abs(along - opt))
        worst["score"] = max(worst["score"], abs(float(h["score"][i]) - opt) / al["score"] if al["score"] else abs(float(h["score"][i]) - opt))
        assert along <= opt + al["score"]
        # 3. sums over the device's spans
        if y:
            want = R.token_sums(x, y, first, last)
            worst["token_logp"] = max(worst["token_logp"], float(np.abs(h["token_logp"][sl].astype(np.float64) - want).max()) / al["token_logp"])
        want = SR.utterances(fx, first, last, [len(u) for u in us], c["window"])
        assert h["utt_begin"][usl].tolist() == want["utt_begin"].tolist() and h["utt_end"][usl].tolist() == want["utt_end"].tolist()
        for name in ("utt_logp", "utt_conf"):
            err = float(np.abs(h[name][usl].astype(np.float64) - want[name]).max()) if len(us) else 0.0
            worst[name] = max(worst[name], err / al[name] if al[name] else err)
        for u, labels in enumerate(us):
            if not labels:
                assert (h["utt_logp"][usl][u], h["utt_conf"][usl][u]) == (0.0, 0.0)
        # 4. the float64 path where the recording is decisive
        if exact_paths and c["decisive"][i]:
            exact += 1
            assert p.tolist() == r["path"].tolist(), "%s: recording %d (gap %.3g, allowance %.3g)" % (what, i, r["gap"], al["score"])
    print("ctc_segment_parity %s: path score %.3f  score %.3f  token_logp %.3f  utt_logp %.3f  utt_conf %.3f  (error / allowance; "
          "allowances %.3g, %.3g, %.3g, %.3g); %d of %d feasible recordings decisive"
          % (what, worst["path_score"], worst["score"], worst["token_logp"], worst["utt_logp"], worst["utt_conf"], al["score"],
             al["token_logp"], al["utt_logp"], al["utt_conf"], exact, len(c["feasible"])))
    assert all(v <= 1.0 for v in worst.values()), (what, worst)


def _equal(a, b, what=""):
    for name in FIELDS + ("offsets", "utt_offsets", "rec_utts"):
        x, y = getattr(a, name), getattr(b, name)
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("case", C.GRID, ids=C.case_id)
def test_segment_against_float64(hb, case):
    c = C.case(case)
    _check(c, _run(hb, c), "window=%d %s" % (c["window"], C.case_id(case)))


def test_the_longest_transcript(hb):
    """One recording at L = 8191 (S = 16 383: every one of the 1 024 threads, the last with one state fewer), V = 5,
    T' = 8 200, free ends: validity, optimality and the sums (the runner-up gap would need the whole float64 trellis twice)."""
    free = 1
    key = ("longest", free)
    if key not in C._CASES:
        rs = np.random.RandomState(8191)
        ys = [1]
        while len(ys) < hb.CTC_SEG_MAX_LABELS:               # 9 frames to spare: no adjacent repeats but four planted ones
            k = ys[-1] if len(ys) in (100, 4000, 4001, 8000) else int(rs.randint(1, 5))
            if k != ys[-1] or len(ys) in (100, 4000, 4001, 8000):
                ys.append(k)
        assert sum(a == b for a, b in zip(ys, ys[1:])) == 4
        recs = [(8200, [ys[:1], ys[1:4000], [], ys[4000:]])]
        z = rs.normal(0, 1, size=(1, 8200, 5)).astype(np.float32)
        C._CASES[key] = dict(z=z, recs=recs, V=5, free_ends=free, window=30, **C.restated(z, recs, free, 30, with_gap=False))
    c = C._CASES[key]
    assert c["feasible"] == [0]
    _check(c, _run(hb, c), "L=8191 T'=8200 V=5 free%d" % free, exact_paths=False)


@pytest.mark.parametrize("case", [c for c in C.GRID if c[3] == 0 and c[1] != "wide"], ids=C.case_id)
def test_without_free_ends_it_is_ctc_align_bit_for_bit(hb, case):
    """free_ends = 0 against ops.ctc_align on the same device inputs, every recording of at most 1 023 labels: path, score,
    first, last and token_logp with torch.equal - on every kernel path of either side (wave4's L = 200 at T' = 403 has
    ctc_align's back-pointers in its workspace)."""
    import ops
    c = C.case(case)
    keep = [i for i, (_, us) in enumerate(c["recs"]) if sum(len(u) for u in us) <= hb.CTC_MAX_LABELS]
    recs = [c["recs"][i] for i in keep]
    logits, lens, ys = _device_inputs(hb, c["z"][keep], recs, c["V"])
    seg = ops.ctc_segment(logits, lens, ys, [[len(u) for u in us] for _, us in recs], free_ends=False, window=c["window"])
    ali = ops.ctc_align(logits, lens, ys, [sum(len(u) for u in us) for _, us in recs])
    assert torch.equal(seg.path, ali.path) and torch.equal(seg.first, ali.first) and torch.equal(seg.last, ali.last)
    assert torch.equal(seg.offsets, ali.offsets)
    assert torch.equal(seg.score.view(torch.int32), ali.score.view(torch.int32))
    assert torch.equal(seg.token_logp.view(torch.int32), ali.token_logp.view(torch.int32))
    assert len(keep) >= 2 and bool(torch.isfinite(ali.score).any())


# ------------------------------------------------------------------------------------------------ planted recordings
def _planted(V, T, a, runs, bad=None, margin=40.0):
    """Logits [T, V] with the text in the frames a ..: `runs` is a list of (label, frames) (label 0: a blank run inside the
    text); the head and the tail favour token V - 1, which the text never uses; every favoured logit is `margin` nats above
    the rest.  bad: (first frame, frames) of a stretch inside the text where token V - 1 stands 1 nat above the planted
    token: x = -log(1 + e) there, and no label of the text gets any cheaper."""
    z = np.zeros((T, V), dtype=np.float32)
    z[:, V - 1] = margin
    t = a
    spans = []
    for k, n in runs:
        z[t:t + n, V - 1] = 0.0
        z[t:t + n, k] = margin
        spans.append((k, t, t + n - 1))
        t += n
    if bad:
        lo, n = bad
        z[lo:lo + n, V - 1] = margin + 1.0
    return z, spans, t - 1


def test_planted_recordings(hb):
    """utt_begin / utt_end are the planted frames, every head and tail frame is -2, the utterance with the planted bad
    stretch has the lowest confidence (the float64 value within the allowance), and without free ends the same recording
    scores lower."""
    import ops
    V, T, window = 7, 300, 10
    # three utterances: labels 1 2 | 3 3 (a blank between the repeats) 4 | 5 1 2, a bad stretch inside the second
    # (the first and the last label run one frame: a longer run of x = 0 would tie with the free end's 0 frame by frame)
    runs = [(1, 1), (2, 9), (0, 4), (3, 7), (0, 3), (3, 25), (4, 8), (0, 5), (5, 6), (1, 11), (2, 1)]
    utts = [[1, 2], [3, 3, 4], [5, 1, 2]]
    recs, zs = [], []
    for a, bad in ((37, (70, 12)), (0, None), (212, None)):
        z, spans, b = _planted(V, T, a, runs, bad)
        zs.append(z)
        recs.append((T if a else b + 1, utts))                        # the second recording: the text fills it end to end
    z = np.stack(zs)
    c = dict(z=z, recs=recs, V=V, free_ends=1, window=window, **C.restated(z, recs, 1, window))
    assert all(c["decisive"].values()) and min(r["gap"] for r in c["r64"]) > 10.0
    res = _run(hb, c)
    _check(c, res, "planted")
    h = _host(res)
    for i, a in enumerate((37, 0, 212)):
        _, spans, b = _planted(V, T, a, runs)
        lab = [(k, s, e) for k, s, e in spans if k]
        assert h["first"][8 * i:8 * i + 8].tolist() == [s for _, s, _ in lab] and h["last"][8 * i:8 * i + 8].tolist() == [e for _, _, e in lab]
        assert h["utt_begin"][3 * i:3 * i + 3].tolist() == [lab[0][1], lab[2][1], lab[5][1]]
        assert h["utt_end"][3 * i:3 * i + 3].tolist() == [lab[1][2], lab[4][2], lab[7][2]]
        t = recs[i][0]
        assert (h["path"][i, :a] == -2).all() and (h["path"][i, b + 1:t] == -2).all() and (h["path"][i, a:b + 1] >= 0).all()
    conf = h["utt_conf"]
    assert conf[1] == conf.min() and conf[1] < -1.0 and (np.delete(conf, 1) > -1e-6).all()
    assert abs(float(conf[1]) - float(c["r64"][0]["utt_conf"][1])) <= c["allows"]["utt_conf"]
    strict = dict(c, free_ends=0, **C.restated(z, recs, 0, window))
    res0 = _run(hb, strict)
    _check(strict, res0, "planted, no free ends")
    s1, s0 = res.score.cpu().numpy(), res0.score.cpu().numpy()
    assert s0[0] < s1[0] - 1.0 and s0[2] < s1[2] - 1.0 and abs(s0[1] - s1[1]) < 1e-3


def test_tie_rule_on_the_device(hb):
    """Two kinds of logits with real ties in fp32.  Flat (all 0.25): a frame gives every token the same x, so a cell's value
    depends only on how many frames it has paid for, and every path that pays for as many frames ties.  Dyadic: one token
    per frame at 0 (the blank on every third frame) and the rest at -200, so exp underflows, lse = 0 and x is 0 or -200
    exactly: every score is an exact multiple of 200, and a blank frame at x = 0 ties with a free end's 0.  The device path
    must be the restatement's on every layout: stay, then s-1, then s-2; S-1 at the end."""
    import ops
    rs = np.random.RandomState(5)
    for V, T, counts in ((4, 70, (0, 1, 5, 17, 31)), (9, 300, (32, 100, 127)), (9, 560, (128, 255, 256)), (3, 1100, (511, 512)),
                         (3, 2200, (1023, 1024))):
        for free in (0, 1):
            for flat in (False, True):
                recs = [(T - j, C.split(rs, C.labels(rs, V, n))) for j, n in enumerate(counts)]
                if flat:
                    z = np.full((len(recs), T, V), 0.25, dtype=np.float32)
                else:
                    z = np.full((len(recs), T, V), -200.0, dtype=np.float32)
                    for t in range(T):
                        z[:, t, 0 if t % 3 == 0 else t % (V - 1) + 1] = 0.0
                logits, lens, ys = _device_inputs(hb, z, recs, V)
                res = ops.ctc_segment(logits, lens, ys, [[len(u) for u in us] for _, us in recs], free_ends=bool(free), window=30)
                h = _host(res)
                o = 0
                for i, (t, us) in enumerate(recs):
                    r = SR.segment(z[i, :t], us, bool(free), 30, with_gap=False)
                    n = sum(len(u) for u in us)
                    assert r["feasible"] and h["path"][i, :t].tolist() == r["path"].tolist(), (V, T, free, flat, i)
                    assert h["first"][o:o + n].tolist() == r["first"].tolist()
                    assert flat or float(h["score"][i]) == float(r["score"])             # (dyadic: fp32 is exact)
                    o += n


# ------------------------------------------------------------------------------------------------ robustness
@pytest.mark.parametrize("det", [False, True])
def test_same_bits_in_every_run(hb, det):
    for case in ((257, "wave4", 1.0, 1), (5, "k16", 1.0, 1)):
        c = C.case(case)
        with hb.deterministic(det):
            a, b = _run(hb, c), _run(hb, c)
        _equal(a, b, case)


def test_time_axis_past_every_recording(hb):
    case = (2, "small", 1.0, 1)
    c = C.case(case)
    T = c["z"].shape[1]
    long, short = _run(hb, c, extra=5), _run(hb, c)
    assert tuple(long.path.shape) == (len(c["recs"]), T + 5)
    _check(c, long, "%s T+5" % C.case_id(case))
    assert torch.equal(long.path[:, :T], short.path) and bool((long.path[:, T:] == -1).all())
    for name in FIELDS[1:]:
        assert torch.equal(getattr(long, name), getattr(short, name)), name


@pytest.mark.parametrize("case", [(34, "small", 1.0, 1), (34, "switch", 1.0, 1), (5, "k16", 1.0, 0)], ids=C.case_id)
def test_a_recording_alone_and_inside_a_batch(hb, case):
    """The last but one recording of the case alone (its own max_label_len and time axis), and as the first row of a batch
    behind which the others follow: every field equal on its frames, labels and utterances."""
    import ops
    c = C.case(case)
    i = len(c["recs"]) - 2
    t, us = c["recs"][i]
    n, m = sum(len(u) for u in us), len(us)
    full = _run(hb, c)
    alone = dict(c, z=c["z"][i:i + 1, :t], recs=[c["recs"][i]])
    one = _run(hb, alone)
    order = [i] + [j for j in range(len(c["recs"])) if j != i]
    moved = _run(hb, dict(c, z=c["z"][order], recs=[c["recs"][j] for j in order]))
    o, u = int(full.offsets[i]), int(full.rec_utts[i])
    for other, row, oo, uu in ((full, i, o, u), (moved, 0, 0, 0)):
        assert torch.equal(one.path[0], other.path[row, :t]) and torch.equal(one.score.view(torch.int32)[0], other.score.view(torch.int32)[row])
        for name in ("first", "last", "token_logp"):
            assert torch.equal(getattr(one, name).view(torch.int32), getattr(other, name)[oo:oo + n].view(torch.int32)), name
        for name in ("utt_begin", "utt_end", "utt_logp", "utt_conf"):
            assert torch.equal(getattr(one, name).view(torch.int32), getattr(other, name)[uu:uu + m].view(torch.int32)), name
    assert bool(torch.isfinite(one.score).all())


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_parity_on_poisoned_buffers(hb, pattern):
    """Outputs and workspace filled with each pattern before the call: the same checks, the same bits."""
    for case in ((5, "small", 1.0, 1), (257, "wave4", 1.0, 0), (34, "switch", 1.0, 1)):
        c = C.case(case)
        clean = _run(hb, c)
        with P.poisoned(pattern) as stats:
            res = _run(hb, c)
        assert stats is not None
        _check(c, res, "%s poisoned %s" % (C.case_id(case), pattern))
        _equal(clean, res, (case, pattern))


def test_launches_and_refusals(hb):
    import ops
    c = C.case((5, "small", 1.0, 1))
    hb.LAUNCHES.clear()
    _run(hb, c)
    assert dict(hb.LAUNCHES) == {"ctc_segment": 1}
    hb.LAUNCHES.clear()
    lens = hb.to_device_i32([4], DEV)
    z5 = torch.zeros(1, 4, 5, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_segment(z5, lens, torch.ones(hb.CTC_SEG_MAX_LABELS + 1, dtype=torch.long, device=DEV), [[8000, 192]])
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_segment(torch.zeros(1, 4, 1, device=DEV), lens, torch.zeros(0, dtype=torch.long, device=DEV), [[]])
    with pytest.raises(ValueError, match="window"):
        ops.ctc_segment(z5, lens, torch.ones(2, dtype=torch.long, device=DEV), [[1, 1]], window=0)
    with pytest.raises(ValueError, match="sum to"):
        ops.ctc_segment(z5, lens, torch.ones(2, dtype=torch.long, device=DEV), [[1, 2]])
    assert not hb.LAUNCHES


# ------------------------------------------------------------------------------------------------ model and solver
def _recordings():
    """The tiny model of tests/test_beam_ctc_gpu.py (a seeded CTC head) and two recordings built from its three utterances:
    silence-like frames (zeros), utterance 0, utterance 1, silence; and silence, utterance 2 (its text in two pieces around an
    empty one), silence."""
    import test_beam_ctc_gpu as tbc
    net, _, xs, ilens, _ = tbc._modules((0, 0.0, 14))
    rs = np.random.RandomState(9)
    V = synth.TINY["output_dim"]
    ys = [torch.from_numpy(rs.randint(3, V, size=n)).to(DEV) for n in (3, 2, 3)]
    D = xs.shape[2]
    sil = lambda n: torch.zeros(n, D, device=xs.device, dtype=xs.dtype)   # noqa: E731
    recs = [torch.cat([sil(8), xs[0, :ilens[0]], xs[1, :ilens[1]], sil(12)]), torch.cat([sil(4), xs[2, :ilens[2]], sil(8)])]
    lens = [int(r.shape[0]) for r in recs]
    order = sorted(range(2), key=lambda i: -lens[i])
    batch = torch.zeros(2, max(lens), D, device=xs.device, dtype=xs.dtype)
    for j, i in enumerate(order):
        batch[j, :lens[i]] = recs[i]
    texts = [[ys[0], ys[1]], [ys[2][:1], ys[2][:0], ys[2][1:]]]
    return net, batch, [lens[i] for i in order], [texts[i] for i in order]


def test_model_segment(hb):
    net, xs, ilens, texts = _recordings()
    out = net.segment(xs, ilens, texts, window=4)
    res = net.last_segmentation
    assert net.segment(xs, ilens, texts, window=4) == out
    _equal(res, net.last_segmentation)
    with torch.no_grad():
        logits, _, _ = net._ctc_logits(xs, ilens, "test")
    z = logits.cpu().numpy()
    enc_lens = net.encoder.enc2.last_lens_dev.cpu().tolist()
    assert enc_lens == [-(-n // net.time_reduction) for n in ilens] == [o["frames"] for o in out]
    recs = [(enc_lens[b], [u.cpu().tolist() for u in texts[b]]) for b in range(2)]
    c = dict(z=z, recs=recs, V=z.shape[2], free_ends=1, window=4, **C.restated(z, recs, 1, 4))
    assert len(c["feasible"]) == 2
    _check(c, res, "tiny model")
    h = _host(res)
    u = 0
    for b, o in enumerate(out):
        assert set(o) == {"score", "frames", "utterances"} and len(o["utterances"]) == len(texts[b])
        assert o["score"] == float(h["score"][b])
        for utt, labels in zip(o["utterances"], recs[b][1]):
            assert set(utt) == {"tokens", "begin", "end", "logp", "confidence"} and utt["tokens"] == labels
            assert (utt["begin"], utt["end"]) == (int(h["utt_begin"][u]), int(h["utt_end"][u]))
            assert (utt["logp"], utt["confidence"]) == (float(h["utt_logp"][u]), float(h["utt_conf"][u]))
            if labels:
                assert 0 <= utt["begin"] <= utt["end"] < o["frames"] and utt["logp"] <= utt["confidence"] <= 0.0
            else:
                assert (utt["begin"], utt["end"], utt["logp"], utt["confidence"]) == (-1, -1, 0.0, 0.0)
            u += 1


def test_model_without_the_head(hb):
    import test_ctc_gpu as tc
    net, xs, ilens, ys = tc._tiny(None)
    net.eval()
    hb.LAUNCHES.clear()
    with pytest.raises(ValueError, match="CTC head"):
        net.segment(xs, ilens, [[y] for y in ys])
    assert not hb.LAUNCHES                                                   # before any launch


def test_solver_segment(hb, tmp_path, monkeypatch):
    import test_ctc_gpu as tc
    solver, dev = tc._solver(str(tmp_path), monkeypatch, ctc_weight=0.3)

    def batches():
        for xs, ilens, ys in solver._feed(solver.dev_loader, sharded=False):
            yield xs, ilens, [[y[:2], y[2:]] for y in ys]
    records = solver.segment(batches())
    assert len(records) == 4 and solver.model.training
    symbols = set(solver.vocab)
    confs = []
    for rec in records:
        assert set(rec) == {"score", "frames", "utterances"} and len(rec["utterances"]) == 2
        for utt in rec["utterances"]:
            assert set(utt) == {"tokens", "begin", "end", "logp", "confidence", "keep"} and set(utt["tokens"]) <= symbols
            assert utt["keep"] is True
            if np.isfinite(rec["score"]) and utt["tokens"]:
                assert 0 <= utt["begin"] <= utt["end"] < rec["frames"]
                confs.append(utt["confidence"])
    assert len(confs) >= 4
    thr = float(np.median(confs))
    again = solver.segment(batches(), min_confidence=thr)
    flags = [utt["keep"] for rec in again for utt in rec["utterances"]]
    assert flags == [utt["confidence"] >= thr for rec in again for utt in rec["utterances"]] and True in flags and False in flags
    assert [[u["confidence"] for u in r["utterances"]] for r in again] == [[u["confidence"] for u in r["utterances"]] for r in records]
