"""The front end on the GPU (csrc/frontend.hip) against the float64 restatement of tests/frontend_ref.py.

fbank: per element, on LINEAR mel energies, |got - ref64| <= a * (the frame's largest ref64 energy) with a = max(4 x the
float32 restatement's worst such ratio in that case, 8 * 2^-24) - test_ctc_align_gpu.py's rule; tests/test_frontend_cpu.py
caps the restatement's ratio at 5e-7 over exactly these inputs.  On LOG energies the first-order allowance
a * framemax / max(ref64, FLT_EPSILON) plus 4 ulps of the value holds every element: the log is ill-conditioned exactly
where a bin lies far below the frame's peak.  Every case prints its allowance and what it measured (profiles/
frontend_parity.txt is that output)."""
import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import frontend_ref as R

pytestmark = pytest.mark.gpu

TILE = 8                     # ASR_FBANK_FRAME_TILE: frames per workgroup of asr_fbank_f32
U = 2.0 ** -24
LOG_FLOOR = np.float32(np.log(np.float64(2.0) ** -23))       # the fp32 nearest to ln(FLT_EPSILON)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    assert torch.cuda.is_available()
    assert hip_backend.FBANK_FRAME_TILE == TILE == R.FRAME_TILE
    return hip_backend


def _plan(hb, kw):
    return hb.FbankPlan(sample_rate=kw["sample_rate"], frame_length=kw["L"], frame_shift=kw["S"], n_fft=kw["n_fft"],
                        n_mels=kw["n_mels"], low_freq=kw["low_freq"], high_freq=kw["high_freq"])


def _run(hb, utts, kw, use_log, tail=None, tail_len=700):
    """-> (out [B, T_max, n_mels] numpy, frame counts).  The packed buffer is followed, inside the same allocation, by
    `tail_len` samples holding `tail` (None: zeros)."""
    dtype = utts[0].dtype
    total = sum(len(u) for u in utts)
    buf = np.zeros(total + tail_len, dtype)
    offs = [0]
    for u in utts:
        buf[offs[-1]:offs[-1] + len(u)] = u
        offs.append(offs[-1] + len(u))
    if tail is not None:
        buf[total:] = tail
    lens = [R.num_frames(len(u), kw["L"], kw["S"]) for u in utts]
    t_max = max(max(lens), 1)
    dev = torch.from_numpy(buf).cuda()
    out = torch.full((len(utts), t_max, kw["n_mels"]), SENTINEL, device="cuda")
    hb.fbank(_plan(hb, kw), dev[:total], torch.tensor(offs, dtype=torch.int64).cuda(), t_max, out, use_log=use_log)
    return out.cpu().numpy(), lens


CASES = {name: (utts, kw) for name, utts, kw in R.fbank_cases()}
_REF = {}


def _refs(name):
    """float64 linear energies of every utterance of a case and the case's allowance, computed once."""
    if name not in _REF:
        utts, kw = CASES[name]
        ref = [R.fbank(u, np.float64, use_log=False, **kw) for u in utts]
        r32 = max(float(R.ratio(R.fbank(u, np.float32, use_log=False, **kw), r).max()) for u, r in zip(utts, ref) if len(r))
        _REF[name] = (ref, r32, max(4.0 * r32, 8.0 * U))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fbank_linear(hb, name):
    utts, kw = CASES[name]
    ref, r32, a = _refs(name)
    got, lens = _run(hb, utts, kw, use_log=False)
    worst = 0.0
    for b, r in enumerate(ref):
        assert lens[b] == len(r)
        assert (got[b, lens[b]:] == SENTINEL).all()                  # rows behind the utterance are not touched
        if lens[b]:
            worst = max(worst, float(R.ratio(got[b, :lens[b]], r).max()))
    print("PARITY fbank linear %-12s restatement32 %.3g allowance %.3g measured %.3g" % (name, r32, a, worst))
    assert worst <= a, (name, worst, a)


@pytest.mark.parametrize("name", list(CASES))
def test_fbank_log(hb, name):
    utts, kw = CASES[name]
    ref, r32, a = _refs(name)
    got, lens = _run(hb, utts, kw, use_log=True)
    worst = 0.0
    for b, r in enumerate(ref):
        if not lens[b]:
            continue
        want = np.log(np.maximum(r, R.FLT_EPSILON))
        allow = a * r.max(axis=1, keepdims=True) / np.maximum(r, R.FLT_EPSILON) + 4.0 * np.spacing(np.abs(want).astype(np.float32))
        err = np.abs(got[b, :lens[b]].astype(np.float64) - want)
        assert np.isfinite(got[b, :lens[b]]).all()
        worst = max(worst, float((err / allow).max()))
        assert (err <= allow).all(), (name, b, float((err / allow).max()))
    print("PARITY fbank log    %-12s allowance %.3g worst error / allowance %.3g" % (name, a, worst))


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_silence_is_the_log_floor(hb, dtype):
    kw = CASES["signals_i16"][1]
    got, lens = _run(hb, [np.zeros(1000, dtype), np.zeros(399, dtype), np.zeros(2000, dtype)], kw, use_log=True)
    assert lens == [4, 0, 11]
    for b, n in enumerate(lens):
        assert (got[b, :n].view(np.int32) == LOG_FLOOR.view(np.int32)).all()
        assert (got[b, n:] == SENTINEL).all()


@pytest.mark.parametrize("name", ["edges_i16", "edges_f32"])
def test_nothing_behind_the_last_offset_is_read(hb, name):
    """The samples behind offsets[B], inside the same allocation: +-32767 (NaN for float32) leave every bit as it was; and
    two calls give the same bits."""
    utts, kw = CASES[name]
    clean, _ = _run(hb, utts, kw, use_log=True)
    again, _ = _run(hb, utts, kw, use_log=True)
    assert np.array_equal(clean.view(np.int32), again.view(np.int32))
    tail = np.where(np.arange(700) % 2 == 0, 32767, -32767).astype(utts[0].dtype)
    if utts[0].dtype == np.float32:
        tail = np.full(700, np.nan, np.float32)
    dirty, _ = _run(hb, utts, kw, use_log=True, tail=tail)
    assert np.array_equal(clean.view(np.int32), dirty.view(np.int32))


def test_refused_shapes(hb):
    kw = CASES["signals_i16"][1]
    for bad in (dict(n_fft=1024), dict(L=513), dict(n_mels=129)):
        with pytest.raises(hb.UnsupportedShape):
            _plan(hb, dict(kw, **bad))
    plan = _plan(hb, kw)
    plan.n_mels = 129                                                # past the host check: the launcher itself refuses
    x = torch.zeros(1000, dtype=torch.int16, device="cuda")
    with pytest.raises(hb.UnsupportedShape):
        hb.fbank(plan, x, torch.tensor([0, 1000]).cuda(), 4, torch.zeros(1, 4, 129, device="cuda"))
    with pytest.raises(hb.UnsupportedShape):
        hb.feat_finish(torch.zeros(1, 4, 8, device="cuda"), 8, torch.tensor([4], dtype=torch.int32).cuda(),
                       torch.zeros(1, 4, 32, device="cuda"), order=3)


# ------------------------------------------------------------------------------------------------ the finish pass
FIN_LENS = [10, 9, 8, 5, 4, 3, 2, 1]          # the clamped edges of the 9-tap filter
FIN_T, FIN_D = 12, 7


def _statics(seed=5):
    """Log-mel-like statics (mean -5, deviation 2); NaN behind every utterance: those rows must never be read."""
    rs = np.random.RandomState(seed)
    x = np.full((len(FIN_LENS), FIN_T, FIN_D), np.nan, np.float32)
    for b, n in enumerate(FIN_LENS):
        x[b, :n] = rs.normal(-5.0, 2.0, (n, FIN_D))
    return x


def _finish(hb, x, order, cmvn, stats=None, masks=None, n_fm=0, n_tm=0):
    xd = torch.from_numpy(x).cuda()
    lens = torch.tensor(FIN_LENS, dtype=torch.int32).cuda()
    out = torch.full((x.shape[0], FIN_T, FIN_D * (1 + order)), SENTINEL, device="cuda")
    code = dict(none=hb.CMVN_NONE, utterance=hb.CMVN_UTTERANCE, **{"global": hb.CMVN_GLOBAL})[cmvn]
    st = None
    if cmvn == "utterance":
        st = hb.feat_cmvn_stats(xd, FIN_D, lens, torch.full((x.shape[0], 2, FIN_D), SENTINEL, device="cuda"))
    elif cmvn == "global":
        st = torch.from_numpy(np.stack(stats).astype(np.float32)).cuda()
    md = torch.from_numpy(np.asarray(masks, dtype=np.int32)).cuda() if masks is not None else None
    hb.feat_finish(xd, FIN_D, lens, out, order=order, cmvn=code, stats=st, masks=md, n_freq_masks=n_fm, n_time_masks=n_tm)
    return out.cpu().numpy(), (st.cpu().numpy() if st is not None else None)


@pytest.mark.parametrize("cmvn", ["none", "global", "utterance"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_finish_against_the_restatement(hb, order, cmvn):
    """Tolerance, from the number format: with s_b = max istd * max |x_b| (the magnitude before the mean is taken off; istd
    1 without CMVN) every output is within 64 * 2^-24 * s_b.  The mean of <= 10 values is off by <= 12 u max|x|, the
    variance about it by a relative 34 u, so istd by 20 u; y = (x - mean) istd, |y| <= 2 s_b, is then off by < 56 u s_b; a
    delta is a sum of <= 9 products with sum |taps| <= 0.6, which adds < 10 u 0.6 |y|."""
    x = _statics()
    rs = np.random.RandomState(9)
    gstats = (rs.normal(-5.0, 0.5, FIN_D).astype(np.float32), rs.uniform(0.3, 0.8, FIN_D).astype(np.float32))
    got, st = _finish(hb, x, order, cmvn, stats=gstats)
    statics = [x[b, :n].astype(np.float64) for b, n in enumerate(FIN_LENS)]
    want = R.finish(statics, FIN_T, order=order, cmvn=cmvn, stats=gstats)
    worst = 0.0
    for b, n in enumerate(FIN_LENS):
        assert (got[b, n:] == 0).all() and not np.signbit(got[b, n:]).any()          # exact zeros behind T_b
        istd = 1.0 if cmvn == "none" else (gstats[1].max() if cmvn == "global" else R.cmvn_stats(statics[b])[1].max())
        s = float(istd) * float(np.abs(statics[b]).max())
        err = np.abs(got[b, :n].astype(np.float64) - want[b, :n]).max()
        worst = max(worst, err / (64 * U * s))
        assert err <= 64 * U * s, (b, n, err, s)
        if cmvn == "none":
            assert np.array_equal(got[b, :n, :FIN_D], x[b, :n])
        if cmvn == "utterance" and n == 1:
            assert (got[b, :1] == 0).all()                                            # one frame: x - mean is exactly 0
    print("PARITY finish order %d cmvn %-9s worst error / (64 u s_b) %.3g" % (order, cmvn, worst))


def test_cmvn_stats(hb):
    """mean within (T/4 + 4) u max|x| (four ordered partial sums), 1 / std within a relative (T + 64) u."""
    rs = np.random.RandomState(4)
    lens = [98, 8, 1, 0]
    x = np.full((4, 98, 80), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rs.normal(-5.0, 2.0, (n, 80))
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    st = hb.feat_cmvn_stats(torch.from_numpy(x).cuda(), 80, ld, torch.full((4, 2, 80), SENTINEL, device="cuda")).cpu().numpy()
    st2 = hb.feat_cmvn_stats(torch.from_numpy(x).cuda(), 80, ld, torch.full((4, 2, 80), SENTINEL, device="cuda")).cpu().numpy()
    assert np.array_equal(st.view(np.int32), st2.view(np.int32))
    for b, n in enumerate(lens[:3]):
        mean, istd = R.cmvn_stats(x[b, :n].astype(np.float64))
        assert np.abs(st[b, 0] - mean).max() <= (n / 4 + 4) * U * np.abs(x[b, :n]).max()
        assert (np.abs(st[b, 1] - istd) / istd).max() <= (n + 64) * U
    assert np.isfinite(st).all()


def test_masks(hb):
    x = _statics()
    B = len(FIN_LENS)
    base, _ = _finish(hb, x, 2, "utterance")
    masks = np.zeros((B, 4, 2), np.int32)                            # 2 frequency masks, then 2 time masks
    masks[0] = [[1, 3], [6, 1], [9, 5], [0, 0]]                      # a time mask that crosses T_b = 10; one of width 0
    masks[1] = [[0, FIN_D], [0, 0], [0, 0], [0, 0]]                  # every bin
    masks[2] = [[0, 0], [0, 0], [0, FIN_T], [0, 0]]                  # every frame
    masks[3] = [[2, 2], [3, 2], [1, 2], [2, 3]]                      # overlapping
    got, _ = _finish(hb, x, 2, "utterance", masks=masks, n_fm=2, n_tm=2)
    want = R.finish([base[b, :n, :FIN_D] for b, n in enumerate(FIN_LENS)], FIN_T, masks=masks, n_freq_masks=2)
    for b, n in enumerate(FIN_LENS):
        hit = np.zeros((FIN_T, 3 * FIN_D), bool)
        for m, (s0, w) in enumerate(masks[b]):
            if m < 2:
                for k in range(3):
                    hit[:, k * FIN_D + s0:k * FIN_D + s0 + w] = True
            else:
                hit[s0:s0 + w] = True
        hit[n:] = True
        assert (got[b][hit] == 0).all()
        assert np.array_equal(got[b][~hit].view(np.int32), base[b][~hit].view(np.int32))
        assert np.array_equal(want[b, :n, :FIN_D] == 0, hit[:n, :FIN_D] | (base[b, :n, :FIN_D] == 0))
    assert (got[1, :FIN_LENS[1]] == 0).all() and (got[2] == 0).all() and (got[0, :9, 0] != 0).all()
    empty, _ = _finish(hb, x, 2, "utterance", masks=np.zeros((B, 4, 2), np.int32), n_fm=2, n_tm=2)
    assert np.array_equal(empty.view(np.int32), base.view(np.int32))


# ------------------------------------------------------------------------------------------------ Frontend and the feed
def _items(n=6, seed=3, dtype=np.int16):
    from dataset import synthetic_waveforms
    data = synthetic_waveforms(n, 9, 0.3, seed=seed, dtype=dtype)
    return [(v["feature"], v["token_ids"]) for v in data.values()]


FE_CFG = dict(n_mels=8, delta_order=0, cmvn="utterance",
              specaug=dict(n_freq_masks=1, max_freq_width=3, n_time_masks=1, max_time_width=6))


def _direct(fe, items, masks=None):
    items = sorted(items, key=lambda it: -len(it[0]))
    offs = np.concatenate([[0], np.cumsum([len(f) for f, _ in items])])
    samples = torch.from_numpy(np.concatenate([f for f, _ in items])).cuda()
    return fe(samples, offs.tolist(), masks=masks)


def test_frontend_against_the_restatement(hb):
    """fbank -> utterance CMVN -> deltas end to end on int16 waveforms.  The log energies carry the fbank allowance; behind
    the CMVN that is an absolute error of istd * (log allowance), checked on the static block where the restatement's own
    float64 statistics apply (deltas of exact statics are covered by test_finish_against_the_restatement)."""
    from frontend import Frontend
    fe = Frontend(dict(n_mels=23, delta_order=2, cmvn="utterance"))
    items = _items(4, seed=8)
    xs, ilens = _direct(fe, items)
    xs2, _ = _direct(fe, items)
    assert torch.equal(xs, xs2) and xs.shape == (4, max(ilens), 69) and fe.output_dim == 69
    got = xs.cpu().numpy()
    items = sorted(items, key=lambda it: -len(it[0]))
    assert ilens == [fe.num_frames(len(f)) for f, _ in items] == sorted(ilens, reverse=True)
    kw = dict(n_mels=23, high_freq=8000.0)
    for b, (f, _) in enumerate(items):
        lin = R.fbank(f, np.float64, use_log=False, **kw)
        r32 = float(R.ratio(R.fbank(f, np.float32, use_log=False, **kw), lin).max())
        a = max(4 * r32, 8 * U)
        logs = np.log(np.maximum(lin, R.FLT_EPSILON))
        mean, istd = R.cmvn_stats(logs)
        dlog = a * lin.max(axis=1, keepdims=True) / np.maximum(lin, R.FLT_EPSILON) + 4 * np.spacing(np.abs(logs).astype(np.float32))
        # y = (x - mean) istd: x and the mean move by at most the largest log allowance of their bin, istd by the same
        # relative to the deviation; plus the 64 u s_b of the finish pass
        tol = istd * (dlog + dlog.max(axis=0)) * (1 + np.abs(logs - mean) * istd) + 64 * U * istd.max() * np.abs(logs).max()
        err = np.abs(got[b, :ilens[b], :23] - (logs - mean) * istd)
        assert (err <= tol).all(), (b, float((err / tol).max()))
        assert (got[b, ilens[b]:] == 0).all()


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("thread", [False, True])
def test_feed_yields_the_front_ends_batch(hb, dtype, thread):
    from feed import DeviceFeed
    from frontend import Frontend
    fe = Frontend(FE_CFG)
    batches = [_items(6, seed=3, dtype=dtype), _items(5, seed=4, dtype=dtype)]
    feed = DeviceFeed(batches, "cuda", frontend=fe, thread=thread)            # not a training feed: no masks
    n = 0
    for items, (xs, ilens, ys) in zip(batches, feed):
        want, want_lens = _direct(fe, items)
        torch.cuda.synchronize()
        assert ilens == want_lens and torch.equal(xs, want)
        order = sorted(items, key=lambda it: -len(it[0]))
        assert [y.tolist() for y in ys] == [t for _, t in order]
        n += 1
    assert n == 2
    assert hb.LAUNCHES["fbank"] > 0 and hb.LAUNCHES["feat_finish"] > 0 and hb.LAUNCHES["feat_cmvn_stats"] > 0


def test_training_feed_masks_and_two_ranks_give_the_one_process_batch(hb):
    from feed import DeviceFeed
    from frontend import Frontend
    fe = Frontend(FE_CFG)
    items = _items(7, seed=6)

    def feeds(**kw):
        np.random.seed(21)                                           # the feeds take their mask seed from this stream
        return DeviceFeed([items], "cuda", frontend=fe, thread=False, train=True, **kw)
    whole = feeds()
    xs, ilens, ys = next(iter(whole))
    order = sorted(items, key=lambda it: -len(it[0]))
    masks = np.stack([fe.draw_masks(whole.mask_seed, 0, i, fe.num_frames(len(f))) for i, (f, _) in enumerate(order)])
    want, _ = _direct(fe, items, masks=masks)
    clean, _ = _direct(fe, items)
    assert torch.equal(xs, want) and not torch.equal(xs, clean) and masks[:, :, 1].max() > 0
    for rank in range(2):
        shard, il, ys_r = next(iter(feeds(rank=rank, world=2)))
        assert il == ilens[rank::2] and shard.info["t_max"] == xs.shape[1] and shard.info["b_global"] == 7
        assert torch.equal(shard.xs, xs[rank::2])
        assert [y.tolist() for y in ys_r] == [y.tolist() for y in ys[rank::2]]
    xs_s, il_s = next(iter(DeviceFeed([items], "cuda", kind="speech", frontend=fe, thread=False)))
    assert torch.equal(xs_s, clean) and il_s == ilens


def test_e2e_forward_on_front_end_output(hb):
    import synth
    import model as M
    from feed import DeviceFeed
    from frontend import Frontend
    cfg = dict(synth.TINY)
    fe = Frontend(dict(FE_CFG, specaug=None))
    assert fe.output_dim == cfg["input_dim"]
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).to("cuda")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
    net.train()
    np.random.seed(5)
    xs, ilens, ys = next(iter(DeviceFeed([_items(3, seed=2)], "cuda", frontend=fe, thread=False)))
    _, lp, _, _ = net(xs, ilens, ys)
    assert torch.isfinite(lp).all() and torch.isfinite(xs).all()
