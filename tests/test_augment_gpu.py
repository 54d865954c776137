"""Reverberation and additive noise on the GPU (csrc/augment.hip) against the float64 restatements of
tests/augment_ref.py, whose docstring derives the three allowances; tests/test_augment_cpu.py holds the float32 restatements
to the same allowances over the same inputs.  Every parity case prints its worst error / allowance as an `augment-parity`
line (profiles/augment_parity.txt is that output)."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import augment_ref as A

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 700
I32 = np.int32


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    assert torch.cuda.is_available()
    return hip_backend


_CASES, _PLANS, _REF = {}, {}, {}


def _case(hb, name):
    """-> (utterances, RIR index per row, the plan of the case's RIRs with no head cut: d is where the table put it)"""
    if not _CASES:
        for n, utts, rirs, ridx in A.reverb_cases(hb.REVERB_TILE, hb.REVERB_CHUNK, hb.REVERB_MAX_TAPS):
            _CASES[n] = (utts, ridx)
            _PLANS[n] = hb.ReverbPlan(rirs, max_taps=hb.REVERB_MAX_TAPS, pre=hb.REVERB_MAX_TAPS)
    return _CASES[name] + (_PLANS[name],)


def _refs(hb, name):
    """float64 outputs and magnitudes of every row of a case, computed once (float32 inputs hold the same values)."""
    if name not in _REF:
        utts, ridx, plan = _case(hb, name)
        _REF[name] = [A.reverb(x, *plan.rir(r)) + (len(plan.rir(r)[0]),) if r >= 0 else None for x, r in zip(utts, ridx)]
    return _REF[name]


def _pack(utts, tail=None):
    total = sum(len(u) for u in utts)
    buf = np.zeros(total + (TAIL if tail is not None else 0), utts[0].dtype)
    offs = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    for u, o in zip(utts, offs):
        buf[o:o + len(u)] = u
    if tail is not None:
        buf[total:] = tail
    return buf, offs


def _reverb(hb, plan, utts, ridx, tail=None, device_index=True):
    """One launch -> (rows, the whole output buffer): TAIL canaries behind the output, TAIL elements of `tail` behind the
    input inside the tensor handed over."""
    buf, offs = _pack(utts, tail)
    out = torch.full((int(offs[-1]) + TAIL,), CANARY, device="cuda")
    idx = torch.tensor(ridx, dtype=torch.int32).cuda() if device_index else list(ridx)
    hb.reverb(plan, torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda(), idx, out, max_len=max(len(u) for u in utts))
    whole = out.cpu().numpy()
    return [whole[a:b] for a, b in zip(offs[:-1], offs[1:])], whole


CASE_NAMES = ["lengths", "max_taps", "tile_edges", "shorter_than_rir", "batch_of_one", "mixed_rows", "full_scale"]


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_convolution_parity_per_element(hb, name, dtype):
    utts, ridx, plan = _case(hb, name)
    rows, whole = _reverb(hb, plan, [u.astype(dtype) for u in utts], ridx)
    worst = 0.0
    for b, (got, ref) in enumerate(zip(rows, _refs(hb, name))):
        if ref is None:
            assert np.array_equal(got.view(I32), utts[b].astype(np.float32).view(I32)), b
            continue
        r64, mag, taps = ref
        assert got.shape == r64.shape
        err, tol = np.abs(got.astype(np.float64) - r64), A.reverb_allowance(mag, taps)
        assert (err[tol == 0] == 0).all()
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("augment-parity reverb %-17s %-7s rows %2d  worst error / allowance %.3f" % (name, np.dtype(dtype).name, len(rows), worst))
    assert worst <= 1.0, (name, worst)
    assert (whole[-TAIL:] == CANARY).all()


def test_case_table_covers_the_kernel_paths(hb):
    T = hb.REVERB_TILE
    assert [len(u) for u in _case(hb, "tile_edges")[0][:3]] == [T - 1, T, 2 * T + 1]
    plan = _case(hb, "lengths")[2]
    taps = sorted({int(g[1]) for g in plan.geometry})
    assert taps == [1, 2, 31, 32, 33, 63, 65, 1000, hb.REVERB_CHUNK, hb.REVERB_CHUNK + 1, hb.REVERB_CHUNK + 63]
    assert {(int(g[1]), int(g[2])) for g in plan.geometry} >= {(1000, 0), (1000, 500), (1000, 999), (33, 32), (2, 1)}
    assert int(_case(hb, "max_taps")[2].geometry[0, 1]) == hb.REVERB_MAX_TAPS and len(_case(hb, "max_taps")[0][0]) == 3000


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_unit_impulse_returns_the_input(hb, dtype):
    rs = np.random.RandomState(4)
    x = [(rs.randn(n) * 2500).astype(dtype) for n in (5000, 1025, 3)]
    rirs = []
    for taps, d in ((65, 0), (65, 64), (2500, 700)):
        h = np.zeros(taps)
        h[d] = 1.0
        rirs.append(h)
    plan = hb.ReverbPlan(rirs, max_taps=hb.REVERB_MAX_TAPS, pre=hb.REVERB_MAX_TAPS)      # unit energy already: the scale is 1
    assert [int(g[2]) for g in plan.geometry] == [0, 64, 700] and set(plan.bank.tolist()) == {0.0, 1.0}
    for r in range(3):
        rows, _ = _reverb(hb, plan, x, [r, r, r])
        for got, want in zip(rows, x):
            assert np.array_equal(got.view(I32), want.astype(np.float32).view(I32)), r


def test_integer_values_are_exact(hb):
    """|x| <= 128, |h| <= 8, 65 taps: every partial sum is an integer below 2^24, so any order gives the float64 result."""
    rs = np.random.RandomState(6)
    x = [rs.randint(-128, 129, n).astype(np.float32) for n in (4097, 1500)]
    h = rs.randint(-8, 9, 65).astype(np.float64)
    h[30] = 9.0                                              # the direct path
    plan = hb.ReverbPlan([h], max_taps=4096, normalize=False, pre=64)
    assert np.array_equal(plan.rir(0)[0], h.astype(np.float32)) and plan.rir(0)[1] == 30
    rows, _ = _reverb(hb, plan, x, [0, 0])
    for got, xi in zip(rows, x):
        want, _ = A.reverb(xi, h, 30)
        assert np.array_equal(got.astype(np.float64), want) and np.abs(want).max() > 1000


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_rows_without_an_rir_are_copied_by_value(hb, dtype):
    rs = np.random.RandomState(3)
    if dtype == np.int16:
        a = rs.randint(-32768, 32768, 4500).astype(np.int16)
        a[:2] = (-32768, 32767)
    else:
        a = (rs.randn(4500) * 1000).astype(np.float32)
        a[:3] = (-0.0, 1e-40, 3.4e38)                        # a signed zero, a subnormal, a value near the largest
    b = a[:1100][::-1].copy()
    other = (rs.randn(1500) * 3000).astype(dtype)
    plan = _case(hb, "batch_of_one")[2]
    rows, _ = _reverb(hb, plan, [other, a, b], [0, -1, -1])
    assert np.array_equal(rows[1].view(I32), a.astype(np.float32).view(I32))
    assert np.array_equal(rows[2].view(I32), b.astype(np.float32).view(I32))
    assert np.abs(rows[0]).max() > 0 and not np.array_equal(rows[0], other.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the mix
def _mix(hb, bank, utts, cidx, start, snr, tail=None, in_place=False, device_args=True):
    """One call -> (rows, gains, the whole output buffer).  Not in place: TAIL canaries behind the output."""
    buf, offs = _pack(utts, tail)
    n = int(offs[-1])
    x = torch.from_numpy(buf).cuda()
    out = None if in_place else torch.full((n + TAIL,), CANARY, device="cuda")
    gains = torch.full((len(utts),), CANARY, device="cuda")
    scale = np.asarray([A.snr_scale(s) for s in snr], dtype=np.float32)
    if device_args:
        args = (torch.tensor(cidx, dtype=torch.int32).cuda(), torch.tensor(start, dtype=torch.int64).cuda(),
                torch.from_numpy(scale).cuda())
    else:
        args = (list(cidx), list(start), scale)
    res = hb.noise_mix(bank, x, torch.from_numpy(offs).cuda(), *args, out=out, max_len=max(len(u) for u in utts), gains=gains)
    whole = res.cpu().numpy()
    return [whole[a:b] for a, b in zip(offs[:-1], offs[1:])], gains.cpu().numpy(), whole


@pytest.mark.parametrize("dtype,in_place", [(np.int16, False), (np.float32, False), (np.float32, True)])
def test_mix_parity(hb, dtype, in_place):
    (name, utts, clips, cidx, start, snr), = A.mix_cases(hb.NOISE_TILE)
    bank = hb.NoiseBank(clips)
    assert len(utts[0]) > 2 * len(clips[0]) and len(utts[1]) < len(clips[1]) and start[2] == len(clips[2]) - 1 and len(clips[3]) == 1
    rows, gains, whole = _mix(hb, bank, [u.astype(dtype) for u in utts], cidx, start, snr, in_place=in_place)
    worst_g = worst_z = worst_db = 0.0
    for b, (got, y) in enumerate(zip(rows, utts)):
        if cidx[b] < 0:
            assert gains[b] == 0 and np.array_equal(got.view(I32), y.astype(np.float32).view(I32))
            continue
        z64, g64, mag = A.mix(y, clips[cidx[b]], start[b], snr[b])
        worst_g = max(worst_g, abs(float(gains[b]) - g64) / (A.GAIN_ALLOWANCE * g64))
        worst_z = max(worst_z, float((np.abs(got.astype(np.float64) - z64) / A.mix_allowance(mag)).max()))
        worst_db = max(worst_db, abs(A.achieved_snr_db(y, got) - snr[b]))
    print("augment-parity mix    %-17s %-7s rows %2d  worst gain error / allowance %.3f, sample error / allowance %.3f, "
          "SNR off by %.2e dB" % ("in_place" if in_place else name, np.dtype(dtype).name, len(rows), worst_g, worst_z, worst_db))
    assert worst_g <= 1.0 and worst_z <= 1.0 and worst_db <= 1e-3
    if not in_place:
        assert (whole[-TAIL:] == CANARY).all()


@pytest.mark.parametrize("in_place", [False, True])
def test_silence_gives_no_gain_and_leaves_the_row(hb, in_place):
    rs = np.random.RandomState(8)
    loud = (rs.randn(5000) * 900).astype(np.float32)
    loud[:2] = (-0.0, 1e-40)
    quiet = np.zeros(4200, np.float32)
    bank = hb.NoiseBank([np.zeros(300, np.float32), (rs.randn(300) * 100).astype(np.float32)])
    rows, gains, _ = _mix(hb, bank, [loud, quiet, loud[:900].copy()], [0, 1, 1], [5, 7, 299], [10.0, 10.0, 10.0], in_place=in_place)
    assert gains[0] == 0 and gains[1] == 0 and gains[2] > 0
    assert np.array_equal(rows[0].view(I32), loud.view(I32)) and np.array_equal(rows[1].view(I32), quiet.view(I32))
    assert not np.array_equal(rows[2], loud[:900])


# ------------------------------------------------------------------------------------------------ bounds, bits, refusals
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_bounds(hb, dtype):
    """Nothing behind offsets[B] is read or written, nothing behind an RIR or a clip is read, and a neighbour in the packed
    buffer is not an utterance's padding: a silent row between two full-scale ones comes out silent."""
    loud_tail = 32767 if dtype == np.int16 else np.nan
    rs = np.random.RandomState(12)
    full = np.full(1300, 32767, np.int16)
    utts = [u.astype(dtype) for u in (full, np.zeros(2100, np.int16), -full, A._speech(rs, 4100))]
    rirs = [A.rir_with(rs, 300, 40), A.rir_with(rs, 1000, 999), A.rir_with(rs, 1000, 0)]
    plan = hb.ReverbPlan(rirs, max_taps=4096, pre=4096)
    other = hb.ReverbPlan(rirs[:2] + [A.rir_with(rs, 700, 3) * 50.0], max_taps=4096, pre=4096, normalize=False)
    other.bank[:plan.geometry[2, 0]] = plan.bank[:plan.geometry[2, 0]]        # the same two RIRs, another tail behind them
    ridx = [1, 0, 1, 0]
    plain, _ = _reverb(hb, plan, utts, ridx)
    rows, whole = _reverb(hb, plan, utts, ridx, tail=loud_tail)
    moved, _ = _reverb(hb, other, utts, ridx, tail=loud_tail)
    for a, b, c in zip(plain, rows, moved):
        assert np.array_equal(a.view(I32), b.view(I32)) and np.array_equal(a.view(I32), c.view(I32))
    assert not plain[1].any() and plain[0].any() and (whole[-TAIL:] == CANARY).all()
    # the mix: a NaN clip behind the last one used, another bank with another tail
    clips = [(rs.randn(500) * 300).astype(np.float32), (rs.randn(1700) * 300).astype(np.float32)]
    bank = hb.NoiseBank(clips + [np.full(64, np.nan, np.float32)])
    bank2 = hb.NoiseBank(clips + [np.full(900, 1e30, np.float32)])
    args = ([1, 0, -1, 1], [1699, 499, 0, 3], [5.0, 10.0, 0.0, 20.0])
    plain, g0, _ = _mix(hb, bank, utts, *args)
    rows, g1, whole = _mix(hb, bank, utts, *args, tail=loud_tail)
    moved, g2, _ = _mix(hb, bank2, utts, *args, tail=loud_tail)
    for a, b, c in zip(plain, rows, moved):
        assert np.isfinite(a).all() and np.array_equal(a.view(I32), b.view(I32)) and np.array_equal(a.view(I32), c.view(I32))
    assert np.array_equal(g0, g1) and np.array_equal(g0, g2) and g0[1] == 0 and g0[2] == 0 and g0[0] > 0
    assert (whole[-TAIL:] == CANARY).all()


def test_two_runs_give_the_same_bits(hb):
    utts, ridx, plan = _case(hb, "mixed_rows")
    first, _ = _reverb(hb, plan, utts, ridx)
    again, _ = _reverb(hb, plan, utts, ridx)
    with hb.deterministic():
        det, _ = _reverb(hb, plan, utts, ridx)
    host, _ = _reverb(hb, plan, utts, ridx, device_index=False)
    for a, b, c, d in zip(first, again, det, host):
        assert all(np.array_equal(a.view(I32), o.view(I32)) for o in (b, c, d))
    (_, utts, clips, cidx, start, snr), = A.mix_cases(hb.NOISE_TILE)
    bank = hb.NoiseBank(clips)
    first, g1, _ = _mix(hb, bank, utts, cidx, start, snr)
    again, g2, _ = _mix(hb, bank, utts, cidx, start, snr)
    with hb.deterministic():
        det, g3, _ = _mix(hb, bank, utts, cidx, start, snr)
    host, g4, _ = _mix(hb, bank, utts, cidx, start, snr, device_args=False)
    for a, b, c, d in zip(first, again, det, host):
        assert all(np.array_equal(a.view(I32), o.view(I32)) for o in (b, c, d))
    assert all(np.array_equal(g1.view(I32), g.view(I32)) for g in (g2, g3, g4))


def test_refused_shapes_launch_nothing(hb):
    plan = _case(hb, "batch_of_one")[2]
    bank = hb.NoiseBank([np.ones(10, np.float32)])
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    offs = torch.tensor([0, 30, 64], dtype=torch.int64).cuda()
    out = torch.full((256,), CANARY, device="cuda")
    before = (hb.LAUNCHES["reverb"], hb.LAUNCHES["noise_mix"])
    for bad in ([0, len(plan)], [-2, 0], [0]):
        with pytest.raises(hb.UnsupportedShape):
            hb.reverb(plan, x, offs, bad, out)
        with pytest.raises(hb.UnsupportedShape):
            hb.noise_mix(bank, x, offs, bad, [0, 0], [1.0, 1.0], out=out)
    B = 65536
    many = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    zi, zl, zf = (torch.zeros(B, dtype=t, device="cuda") for t in (torch.int32, torch.int64, torch.float32))
    with pytest.raises(hb.UnsupportedShape):
        hb.reverb(plan, x, many, zi, out)
    with pytest.raises(hb.UnsupportedShape):
        hb.noise_mix(bank, x, many, zi, zl, zf, out=out)
    with pytest.raises(RuntimeError):
        hb.reverb(plan, x.cpu(), offs, [0, 0], out)
    with pytest.raises(RuntimeError):
        hb.noise_mix(bank, x, offs, [0, 0], [0, 0], [1.0, 1.0])              # int16 in place
    # the C entries themselves: a plan beyond its limits, geometry outside the bank, a dtype code that is neither of the two
    lib, c_p = hb.load(), ctypes.c_void_p
    rbank, rgeo = plan.on("cuda")
    nbank, noffs = bank.on("cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")

    def call_reverb(geometry, dtype_code, src=x, dst=out):
        g = np.ascontiguousarray(geometry, dtype=np.int64)
        return lib.asr_reverb_f32(2, 64, c_p(src.data_ptr()), dtype_code, 64, c_p(offs.data_ptr()), c_p(zi.data_ptr()), g.shape[0],
                                  c_p(g.ctypes.data), c_p(rgeo.data_ptr()), c_p(rbank.data_ptr()), rbank.numel(),
                                  c_p(dst.data_ptr()), dst.numel(), hb.stream())

    def call_mix(offsets, dtype_code, ws_bytes=512, src=x):
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        return lib.asr_noise_mix_f32(2, 64, c_p(src.data_ptr()), dtype_code, 64, c_p(offs.data_ptr()), c_p(zi.data_ptr()),
                                     c_p(zl.data_ptr()), c_p(zf.data_ptr()), o.size - 1, c_p(o.ctypes.data), c_p(noffs.data_ptr()),
                                     c_p(nbank.data_ptr()), nbank.numel(), c_p(ws.data_ptr()), ws_bytes, c_p(out.data_ptr()),
                                     out.numel(), None, hb.stream())
    good = plan.geometry
    assert call_reverb([[0, hb.REVERB_MAX_TAPS + 1, 0]], hb.SAMPLES_I16) == hb.ASR_E_SHAPE
    assert call_reverb(good, 2) == hb.ASR_E_SHAPE and call_reverb(good, -1) == hb.ASR_E_SHAPE
    assert call_reverb([[0, rbank.numel() + 1, 0]], hb.SAMPLES_I16) == -1                   # ASR_E_ARG: outside the bank
    assert call_reverb([[0, 33, 33]], hb.SAMPLES_I16) == -1                                 # d outside the RIR
    assert call_reverb(good, hb.SAMPLES_F32, src=out, dst=out) == -1                        # in place
    assert call_mix(bank.offsets, 2) == hb.ASR_E_SHAPE
    assert call_mix([0, 11], hb.SAMPLES_I16) == -1 and call_mix([0, 5, 5], hb.SAMPLES_I16) == -1
    assert call_mix(bank.offsets, hb.SAMPLES_I16, ws_bytes=16) == -1
    torch.cuda.synchronize()
    assert (hb.LAUNCHES["reverb"], hb.LAUNCHES["noise_mix"]) == before and (out == CANARY).all()


# ------------------------------------------------------------------------------------------------ Frontend and the feed
def _items(n=6, seed=3, dtype=np.int16):
    from dataset import synthetic_waveforms
    data = synthetic_waveforms(n, 9, 0.3, seed=seed, dtype=dtype)
    return [(v["feature"], v["token_ids"]) for v in data.values()]


def _bank_dict(clips):
    clips = [np.asarray(c, dtype=np.float32) for c in clips]
    return dict(samples=np.concatenate(clips), offsets=np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64))


def _augment_cfg(prob=0.6):
    rs = np.random.RandomState(31)
    rirs = [A.rir_with(rs, 900 + 300 * i, 10 + 30 * i) for i in range(3)]
    clips = [rs.randn(n) * 400 for n in (1500, 9000, 1)]
    return dict(reverb=dict(bank=_bank_dict(rirs), prob=prob, max_taps=1024), noise=dict(bank=_bank_dict(clips), prob=prob, snr_db=[5, 20]))


FE_CFG = dict(n_mels=8, delta_order=0, cmvn="utterance",
              specaug=dict(n_freq_masks=1, max_freq_width=3, n_time_masks=1, max_time_width=6))
SPEEDS = [0.9, 1.0, 1.1]
KEYS = ("resample", "reverb", "noise_mix", "fbank", "feat_cmvn_stats", "feat_finish")


def _packed(items):
    offs = np.concatenate([[0], np.cumsum([len(f) for f, _ in items])])
    return torch.from_numpy(np.concatenate([f for f, _ in items])).cuda(), offs.tolist()


def _delta(hb, before):
    return {k: hb.LAUNCHES[k] - before.get(k, 0) for k in KEYS}


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_frontend_composes_the_launches(hb, dtype):
    """Frontend with augment= adds nothing of its own: it equals, bit for bit, the front end run on the output of hb.resample,
    hb.reverb and hb.noise_mix called by hand; one launch of each."""
    from frontend import Frontend
    fe = Frontend(dict(FE_CFG, specaug=None, delta_order=1, speed_perturb=SPEEDS, **_augment_cfg()))
    bare = Frontend(dict(FE_CFG, specaug=None, delta_order=1))
    items = _items(5, seed=8, dtype=dtype)
    fidx = [0, 2, 1, 0, 2]
    draws = [(0, 1, 8000, 12.0), (-1, 0, 1499, 5.0), (2, -1, 0, 9.0), (-1, -1, 3, 20.0), (1, 2, 0, 7.5)]
    samples, offs = _packed(items)
    kept = samples.clone()
    before = dict(hb.LAUNCHES)
    xs, ilens = fe(samples, offs, factor_index=fidx, augment=draws)
    assert _delta(hb, before) == dict.fromkeys(KEYS, 1)
    assert torch.equal(samples, kept)
    counts = [fe.perturbed_samples(len(f), i) for (f, _), i in zip(items, fidx)]
    assert ilens == [fe.num_frames(c) for c in counts]
    out_offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).cuda()
    dry = torch.empty(sum(counts), device="cuda")
    hb.resample(fe.resample_plan, samples, torch.tensor(offs, dtype=torch.int64).cuda(), fidx, out_offs, dry, max_out=max(counts))
    wet = hb.reverb(fe.reverb_plan, dry, out_offs, [a[0] for a in draws], torch.empty_like(dry), max_len=max(counts))
    assert not torch.equal(wet, dry)
    hb.noise_mix(fe.noise_bank, wet, out_offs, [a[1] for a in draws], [a[2] for a in draws],
                 np.asarray([fe.snr_scale(a[3]) for a in draws], dtype=np.float32), max_len=max(counts))
    want, want_lens = bare(wet, out_offs.tolist())
    assert want_lens == ilens and torch.equal(xs, want)
    # each launch only with its key; without draws none
    for cfg, expect, only in ((dict(reverb=_augment_cfg()["reverb"]), dict(reverb=1, noise_mix=0), [(a[0], -1, 0, a[3]) for a in draws]),
                              (dict(noise=_augment_cfg()["noise"]), dict(reverb=0, noise_mix=1), [(-1,) + a[1:] for a in draws])):
        one = Frontend(dict(FE_CFG, specaug=None, **cfg))
        before = dict(hb.LAUNCHES)
        got, got_lens = one(samples, offs, augment=only)
        assert _delta(hb, before) == dict(dict.fromkeys(KEYS, 1), resample=0, **expect)
        assert got_lens == [one.num_frames(len(f)) for f, _ in items] and torch.equal(samples, kept)
    before = dict(hb.LAUNCHES)
    plain, _ = fe(samples, offs)
    assert _delta(hb, before) == dict(dict.fromkeys(KEYS, 1), resample=0, reverb=0, noise_mix=0)
    assert torch.equal(plain, bare(samples, offs)[0])
    with pytest.raises(hb.UnsupportedShape):
        fe(samples, offs, augment=[(3, 0, 0, 5.0)] * 5)
    with pytest.raises(ValueError):
        bare(samples, offs, augment=draws)


def _direct(fe, items, augment_seed, mask_seed, batch_index):
    """The augmented batch computed directly: sort by sample count (stable), draw by COLLATED row, Frontend.__call__."""
    order = sorted(range(len(items)), key=lambda i: -len(items[i][0]))
    draws = [fe.draw_augment(augment_seed, batch_index, i) for i in order]
    items = [items[i] for i in order]
    frames = [fe.num_frames(len(f)) for f, _ in items]
    masks = np.stack([fe.draw_masks(mask_seed, batch_index, r, T) for r, T in enumerate(frames)])
    samples, offs = _packed(items)
    xs, ilens = fe(samples, offs, masks=masks, augment=draws)
    return xs, ilens, items, draws, frames


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("thread", [False, True])
def test_training_feed_augments(hb, dtype, thread):
    from feed import DeviceFeed
    from frontend import Frontend
    fe, plain = Frontend(dict(FE_CFG, **_augment_cfg())), Frontend(FE_CFG)
    batches = [_items(6, seed=3, dtype=dtype), _items(7, seed=4, dtype=dtype)]

    def feeds(**kw):
        np.random.seed(21)                                   # the feeds take their mask and augment seeds from this stream
        return DeviceFeed(batches, "cuda", frontend=fe, thread=thread, train=True, **kw)
    whole = feeds()
    assert whole.augment_seed is not None and whole.mask_seed is not None and whole.speed_seed is None
    shards = [iter(feeds(rank=rank, world=2)) for rank in range(2)]
    seen_rir, seen_clip, n = set(), set(), 0
    for bi, (items, (xs, ilens, ys)) in enumerate(zip(batches, whole)):
        want, want_lens, order, draws, frames = _direct(fe, items, whole.augment_seed, whole.mask_seed, bi)
        torch.cuda.synchronize()
        assert ilens == want_lens == frames == [plain.num_frames(len(f)) for f, _ in order]      # the unaugmented counts
        assert torch.equal(xs, want) and xs.shape[1] == max(frames)
        assert [y.tolist() for y in ys] == [t for _, t in order]
        seen_rir.update(a[0] for a in draws)
        seen_clip.update(a[1] for a in draws)
        for rank in range(2):
            shard, il, ys_r = next(shards[rank])
            torch.cuda.synchronize()
            assert il == ilens[rank::2] and shard.info["t_max"] == xs.shape[1] and shard.info["b_global"] == len(items)
            assert torch.equal(shard.xs, xs[rank::2])
            assert [y.tolist() for y in ys_r] == [y.tolist() for y in ys[rank::2]]
        n += 1
    assert n == 2 and -1 in seen_rir and -1 in seen_clip and len(seen_rir) > 1 and len(seen_clip) > 1
    for it in shards:
        assert next(it, None) is None


def test_training_feed_with_speed_draws_by_collated_row(hb):
    from feed import DeviceFeed, plan_speed_batch
    from frontend import Frontend
    fe = Frontend(dict(FE_CFG, speed_perturb=SPEEDS, **_augment_cfg()))
    items = _items(7, seed=5)
    np.random.seed(21)
    feed = DeviceFeed([items], "cuda", frontend=fe, thread=False, train=True)
    before = dict(hb.LAUNCHES)
    xs, ilens, _ = next(iter(feed))
    assert _delta(hb, before) == dict.fromkeys(KEYS, 1)
    order, fidx, pert = plan_speed_batch(fe, feed.speed_seed, 0, [len(f) for f, _ in items])
    draws = [fe.draw_augment(feed.augment_seed, 0, i) for i in order]
    frames = [fe.num_frames(p) for p in pert]
    masks = np.stack([fe.draw_masks(feed.mask_seed, 0, r, T) for r, T in enumerate(frames)])
    samples, offs = _packed([items[i] for i in order])
    want, want_lens = fe(samples, offs, masks=masks, factor_index=fidx, augment=draws)
    torch.cuda.synchronize()
    assert ilens == want_lens == frames and torch.equal(xs, want)


def test_other_feeds_give_todays_batch(hb):
    """train=False with the keys, and a training feed whose front end has none: today's batch, bit for bit, today's draws from
    the process's numpy stream, and no new launch."""
    from feed import DeviceFeed
    from frontend import Frontend
    fe, plain = Frontend(dict(FE_CFG, **_augment_cfg())), Frontend(FE_CFG)
    items = _items(7, seed=6)
    before = dict(hb.LAUNCHES)
    np.random.seed(21)
    first, second = int(np.random.randint(0, 2 ** 31 - 1)), int(np.random.randint(0, 2 ** 31 - 1))
    np.random.seed(21)
    feed = DeviceFeed([items], "cuda", frontend=plain, thread=False, train=True)
    assert (feed.mask_seed, feed.speed_seed, feed.augment_seed) == (first, None, None)
    assert int(np.random.randint(0, 2 ** 31 - 1)) == second           # one draw taken, as before
    xs, ilens, _ = next(iter(feed))
    order = sorted(items, key=lambda it: -len(it[0]))
    masks = np.stack([plain.draw_masks(first, 0, i, plain.num_frames(len(f))) for i, (f, _) in enumerate(order)])
    samples, offs = _packed(order)
    want, want_lens = plain(samples, offs, masks=masks)
    assert ilens == want_lens and torch.equal(xs, want)
    clean, clean_lens = plain(samples, offs)
    for kw in (dict(), dict(kind="speech")):
        np.random.seed(21)
        feed = DeviceFeed([items], "cuda", frontend=fe, thread=False, train=False, **kw)
        assert (feed.mask_seed, feed.speed_seed, feed.augment_seed) == (None, None, None)
        assert int(np.random.randint(0, 2 ** 31 - 1)) == first        # nothing taken
        batch = next(iter(feed))
        assert batch.ilens == clean_lens and torch.equal(batch.xs, clean)
    assert hb.LAUNCHES["reverb"] == before.get("reverb", 0) and hb.LAUNCHES["noise_mix"] == before.get("noise_mix", 0)
    assert hb.LAUNCHES["resample"] == before.get("resample", 0)


def test_e2e_forward_backward_on_an_augmented_batch(hb):
    import synth
    import model as M
    from feed import DeviceFeed
    from frontend import Frontend
    cfg = dict(synth.TINY)
    fe = Frontend(dict(FE_CFG, **_augment_cfg(prob=1.0)))
    assert fe.output_dim == cfg["input_dim"]
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).to("cuda")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
    net.train()
    np.random.seed(5)
    before = dict(hb.LAUNCHES)
    xs, ilens, ys = next(iter(DeviceFeed([_items(3, seed=2)], "cuda", frontend=fe, thread=False, train=True)))
    assert _delta(hb, before) == dict(dict.fromkeys(KEYS, 1), resample=0)
    _, lp, _, _ = net(xs, ilens, ys)
    loss = -lp.mean()
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xs).all()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
