"""Reverberation and additive noise without a GPU: the float32 restatements of tests/augment_ref.py against the
float64 ones over exactly the GPU tests' inputs and allowances, the host's bank preparation, the draws, the feed's seeds and
the header."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import augment_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    return hip_backend


def _bank(clips):
    clips = [np.asarray(c) for c in clips]
    return dict(samples=np.concatenate(clips), offsets=np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64))


def _rirs(n=3, seed=2):
    rs = np.random.RandomState(seed)
    return [A.rir_with(rs, 200 + 50 * i, 20 + i).astype(np.float32) for i in range(n)]


def _clips(seed=3):
    rs = np.random.RandomState(seed)
    return [(rs.randn(n) * 800).astype(np.float32) for n in (900, 1, 4000, 2500)]


def _frontend(reverb=True, noise=True, **kw):
    from frontend import Frontend
    cfg = dict(n_mels=8)
    if reverb:
        cfg["reverb"] = dict(dict(bank=_bank(_rirs()), prob=0.5), **kw.pop("reverb_kw", {}))
    if noise:
        cfg["noise"] = dict(dict(bank=_bank(_clips()), prob=0.5, snr_db=[5, 20]), **kw.pop("noise_kw", {}))
    return Frontend(dict(cfg, **kw))


# ------------------------------------------------------------------------------------------------ the restatements
def test_float32_convolution_stays_inside_the_allowance():
    worst = 0.0
    for name, utts, rirs, ridx in A.reverb_cases(4096, 2048, 8192):
        for x, r in zip(utts, ridx):
            if r < 0:
                continue
            h, d = A.prepare_rir(rirs[r], max_taps=8192, pre=len(rirs[r]))
            assert h[d] == np.abs(h).max() and len(h) == len(rirs[r])       # (no head cut: d is where the table put it)
            r64, mag = A.reverb(x, h, d)
            r32, _ = A.reverb(x, h, d, np.float32)
            assert r64.shape == r32.shape == x.shape
            err, tol = np.abs(r32.astype(np.float64) - r64), A.reverb_allowance(mag, len(h))
            assert (err <= tol).all(), (name, len(x), r)
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("augment-parity float32 convolution restatement: worst error / allowance %.3f" % worst)
    assert 0.0 < worst <= 1.0


def test_convolution_restatement_is_the_definition():
    """The convolve-and-slice form against the sum written out, on a case small enough to write out."""
    rs = np.random.RandomState(1)
    x, h, d = rs.randn(9), rs.randn(5), 3
    want = [sum(h[k] * x[n + d - k] for k in range(5) if 0 <= n + d - k < 9) for n in range(9)]
    got, mag = A.reverb(x, h.astype(np.float32).astype(np.float64), d)
    assert np.allclose(got, [sum(np.float32(h[k]).astype(np.float64) * x[n + d - k] for k in range(5) if 0 <= n + d - k < 9)
                             for n in range(9)], rtol=0, atol=1e-14)
    assert np.allclose(got, want, rtol=0, atol=1e-6) and (mag >= np.abs(got) - 1e-12).all()


def test_float32_mix_stays_inside_the_allowances():
    for name, utts, clips, cidx, start, snr in A.mix_cases(4096):
        for y, c, s, db in zip(utts, cidx, start, snr):
            if c < 0:
                continue
            z64, g64, mag = A.mix(y, clips[c], s, db)
            z32, g32, _ = A.mix(y, clips[c], s, db, np.float32)
            assert g64 > 0 and abs(float(g32) - g64) <= A.GAIN_ALLOWANCE * g64
            assert (np.abs(z32.astype(np.float64) - z64) <= A.mix_allowance(mag)).all(), (name, len(y), c)
            assert abs(A.achieved_snr_db(y, z32) - db) <= 1e-3
    silent = np.zeros(50, np.int16)
    assert A.mix(silent, clips[0], 0, 10.0)[1] == 0.0 and A.mix(utts[0], np.zeros(7, np.float32), 3, 10.0, np.float32)[1] == 0.0
    v = A.noise_of(np.arange(5), 3, 12)
    assert v.tolist() == [3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ bank preparation
def test_reverb_plan_prepares_the_bank(hb):
    rs = np.random.RandomState(5)
    long = A.rir_with(rs, 12000, 3000)                     # longer than the limit: cut, not refused
    early = A.rir_with(rs, 300, 5)                         # d < 32: the whole head stays
    twice = A.rir_with(rs, 100, 60)
    twice[80] = -1.0                                       # the same magnitude again, later: the FIRST one is the direct path
    plan = hb.ReverbPlan([long, early, twice], max_taps=4096)
    assert len(plan) == 3 and plan.bank.dtype == np.float32 and plan.geometry.dtype == np.int64
    used = 0
    for r, (raw, d_raw) in enumerate(((long, 3000), (early, 5), (twice, 60))):
        h, d = plan.rir(r)
        want, want_d = A.prepare_rir(raw, 4096)
        pre = min(d_raw, 32)
        assert d == want_d == pre and len(h) == min(4096, len(raw) - (d_raw - pre))
        assert plan.geometry[r].tolist() == [used, len(h), d]
        assert np.array_equal(h, want)
        assert abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) < 1e-6 and np.argmax(np.abs(h)) == d
        used += len(h)
    assert plan.rir(0)[0].size == 4096 and plan.bank.size == used
    # exact taps for the exact tests, and any d for the kernel's
    raw = hb.ReverbPlan([twice], max_taps=8192, normalize=False, pre=len(twice))
    assert np.array_equal(raw.rir(0)[0], twice.astype(np.float32)) and raw.rir(0)[1] == 60
    with pytest.raises(hb.UnsupportedShape):
        hb.ReverbPlan([early], max_taps=hb.REVERB_MAX_TAPS + 1)
    with pytest.raises(ValueError):
        hb.ReverbPlan([np.zeros(10)])
    assert len(hb.ReverbPlan([long], max_taps=hb.REVERB_MAX_TAPS).rir(0)[0]) == hb.REVERB_MAX_TAPS


def test_banks_load_from_npz_and_dict(hb, tmp_path):
    clips = [np.arange(1, 6, dtype=np.int16), np.asarray([-7, 9], dtype=np.int16)]
    bank = _bank(clips)
    path = str(tmp_path / "noise.npz")
    np.savez(path, **bank)
    for source in (bank, path):
        nb = hb.NoiseBank(hb.load_bank(source))
        assert len(nb) == 2 and nb.bank.dtype == np.float32 and nb.offsets.tolist() == [0, 5, 7]
        assert nb.clip(1).tolist() == [-7.0, 9.0] and nb.clip_len(0) == 5
    with pytest.raises(ValueError):
        hb.load_bank(dict(samples=bank["samples"], offsets=np.asarray([0, 5, 5, 7])))      # an empty clip
    with pytest.raises(ValueError):
        hb.load_bank(dict(samples=bank["samples"].astype(np.float64), offsets=bank["offsets"]))


# ------------------------------------------------------------------------------------------------ draws and seeds
def test_draw_augment_is_a_function_of_seed_batch_row(hb):
    fe = _frontend()
    draws = [[fe.draw_augment(7, b, r) for r in range(40)] for b in range(2)]
    assert draws == [[fe.draw_augment(7, b, r) for r in range(40)] for b in range(2)]
    assert draws[0] != draws[1] and draws[0] != [fe.draw_augment(8, 0, r) for r in range(40)]
    flat = draws[0] + draws[1]
    n_rirs, n_clips = len(fe.reverb_plan), len(fe.noise_bank)
    assert {a[0] for a in flat} == set(range(-1, n_rirs)) and {a[1] for a in flat} == set(range(-1, n_clips))
    for rir, clip, start, snr in flat:
        assert 5.0 <= snr <= 20.0
        assert 0 <= start < (fe.noise_bank.clip_len(clip) if clip >= 0 else max(fe.noise_bank.clip_len(c) for c in range(n_clips)))
    assert any(a[2] > 0 for a in flat)
    assert abs(float(fe.snr_scale(20.0)) - 0.1) < 1e-8 and fe.snr_scale(6.0).dtype == np.float32


def test_draw_augment_fields_do_not_depend_on_each_other(hb):
    """Every variate is taken whether or not it is used: switching one stage off or to `always`, or dropping its key, moves
    no other field of any row."""
    both = _frontend()
    always_rir = _frontend(reverb_kw=dict(prob=1.0))
    never_rir = _frontend(reverb_kw=dict(prob=0.0))
    no_rir = _frontend(reverb=False)
    always_noise = _frontend(noise_kw=dict(prob=1.0))
    no_noise = _frontend(noise=False)
    for row in range(30):
        rir, clip, start, snr = both.draw_augment(3, 1, row)
        for other in (always_rir, never_rir, no_rir):
            assert other.draw_augment(3, 1, row)[1:] == (clip, start, snr)
        assert always_rir.draw_augment(3, 1, row)[0] >= 0 and never_rir.draw_augment(3, 1, row)[0] == -1
        assert no_rir.draw_augment(3, 1, row)[0] == -1
        if rir >= 0:
            assert always_rir.draw_augment(3, 1, row)[0] == rir
        a = always_noise.draw_augment(3, 1, row)
        assert a[0] == rir and a[1] >= 0 and a[3] == snr and (clip < 0 or (a[1], a[2]) == (clip, start))
        assert no_noise.draw_augment(3, 1, row) == (rir, -1, 0, 0.0)
    assert not _frontend(reverb=False, noise=False).augments and both.augments and no_noise.augments


def test_feed_seeds(hb):
    """A feed without the keys takes exactly today's draws from the process's numpy stream; the augment seed comes third."""
    from feed import draw_feed_seeds
    specaug = dict(n_freq_masks=1, max_freq_width=3, n_time_masks=1, max_time_width=6)
    np.random.seed(21)
    first, second, third, fourth = (int(np.random.randint(0, 2 ** 31 - 1)) for _ in range(4))

    def seeds(fe, train=True):
        np.random.seed(21)
        return draw_feed_seeds(fe, train), int(np.random.randint(0, 2 ** 31 - 1))
    plain = _frontend(reverb=False, noise=False, specaug=specaug, speed_perturb=[0.9, 1.0, 1.1])
    assert seeds(plain) == ((first, second, None), third)                 # today's two draws, nothing more
    assert seeds(_frontend(reverb=False, noise=False)) == ((None, None, None), first)
    full = _frontend(specaug=specaug, speed_perturb=[0.9, 1.0, 1.1])
    assert seeds(full) == ((first, second, third), fourth)
    assert seeds(_frontend(noise=False)) == ((None, None, first), second)  # one key is enough, and it is the only draw then
    assert seeds(full, train=False) == ((None, None, None), first)


def test_header_declares_the_entries(hb):
    with open(os.path.join(ROOT, "include", "asr_hip.h")) as f:
        header = f.read()
    for name in ("REVERB_TILE", "REVERB_CHUNK", "REVERB_MAX_TAPS", "NOISE_TILE"):
        m = re.search(r"#define ASR_%s (\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(hb, name), name
    assert re.search(r"\bint asr_reverb_f32\(", header) and re.search(r"\bint asr_noise_mix_f32\(", header)
    assert "asr_reverb_f32" in hb.EXPORTS and "asr_noise_mix_f32" in hb.EXPORTS
    lib = hb.load()
    assert hasattr(lib, "asr_reverb_f32") and hasattr(lib, "asr_noise_mix_f32")
    assert hb.REVERB_MAX_TAPS >= 8192 and hb.REVERB_MAX_TAPS % hb.REVERB_CHUNK == 0 and hb.REVERB_TILE == 4 * 1024
    # refusals need no GPU: nothing is launched
    assert lib.asr_reverb_f32(1, 10, None, 0, 0, None, None, 1, None, None, None, 0, None, 0, None) == -1     # ASR_E_ARG
