"""Speed perturbation without a GPU: the bank geometry and output lengths, hb.ResamplePlan against the float64
restatement of tests/resample_ref.py, the header's limits, the host draws, and the feed's host arithmetic (sort by perturbed
length, data-parallel split).  The float32 restatement is held to the GPU tests' allowance over exactly their inputs."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEED_SEED = 5               # test_draw_speed checks that this seed draws every factor over 2 batches of 6 rows


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    return hip_backend


def _header():
    with open(os.path.join(ROOT, "include", "asr_hip.h")) as f:
        return f.read()


def test_bank_geometry_and_lengths():
    want = {0.9: (9, 10, 7, 23), 1.1: (11, 10, 7, 25), 0.95: (19, 20, 7, 33)}
    for s, (orig, new, width, taps) in want.items():
        assert R.ratio(s) == (orig, new)
        w, h = R.bank(orig, new)
        assert (w, h.shape) == (width, (new, taps))
    assert [R.out_samples(3001, *R.ratio(s)) for s in (0.9, 1.1, 0.95, 1.0)] == [3335, 2729, 3159, 3001]
    # a unit-gain low-pass: every phase sums to ~1, so a constant stays that constant away from the edges
    for s in want:
        _, h = R.bank(*R.ratio(s))
        assert np.abs(h.sum(axis=1) - 1.0).max() < 2e-3


def test_header_constants_and_exports(hb):
    header = _header()
    for name in ("TILE", "MAX_FACTORS", "MAX_PHASES", "MAX_TAPS", "MAX_SPAN"):
        m = re.search(r"#define ASR_RESAMPLE_%s (\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(hb, "RESAMPLE_" + name), name
    assert "asr_resample_plan_bytes" in hb.EXPORTS and "asr_resample_f32" in hb.EXPORTS
    assert hb.RESAMPLE_TILE % 256 == 0


@pytest.mark.parametrize("sample_rate", [8000, 16000])
def test_plan_equals_the_restatement(hb, sample_rate):
    factors = [0.9, 0.95, 1.0, 1.05, 1.1]
    plan = hb.ResamplePlan(sample_rate, factors)
    assert len(plan) == 5 and plan.tables.dtype == np.float32
    used = 0
    for f, s in enumerate(factors):
        orig, new = R.ratio(s, sample_rate)
        width, h = R.bank(orig, new)
        assert plan.geometry[f].tolist() == [orig, new, width, h.shape[1], used]
        assert np.array_equal(plan.bank(f), h.astype(np.float32))
        assert plan.out_samples(3001, f) == R.out_samples(3001, orig, new)
        used += h.size
    assert plan.tables.size == used and hb.resample_plan_bytes(plan.geometry) == 4 * used


def test_limits_are_refused(hb):
    with pytest.raises(hb.UnsupportedShape):
        hb.ResamplePlan(16000, [0.97])                     # 97 / 100: 100 phases
    with pytest.raises(hb.UnsupportedShape):
        hb.ResamplePlan(16000, [1.0] * (hb.RESAMPLE_MAX_FACTORS + 1))
    with pytest.raises(hb.UnsupportedShape):
        hb.ResamplePlan(16000, [2.5])                      # a tile's input span beyond ASR_RESAMPLE_MAX_SPAN
    with pytest.raises(hb.UnsupportedShape):
        hb.ResamplePlan(16000, [1.33])                     # 133 / 100: phases and taps
    good = hb.ResamplePlan(16000, [0.9]).geometry
    for col, limit in ((1, hb.RESAMPLE_MAX_PHASES), (3, hb.RESAMPLE_MAX_TAPS)):
        g = good.copy()
        g[0, col] = limit + 1
        if col == 3:
            g[0, 0] = limit + 1 - 2 * g[0, 2]              # keep taps = 2 width + orig
        with pytest.raises(hb.UnsupportedShape):
            hb.resample_plan_bytes(g)
    assert hb.load().asr_resample_plan_bytes(hb.RESAMPLE_MAX_FACTORS + 1, good.ctypes.data, None) == -1       # ASR_E_ARG


def test_float32_restatement_stays_inside_the_allowance():
    worst = 0.0
    for name, utts, fidx in R.cases(1024):
        for x, f in zip(utts, fidx):
            orig, new = R.ratio(R.FACTORS[f])
            r64, mag, taps = R.resample(x, orig, new)
            r32, _, _ = R.resample(x, orig, new, np.float32)
            assert len(r64) == len(r32) == R.out_samples(len(x), orig, new)
            err, tol = np.abs(r32.astype(np.float64) - r64), R.allowance(mag, taps)
            assert (err <= tol).all(), (name, len(x), f)
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("resample-parity float32 restatement: worst error / allowance %.3f" % worst)
    assert 0.0 < worst <= 1.0


def _frontend(**kw):
    from frontend import Frontend
    return Frontend(dict(dict(n_mels=8, speed_perturb=[0.9, 1.0, 1.1]), **kw))


def test_draw_speed(hb):
    fe = _frontend()
    draws = [[fe.draw_speed(SPEED_SEED, b, r) for r in range(6)] for b in range(2)]
    assert draws == [[fe.draw_speed(SPEED_SEED, b, r) for r in range(6)] for b in range(2)]
    assert set(draws[0] + draws[1]) == {0, 1, 2}
    assert draws[0] != draws[1]
    assert [fe.perturbed_samples(3001, f) for f in range(3)] == [3335, 3001, 2729]
    assert fe.num_frames(fe.perturbed_samples(3001, 0)) == 1 + (3335 - 400) // 160
    assert fe.frames_of(np.zeros(3001, np.int16)) == 1 + (3001 - 400) // 160     # the corpus' view: unperturbed
    off = _frontend(speed_perturb=[])
    assert off.n_speeds == 0 and off.resample_plan is None and _frontend(speed_perturb=None).resample_plan is None


def test_feed_host_arithmetic(hb):
    import parallel
    from feed import plan_speed_batch
    fe = _frontend()
    counts = [3001, 2990, 2700, 2650, 2600, 2500, 5000]            # close enough that the draws reorder them
    order, fidx, pert = plan_speed_batch(fe, SPEED_SEED, 1, counts)
    draws = [fe.draw_speed(SPEED_SEED, 1, i) for i in range(len(counts))]         # by COLLATED row
    assert sorted(order) == list(range(len(counts)))
    assert fidx == [draws[i] for i in order]
    assert pert == [fe.perturbed_samples(counts[i], draws[i]) for i in order] == sorted(pert, reverse=True)
    assert order != sorted(range(len(counts)), key=lambda i: -counts[i]), "the draws of this seed must change the order"
    ilens = [fe.num_frames(p) for p in pert]
    assert ilens == sorted(ilens, reverse=True)
    # equal perturbed counts keep their collated order (a stable sort)
    o2, _, p2 = plan_speed_batch(_frontend(speed_perturb=[1.0]), SPEED_SEED, 0, [500, 700, 500, 700])
    assert (o2, p2) == ([1, 3, 0, 2], [700, 700, 500, 500])
    # two ranks: each computes the whole plan and takes its strided rows; together they are the one-process batch
    seen = {}
    for rank in range(2):
        o_r, f_r, p_r = plan_speed_batch(fe, SPEED_SEED, 1, counts)
        for i in parallel.shard_indices(len(counts), rank, 2):
            seen[i] = (o_r[i], f_r[i], p_r[i])
    assert [seen[i] for i in range(len(counts))] == list(zip(order, fidx, pert))
