"""tests/stream_ref.py held to independent implementations, and the inputs of tests/test_stream_kernels_gpu.py held to what
that suite relies on - without a GPU: the numpy Adam restatement against torch.optim.Adam in float64, the five wrong
variants of the update visible on the grid's own inputs, the dropout hash against a table of keep values and its keep
rate, the label log-probability closed form against torch autograd, the planted argmax ties exact in float32."""
import numpy as np
import pytest
import torch

import stream_ref as R


# ------------------------------------------------------------------------------------------------ optimiser
@pytest.mark.parametrize("amsgrad,wd,clip,eps", [c for c in R.ADAM_GRID if c[3] == 1e-8 or c[2] == "active"])
def test_adam_restatement_equals_torch_float64(amsgrad, wd, clip, eps):
    """adam_update chained over 4 steps against torch.optim.Adam(foreach=False) + clip_grad_norm_ in float64: 1e-12 relative to
    each tensor's largest value, every step, for p, exp_avg, exp_avg_sq and max_exp_avg_sq."""
    for name in ("n1", "n257", "odd"):
        sizes = R.ADAM_LISTS[name]
        params, grads = R.adam_inputs(sizes)
        mine = R.adam_run_np(params, grads, amsgrad, wd, clip, eps)
        ref = R.adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float64)
        for s in range(R.ADAM_STEPS):
            for key in ("p", "m", "v") + (("vmax",) if amsgrad else ()):
                want = np.concatenate(ref[s][key])
                err = np.abs(mine[s][key] - want).max()
                assert err <= 1e-12 * np.abs(want).max(), (name, s, key, err)
            assert abs(mine[s]["norm_sq"] - ref[s]["norm_sq"]) <= 1e-12 * ref[s]["norm_sq"]


def _visible_fraction(mutation, amsgrad, wd, clip, eps, name):
    """The largest share of a case's elements, over the compared tensors, on which the mutated update's float64 result after
    4 steps is further than 10 allowances from the true one."""
    sizes = R.ADAM_LISTS[name]
    params, grads = R.adam_inputs(sizes)
    true = R.adam_run_np(params, grads, amsgrad, wd, clip, eps)[-1]
    bad = R.adam_run_np(params, grads, amsgrad, wd, clip, eps, mutation=mutation)[-1]
    r64 = R.adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float64)[-1]
    r32 = [run[-1] for run in R.adam_yardsticks(params, grads, amsgrad, wd, clip, eps)]
    best = 0.0
    for key in ("p", "m", "v") + (("vmax",) if amsgrad else ()):
        allow = np.concatenate([R.allowance(a, [r[key][i] for r in r32]) for i, a in enumerate(r64[key])])
        best = max(best, float(np.mean(np.abs(bad[key] - true[key]) > 10.0 * allow)))
    return best


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_adam_grid_sees_each_wrong_update(mutation):
    """Each wrong variant of the update (eps under the square root, the second bias correction dropped, the decay added in
    front of the clip scaling or applied decoupled, the amsgrad maximum dropped, the clip coefficient taken from norm^2)
    moves more than half of the elements of a compared tensor by more than 10 allowances in at least one case of the grid."""
    seen = []
    for amsgrad, wd, clip, eps in R.ADAM_GRID:
        frac = _visible_fraction(mutation, amsgrad, wd, clip, eps, "odd")
        seen.append((frac, amsgrad, wd, clip, eps))
    best = max(seen)
    print("mutation %s: visible on %.1f %% of the elements at amsgrad %s, wd %g, clip %s, eps %g" % ((mutation, 100 * best[0]) + best[1:]))
    assert best[0] >= 0.5, (mutation, best)


def _kernel_order_ratio(name, amsgrad, wd, clip, eps, plain_only=False):
    """Worst error / allowance of the kernel's operation order in float32 on the CPU, over steps and tensors."""
    sizes = R.ADAM_LISTS[name]
    params, grads = R.adam_inputs(sizes)
    r64 = R.adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float64)
    r32 = R.adam_yardsticks(params, grads, amsgrad, wd, clip, eps)
    if plain_only:
        r32 = r32[:1]
    got = R.adam_run_kernel_order(params, grads, amsgrad, wd, clip, eps)
    worst = 0.0
    for s in range(R.ADAM_STEPS):
        for key in ("p", "m", "v") + (("vmax",) if amsgrad else ()):
            for i, (g, a) in enumerate(zip(R.split(got[s][key].astype(np.float64), sizes), r64[s][key])):
                worst = max(worst, float((np.abs(g - a) / R.allowance(a, [r[s][key][i] for r in r32])).max()))
    return worst


@pytest.mark.parametrize("amsgrad,wd,clip,eps", R.ADAM_GRID)
def test_adam_allowance_fits_float32_in_the_kernels_order(amsgrad, wd, clip, eps):
    """The allowance is not so tight that correct float32 arithmetic in the kernel's order misses it, on any list up to 4139
    elements."""
    for name in ("n1", "n255", "n256", "n257", "odd"):
        assert _kernel_order_ratio(name, amsgrad, wd, clip, eps) <= 1.0, name


def test_adam_one_element_needs_the_moved_clip_coefficient():
    """Why adam_yardsticks runs three times for the list of one element under an active clip: with the plain float32
    optimiser alone (its norm of one element is exact) the kernel's order sits outside 4 x in some case of the grid."""
    worst = max((_kernel_order_ratio("n1", a, wd, clip, eps, plain_only=True), a, wd, eps)
                for a, wd, clip, eps in R.ADAM_GRID if clip == "active")
    print("n = 1, active clip, plain yardstick: %.2f allowances at amsgrad %s, wd %g, eps %g" % worst)
    assert worst[0] > 1.0


def test_adam_max_norms_are_what_their_names_say():
    for name, sizes in R.ADAM_LISTS.items():
        if name == "stride":
            continue
        _, grads = R.adam_inputs(sizes)
        for s, gs in enumerate(grads):
            norm = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gs)))
            assert norm < R.adam_max_norm("inactive", sizes, s)
            if R.adam_total(sizes) >= 255:
                assert 15.0 < norm / R.adam_max_norm("active", sizes, s) < 25.0, (name, s)
    sizes = R.ADAM_LISTS["stride"]
    assert R.adam_total(sizes) > 2048 * 256 and (R.adam_total(sizes) - 2048 * 256) % 256 != 0


# ------------------------------------------------------------------------------------------------ rows, pyramid
def test_fill_cases_cover_the_frame_lane_fold():
    lanes = [R.fill_lanes(c) for c in R.FILL_C4]
    assert lanes == [8, 8, 8, 8, 7, 6, 4, 2, 1, 1]
    assert [512 % c for c in (65, 80)] == [57, 32]                  # C4 that do not divide 512
    for c in R.FILL_C4:
        T, lens = R.fill_case(c)
        FL = R.fill_lanes(c)
        assert sorted(T - n for n in lens) == sorted([0, 1, FL - 1, FL, FL + 1, 3 * FL + 2]) and min(lens) >= 1
    assert sorted({(c // 4 >= 256) + (c // 4 >= 128) for c in R.ROW_C}) == [0, 1, 2]
    assert {c // 4 for c in R.ROW_C} >= {63, 64, 127, 128, 255, 256}


def test_row_and_pyramid_restatements_are_adjoint_and_inverse():
    """pack then unpack returns the valid frames; the pyramid backward is the adjoint of the forward (float64 dot test)."""
    rng = np.random.RandomState(3)
    lens, ext = np.array([5, 1, 3]), np.array([8, 4, 4])
    base = np.concatenate([[0], np.cumsum(ext)[:-1]])
    x = rng.randn(3, 5, 8).astype(np.float32)
    for b in range(3):
        x[b, lens[b]:] = np.nan
    rows = R.pack_ref(x, lens, base, ext)
    assert np.isfinite(rows).all() and rows.shape == (16, 8)
    back = R.unpack_fwd_ref(rows, lens, base, 5, None, False, None)
    for b in range(3):
        assert np.array_equal(back[b, :lens[b]], x[b, :lens[b]]) and not back[b, lens[b]:].any()
    for T in (1, 2, 3, 10, 11):
        a = rng.randn(T, 2, 4)
        m = rng.rand(T, 2, 4)
        d = rng.randn((T + 1) // 2, 2, 8)
        lhs = float((R.pyramid_fwd_ref(a, m) * d).sum())
        rhs = float((a * R.pyramid_bwd_ref(d.astype(np.float32), T, m.astype(np.float32)).astype(np.float64)).sum())
        assert abs(lhs - rhs) <= 1e-5 * (np.abs(a).sum() + 1)
    n_out = (R.PYRAMID_LARGE[0] + 1) // 2 * R.PYRAMID_LARGE[1] * R.PYRAMID_LARGE[2] // 2
    n_in = R.PYRAMID_LARGE[0] * R.PYRAMID_LARGE[1] * R.PYRAMID_LARGE[2] // 4
    assert (n_out, n_in) == (540672, 532480) and min(n_out, n_in) > 2048 * 256 and n_out % 256 == 0 and n_in % (2048 * 256) != 0


# ------------------------------------------------------------------------------------------------ dropout mask
# (seed, element index, p) -> keep: written down once; a change of the hash changes what a stored seed means
KEEP_TABLE = [
    (12345, 0, 0.3, True), (12345, 1, 0.3, True), (12345, 2, 0.3, True), (12345, 3, 0.3, True),
    (12345, 1027, 0.5, False), (12345, 2097159, 0.5, False), (12345, 4294967296, 0.5, True), (12345, 4294967297, 0.5, False),
    (1141982600087, 0, 0.3, False), (1141982600087, 1, 0.3, True), (1141982600087, 5, 0.5, True),
    (1141982600087, 4294967301, 0.5, True), (1141982600087, 7, 0.999, False), (1141982600087, 551, 0.999, True),
    (12345, 3157, 0.999, True), (0, 0, 0.5, False), (0, 0, 0.0, True),
]


def _keep_python(seed, idx, thresh):
    """asr_drop_keep once more, on Python integers."""
    def mix(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        x ^= x >> 16
        return x
    h = mix((idx & 0xffffffff) ^ (seed & 0xffffffff))
    h = mix((h + (idx >> 32) * 0x9e3779b9 + (seed >> 32)) & 0xffffffff)
    return h >= thresh


def test_dropout_keep_table():
    assert R.DROP_SEEDS[1] == 1141982600087 and R.DROP_SEEDS[1] > 2 ** 32
    assert [int(v) for v in R.mix32([0, 1, 0xffffffff])] == [0, 1753845952, 1734902346]
    assert [R.drop_thresh(p) for p in R.DROP_P] == [0, 1288490240, 2147483648, 4290672384]
    for seed, idx, p, keep in KEEP_TABLE:
        got = bool(R.drop_keep(seed, np.array([idx], dtype=np.uint64), R.drop_thresh(p))[0])
        assert got == keep == _keep_python(seed, idx, R.drop_thresh(p)), (seed, idx, p)


@pytest.mark.parametrize("p", R.DROP_P)
@pytest.mark.parametrize("seed", R.DROP_SEEDS)
def test_dropout_keep_rate(seed, p):
    m = R.drop_mask(seed, p, 1 << 20)
    assert abs(float(np.mean(m != 0)) - (1.0 - p)) <= 5e-3
    assert set(np.unique(m)) <= {np.float32(0.0), R.drop_scale(p)}
    idx = np.arange(1 << 12, dtype=np.uint64) + np.uint64(1 << 32)
    assert [bool(k) for k in R.drop_keep(seed, idx[:64], R.drop_thresh(0.5))] == \
        [_keep_python(seed, int(i), R.drop_thresh(0.5)) for i in idx[:64]]


# ------------------------------------------------------------------------------------------------ label log-probabilities
@pytest.mark.parametrize("V,rows", R.LOSS_CASES)
def test_label_logprob_closed_form_equals_autograd(V, rows):
    for scale in R.LOSS_SCALE:
        z, idx, dist, g = R.loss_inputs(V, rows, scale)
        for ls, with_dist in ((0.0, False), (0.1, False), (0.0, True), (0.1, True)):
            out, dz = R.label_logprob_ref(z, idx, dist if with_dist else None, ls, g, np.float32(0.7))
            zt = torch.from_numpy(z).double().requires_grad_(True)
            lp = torch.log_softmax(zt, dim=1)
            ref = lp.gather(1, torch.from_numpy(idx)[:, None])[:, 0]
            if with_dist:
                ref = (1 - ls) * ref + ls * (lp * torch.from_numpy(dist).double()).sum(1)
            ref.backward(torch.from_numpy(g).double() * float(np.float32(0.7)))
            assert np.abs(out - ref.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(out).max())
            assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dz).max())
            assert rows < 2 or {0, V - 1} <= set(idx.tolist())


@pytest.mark.parametrize("V", R.LOSS_V)
def test_planted_ties_are_exact_in_float32(V):
    z, plants = R.tie_cases(V)
    assert z.dtype == np.float32
    lanes = set()
    for r, where in enumerate(plants):
        top = z[r].max()
        assert sorted(np.nonzero(z[r] == top)[0].tolist()) == where
        assert int(np.argmax(z[r])) == where[0]
        if len(where) > 1:
            lanes.add("same" if len({v % 64 for v in where}) < len(where) else "other")
    assert any(w == [0] for w in plants) and any(w == [V - 1] for w in plants) and any(len(w) == V for w in plants)
    if V > 64:
        assert lanes == {"same", "other"}
