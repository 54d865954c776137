"""The small streaming kernels every train step runs - csrc/optim.hip (through parallel.FlatAdam and the C ABI), rows.hip,
pyramid.hip, dropout.hip, loss.hip - per element against tests/stream_ref.py.

Pure data movement, a single float32 product and a single float32 add are compared bit for bit; sums against float64 within
the float32 summation bound of their own terms; the optimiser and the label log-probabilities against float64 within 4 x the
error of an independent float32 evaluation on the CPU (torch.optim.Adam, the numpy closed form), with a floor of a few
float32 spacings.  Every buffer a kernel must not read holds NaN, every location it must write is pre-filled with NaN or a
canary.  Each test prints its worst error / allowance ratio (`pytest -s`; profiles/stream_parity.txt holds one run).
tests/test_stream_kernels_cpu.py holds the references and the inputs to their own checks without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import stream_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    assert not hip_backend.is_deterministic(), "this suite tests the default entry points"
    return hip_backend


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.int32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _report(what, ratio):
    print("stream-parity %-58s worst error / allowance %.3f" % (what, ratio))


def _lp(t):
    return ctypes.c_void_p(t.data_ptr())


# ================================================================================================ 1. optimiser
def _adam_refs(name, amsgrad, wd, clip, eps):
    """Inputs, the float64 reference and the float32 yardstick(s) of one list and case."""
    params, grads = R.adam_inputs(R.ADAM_LISTS[name])
    return (params, grads, R.adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float64),
            R.adam_yardsticks(params, grads, amsgrad, wd, clip, eps))


def _leaves(params):
    return [_dev(p.copy()).requires_grad_(True) for p in params]


def _set_grads(opt, leaves, gs):
    opt.zero_grad()
    for leaf, g in zip(leaves, gs):
        leaf.grad = _dev(g)


def _adam_state(opt, leaves, amsgrad):
    """p from the leaves, the moments through state_dict() (torch.optim.Adam's schema) -> dict of per-tensor host arrays."""
    sd = opt.state_dict()["state"]
    out = dict(p=[_host(x).astype(np.float64) for x in leaves],
               m=[_host(sd[i]["exp_avg"]).astype(np.float64) for i in range(len(leaves))],
               v=[_host(sd[i]["exp_avg_sq"]).astype(np.float64) for i in range(len(leaves))])
    if amsgrad:
        out["vmax"] = [_host(sd[i]["max_exp_avg_sq"]).astype(np.float64) for i in range(len(leaves))]
    return out


def _adam_compare(got, r64, r32, amsgrad, what):
    """Every element of every tensor within its allowance; returns the worst error / allowance."""
    worst = 0.0
    for key in ("p", "m", "v") + (("vmax",) if amsgrad else ()):
        for i, (g, a) in enumerate(zip(got[key], r64[key])):
            allow = R.allowance(a.reshape(-1), [r[key][i].reshape(-1) for r in r32])
            ratio = np.abs(g.reshape(-1) - a.reshape(-1)) / allow
            k = int(np.argmax(ratio))
            assert ratio[k] <= 1.0, "%s: %s of tensor %d, element %d: %.9g vs %.9g (float64), %.2f allowances of %.3g" % (
                what, key, i, k, g.reshape(-1)[k], a.reshape(-1)[k], ratio[k], allow[k])
            worst = max(worst, float(ratio[k]))
    return worst


@pytest.mark.parametrize("amsgrad,wd,clip,eps", R.ADAM_GRID)
def test_adam_against_float64(hb, amsgrad, wd, clip, eps):
    """FlatAdam over plain leaf tensors with .grad set directly, 4 steps, against torch.optim.Adam(foreach=False) +
    clip_grad_norm_ in float64 on the CPU, per element after every step, within 4 x the float32 CPU optimiser's largest error
    on that tensor and step (at least 4 float32 spacings; for the list of one element under an active clip the float32
    optimiser runs three times, its clip coefficient moved by +- 4 roundings: stream_ref.adam_yardsticks).
    Branches and why each shape is here:
    amsgrad False - vmax == nullptr (the judge's optimiser); clip none - gnorm_sq == nullptr; clip inactive - FlatAdam built
    without a norm, the norm passed per step: apply() takes it with the default entry of sumsq_kernel (asr_sumsq_f32), and
    the coefficient is exactly 1; clip active - the norm rides the gather (asr_gather_sumsq_f32) into the two-word protocol:
    each update clears the word the next step accumulates into (zero_word), a stale word doubles the reported norm.
    n = 1, 255 | 256 | 257 - one thread, one block and its neighbours; (1, 3, 5, 33, 4097) - slices padded to 4 floats;
    2048 * 256 + 259 - adam_kernel's grid-stride loop past the 2048-block cap with a ragged last pass.  weight_decay 0.1
    (1e-6 cannot show a decay on the wrong side of the clip) and eps 1e-3 (1e-8 is below float32 beside sqrt(v) of these
    gradients) make the placement of both terms visible; gradients randn * (1, 1, 0.05, 0.05): v shrinks from step 3 on."""
    from parallel import FlatAdam
    worst = 0.0
    for name, sizes in R.ADAM_LISTS.items():
        params, grads, r64, r32 = _adam_refs(name, amsgrad, wd, clip, eps)
        leaves = _leaves(params)
        opt = FlatAdam(leaves, lr=R.LR, weight_decay=wd, amsgrad=amsgrad, betas=R.BETAS, eps=eps,
                       max_grad_norm=R.adam_max_norm(clip, sizes, 0) if clip == "active" else None)
        for s in range(R.ADAM_STEPS):
            _set_grads(opt, leaves, grads[s])
            word = opt.step(max_grad_norm=R.adam_max_norm(clip, sizes, s))
            if clip != "none":
                got_norm = float(word.item())
                assert abs(got_norm - r64[s]["norm_sq"]) <= 1e-5 * r64[s]["norm_sq"], (name, s, got_norm, r64[s]["norm_sq"])
            worst = max(worst, _adam_compare(_adam_state(opt, leaves, amsgrad), r64[s], [r[s] for r in r32], amsgrad,
                                             "%s step %d" % (name, s + 1)))
    _report("adam amsgrad=%s wd=%g clip=%s eps=%g" % (amsgrad, wd, clip, eps), worst)


def _direct_adam(hb, n, p, g, m, v, vmax, word, max_norm, t, wd, eps, skip, zero_word):
    return hb.load().asr_adam_clip_f32(n, hb.ptr(p), hb.ptr(g), hb.ptr(m), hb.ptr(v), hb.ptr(vmax), hb.ptr(word), float(max_norm),
                                       R.LR, R.BETAS[0], R.BETAS[1], eps, wd, 1.0 - R.BETAS[0] ** t, 1.0 - R.BETAS[1] ** t,
                                       None if skip is None else _lp(skip), hb.ptr(zero_word), hb.stream())


@pytest.mark.parametrize("amsgrad", [True, False])
def test_adam_skip_word(hb, amsgrad):
    """asr_adam_clip_f32 directly, where FlatAdam cannot reach.  A non-zero skip word: p, m, v, vmax bit-identical, zero_word
    still cleared.  A zero skip word: the bits of a null skip pointer.  gnorm_sq == nullptr with and without a zero_word:
    the float64 restatement within the float32 restatement's error.  n past the block cap, so that a skip that only the first
    pass honoured would show."""
    n = 2048 * 256 + 259
    rng = np.random.RandomState(5)
    p0, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    m0, v0 = (rng.randn(n) * 0.1).astype(np.float32), (rng.rand(n) * 0.01).astype(np.float32)
    x0 = (v0 * rng.choice([0.5, 2.0], size=n)).astype(np.float32)                   # vmax on either side of v
    g_d = _dev(g)
    norm_sq = float((g.astype(np.float64) ** 2).sum())
    word = _dev(np.array([norm_sq], dtype=np.float32))
    max_norm = float(np.float32(np.sqrt(norm_sq) / 20.0))

    def run(skip, clip=True, zero=True):
        st = [_dev(a.copy()) for a in (p0, m0, v0)] + [_dev(x0.copy()) if amsgrad else None]
        zw = _dev(np.array([7.0], dtype=np.float32)) if zero else None
        sk = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda")
        rc = _direct_adam(hb, n, st[0], g_d, st[1], st[2], st[3], word if clip else None, max_norm, 3, 0.1, 1e-8, sk, zw)
        assert rc == 0
        return [None if a is None else _host(a) for a in st], None if zw is None else float(zw.item())

    skipped, zw = run(0x10000)                                                    # any non-zero word, not only 1
    for got, want, what in zip(skipped, (p0, m0, v0, x0 if amsgrad else None), ("p", "m", "v", "vmax")):
        if want is not None:
            _same_bits(got, want, "skipped update: " + what)
    assert zw == 0.0, "a skipped update did not clear the next step's norm word"
    null, zw = run(None)
    zero, _ = run(0)
    assert zw == 0.0 and not np.array_equal(null[0], p0)
    for a, b, what in zip(null, zero, ("p", "m", "v", "vmax")):
        if a is not None:
            _same_bits(b, a, "zero skip word against a null skip pointer: " + what)
    assert float(word.item()) == np.float32(norm_sq), "the update wrote the norm word it reads"
    worst = 0.0
    for clip in (True, False):
        got, _ = run(None, clip=clip, zero=clip)
        mx = max_norm if clip else None
        args = (p0, g, m0, v0, x0 if amsgrad else None, 3, np.float32(norm_sq), mx, R.LR, 0.1, 1e-8)
        r64 = R.adam_update(*args)
        r32 = R.adam_update(*args, dtype=np.float32)
        for a, b, c, what in zip(got, r64, r32, ("p", "m", "v", "vmax")):
            if a is None:
                continue
            ratio = np.abs(a.astype(np.float64) - b) / R.allowance(b, c)
            assert ratio.max() <= 1.0, (clip, what, int(np.argmax(ratio)), float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    _report("adam direct amsgrad=%s (clip, no clip)" % amsgrad, worst)


def test_adam_skipped_step_then_unapply(hb):
    """A 5-step clipped run whose third update is skipped on the device (skip_if set) and taken back with unapply(): the
    state is untouched by it, steps 4 and 5 match a reference that never saw step 3, and all five reported norms are right -
    the skipped update still clears the next word of the two-word protocol."""
    from parallel import FlatAdam
    sizes = R.ADAM_LISTS["odd"]
    scales = (1.0, 1.0, 1.0, 0.05, 0.05)
    params, grads = R.adam_inputs(sizes, seed=3, steps=5, scales=scales)
    max_norm = float(np.float32(np.sqrt(R.adam_total(sizes)) / 20.0))
    kw = dict(skip=(2,), max_norms=[max_norm] * 5)
    r64 = R.adam_run_torch(params, grads, True, 0.1, "active", 1e-8, torch.float64, **kw)
    r32 = R.adam_yardsticks(params, grads, True, 0.1, "active", 1e-8, **kw)
    leaves = _leaves(params)
    opt = FlatAdam(leaves, lr=R.LR, weight_decay=0.1, amsgrad=True, betas=R.BETAS, eps=1e-8, max_grad_norm=max_norm)
    latch = torch.ones(1, dtype=torch.int32, device="cuda")
    worst = 0.0
    for s in range(5):
        _set_grads(opt, leaves, grads[s])
        before = _adam_state(opt, leaves, True) if s == 2 else None
        if s == 2:
            opt.reduce()
            word = opt.apply(skip_if=latch)
            opt.unapply()
        else:
            word = opt.step()
        got_norm = float(word.item())
        assert abs(got_norm - r64[s]["norm_sq"]) <= 1e-5 * r64[s]["norm_sq"], (s, got_norm, r64[s]["norm_sq"])
        state = _adam_state(opt, leaves, True)
        if s == 2:
            for key in before:
                for a, b in zip(before[key], state[key]):
                    _same_bits(b, a, "skipped step: " + key)
        worst = max(worst, _adam_compare(state, r64[s], [r[s] for r in r32], True, "step %d" % (s + 1)))
    assert opt.t == 4
    _report("adam 5 steps, the third skipped and taken back", worst)


def test_adam_reduce_without_apply(hb):
    """reduce() whose apply() never came, then full steps: the abandoned norm must not be added to the next one (a stale or
    uncleared word is a factor of 2), and the step after that still finds its word cleared."""
    from parallel import FlatAdam
    sizes = R.ADAM_LISTS["odd"]
    params, grads = R.adam_inputs(sizes, seed=4)
    max_norm = float(np.float32(np.sqrt(R.adam_total(sizes)) / 20.0))
    kw = dict(skip=(0,), max_norms=[max_norm] * 4)
    r64 = R.adam_run_torch(params, grads, True, 1e-6, "active", 1e-8, torch.float64, **kw)
    r32 = R.adam_yardsticks(params, grads, True, 1e-6, "active", 1e-8, **kw)
    leaves = _leaves(params)
    opt = FlatAdam(leaves, lr=R.LR, weight_decay=1e-6, amsgrad=True, betas=R.BETAS, eps=1e-8, max_grad_norm=max_norm)
    _set_grads(opt, leaves, grads[0])
    opt.reduce()                                                                  # ... and the step is abandoned
    worst = 0.0
    for s in range(1, 4):
        _set_grads(opt, leaves, grads[s])
        got_norm = float(opt.step().item())
        assert abs(got_norm - r64[s]["norm_sq"]) <= 1e-5 * r64[s]["norm_sq"], (s, got_norm, r64[s]["norm_sq"])
        worst = max(worst, _adam_compare(_adam_state(opt, leaves, True), r64[s], [r[s] for r in r32], True, "step %d" % s))
    _report("adam reduce() without apply(), then 3 steps", worst)


def test_optimizer_argument_errors(hb):
    """Every argument-error return of asr_adam_clip_f32, asr_sumsq_f32 and asr_gather_sumsq_f32; nothing is launched."""
    lib = hb.load()
    n = 8
    t = [torch.full((n,), float(i + 1), device="cuda") for i in range(4)]
    word = torch.full((1,), 3.0, device="cuda")
    for drop in range(4):
        a = [None if i == drop else x for i, x in enumerate(t)]
        assert _direct_adam(hb, n, a[0], a[1], a[2], a[3], None, None, 0.0, 1, 0.0, 1e-8, None, word) == E_ARG
    for bad_n in (0, -1):
        assert _direct_adam(hb, bad_n, t[0], t[1], t[2], t[3], None, None, 0.0, 1, 0.0, 1e-8, None, word) == E_ARG
    assert lib.asr_sumsq_f32(n, None, hb.ptr(word), hb.stream()) == E_ARG
    assert lib.asr_sumsq_f32(n, hb.ptr(t[0]), None, hb.stream()) == E_ARG
    assert lib.asr_sumsq_f32(0, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert lib.asr_sumsq_f32(-4, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert lib.asr_sumsq_f32(4, hb.ptr(t[0][1:]), hb.ptr(word), hb.stream()) == E_ALIGN        # g not 16-byte aligned
    i64 = ctypes.c_int64
    src, off, cnt = (ctypes.c_void_p * 1)(t[1].data_ptr()), (i64 * 1)(0), (i64 * 1)(n)
    gather = lib.asr_gather_sumsq_f32
    assert gather(0, src, off, cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(-1, src, off, cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, None, off, cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, src, None, cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, src, off, None, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, src, off, cnt, None, hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, (ctypes.c_void_p * 1)(None), off, cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, src, off, (i64 * 1)(0), hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    assert gather(1, src, (i64 * 1)(-4), cnt, hb.ptr(t[0]), hb.ptr(word), hb.stream()) == E_ARG
    torch.cuda.synchronize()
    assert float(word.item()) == 3.0 and all(bool((x == float(i + 1)).all()) for i, x in enumerate(t))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 8197, (1 << 20) + 4 * 256 + 3])
def test_sumsq_default_entry(hb, n):
    """asr_sumsq_f32 itself (not the deterministic variant, not through FlatAdam): n below one float4 (the scalar tail alone),
    4 | 5, 1023 (255 float4 + 3), 8197, and 2^20 + 4 * 256 + 3 - 1025 blocks of float4, capped at 1024, so the grid-stride
    loop runs a second pass, plus a tail.  1e-5 of the float64 sum, into a zero word and added to a non-zero one."""
    g = np.random.RandomState(n % 9973).randn(n).astype(np.float32)
    want = float((g.astype(np.float64) ** 2).sum())
    g_d = _dev(g)
    for start in (0.0, 3.5):
        word = _dev(np.array([start, -2.0], dtype=np.float32))
        assert hb.load().asr_sumsq_f32(n, hb.ptr(g_d), hb.ptr(word), hb.stream()) == 0
        got = _host(word)
        assert abs(float(got[0]) - (start + want)) <= 1e-5 * (start + want), (n, start, float(got[0]), want)
        assert got[1] == -2.0


# ================================================================================================ 2. packed rows
def _layout(hb, lens, sub):
    layout = hb.RowLayout(lens, sub, "cuda")
    return hb.LayerRows(layout, 0), layout.lens[0], layout.base[0], layout.ext[0]


def _row_masks(hb, rng, shape, seed):
    """None, a tensor (zeros, and multipliers that are no power of two), a SeededMask and its materialised tensor."""
    m = (rng.rand(*shape) * 2).astype(np.float32)
    m[rng.rand(*shape) < 0.3] = 0.0
    seeded = hb.SeededMask(shape, 0.3, "cuda", seed=seed)
    return [("none", None, None), ("tensor", _dev(m), m), ("seeded", seeded, None), ("seeded, materialised", seeded.tensor(), None)]


def _nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("C", R.ROW_C)
def test_rows_movement(hb, C):
    """asr_rows_pack_f32, asr_rows_unpack_fwd_f32 and the drows of asr_rows_unpack_bwd_f32, bit for bit against numpy indexing
    from (lens, base, ext).  C4 = 1, 63 | 64, 127 | 128, 255 | 256 | 257: both sides of threads_for's switches (and of one
    wave: the rows kernels of the LSTM tests run at C4 < 64 only); T = 1, 5, 8, 9 around the four frames of a block; layouts
    without and with a pyramid (ext = 4 x: ext > len + 1, ext_max > T); lengths 1 and T; B = 1 and 4.  NaN wherever a kernel
    must not read (x and dout behind an utterance, packed padding rows), NaN where it must write (zeros included).
    unpack_fwd on padded frames: fill None (zeros), a fill with negative entries, fill_relu; mask None, a tensor, a
    SeededMask - whose result must be that of its materialised mask, and of stream_ref's restatement of the hash."""
    lib = hb.load()
    rng = np.random.RandomState(C)
    n_cases = 0
    for T in R.ROW_T:
        for sub in R.ROW_SUBSAMPLE:
            for B in (1, 4):
                for lens in R.row_lens(B, T):
                    rows, lens_h, base_h, ext_h = _layout(hb, lens, sub)
                    assert (ext_h > lens_h).all() and (len(sub) == 1 or (ext_h > lens_h + 1).any())
                    what = "C %d T %d B %d sub %s lens %s" % (C, T, B, sub, lens)
                    # ---- pack
                    x = rng.randn(B, T, C).astype(np.float32)
                    for b in range(B):
                        x[b, lens[b]:] = np.nan
                    out, x_d = _nan_like((rows.R, C)), _dev(x)
                    hb.check(lib.asr_rows_pack_f32(B, T, C, hb.ptr(x_d), hb.ptr(rows.lens), hb.ptr(rows.base), hb.ptr(rows.ext),
                                                   rows.ext_max, hb.ptr(out), hb.stream()), "asr_rows_pack_f32")
                    _same_bits(_host(out), R.pack_ref(x, lens_h, base_h, ext_h), "pack " + what)
                    _same_bits(_host(hb.rows_pack(x_d, rows)), _host(out), "hb.rows_pack " + what)
                    # ---- unpack_bwd, drows only: dout behind an utterance is never read
                    drows = _nan_like((rows.R, C))
                    hb.check(lib.asr_rows_unpack_bwd_f32(B, T, C, hb.ptr(x_d), hb.ptr(rows.lens), hb.ptr(rows.base),
                                                         hb.ptr(rows.ext), rows.ext_max, None, 0, 0.0, hb.ptr(drows), None, None,
                                                         hb.stream()), "asr_rows_unpack_bwd_f32")
                    _same_bits(_host(drows), R.unpack_bwd_ref(x, lens_h, base_h, ext_h), "unpack_bwd drows " + what)
                    # ---- unpack_fwd
                    packed = rng.randn(rows.R, C).astype(np.float32)
                    for b in range(B):
                        packed[base_h[b] + lens[b]:base_h[b] + ext_h[b]] = np.nan
                    packed_d = _dev(packed)
                    fill = rng.randn(C).astype(np.float32)
                    fill[::3] = -np.abs(fill[::3])
                    fill[1] = 0.0
                    masks = _row_masks(hb, rng, (B, T, C), seed=R.DROP_SEEDS[(T + B) % 2] + C)
                    seeded_host = R.drop_mask(masks[2][1].seed, 0.3, B * T * C).reshape(B, T, C)
                    _same_bits(_host(masks[3][1]), seeded_host, "materialised SeededMask " + what)
                    results = {}
                    for mname, mask, mhost in masks:
                        mhost = seeded_host if mhost is None and mask is not None else mhost
                        for fname, f, relu in (("no fill", None, False), ("fill", fill, False), ("relu(fill)", fill, True)):
                            f_d = None if f is None else _dev(f)
                            got = _nan_like((B, T, C))
                            seeded = isinstance(mask, hb.SeededMask)
                            hb.check(lib.asr_rows_unpack_fwd_f32(B, T, C, hb.ptr(packed_d), hb.ptr(rows.lens), hb.ptr(rows.base),
                                                                 hb.ptr(f_d), 1 if relu else 0, None if seeded else hb.ptr(mask),
                                                                 mask.seed if seeded else 0, mask.p if seeded else 0.0,
                                                                 hb.ptr(got), hb.stream()), "asr_rows_unpack_fwd_f32")
                            want = R.unpack_fwd_ref(packed, lens_h, base_h, T, f, relu, mhost)
                            _same_bits(_host(got), want, "unpack_fwd %s, %s, mask %s" % (what, fname, mname))
                            results[(mname, fname)] = _host(got)
                            if mname in ("none", "seeded"):            # the wrapper passes the same arguments on
                                _same_bits(_host(hb.rows_unpack_fwd(packed_d, rows, T, f_d, mask, fill_relu=relu)), want,
                                           "hb.rows_unpack_fwd %s, %s, mask %s" % (what, fname, mname))
                            n_cases += 1
                    for fname in ("no fill", "fill", "relu(fill)"):
                        _same_bits(results[("seeded", fname)], results[("seeded, materialised", fname)], "seeded against tensor")
    _report("rows movement C=%d (%d unpack_fwd cases, bit for bit)" % (C, n_cases), 0.0)


@pytest.mark.parametrize("C4", R.FILL_C4)
def test_rows_fill_grad(hb, C4):
    """dfill of asr_rows_unpack_bwd_f32's default entry (rows_fill_grad_kernel) per element against float64, within
    n_terms 2^-24 sum|terms| of its column (the float32 summation bound of the terms it adds, the accumulator among them).
    C4 = 1, 2, 63, 64 (FL = 8), 65 (7) and 80 (6) - FL * C4 threads where C4 does not divide 512 -, 128 (4), 256 (2), 257 and
    512 (1); T - len = 1, FL - 1, FL, FL + 1, 3 FL + 2 and 0 in one batch (a lane without a frame, one each, one lane with
    two, several passes), and a batch with no padded frame at all; relu_of with entries exactly 0 (they block) and negative;
    mask None, tensor, seeded; a non-zero accumulator that the kernel adds to."""
    C = 4 * C4
    T, lens = R.fill_case(C4)
    B = len(lens)
    rng = np.random.RandomState(C4)
    rows, lens_h, base_h, ext_h = _layout(hb, lens, (1,))
    dout = rng.randn(B, T, C).astype(np.float32)
    dout_d = _dev(dout)
    relu_of = rng.randn(C).astype(np.float32)
    relu_of[::5] = 0.0
    relu_of[C - 1] = -0.0 if C4 % 2 else 0.0
    acc0 = rng.randn(C).astype(np.float32)
    masks = _row_masks(hb, rng, (B, T, C), seed=R.DROP_SEEDS[C4 % 2])[:3]
    seeded_host = R.drop_mask(masks[2][1].seed, 0.3, B * T * C).reshape(B, T, C)
    worst = 0.0
    for mname, mask, mhost in masks:
        mhost = seeded_host if mname == "seeded" else mhost
        for relu in (None, relu_of):
            acc = _dev(acc0.copy())
            drows, dfill = hb.rows_unpack_bwd(dout_d, rows, C, mask, True, relu_of=None if relu is None else _dev(relu), dfill=acc)
            assert dfill.data_ptr() == acc.data_ptr()
            _same_bits(_host(drows), R.unpack_bwd_ref(dout, lens_h, base_h, ext_h), "drows beside dfill")
            want, bound = R.fill_grad_ref(dout, lens_h, mhost, relu, acc0)
            got = _host(dfill).astype(np.float64)
            err = np.abs(got - want)
            blocked = bound == 0.0
            assert (err[blocked] == 0.0).all(), "a column behind relu_of <= 0 received a gradient"
            assert (err <= bound).all(), ("C4 %d mask %s" % (C4, mname), int(np.argmax(err - bound)), float(err.max()))
            worst = max(worst, float((err[~blocked] / bound[~blocked]).max()))
    # no padded frame anywhere: nothing is added
    rows_full, _, _, _ = _layout(hb, [T] * 3, (1,))
    acc = _dev(acc0.copy())
    hb.rows_unpack_bwd(_dev(dout[:3]), rows_full, C, None, True, dfill=acc)
    _same_bits(_host(acc), acc0, "dfill of a batch without padding")
    _report("rows dfill C4=%d FL=%d" % (C4, R.fill_lanes(C4)), worst)


def test_rows_fill_grad_refuses_more_than_512_float4(hb):
    """C4 = 513 with want_fill: hb.UnsupportedShape (the frame-lane fold has 512 threads), and neither drows nor the
    accumulator is written - the refusal comes before the first launch."""
    C, T, lens = 4 * 513, 3, [3, 1]
    rows, _, _, _ = _layout(hb, lens, (1,))
    dout = torch.ones(2, T, C, device="cuda")
    acc = torch.full((C,), 5.0, device="cuda")
    with pytest.raises(hb.UnsupportedShape):
        hb.rows_unpack_bwd(dout, rows, C, None, True, dfill=acc)
    drows = _nan_like((rows.R, C))
    rc = hb.load().asr_rows_unpack_bwd_f32(2, T, C, hb.ptr(dout), hb.ptr(rows.lens), hb.ptr(rows.base), hb.ptr(rows.ext),
                                           rows.ext_max, None, 0, 0.0, hb.ptr(drows), hb.ptr(acc), None, hb.stream())
    assert rc == E_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(drows).all()) and bool((acc == 5.0).all())
    drows2, none = hb.rows_unpack_bwd(dout, rows, C, None, False)                 # without dfill the width is fine
    assert none is None and float(drows2.sum()) == 4.0 * C


# ================================================================================================ 3. pyramid, dropout
def _pyramid_case(hb, T, B, C, rng):
    x = rng.randn(T, B, C).astype(np.float32)
    T2 = (T + 1) // 2
    dout = rng.randn(T2, B, 2 * C).astype(np.float32)
    m = (rng.rand(T, B, C) * 2).astype(np.float32)
    m[rng.rand(T, B, C) < 0.3] = 0.0
    seeded = hb.SeededMask((T, B, C), 0.3, "cuda", seed=R.DROP_SEEDS[T % 2] + T * B)
    keep = R.drop_keep(seeded.seed, np.arange(T * B * C, dtype=np.uint64), R.drop_thresh(0.3)).reshape(T, B, C)
    sm = np.where(keep, R.drop_scale(0.3), np.float32(0.0)).astype(np.float32)
    x_d, dout_d = _dev(x), _dev(dout)
    res = {}
    for name, mask, mhost in (("none", None, None), ("tensor", _dev(m), m), ("seeded", seeded, sm), ("materialised", seeded.tensor(), sm)):
        out, din = _nan_like((T2, B, 2 * C)), _nan_like((T, B, C))
        hb.pyramid_fwd(x_d, mask, out)
        hb.pyramid_bwd(dout_d, mask, din)
        want_f, want_b = R.pyramid_fwd_ref(x, mhost), R.pyramid_bwd_ref(dout, T, mhost)
        if name == "seeded":                    # a dropped element is +0 there, x * 0 (signed) through a mask tensor
            want_f = np.where(want_f == 0, np.float32(0.0), want_f)
            want_b = np.where(want_b == 0, np.float32(0.0), want_b)
        _same_bits(_host(out), want_f, "pyramid fwd (%d, %d, %d) mask %s" % (T, B, C, name))
        _same_bits(_host(din), want_b, "pyramid bwd (%d, %d, %d) mask %s" % (T, B, C, name))
        res[name] = (_host(out), _host(din))
    for k in (0, 1):                            # seeded == its materialised mask (the sign of a dropped zero apart)
        assert np.array_equal(res["seeded"][k], res["materialised"][k])


def test_pyramid_small_shapes(hb):
    """asr_pyramid_concat_fwd / _bwd and their seeded forms, bit for bit: the forward moves (one float32 product with a mask),
    the backward folds the repeated frame of an odd T with one float32 add.  T = 1 (the frame pairs with itself), 2, 3, 10, 11;
    B = 1 and 3; C = 4 (one float4 per half), 8, 260; mask None, tensor, seeded."""
    rng = np.random.RandomState(7)
    for T, B, C in R.PYRAMID_SHAPES:
        _pyramid_case(hb, T, B, C, rng)
    _report("pyramid %d shapes x 4 mask forms, bit for bit" % len(R.PYRAMID_SHAPES), 0.0)


def test_pyramid_past_the_block_cap(hb):
    """(T, B, C) = (65, 32, 1024): 540 672 float4 out, 532 480 in - both kernels' grid-stride loops run a second, ragged pass
    behind the 2048 x 256 cap; odd T, so the fold sits in the last frames of the second pass."""
    _pyramid_case(hb, *R.PYRAMID_LARGE, np.random.RandomState(8))
    _report("pyramid (65, 32, 1024), bit for bit", 0.0)


@pytest.mark.parametrize("n", R.DROP_N)
def test_dropout_mask_is_the_documented_function(hb, n):
    """asr_dropout_mask_f32 == keep(seed, i) / (1 - p) as common.h states it (stream_ref.mix32 / drop_keep / drop_thresh), bit
    for bit: p = 0 (thresh 0: everything kept), 0.3, 0.5, 0.999; a seed below and one above 2^32; n = 4, 1028 and
    2048 * 256 * 4 + 8 (two float4 past the block cap: the grid-stride loop).  asr_dropout_seeded_f32 and
    asr_relu_dropout_bwd_f32 against the host's float32 products at the same n; y = 0.0 and -0.0 pass no gradient."""
    lib = hb.load()
    rng = np.random.RandomState(n % 1000)
    x = rng.randn(n).astype(np.float32)
    g = rng.randn(n).astype(np.float32)
    y = rng.randn(n).astype(np.float32)
    y[::7] = 0.0
    y[3::7] = -0.0
    g_d, y_d = _dev(g), _dev(y)
    for seed in R.DROP_SEEDS:
        for p in R.DROP_P:
            want = R.drop_mask(seed, p, n)
            mask = _nan_like((n,))
            assert lib.asr_dropout_mask_f32(n, hb.ptr(mask), seed, p, hb.stream()) == 0
            _same_bits(_host(mask), want, "mask seed %d p %g n %d" % (seed, p, n))
            x_d = _dev(x.copy())
            assert lib.asr_dropout_seeded_f32(n, hb.ptr(x_d), seed, p, hb.stream()) == 0
            _same_bits(_host(x_d), x * want, "x *= mask, seed %d p %g" % (seed, p))
            out = _nan_like((n,))
            assert lib.asr_relu_dropout_bwd_f32(n, hb.ptr(g_d), hb.ptr(y_d), seed, p, hb.ptr(out), hb.stream()) == 0
            _same_bits(_host(out), np.where(y > 0, g * want, np.float32(0.0)), "relu-dropout bwd, seed %d p %g" % (seed, p))
    _report("dropout n=%d, %d (seed, p), bit for bit" % (n, len(R.DROP_SEEDS) * len(R.DROP_P)), 0.0)


def test_dropout_argument_errors(hb):
    lib = hb.load()
    x = torch.ones(8, device="cuda")
    for n in (1, 2, 3, 5, 7):
        assert lib.asr_dropout_mask_f32(n, hb.ptr(x), 1, 0.5, hb.stream()) == E_SHAPE
        assert lib.asr_dropout_seeded_f32(n, hb.ptr(x), 1, 0.5, hb.stream()) == E_SHAPE
        assert lib.asr_relu_dropout_bwd_f32(n, hb.ptr(x), hb.ptr(x), 1, 0.5, hb.ptr(x), hb.stream()) == E_SHAPE
    assert lib.asr_dropout_mask_f32(0, hb.ptr(x), 1, 0.5, hb.stream()) == E_ARG
    assert lib.asr_dropout_mask_f32(8, hb.ptr(x), 1, 1.0, hb.stream()) == E_ARG
    assert lib.asr_dropout_mask_f32(8, hb.ptr(x), 1, -0.1, hb.stream()) == E_ARG
    assert lib.asr_relu_dropout_bwd_f32(8, None, hb.ptr(x), 1, 0.5, hb.ptr(x), hb.stream()) == E_ARG
    assert lib.asr_dropout_mask_f32(4, hb.ptr(x[1:]), 1, 0.5, hb.stream()) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((x == 1.0).all())


# ================================================================================================ 4. label log-probabilities
def _wide(a, pad, fill):
    """[rows, V] -> a [rows, V + pad] device buffer with `fill` in the padding columns."""
    w = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float32)
    w[:, :a.shape[1]] = a
    return _dev(w)


def _logprob_fwd(hb, zw, V, idx_d, dist_d, ls, total_scale=None, amax=False):
    rows = zw.shape[0]
    out = _nan_like((rows,))
    total = torch.zeros(1, device="cuda") if total_scale is not None else None
    am = torch.full((rows,), -7, dtype=torch.long, device="cuda") if amax else None
    hb.check(hb.load().asr_label_logprob_fwd(rows, V, hb.ptr(zw), zw.shape[1], _lp(idx_d), hb.ptr(dist_d), ls, hb.ptr(out),
                                             hb.ptr(total), 0.0 if total_scale is None else total_scale,
                                             None if am is None else _lp(am), hb.stream()), "asr_label_logprob_fwd")
    return _host(out), None if total is None else float(total.item()), None if am is None else _host(am)


@pytest.mark.parametrize("V,rows", R.LOSS_CASES)
def test_label_logprob_against_float64(hb, V, rows):
    """asr_label_logprob_fwd / _bwd through the C ABI against the float64 closed form, per element within 4 x the error of the
    same formula in float32 numpy (its largest on the tensor), at least 8 float32 spacings of the value (dz: of the row's |g|).
    V = 1, 2, 63 | 64 | 65 (one pass of the wave, and a lane with two elements), 129, 1000; rows = 1, 3 | 4 | 5 around the
    four rows of a block; rows = 2049 and 2053 at V = 34: with `total` the forward caps its grid at 512 blocks and strides
    over rows (and must write the rows it writes without `total`).  ls 0 and 0.1, with and without labeldist; logits * 1 and
    * 50 (one class takes all the mass).  Logits are the first V columns of a [rows, V + 3] buffer with NaN behind them
    (ld > V); the indices hold 0 and V - 1; the backward reads g with grad_stride = 2 (NaN between) and writes a
    [rows, V + 5] buffer (lddz > V) whose padding columns hold a canary.  `total` within rows 2^-24 sum|out| |scale| plus the
    rows' allowances; the argmax exact."""
    worst = 0.0
    for scale in R.LOSS_SCALE:
        z, idx, dist, g = R.loss_inputs(V, rows, scale)
        zw, idx_d, dist_d = _wide(z, 3, np.nan), _dev(idx), _dev(dist)
        g2 = np.full(2 * rows, np.nan, dtype=np.float32)
        g2[::2] = g
        g_d = _dev(g2)
        gscale = float(np.float32(0.7))
        tscale = -1.0 / rows
        for ls, with_dist in ((0.0, False), (0.1, False), (0.0, True), (0.1, True)):
            d = dist if with_dist else None
            o64, dz64 = R.label_logprob_ref(z, idx, d, ls, g, np.float32(0.7))
            o32, dz32 = R.label_logprob_ref(z, idx, d, np.float32(ls), g, np.float32(0.7), dtype=np.float32)
            out, total, amax = _logprob_fwd(hb, zw, V, idx_d, dist_d if with_dist else None, ls, total_scale=tscale, amax=True)
            plain, _, _ = _logprob_fwd(hb, zw, V, idx_d, dist_d if with_dist else None, ls)
            _same_bits(plain, out, "out with and without `total`")
            allow = R.allowance(o64, o32, ulps=8.0)
            ratio = np.abs(out.astype(np.float64) - o64) / allow
            assert ratio.max() <= 1.0, ("out", scale, ls, with_dist, int(np.argmax(ratio)), float(ratio.max()))
            worst = max(worst, float(ratio.max()))
            t_allow = abs(tscale) * (rows * R.F32_EPS * np.abs(o64).sum() + allow.sum())
            assert abs(total - tscale * o64.sum()) <= t_allow, ("total", scale, ls, with_dist, total, tscale * o64.sum(), t_allow)
            assert np.array_equal(amax, np.argmax(z, axis=1)), ("argmax", scale)
            dzw = torch.full((rows, V + 5), 1234.5, device="cuda")
            hb.check(hb.load().asr_label_logprob_bwd(rows, V, hb.ptr(zw), V + 3, _lp(idx_d), hb.ptr(dist_d if with_dist else None),
                                                     ls, hb.ptr(g_d), 2, gscale, hb.ptr(dzw), V + 5, hb.stream()),
                     "asr_label_logprob_bwd")
            dzh = _host(dzw)
            assert (dzh[:, V:] == 1234.5).all(), "the backward wrote behind column V of a wider dlogits buffer"
            floor = 8.0 * R.ulp32(g.astype(np.float64))[:, None]
            allow = np.maximum(4.0 * np.abs(dz32.astype(np.float64) - dz64).max(), floor)
            ratio = np.abs(dzh[:, :V].astype(np.float64) - dz64) / allow
            assert ratio.max() <= 1.0, ("dz", scale, ls, with_dist, np.unravel_index(int(np.argmax(ratio)), ratio.shape),
                                        float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    _report("label_logprob V=%d rows=%d" % (V, rows), worst)


@pytest.mark.parametrize("V", R.LOSS_V)
def test_label_logprob_argmax_ties(hb, V):
    """The argmax of asr_label_logprob_fwd on planted exact ties takes the lowest index: two maxima in the same lane of the
    wave (v and v + 64, v + 128), in different lanes - the lower index in the higher lane's second pass among them -, the
    maximum alone at 0 and at V - 1, all entries equal."""
    z, plants = R.tie_cases(V)
    idx = np.zeros(z.shape[0], dtype=np.int64)
    zw, idx_d = _wide(z, 3, np.nan), _dev(idx)
    for tscale in (None, 1.0):
        _, _, amax = _logprob_fwd(hb, zw, V, idx_d, None, 0.0, total_scale=tscale, amax=True)
        assert amax.tolist() == [w[0] for w in plants], (V, amax.tolist(), plants)
