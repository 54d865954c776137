"""Plain restatements of the small streaming kernels every train step runs (csrc/optim.hip, rows.hip, pyramid.hip,
dropout.hip, loss.hip), and the inputs of tests/test_stream_kernels_{cpu,gpu}.py.  numpy only (torch where the case builder
of the optimiser asks the independent reference, torch.optim.Adam, for its answer); nothing here needs a GPU.

The optimiser grid, the row / pyramid shapes, the dropout (seed, p, n) triples and the label log-probability cases are
tables of this module, so that the CPU test can hold the inputs to what the GPU test relies on (mutations of the update are
visible, planted ties are ties) without a GPU."""
import numpy as np

F32_EPS = 2.0 ** -24          # unit roundoff of float32


def ulp32(x):
    """The spacing of float32 at |x| (x float64), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ optimiser
# the betas as the C ABI carries them (floats): the reference gets the values the kernel multiplies by
BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))
LR = 1e-3
ADAM_STEPS = 4
GRAD_SCALE = (1.0, 1.0, 0.05, 0.05)                  # s_t: from step 3 on v shrinks, the amsgrad maximum carries the update
ADAM_LISTS = {                                       # parameter lists by the sizes of their tensors
    "n1": (1,),
    "n255": (255,),
    "n256": (256,),                                  # one full block of adam_kernel
    "n257": (257,),
    "odd": (1, 3, 5, 33, 4097),                      # every slice of the flat buffer padded to 4 floats
    "stride": (2048 * 256 + 259,),                   # past the 2048-block cap: a grid-stride pass and a ragged last one
}
ADAM_GRID = [(ams, wd, clip, eps) for ams in (True, False) for wd in (0.0, 1e-6, 0.1) for clip in ("none", "inactive", "active")
             for eps in (1e-8, 1e-3)]
MUTATIONS = ("eps_in_sqrt", "no_bias2", "wd_before_clip", "wd_decoupled", "no_amsgrad_max", "clip_from_norm_sq")


def adam_total(sizes):
    return int(sum(sizes))


def adam_max_norm(clip, sizes, step):
    """max_norm of step `step` (0-based).  The gradients are randn * s_t, their norm about s_t sqrt(n): `inactive` sits far
    above every norm (the coefficient is exactly 1), `active` at a twentieth of the expected one."""
    n = adam_total(sizes)
    if clip == "none":
        return None
    if clip == "inactive":
        return 8.0 * np.sqrt(n) + 8.0
    return float(np.float32(GRAD_SCALE[step] * np.sqrt(n) / 20.0))


def adam_inputs(sizes, seed=0, steps=ADAM_STEPS, scales=GRAD_SCALE):
    """-> params [tensor], grads [step][tensor], float32.  Parameters are randn; every tensor at an odd place of its list is
    scaled to 1e-4 as a whole and so is the last tensor of a list of several, every fourth element of the others: |p| smaller
    than one update (lr = 1e-3), where a relative error of the update is an absolute error of p."""
    rng = np.random.RandomState(1000 + seed + 7 * adam_total(sizes) % 9973)
    params = []
    for i, n in enumerate(sizes):
        p = rng.randn(n).astype(np.float32)
        if i % 2 == 1 or (len(sizes) > 1 and i == len(sizes) - 1):
            p *= np.float32(1e-4)
        else:
            p[1::4] *= np.float32(1e-4)
        params.append(p)
    grads = [[(rng.randn(n) * scales[t]).astype(np.float32) for n in sizes] for t in range(steps)]
    return params, grads


def adam_update(p, g, m, v, vmax, t, norm_sq, max_norm, lr, wd, eps, betas=BETAS, dtype=np.float64, mutation=None):
    """One clip_grad_norm_ + torch.optim.Adam step on flat arrays, restated (t = 1, 2, ...; vmax None: no amsgrad; max_norm
    None: no clip; norm_sq: the sum of squares of ALL gradients of the step).  Returns p, m, v, vmax.  mutation: one of
    MUTATIONS - the same update with one term in the wrong place (what the test grid has to be able to see)."""
    f = dtype
    b1, b2 = f(betas[0]), f(betas[1])
    one = f(1.0)
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    coef = one
    if max_norm is not None:
        nrm = f(norm_sq) if mutation == "clip_from_norm_sq" else np.sqrt(f(norm_sq))
        coef = np.minimum(one, f(max_norm) / (nrm + f(1e-6)))
    wd = f(wd)
    if mutation == "wd_before_clip":
        g = (g + wd * p) * coef
    elif mutation == "wd_decoupled":
        g = g * coef
        p = p - f(lr) * wd * p
    else:
        g = g * coef + wd * p
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    vv = v
    if vmax is not None:
        vmax = v.copy() if mutation == "no_amsgrad_max" else np.maximum(np.asarray(vmax, dtype=f), v)
        vv = vmax
    c1 = one - f(betas[0] ** t)
    c2 = one if mutation == "no_bias2" else one - f(betas[1] ** t)
    if mutation == "eps_in_sqrt":
        denom = np.sqrt(vv / c2 + f(eps))
    else:
        denom = np.sqrt(vv) / np.sqrt(c2) + f(eps)
    p = p - (f(lr) / c1) * m / denom
    return p, m, v, vmax


def adam_run_np(params, grads, amsgrad, wd, clip, eps, dtype=np.float64, mutation=None, skip=(), max_norms=None):
    """The restatement over all steps on the concatenated list -> [step] dict(p, m, v, vmax, norm_sq) (flat arrays).
    skip: steps whose update does not happen (their norm is still reported); max_norms: one per step instead of the grid's."""
    sizes = [len(p) for p in params]
    p = np.concatenate(params).astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    vmax = np.zeros_like(p) if amsgrad else None
    out, t = [], 0
    for s, gs in enumerate(grads):
        g = np.concatenate(gs).astype(dtype)
        norm_sq = float(np.sum(g.astype(np.float64) ** 2))
        if s not in skip:
            t += 1
            mx = adam_max_norm(clip, sizes, s) if max_norms is None else max_norms[s]
            p, m, v, vmax = adam_update(p, g, m, v, vmax, t, dtype(norm_sq), mx, LR, wd, eps,
                                        dtype=dtype, mutation=mutation)
        out.append(dict(p=p.copy(), m=m.copy(), v=v.copy(), vmax=None if vmax is None else vmax.copy(), norm_sq=norm_sq))
    return out


def adam_run_torch(params, grads, amsgrad, wd, clip, eps, dtype, skip=(), max_norms=None):
    """The independent reference: torch.optim.Adam(foreach=False) + clip_grad_norm_ on the CPU in `dtype`, fed the same
    float32 gradients -> [step] dict(p, m, v, vmax, norm_sq) with one array per tensor of the list."""
    import torch
    sizes = [len(p) for p in params]
    ps = [torch.from_numpy(p.copy()).to(dtype).requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=eps, weight_decay=wd, amsgrad=amsgrad, foreach=False)
    out = []
    for s, gs in enumerate(grads):
        norm_sq = float(sum(float((torch.from_numpy(g).double() ** 2).sum()) for g in gs))
        if s not in skip:
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy()).to(dtype)
            mx = adam_max_norm(clip, sizes, s) if max_norms is None else max_norms[s]
            if mx is not None:
                torch.nn.utils.clip_grad_norm_(ps, mx, foreach=False)
            opt.step()
        st = [opt.state[p] for p in ps]
        done = all(len(e) > 0 for e in st)
        zero = [np.zeros(n) for n in sizes]
        out.append(dict(p=[p.detach().double().numpy().copy() for p in ps],
                        m=[e["exp_avg"].double().numpy().copy() for e in st] if done else zero,
                        v=[e["exp_avg_sq"].double().numpy().copy() for e in st] if done else zero,
                        vmax=([e["max_exp_avg_sq"].double().numpy().copy() for e in st] if done else zero) if amsgrad else None,
                        norm_sq=norm_sq))
    return out


CLIP_COEF_ROUNDINGS = 4       # sum of squares, square root, + 1e-6, divide: each rounds the clip coefficient once


def adam_yardsticks(params, grads, amsgrad, wd, clip, eps, skip=(), max_norms=None):
    """The float32 CPU optimiser as the yardstick of rounding -> a list of runs: one.  Only for a list of ONE element under an
    active clip there are three: as it is, and with max_norm - that is, the clip coefficient - moved by +- CLIP_COEF_ROUNDINGS
    2^-24.  The norm of one element is |g|: torch gets it without any rounding, where a kernel squares, takes the root, adds
    1e-6 and divides in float32, so the plain run omits the coefficient's last bits altogether (adam_run_kernel_order, the
    kernel's operation order on the CPU, sits several allowances out in exp_avg without them: test_stream_kernels_cpu.py).
    From 255 elements on torch's norm rounds like anyone's sum and the plain run is the yardstick as it stands."""
    import torch
    sizes = [len(p) for p in params]
    steps = range(len(grads))
    base = [adam_max_norm(clip, sizes, s) for s in steps] if max_norms is None else list(max_norms)
    runs = [adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float32, skip=skip, max_norms=base)]
    if clip == "active" and adam_total(sizes) == 1:
        for sign in (1.0, -1.0):
            moved = [mx * (1.0 + sign * CLIP_COEF_ROUNDINGS * F32_EPS) for mx in base]
            runs.append(adam_run_torch(params, grads, amsgrad, wd, clip, eps, torch.float32, skip=skip, max_norms=moved))
    return runs


def adam_run_kernel_order(params, grads, amsgrad, wd, clip, eps):
    """adam_kernel's own operation order (csrc/optim.hip: adam_one) in float32 numpy, without fused multiply-adds and with the
    norm summed in one piece -> [step] dict(p, m, v, vmax) flat.  Not a reference: a stand-in for the kernel that shows,
    without a GPU, whether correct float32 arithmetic in another order fits the allowances."""
    f = np.float32
    sizes = [len(p) for p in params]
    p = np.concatenate(params).astype(f)
    m, v, vmax = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    b1, b2 = f(BETAS[0]), f(BETAS[1])
    out = []
    for s, gs in enumerate(grads):
        t = s + 1
        g = np.concatenate(gs).astype(f)
        mx = adam_max_norm(clip, sizes, s)
        coef = f(1.0)
        if mx is not None:
            coef = min(f(1.0), f(mx) / (np.sqrt(np.sum(g * g, dtype=f)) + f(1e-6)))
        lr_c1 = f(LR) / f(1.0 - BETAS[0] ** t)
        rs_c2 = f(1.0) / np.sqrt(f(1.0 - BETAS[1] ** t))
        g = g * coef + f(wd) * p
        m = b1 * m + (f(1.0) - b1) * g
        v = b2 * v + (f(1.0) - b2) * g * g
        vv = v
        if amsgrad:
            vmax = np.maximum(vmax, v)
            vv = vmax
        p = p - lr_c1 * m / (np.sqrt(vv) * rs_c2 + f(eps))
        out.append(dict(p=p.copy(), m=m.copy(), v=v.copy(), vmax=vmax.copy() if amsgrad else None))
    return out


def allowance(ref64, ref32, factor=4.0, ulps=4.0):
    """Per element: factor x the float32 reference's largest error against float64 on this tensor (ref32: one array, or a list
    of them - the largest over the list), at least `ulps` float32 spacings of the float64 value."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    runs = ref32 if isinstance(ref32, (list, tuple)) else [ref32]
    worst = max(float(np.max(np.abs(np.asarray(r, dtype=np.float64) - ref64))) for r in runs) if ref64.size else 0.0
    return np.maximum(factor * worst, ulps * ulp32(ref64))


def split(flat, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(flat[o:o + n])
        o += n
    return out


# ------------------------------------------------------------------------------------------------ packed rows
ROW_C = (4, 252, 256, 508, 512, 1020, 1024, 1028)    # C4 = 1 | 63 64 | 127 128 | 255 256 257: threads_for's switches
ROW_T = (1, 5, 8, 9)                                  # blocks of four frames: one partial, 4 + 1, two whole, 8 + 1
ROW_SUBSAMPLE = ((1,), (2, 2))                        # without / with a pyramid above layer 0 (ext = 4 x, > len + 1)
FILL_C4 = (1, 2, 63, 64, 65, 80, 128, 256, 257, 512)


def row_lens(B, T):
    """Lengths of a batch: T and 1 among them."""
    if B == 1:
        return [[T], [1]]
    return [[T, 1, max(1, T // 2), max(1, T - 1)][:B]]


def fill_lanes(C4):
    return min(8, 512 // C4)


def fill_case(C4):
    """-> T, lens: T - len takes 1, FL - 1, FL, FL + 1, 3 FL + 2 and 0 within one batch."""
    FL = fill_lanes(C4)
    T = 3 * FL + 4
    return T, [T - d for d in (1, FL - 1, FL, FL + 1, 3 * FL + 2, 0)]


def pack_ref(x, lens, base, ext):
    """x [B, T, C] -> rows [R, C]: zeros on every padding row."""
    B, T, C = x.shape
    out = np.zeros((int(np.sum(ext)), C), dtype=x.dtype)
    for b in range(B):
        n = min(int(lens[b]), T)
        out[base[b]:base[b] + n] = x[b, :n]
    return out


def unpack_fwd_ref(rows, lens, base, T, fill, fill_relu, mask):
    """rows [R, C] -> [B, T, C] float32; padded frames = (relu)(fill) * mask, one float32 product."""
    B, C = len(lens), rows.shape[1]
    f = np.zeros(C, dtype=np.float32) if fill is None else fill.astype(np.float32)
    if fill_relu:
        f = np.maximum(f, np.float32(0.0))
    out = np.empty((B, T, C), dtype=np.float32)
    for b in range(B):
        n = int(lens[b])
        out[b, :n] = rows[base[b]:base[b] + n]
        pad = np.broadcast_to(f, (T - n, C))
        out[b, n:] = pad if mask is None else pad * mask[b, n:]
    return out


def unpack_bwd_ref(dout, lens, base, ext):
    return pack_ref(dout, lens, base, ext)


def fill_grad_ref(dout, lens, mask, relu_of, acc0):
    """-> (dfill float64 [C], bound [C]): acc0 + the sum over padded frames of dout * mask where relu_of > 0 (acc0 elsewhere);
    bound = n_terms 2^-24 sum|terms|, the terms being the products and the accumulator: every float32 product and every add
    of the chain rounds once."""
    B, T, C = dout.shape
    tot = np.asarray(acc0, dtype=np.float64).copy()
    mag = np.abs(tot)
    n_terms = 1
    for b in range(B):
        n = int(lens[b])
        if n >= T:
            continue
        t = dout[b, n:].astype(np.float64)
        if mask is not None:
            t = t * mask[b, n:].astype(np.float64)
        tot += t.sum(0)
        mag += np.abs(t).sum(0)
        n_terms += T - n
    bound = n_terms * F32_EPS * mag
    if relu_of is not None:
        blocked = ~(relu_of > 0)
        tot[blocked] = np.asarray(acc0, dtype=np.float64)[blocked]
        bound[blocked] = 0.0
    return tot, bound


# ------------------------------------------------------------------------------------------------ pyramid
PYRAMID_SHAPES = [(T, B, C) for T in (1, 2, 3, 10, 11) for B in (1, 3) for C in (4, 8, 260)]
PYRAMID_LARGE = (65, 32, 1024)        # 33 * 32 * 512 = 540 672 and 65 * 32 * 256 = 532 480 float4: both past 2048 * 256


def pyramid_fwd_ref(x, mask):
    """x [T, B, C] (* mask, input-shaped) -> [ceil(T / 2), B, 2 C]; an odd T repeats its last frame."""
    T = x.shape[0]
    xm = x if mask is None else x * mask
    even, odd = np.arange(0, T, 2), np.minimum(np.arange(1, T + 1, 2), T - 1)
    return np.concatenate([xm[even], xm[odd]], axis=2)


def pyramid_bwd_ref(dout, T, mask):
    """The adjoint in float32: the repeated frame's gradient is one float32 add into din[T - 1], the mask one multiply."""
    T2, B, C2 = dout.shape
    C = C2 // 2
    din = np.empty((T, B, C), dtype=np.float32)
    din[0::2] = dout[:, :, :C][:(T + 1) // 2]
    din[1::2] = dout[:, :, C:][:T // 2]
    if T % 2:
        din[T - 1] = din[T - 1] + dout[T2 - 1, :, C:]
    return din if mask is None else din * mask


# ------------------------------------------------------------------------------------------------ dropout mask
DROP_P = (0.0, 0.3, 0.5, 0.999)
DROP_SEEDS = (12345, (1 << 40) + 0x9e3779b97)         # the second one above 2^32: its high word enters the second round
DROP_N = (4, 1028, 2048 * 256 * 4 + 8)                 # one float4; two blocks; past the 2048-block cap with a ragged pass


def mix32(x):
    """asr_mix32 (common.h) on uint32 arrays: wrapping arithmetic."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def drop_thresh(p):
    """asr_drop_thresh: p (as float32) * 2^32, truncated, saturating."""
    t = float(np.float32(p)) * 4294967296.0
    return 0 if t <= 0.0 else (4294967295 if t >= 4294967295.0 else int(t))


def drop_keep(seed, idx, thresh):
    """asr_drop_keep on an array of 64-bit element indices."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & 0xffffffffffffffff
    with np.errstate(over="ignore"):
        h = mix32((idx & np.uint64(0xffffffff)).astype(np.uint32) ^ np.uint32(seed & 0xffffffff))
        h = mix32(h + (idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9e3779b9) + np.uint32(seed >> 32))
    return h >= np.uint32(thresh)


def drop_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_mask(seed, p, n, first=0):
    """mask(i) = keep(seed, i) / (1 - p) for i = first .. first + n - 1, float32 (asr_dropout_mask_f32)."""
    thresh = drop_thresh(p)
    idx = np.arange(first, first + n, dtype=np.uint64)
    if thresh == 0:
        return np.full(n, drop_scale(p), dtype=np.float32)
    return np.where(drop_keep(seed, idx, thresh), drop_scale(p), np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ label log-probabilities
LOSS_V = (1, 2, 63, 64, 65, 129, 1000)
LOSS_ROWS = (1, 3, 4, 5)
LOSS_STRIDE_ROWS = (2049, 2053)       # more than 512 blocks of four rows: the forward with `total` strides over rows
LOSS_STRIDE_V = 34
LOSS_LS = (0.0, 0.1)
LOSS_SCALE = (1.0, 50.0)
LOSS_CASES = ([(V, rows) for V in LOSS_V for rows in LOSS_ROWS] + [(LOSS_STRIDE_V, rows) for rows in LOSS_STRIDE_ROWS])


def loss_inputs(V, rows, scale):
    """-> z float32 [rows, V], idx int64 [rows] (0 and V - 1 among them), dist float32 [V], g float32 [rows]."""
    rng = np.random.RandomState(31 * V + rows + int(scale))
    z = (rng.randn(rows, V) * scale).astype(np.float32)
    idx = rng.randint(0, V, size=rows).astype(np.int64)
    idx[0] = 0
    idx[-1] = V - 1
    if rows > 2:
        idx[1] = V - 1
        idx[2] = 0
    dist = rng.rand(V).astype(np.float32)
    dist = (dist / dist.sum()).astype(np.float32)
    g = rng.randn(rows).astype(np.float32)
    return z, idx, dist, g


def label_logprob_ref(z, idx, dist, ls, g, gscale, dtype=np.float64):
    """out[r] = (1 - ls) logp[r][idx[r]] + ls sum_v dist_v logp[r][v] (dist None: logp[r][idx[r]]) and its gradient for an
    upstream gscale * g[r], by the closed form, in `dtype`."""
    f = dtype
    z = z.astype(f)
    rows = np.arange(z.shape[0])
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(axis=1, keepdims=True, dtype=f)
    lse = (mx + np.log(se))[:, 0]
    lp = z[rows, idx] - lse
    prob = e / se
    gr = (f(gscale) * g.astype(f))[:, None]
    onehot = np.zeros_like(z)
    onehot[rows, idx] = f(1.0)
    if dist is None:
        return lp.astype(f), (gr * (onehot - prob)).astype(f)
    d = dist.astype(f)
    ls = f(ls)
    sd = d.sum(dtype=f)
    out = (f(1.0) - ls) * lp + ls * ((z * d).sum(axis=1, dtype=f) - sd * lse)
    dz = gr * ((f(1.0) - ls) * (onehot - prob) + ls * (d[None, :] - prob * sd))
    return out.astype(f), dz.astype(f)


def tie_cases(V):
    """Logits with planted exact maxima -> z float32 [rows, V], the planted index sets per row.  Same lane of the wave that
    walks a row (v and v + 64), different lanes, the maximum at 0 and at V - 1 alone, all entries equal."""
    rng = np.random.RandomState(V)
    plants = [[0], [V - 1], list(range(V))]
    if V >= 2:
        plants += [[V - 2, V - 1], [0, V - 1]]
    if V >= 8:
        plants += [[5, 6], [7, 3]]
    if V > 64:
        plants += [[0, 64], [V - 1, V - 65], [64, 1]]
    if V > 70:
        plants += [[3, 67], [70, 10], [66, 2, 1]]
    if V > 128:
        plants += [[0, 64, 128], [127, 128], [65, 128]]
    z = (rng.randn(len(plants), V) * 3).astype(np.float32)
    for r, where in enumerate(plants):
        top = np.float32(z[r].max() + np.float32(1.5))
        z[r, where] = top
    return z, [sorted(set(w)) for w in plants]
