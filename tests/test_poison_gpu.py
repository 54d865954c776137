"""No result may depend on undefined memory (tests/poison.py; DESIGN "Undefined on entry, or state").

Every case runs the same inputs three times - torch.empty & co filled with zero, NaN and 3e38 - first from an emptied pool,
then served from a pooled workspace that a larger call left behind and that was poisoned where it lay (asserted by data_ptr).
  (a) deterministic mode and the operators without float atomics: every output and gradient bit-identical across all runs;
  (b) the default (atomic) path: finite, and inside the gate the operator's own parity test holds it to against float64
      (the gate and the reference are imported from that test);
  (c) regions documented as zero hold exactly zero;
  (d) the case poisoned something: a case whose counter is 0 fails.
Integer tensors only ever receive 0 or 1 (poison.fill_value): nothing here can send an index out of bounds.

Float workspaces with integer regions that ARE poisoned with NaN / 3e38 here, and where the kernel writes each region before
it reads it in the same call (read before this test was written):
  CtcWs.head   csrc/ctc.hip:61 (all V entries zeroed by the alpha kernel), :85 (run heads); read :275 by the gradient kernel,
               a later launch, and only for rows whose w.raw (written :67 / :144 for every row) is finite
  CtcWs.order  csrc/ctc.hip:84 writes entries 0 .. L-1 of a row that got past the early return (:64); read :279 / :282 at
               h + j < L through a head entry of the same launch pair, only for such rows
  BeamWs.hist  csrc/ctc_beam.hip:416 writes entry (t, tid) in every frame t < len for every slot tid < nsel (:352) of that
               frame; the walks (:473, :518, :548) start at a slot tid < nlive = nsel of the last frame (:428) and follow
               e.x = k, the parent's slot, which was < nsel of the frame before - only entries written in this launch.  The
               same kernel serves the n-gram and word-LM variants (template flags).  The word LM has no scratch of its own:
               ops.word_lm_score and the fused search take outputs and this workspace only.
  ctc_align    csrc/ctc_align.hip:141-143 writes both back-pointer words of every (t, word < nw) for t = 1 .. len - 1; the
               backtrace (:163-164) reads (t, s >> 6) for t = len - 1 .. 1 with s < S.  w.state: st[t] written :162 / :167
               for every t < len of a feasible row, read :186 / :189 / :190 for t < len only (neighbours guarded by t == 0
               and t == len - 1), after the barrier at :170.  first / last are int32 tensors (0 / 1 under poison), read :195
               into a loop bounded by len (:197).
No read before a write was found in any of them.

One line per case on stdout (pytest -s): what was poisoned and the verdict; collected in profiles/poison_coverage.txt."""
import numpy as np
import pytest
import torch

import poison as P

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture(autouse=True)
def _clean_pools():
    """Every case starts from empty pools and leaves none of its poison behind for the next test module."""
    import ops
    P.empty_pool()
    ops._ARENA.__init__()
    yield
    P.empty_pool()
    ops._ARENA.__init__()
    assert not hasattr(torch.empty, "__wrapped__"), "a poisoned() scope is still open"


def _pool_ptrs():
    return sorted(t.data_ptr() for root in P.pool_roots()[:2] for t in P.walk_tensors(root))


def GEMM_GATE():
    """The gate of test_hip_parity.test_gemm_variants for the default bf16x6 products (and of test_gemm_skinny_and_colsum, of
    test_gemm_side_on_a_subset_of_the_xcds): rtol of the largest output + atol, from that module."""
    import test_hip_parity as TP
    assert TP.GEMM_ARITH[0][0] == "bf16x6"
    return dict(rtol=TP.GEMM_ARITH[0][1], atol=TP.GEMM_ATOL)


def _has_pool():
    import ops
    return any(ops._POOL.free.values())


class _leases_recorded(object):
    """Inside the scope every ops._POOL.acquire appends the data_ptrs of the workspace it hands out to `into`."""

    def __init__(self, into):
        self.into = into

    def __enter__(self):
        import ops
        orig = ops._Pool.acquire

        def acquire(pool, key, factory):
            lease = orig(pool, key, factory)
            self.into.append(sorted(t.data_ptr() for t in P.walk_tensors(lease.ws)))
            return lease
        self.orig, ops._Pool.acquire = orig, acquire

    def __exit__(self, *exc):
        import ops
        ops._Pool.acquire = self.orig
        return False


def _cpu(out):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items() if v is not None}


def _sweep(name, fn, prime=None, identical=True, gate=None, zero=None):
    """fn() -> dict of device tensors (every output and gradient).  Runs it under the three patterns from an emptied pool
    and - with prime(), the larger call that leaves its workspace behind - from the poisoned leftover; asserts (a) or (b),
    (c) through zero(out), and (d).  -> the runs."""
    runs, total = {}, P.Stats()
    for variant in ("fresh",) + (("leftover",) if prime is not None else ()):
        for pattern in P.PATTERNS:
            P.empty_pool()
            st = P.Stats()
            if variant == "leftover":
                prime()
                torch.cuda.synchronize()
                before = _pool_ptrs()
                assert before, "%s: the larger call left no workspace in the pool" % name
                assert P.poison_pool(pattern, st) > 0
            leases = []
            with _leases_recorded(leases), P.poisoned(pattern, st):
                out = _cpu(fn())
            if variant == "leftover":
                # every lease of the call IS storage the larger call left and poison_pool filled, pointer for pointer, and
                # nothing new was allocated for it (the scratch of the ordered reductions has no lease: the pointer set)
                for ptrs in leases:
                    assert ptrs and set(ptrs) <= set(before), "%s: a lease was not the poisoned leftover" % name
                assert leases or not _has_pool(), "%s: a pooled operator took no lease" % name
                assert _pool_ptrs() == before, "%s: the call was not served from the pooled workspace" % name
            assert st.total > 0, "%s %s %s: nothing was poisoned - the case is vacuous" % (name, variant, pattern)
            total.merge(st)
            for k, v in out.items():
                assert bool(torch.isfinite(v.double()).all()) or not v.is_floating_point(), \
                    "%s %s %s: %s is not finite" % (name, variant, pattern, k)
            if zero is not None:
                zero(out, "%s %s %s" % (name, variant, pattern))
            if gate is not None:
                gate(out, "%s %s %s" % (name, variant, pattern))
            runs[(variant, pattern)] = out
    first = runs[("fresh", "zero")]
    if identical:
        for key, out in runs.items():
            assert set(out) == set(first)
            for k in out:
                assert torch.equal(out[k], first[k]), "%s: %s differs between fresh/zero and %s/%s (max %.3g)" % (
                    name, k, key[0], key[1], float((out[k].double() - first[k].double()).abs().max()))
    print("poison_coverage %-44s %s; %d runs; %s" % (name, total.line(), len(runs),
                                                    "bit-identical" if identical else "finite, inside the parity gate"))
    return runs


# ------------------------------------------------------------------------------------------------- the harness sees a read
def test_positive_control_accumulating_into_undefined_memory_gives_nan(hb):
    """hb.gemm(..., out=torch.empty(...), accumulate=True) READS its output: under `nan` the result is NaN.  A wrong number,
    not a fault - and the proof that a read of undefined memory does not get past this module."""
    g = torch.Generator().manual_seed(1)
    A, B = torch.randn(130, 64, generator=g).to(DEV), torch.randn(64, 80, generator=g).to(DEV)
    with P.poisoned("nan") as st:
        out = hb.gemm(A, B, out=torch.empty(130, 80, device=DEV), accumulate=True)
    assert st.n_allocs == 1 and bool(torch.isnan(out).all())
    with P.poisoned("zero"):
        clean = hb.gemm(A, B, out=torch.empty(130, 80, device=DEV), accumulate=True)
    assert bool(torch.isfinite(clean).all())
    print("poison_coverage %-44s %s; NaN reported" % ("positive control", st.line()))


# ------------------------------------------------------------------------------------------------- GEMM and reductions
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", [(130, 80, 2051), (17, 130, 1000)])
def test_gemm_fresh_output_split_k(hb, M, N, K, ta, tb):
    """out=None: the output is torch.empty and the library splits the long K (its partial products meet in atomics, so the
    zero pass is the library's own).  (b): the gate of test_hip_parity.test_gemm_variants, rtol 1e-5 of the largest output +
    1e-4, against the float64 product."""
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    Ad, Bd, bd = A.to(DEV), B.to(DEV), bias.to(DEV)

    def fn():
        return dict(plain=hb.gemm(Ad, Bd, trans_a=ta, trans_b=tb), split3=hb.gemm(Ad, Bd, trans_a=ta, trans_b=tb, split_k=3),
                    epilogue=hb.gemm(Ad, Bd, trans_a=ta, trans_b=tb, bias=bd, relu=True))

    def gate(out, what):
        TP._close(out["plain"], ref.float(), **GEMM_GATE(), what=what + " plain")
        TP._close(out["split3"], ref.float(), **GEMM_GATE(), what=what + " split 3")
        TP._close(out["epilogue"], torch.relu(ref + bias).float(), **GEMM_GATE(), what=what + " bias+relu")
    _sweep("gemm %dx%dx%d %s%s" % (M, N, K, "T" if ta else "N", "T" if tb else "N"), fn, identical=False, gate=gate)


@pytest.mark.parametrize("split", [None, 7])
def test_gemm_det_slabs_live_in_poisoned_scratch(hb, split):
    """hb.gemm_det at 130 x 80 x 2051: the slabs lie in hb._det_ws_cache (torch.empty).  Leftover: a 512 x 160 x 4100 product
    first, whose larger scratch then serves this one."""
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(2051, 130, generator=g).to(DEV), torch.randn(2051, 80, generator=g).to(DEV)
    A2, B2 = torch.randn(4100, 512, generator=g).to(DEV), torch.randn(4100, 160, generator=g).to(DEV)
    assert hb.gemm_det_split(130, 80, 2051, trans_a=True, split=split)["split"] > 1
    assert hb.gemm_det_split(512, 160, 4100, trans_a=True)["bytes"] > hb.gemm_det_split(130, 80, 2051, trans_a=True, split=split)["bytes"]
    runs = _sweep("gemm_det 130x80x2051 split %s" % split, lambda: dict(c=hb.gemm_det(A, B, trans_a=True, split=split)),
                  prime=lambda: hb.gemm_det(A2, B2, trans_a=True))
    ref = A.double().t() @ B.double()
    g = GEMM_GATE()
    assert float((runs[("fresh", "nan")]["c"].double() - ref.cpu()).abs().max()) <= g["rtol"] * float(ref.abs().max()) + g["atol"]


@pytest.mark.parametrize("det", [False, True])
def test_reductions(hb, det):
    """hb.colsum (fresh output; above 256 rows the ordered one keeps partial rows in the scratch), hb.sumsq, hb.gather_sumsq
    into a torch.empty flat buffer - default and deterministic.  Gates: test_gemm_skinny_and_colsum (rtol 1e-5, atol 1e-4),
    test_gather_sumsq_kernel (1e-5 of the sum).  The ordered ones are bit-identical as well."""
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(9)
    X = torch.randn(1025, 263, generator=g).to(DEV)[:, :260]
    x = torch.randn(8197, generator=g).to(DEV)
    sizes = [1, 3, 4, 5, 4097, 33, 7]
    srcs = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4

    def fn():
        with hb.deterministic(det):
            flat = torch.empty(off, device=DEV)
            acc = torch.zeros(1, device=DEV)
            hb.gather_sumsq(srcs, offs, flat, acc)
            return dict(colsum=hb.colsum(X), sumsq=hb.sumsq(x, torch.zeros(1, device=DEV)), gathered_sumsq=acc,
                        gathered=torch.cat([flat[o:o + n] for o, n in zip(offs, sizes)]))

    def gate(out, what):
        TP._close(out["colsum"], X.double().sum(0).float().cpu(), **GEMM_GATE(), what=what + " colsum")
        want = float((x.double() ** 2).sum())
        assert abs(float(out["sumsq"]) - want) <= 1e-5 * want, what
        want = sum(float((s.double() ** 2).sum()) for s in srcs)
        assert abs(float(out["gathered_sumsq"]) - want) <= 1e-5 * want, what
        assert torch.equal(out["gathered"], torch.cat(srcs).cpu()), what
    _sweep("colsum, sumsq, gather_sumsq %s" % ("deterministic" if det else "default"), fn, identical=det, gate=gate)


@pytest.mark.parametrize("det", [False, True])
def test_linear_inside_and_outside_the_step_arena(hb, det):
    """ops.linear forward and backward: outside a scope (torch.empty output, the library's zero pass), in the first scope (the
    arena has no buffer yet: the fallback) and in the second and third (out_zeroed: the product trusts the arena's zeros, dW
    and db accumulate into arena slices).  After every scope a new one opens and the WHOLE arena is zero."""
    import ops
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(600, 40, generator=g), torch.randn(24, 40, generator=g) * 0.3, torch.randn(24, generator=g)
    dy = torch.randn(600, 24, generator=g)
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    yr = torch.relu(xr @ wr.t() + br)
    yr.backward(dy.double())
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)

    def once(tag, out):
        xg, wg, bg = (t.clone().requires_grad_() for t in (xd, wd, bd))
        y = ops.linear(xg, wg, bg, relu=True)
        y.backward(dyd)
        out.update({tag + k: v.clone() for k, v in dict(y=y, dx=xg.grad, dw=wg.grad, db=bg.grad).items()})

    def fn():
        out = {}
        ops._ARENA.__init__()
        with hb.deterministic(det):
            once("outside/", out)
            for i in range(3):
                with ops.step_arena(DEV):
                    assert P.arena_is_zero(), "a value survived in the step arena behind scope %d" % i
                    once("scope%d/" % i, out)
            with ops.step_arena(DEV):
                assert ops._ARENA.buf is not None and P.arena_is_zero(), "a value survived behind the last scope"
        return out

    def gate(out, what):
        for tag in ("outside/", "scope0/", "scope1/", "scope2/"):
            TP._close(out[tag + "y"], yr.detach().float(), **GEMM_GATE(), what=what + tag + "y")
            TP._close(out[tag + "dx"], xr.grad.float(), **GEMM_GATE(), what=what + tag + "dx")
            TP._close(out[tag + "dw"], wr.grad.float(), **GEMM_GATE(), what=what + tag + "dw")
            TP._close(out[tag + "db"], br.grad.float(), **GEMM_GATE(), what=what + tag + "db")
    _sweep("ops.linear arena + fallback %s" % ("deterministic" if det else "default"), fn, identical=det, gate=gate)


def test_gemm_side_on_one_xcd_mask(hb):
    """hb.gemm_side adds into a zeroed output through a zeroed queue word; its operands here come from poisoned allocations
    (clones).  Gate of test_gemm_side_on_a_subset_of_the_xcds: rtol 1e-5, atol 1e-4."""
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(4)
    A, B = torch.randn(2051, 130, generator=g), torch.randn(2051, 80, generator=g)
    ref = (A.double().t() @ B.double()).float()
    Ad, Bd = A.to(DEV), B.to(DEV)

    def fn():
        a, b = torch.empty_like(Ad).copy_(Ad), torch.empty_like(Bd).copy_(Bd)
        out, queue = torch.zeros(130, 80, device=DEV), torch.zeros(1, device=DEV)
        assert hb.gemm_side(a, b, out, queue, 0xf0, trans_a=True)
        return dict(c=out)
    _sweep("gemm_side mask 0xf0", fn, identical=False,
           gate=lambda out, what: TP._close(out["c"], ref, **GEMM_GATE(), what=what))


# ------------------------------------------------------------------------------------------------- LSTM layer
_LSTM = {}


def _lstm_inputs(ndir, B, T, I, H, lens, seed):
    key = (ndir, B, T, I, H, tuple(lens), seed)
    if key not in _LSTM:
        from oracle import asr_oracle as O
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, T, I, generator=g)
        for b_, n_ in enumerate(lens):
            x[b_, n_:] = 0.0
        k = 1.0 / np.sqrt(H)
        prm = [torch.empty(*s).uniform_(-k, k, generator=g) for _ in range(ndir) for s in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,))]
        dy = torch.randn(B, T, ndir * H, generator=g)
        cp = [p.clone().requires_grad_(True) for p in prm]
        xc = x.clone().requires_grad_(True)
        ref = torch.cat([O.lstm_direction(xc, lens, *cp[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(ndir)], 2)
        ref.backward(dy)
        _LSTM[key] = dict(x=x, prm=prm, dy=dy, ref=ref.detach(), dx=xc.grad, dprm=[p.grad for p in cp])
    return _LSTM[key]


def _lstm_run(hb, c, ndir, lens, packed, persistent):
    """ops.lstm_layer forward + backward on the case -> y [B, T, ndir H], dx [B, T, I] (padded layout either way), gradients."""
    import ops
    B, T, _ = c["x"].shape
    gp = [p.to(DEV).requires_grad_(True) for p in c["prm"]]
    out = {}
    if packed:
        layout = hb.RowLayout(lens, [1], DEV)
        rows = hb.LayerRows(layout, 0)
        xp = hb.rows_pack(c["x"].to(DEV), rows).requires_grad_(True)
        dyp = torch.full((rows.R, c["dy"].shape[2]), 7.0)          # noise on the padding rows: must not reach a gradient
        for b_, n_ in enumerate(lens):
            r0 = int(layout.base[0][b_])
            dyp[r0:r0 + n_] = c["dy"][b_, :n_]
        run = lambda: ops.lstm_layer(xp, None, gp, ndir, rows=rows)
    else:
        xg = c["x"].to(DEV).requires_grad_(True)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
        run = lambda: ops.lstm_layer(xg.transpose(0, 1), lens_dev, gp, ndir)
    if persistent:
        with hb.require_persistent():
            got = run()
            got.backward(dyp.to(DEV) if packed else c["dy"].transpose(0, 1).contiguous().to(DEV))
        assert not hb.persist_aborted(torch.device(DEV))
    else:
        got = run()
        got.backward(dyp.to(DEV) if packed else c["dy"].transpose(0, 1).contiguous().to(DEV))
    if packed:
        out.update(y_rows=got, dx_rows=xp.grad, pad_rows=torch.tensor(
            [r for b_, n_ in enumerate(lens) for r in range(int(layout.base[0][b_]) + n_, int(layout.base[0][b_]) + int(layout.ext[0][b_]))]))
    else:
        out.update(y=got.transpose(0, 1), dx=xg.grad)
    out.update({"dprm%d" % i: p.grad for i, p in enumerate(gp)})
    return out


def _lstm_gate(c, lens, packed, hb):
    import test_hip_parity as TP
    layout = hb.RowLayout(lens, [1], DEV) if packed else None

    def gate(out, what):
        """The gates of test_lstm_layer_fwd_bwd / _packed_lstm_case: y rtol 1e-4, gradients rtol 1e-3, atol 1e-5."""
        if packed:
            for b_, n_ in enumerate(lens):
                r0 = int(layout.base[0][b_])
                TP._close(out["y_rows"][r0:r0 + n_], c["ref"][b_, :n_], what=what + " y", **TP.LSTM_Y_GATE)
                TP._close(out["dx_rows"][r0:r0 + n_], c["dx"][b_, :n_], what=what + " dx", **TP.LSTM_GRAD_GATE)
        else:
            TP._close(out["y"], c["ref"], what=what + " y", **TP.LSTM_Y_GATE)
            TP._close(out["dx"], c["dx"], what=what + " dx", **TP.LSTM_GRAD_GATE)
        for i, want in enumerate(c["dprm"]):
            TP._close(out["dprm%d" % i], want, what=what + " param %d" % i, **TP.LSTM_GRAD_GATE)

    def zero(out, what):
        """(c) the padding rows of every block hold zeros in y and in dx, whatever the upstream gradient holds there."""
        if packed:
            pad = out["pad_rows"]
            assert float(out["y_rows"][pad].abs().max()) == 0.0 and float(out["dx_rows"][pad].abs().max()) == 0.0, what
    return gate, zero


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("persistent", [False, True])
def test_lstm_layer(hb, persistent, packed, det):
    """Per-step kernels: H = 16, B = 3, T = 9, lens [9, 7, 4], both directions.  Persistent kernels: H = 128, B = 8, T = 48
    ragged.  Padded batch and packed rows.  Leftover: the pooled workspace of a LONGER batch of the same capacity class
    (ops._row_capacity: 512 rows for T = 48 and for T = 36 at B = 8; 256 rows at B = 3) serves the shorter one, poisoned."""
    if persistent:
        B, I, H, lens_long = 8, 16, 128, [48, 48, 45, 40, 33, 20, 9, 1]
        lens = [min(n, 36) for n in lens_long]
    else:
        B, I, H, lens_long, lens = 3, 8, 16, [9, 7, 4], [7, 5, 4]
    if persistent and not hb.USE_PERSIST:
        pytest.fail("the persistent kernels are switched off in this process")
    big = _lstm_inputs(2, B, max(lens_long), I, H, lens_long, 11)
    small = _lstm_inputs(2, B, max(lens), I, H, lens, 12)
    for c, ln in ((big, lens_long), (small, lens)):
        gate, zero = _lstm_gate(c, ln, packed, hb)

        def fn(c=c, ln=ln):
            with hb.deterministic(det):
                return _lstm_run(hb, c, 2, ln, packed, persistent)

        def prime():
            with hb.deterministic(det):
                _lstm_run(hb, big, 2, lens_long, packed, persistent)
        _sweep("lstm %s %s %s T=%d" % ("persistent H=128" if persistent else "per-step H=16", "packed" if packed else "padded",
                                       "deterministic" if det else "default", max(ln)),
               fn, prime=prime if c is small else None, identical=det, gate=gate, zero=zero)


# ------------------------------------------------------------------------------------------------- pyramid, rows
def test_pyramid_concat_and_rows(hb):
    """No float atomics outside the fill gradient: pyramid_concat (mask tensor, seeded mask, odd T) forward and backward,
    rows_pack, rows_unpack forward and backward with relu(fill) behind the lengths and a seeded mask - bit-identical, and
    exact against the oracle where test_pyramid_concat is (rtol 0).  (c): the padding rows of rows_pack are zero; frames
    behind a length hold relu(fill) exactly (no mask) in rows_unpack."""
    import ops
    import test_hip_parity as TP
    from oracle import asr_oracle as O
    g = torch.Generator().manual_seed(7)
    T, B, C, lens = 11, 3, 8, [11, 7, 4]
    x = torch.randn(T, B, C, generator=g)
    mask = (torch.rand(T, B, C, generator=g) > 0.3).float() / 0.7
    dy = torch.randn((T + 1) // 2, B, 2 * C, generator=g)
    xr = x.clone().requires_grad_(True)
    ref = O.pair_concat((xr * mask).transpose(0, 1)).transpose(0, 1)
    ref.backward(dy)
    xb = torch.randn(B, T, C, generator=g)
    for b_, n_ in enumerate(lens):
        xb[b_, n_:] = 0.0
    fill, dout = torch.randn(C, generator=g), torch.randn(B, T, C, generator=g)
    layout = hb.RowLayout(lens, [], DEV)
    rows = hb.LayerRows(layout, 0)
    pad = torch.tensor([r for b_, n_ in enumerate(lens) for r in range(int(layout.base[0][b_]) + n_,
                                                                      int(layout.base[0][b_]) + int(layout.ext[0][b_]))])

    def fn():
        out = {}
        with hb.deterministic():
            for name, m in (("mask", mask.to(DEV)), ("seeded", hb.SeededMask((T, B, C), 0.3, DEV, seed=99)), ("plain", None)):
                xg = x.to(DEV).requires_grad_(True)
                y = ops.pyramid_concat(xg, m)
                y.backward(dy.to(DEV))
                out.update({"pyr_%s_y" % name: y, "pyr_%s_dx" % name: xg.grad})
            packed = hb.rows_pack(xb.to(DEV), rows)
            out["packed"] = packed
            for name, m in (("plain", None), ("seeded", hb.SeededMask((B, T, C), 0.3, DEV, seed=5))):
                pk, fl = packed.clone().requires_grad_(True), fill.to(DEV).requires_grad_(True)
                u = ops.rows_unpack(pk, rows, T, fl, m, True)
                u.backward(dout.to(DEV))
                out.update({"unpack_%s" % name: u, "unpack_%s_drows" % name: pk.grad, "unpack_%s_dfill" % name: fl.grad})
        return out

    def zero(out, what):
        assert torch.equal(out["pyr_mask_y"], ref.detach()), what
        TP._close(out["pyr_mask_dx"], xr.grad, rtol=1e-6, atol=1e-6, what=what)
        assert float(out["packed"][pad].abs().max()) == 0.0, what
        for b_, n_ in enumerate(lens):
            r0 = int(layout.base[0][b_])
            assert torch.equal(out["packed"][r0:r0 + n_], xb[b_, :n_]), what
            assert torch.equal(out["unpack_plain"][b_, :n_], xb[b_, :n_]), what
            assert torch.equal(out["unpack_plain"][b_, n_:], torch.relu(fill).expand(T - n_, C)), what
        assert float(out["unpack_plain_drows"][pad].abs().max()) == 0.0, what
    _sweep("pyramid_concat, rows_pack, rows_unpack", fn, zero=zero)


# ------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("det", [False, True])
def test_label_logprob(hb, det):
    """Forward and backward with the sum and the argmax (V = 34, label smoothing 0.05).  Gate of test_label_logprob_kernels /
    test_loss_total_det: rtol 1e-5 + 1e-6.  The default total is one atomic per block into a zeroed word: (b); everything
    else, and the ordered total, (a)."""
    import ops
    import test_deterministic_gpu as TD
    L, B, V = 5, 7, 34
    g = torch.Generator().manual_seed(L + V)
    logits = (torch.randn(L, B, V, generator=g) * 3)
    idx = torch.randint(0, V, (L, B), generator=g)
    dist = torch.rand(V, generator=g)
    dist = dist / dist.sum()
    go = torch.randn(L, B, generator=g)
    scale = -1.0 / (L * B)
    zr = logits.double().requires_grad_()
    lp = torch.log_softmax(zr, dim=2)
    ref = 0.95 * torch.gather(lp, 2, idx.unsqueeze(2)).squeeze(2) + 0.05 * torch.sum(lp * dist.double(), dim=2)
    ((ref * go.double()).sum() + 2.0 * ref.sum() * scale).backward()
    ld, id_, dd, god = logits.to(DEV), idx.to(DEV), dist.to(DEV), go.to(DEV)

    def fn():
        with hb.deterministic(det):
            z = ld.clone().requires_grad_()
            out, total, amax = ops.label_logprob(z, id_, dd, 0.05, with_sum=True, sum_scale=scale, with_argmax=True)
            ((out * god).sum() + 2.0 * total).backward()
            return dict(out=out, total=total.reshape(1).clone(), argmax=amax, dz=z.grad)

    def gate(out, what):
        TD._close(out["out"], ref.detach(), *TD.LOGPROB_GATE, what + " out")
        TD._close(out["total"], (ref.sum() * scale).reshape(1).detach(), *TD.LOGPROB_GATE, what + " total")
        TD._close(out["dz"], zr.grad, *TD.LOGPROB_GATE, what + " dz")
        assert torch.equal(out["argmax"], logits.argmax(-1)), what
    runs = _sweep("label_logprob sum + argmax %s" % ("deterministic" if det else "default"), fn, identical=det, gate=gate)
    for out in runs.values():                     # (no atomics in these, whatever the mode)
        for k in ("out", "argmax", "dz"):
            assert torch.equal(out[k], runs[("fresh", "zero")][k]), k


@pytest.mark.parametrize("zero_infinity", [True, False])
def test_ctc_loss(hb, zero_infinity):
    """ops.ctc_loss on test_ctc_gpu's case V = 34, group `block` (with its infeasible row; ld = V + 3, NaN behind every length):
    its float64 reference and allowance (_check).  The workspace - alpha, lse, and the integer regions order / head, see the
    module docstring - is the pooled one.  Leftover: the workspace of a call with a LONGER Lmax (140: the strided kernels) and
    the other zero_infinity, in the same capacity class of the pool, poisoned.  Ordered sums only: bit-identical.  (c): zero gradient behind every length, in the three
    padding columns and - zero_infinity - in the infeasible row (asserted by _check and here)."""
    import ops
    import test_ctc_gpu as TC
    c = TC._case(34, "block", 3.0)
    bad = int((~c["feasible"]).nonzero()[0])
    rows = torch.arange(c["B"]) if zero_infinity else c["feasible"].nonzero().flatten()

    def fn():
        nll, grad = TC._run(hb, c, zero_infinity)
        out = dict(nll_feasible=nll[c["feasible"]], grad=grad[:, :, :c["V"]], grad_pad=grad[:, :, c["V"]:])
        TC._check(c, nll, grad, rows, "poisoned ctc_loss")
        if zero_infinity:
            assert float(nll[bad]) == 0.0 and bool((grad[bad] == 0).all())
        else:
            assert bool(torch.isinf(nll[bad])) and float(nll[bad]) > 0
        return out

    # the leftover: the same logits with the longest utterance relabelled with 140 labels - the strided kernels' label count,
    # a longer Lmax, so order / head / alpha lie elsewhere in the workspace and order holds MORE entries than this call
    # writes - whose workspace falls into the same capacity class of the pool (asserted), poisoned where it lay
    long_i = max(range(c["B"]), key=lambda i: c["ylens"][i])
    assert c["ylens"][long_i] == 127 and c["lens"][long_i] >= 2 * 140 - 30
    ylens2 = list(c["ylens"])
    ylens2[long_i] = 140
    parts, o = [], 0
    for i, n in enumerate(c["ylens"]):
        parts.append(torch.tensor([1 + (j % 2) for j in range(140)], dtype=torch.long) if i == long_i else c["ys"][o:o + n])
        o += n
    ys2 = torch.cat(parts)
    words = lambda lmax: (hb.ctc_ws_bytes(c["B"], c["T"], c["V"], lmax) + 3) // 4
    assert words(140) > words(127) and ops._row_capacity(words(140)) == ops._row_capacity(words(127))

    def prime():
        z = c["z"].to(DEV).requires_grad_()
        nll = ops.ctc_loss(z, hb.to_device_i32(c["lens"], DEV), ys2.to(DEV), ylens2, not zero_infinity)
        nll.sum().backward()
        assert any(k[0] == "ctc" and v for k, v in ops._POOL.free.items())
    _sweep("ctc_loss V=34 block zero_infinity=%s" % zero_infinity, fn, prime=prime)


# ------------------------------------------------------------------------------------------------- the whole train step
@pytest.mark.parametrize("shape", ["tiny", "persistent H=128"])
def test_supervised_train_steps_do_not_depend_on_undefined_memory(hb, tmp_path, monkeypatch, shape):
    """Three consecutive Solver.sup_train_one_iteration in deterministic mode (dropout 0.3, tf_rate 0.5): the loss, every
    parameter and every Adam tensor after every step, bit for bit across zero / nan / huge.  Step 1 takes the arena's
    fallback path (no buffer yet), steps 2 and 3 the arena; after every step a new scope opens and the whole arena is zero
    (the ASR_ARENA_DEBUG check as a test).  The solver and its inputs are those of test_deterministic_gpu."""
    import ops
    import synth
    import test_deterministic_gpu as TD
    if shape == "tiny":
        t, batch = synth.TINY, synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    else:
        t, batch = dict(synth.TINY, input_dim=16, enc_hidden_dim=128), synth.ragged_batch(8, 48, 16, 9, 21)
    records, total = {}, P.Stats()
    for pattern in P.PATTERNS:
        solver, dev = TD._solver(str(tmp_path / pattern), monkeypatch, t, synth.TINY_LM, deterministic=True, dropout_rate=0.3)
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        P.empty_pool()
        ops._ARENA.__init__()
        st, rec = P.Stats(), []
        xs, ilens, ys = batch
        with P.poisoned(pattern, st):
            xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
            for i in range(3):
                loss = solver.sup_train_one_iteration(xs_d, ilens, ys_d, 0.5)
                solver.flush()
                rec.append((float(loss), TD._state(solver, solver.gen_opt)))
                with ops.step_arena(dev):
                    assert P.arena_is_zero(), "%s step %d: a value survived in the step arena" % (pattern, i)
                if i == 0:
                    assert P.poison_pool(pattern, st) > 0         # the workspaces the first step left serve the next ones
        assert ops._ARENA.buf is not None, "steps 2 and 3 ran on the arena"
        assert not hb.persist_aborted(dev)
        assert st.n_allocs > 0 and st.pool_tensors > 0
        total.merge(st)
        records[pattern] = rec
    for pattern in ("nan", "huge"):
        for i, ((la, sa), (lb, sb)) in enumerate(zip(records["zero"], records[pattern])):
            assert np.isfinite(la) and la == lb, "step %d: loss %.9g under zero, %.9g under %s" % (i, la, lb, pattern)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), "step %d: %s differs between zero and %s (max %.3g)" % (
                    i, k, pattern, float((sa[k] - sb[k]).abs().max()))
    assert len(set(r[0] for r in records["zero"])) == 3, "three different steps"
    print("poison_coverage %-44s %s; 9 steps; bit-identical" % ("sup train step x3 %s" % shape, total.line()))


def test_poison_pool_marks_every_row_of_a_pooled_lstm_workspace_stale(hb):
    """poison.py fills gates_buf / y_buf of a pooled LSTM workspace including the row behind the written ones, which the
    packed-row dW_hh product reads, and says so in the workspace's own `rows_written` (ops._LstmLayer zeroes that row when
    rows_written exceeds the call's rows).  If ops renames the field this fails, not the coverage of that row."""
    import ops
    lens = [9, 7, 4]
    _lstm_run(hb, _lstm_inputs(2, 3, 9, 8, 16, lens, 11), 2, lens, True, False)
    pooled = [ws for key, lst in ops._POOL.free.items() if key[0] == "lstm" for ws in lst]
    assert pooled and all("rows_written" in ws and 0 < ws["rows_written"] < ws["gates_buf"].shape[0] for ws in pooled)
    assert P.poison_pool("nan") > 0
    for ws in pooled:
        assert ws["rows_written"] == ws["gates_buf"].shape[0] == ws["y_buf"].shape[0]
        assert bool(torch.isnan(ws["gates_buf"]).all()) and bool(torch.isnan(ws["y_buf"]).all())


def _finite_state(solver, opt, what):
    import test_deterministic_gpu as TD
    for k, v in TD._state(solver, opt).items():
        assert bool(torch.isfinite(v).all()), "%s: %s is not finite" % (what, k)


def _arena_zero_after_scope(dev, what):
    import ops
    with ops.step_arena(dev):
        assert P.arena_is_zero(), "%s: a value survived in the step arena" % what


@pytest.mark.parametrize("shape", ["tiny", "persistent H=128"])
def test_default_path_train_steps_larger_then_smaller(hb, tmp_path, monkeypatch, shape):
    """The supervised steps of the test above on the DEFAULT path (float atomics, the side stream, out_zeroed products on
    arena slices): two steps on the batch, then two on a SMALLER one (fewer frames, so the arena's cursor stops short of what
    the larger step dirtied and every pooled workspace is a larger call's leftover).  The pool is poisoned after every step.
    (b): loss, parameters and Adam tensors finite after every step; the whole arena zero after every scope; and the FIRST
    step's loss - the only one no Adam update has amplified - within twice the gate that test_deterministic_gpu.
    test_the_mode_is_the_same_model holds the loss of either mode to against one reference (LOSS_GATE: 1e-5 relative +
    1e-5) of the deterministic mode's loss of the same step; every parameter after EVERY step within that test's gradient
    gate (GRAD_GATE) of the deterministic run's parameters after the same step."""
    import ops
    import synth
    import test_deterministic_gpu as TD
    if shape == "tiny":
        t, big = synth.TINY, synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
        small = synth.batch(8, 9, [7, 5, 4], [3, 2, 2], 14)
    else:
        t, big = dict(synth.TINY, input_dim=16, enc_hidden_dim=128), synth.ragged_batch(8, 48, 16, 9, 21)
        small = synth.ragged_batch(8, 30, 16, 9, 22)
    import collections
    params = collections.defaultdict(list)
    first, total = {}, P.Stats()
    for pattern, det in [("zero", True)] + [(p, False) for p in P.PATTERNS]:
        solver, dev = TD._solver(str(tmp_path / ("%s%d" % (pattern, det))), monkeypatch, t, synth.TINY_LM, deterministic=det,
                                 dropout_rate=0.3)
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        P.empty_pool()
        ops._ARENA.__init__()
        st = P.Stats()
        with P.poisoned(pattern, st):
            for i, (xs, ilens, ys) in enumerate((big, big, small, small)):
                what = "%s %s step %d" % (shape, pattern, i)
                loss = solver.sup_train_one_iteration(torch.from_numpy(xs).to(dev), ilens,
                                                      [torch.from_numpy(y).to(dev) for y in ys], 0.5)
                solver.flush()
                assert np.isfinite(float(loss)), what
                if i == 0:
                    first[(pattern, det)] = float(loss)
                _finite_state(solver, solver.gen_opt, what)
                _arena_zero_after_scope(dev, what)
                assert P.poison_pool(pattern, st) > 0
                params[(pattern, det)].append({n: p.detach().cpu().clone() for n, p in solver.model.named_parameters()})
        assert not hb.persist_aborted(dev)
        assert st.n_allocs > 0 and st.pool_tensors > 0
        total.merge(st)
    ref = first[("zero", True)]
    rtol, atol = TD.LOSS_GATE
    for pattern in P.PATTERNS:
        got = first[(pattern, False)]
        assert abs(got - ref) <= 2.0 * (rtol * abs(ref) + atol), "first loss %.9g under %s, deterministic %.9g" % (got, pattern, ref)
    # every parameter after every default-path step - the steps on the arena and on poisoned leftovers among them - against
    # the deterministic run's, under the gate test_the_mode_is_the_same_model holds every gradient to (TD.GRAD_GATE)
    for pattern in P.PATTERNS:
        for i, (got_p, want_p) in enumerate(zip(params[(pattern, False)], params[("zero", True)])):
            for n in want_p:
                TD._close(got_p[n], want_p[n], *TD.GRAD_GATE, "%s %s step %d: %s" % (shape, pattern, i, n))
    assert len(params[("zero", True)]) == 4
    print("poison_coverage %-44s %s; 12 steps; finite, arena zero, first loss inside the gate"
          % ("default-path sup steps big,big,small,small %s" % shape, total.line()))


def test_default_path_judge_and_generator_steps_against_the_reference(hb, tmp_path, monkeypatch):
    """Solver.judge_train_one_iteration and Solver.gen_train_one_iteration on the default path under the three patterns,
    each after a supervised step whose pooled workspaces were poisoned, held to what test_solver_gpu holds them to: the
    reference's own losses and gradients (tests/golden/tiny_lm.npz, tiny_ssl.npz) under that module's bounds."""
    import synth
    import test_solver_gpu as TS
    gl, gs = TS._golden("tiny_lm.npz"), TS._golden("tiny_ssl.npz")
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    uxs, uilens, _ = synth.batch(8, 9, [12, 10, 7], [2, 2, 2], 41)
    total = P.Stats()
    for pattern in P.PATTERNS:
        st = P.Stats()
        for kind in ("judge", "generator"):
            root = tmp_path / (pattern + kind)
            root.mkdir()
            solver, dev = TS._tiny_solver(str(root), monkeypatch)
            P.empty_pool()
            if kind == "generator":       # the workspaces a supervised step of ANOTHER solver of the same shapes left, poisoned
                other, _ = TS._tiny_solver(str(root), monkeypatch)
                other.sup_train_one_iteration(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys], 1.0)
                other.flush()
                assert P.poison_pool(pattern, st) > 0
            with P.poisoned(pattern, st):
                if kind == "judge":
                    meta = solver.judge_train_one_iteration([torch.from_numpy(gl["ys%d" % i]).to(dev) for i in range(3)])
                    assert abs(meta["loss"] - float(gl["d_loss"])) <= 1e-5 * abs(float(gl["d_loss"]))
                    assert abs(meta["avg_prob"] - float(gl["d_avg_prob"])) <= 1e-5 * abs(float(gl["d_avg_prob"]))
                    for n, p in solver.judge.named_parameters():
                        want = gl["after1/" + n]
                        assert float((p.detach().cpu() - torch.from_numpy(want)).abs().max()) <= 1e-4 * float(np.abs(want).max()) + 2e-6, n
                else:
                    np.random.seed(9)
                    meta = solver.gen_train_one_iteration(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys],
                                                          torch.from_numpy(uxs).to(dev), uilens)
                    assert abs(meta["sup_loss"] - float(gs["sup"])) <= 1e-5 * abs(float(gs["sup"]))
                    assert abs(meta["unsup_loss"] - float(gs["unsup"])) <= 1e-4 * abs(float(gs["unsup"]))
                    assert abs(meta["loss"] - float(gs["loss"])) <= 1e-4 * abs(float(gs["loss"]))
                    for n, p in solver.model.named_parameters():
                        want = gs["grad/" + n]
                        err = float((p.grad.cpu() - torch.from_numpy(want)).abs().max())
                        assert err <= 1e-3 * float(np.abs(want).max()) + 1e-6, (pattern, n, err)
                _arena_zero_after_scope(dev, "%s %s" % (pattern, kind))
        assert st.n_allocs > 0 and st.pool_tensors > 0
        total.merge(st)
    print("poison_coverage %-44s %s; 6 steps; inside the reference's gates" % ("default-path judge + generator step", total.line()))


def test_deterministic_judge_generator_and_ctc_steps(hb, tmp_path, monkeypatch):
    """In deterministic mode: one judge and one generator iteration (smooth-embedding feedback, both model passes, dropout
    0.3 in both nets - test_deterministic_gpu.test_judge_and_generator_steps_reproduce) and one supervised step with
    ctc_weight 0.3 (test_ctc_gpu.test_one_train_step): loss, every parameter and every Adam tensor bit for bit across the
    three patterns, the pooled workspaces poisoned between the iterations."""
    import synth
    import test_ctc_gpu as TC
    import test_deterministic_gpu as TD
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    uxs, uilens, _ = synth.batch(8, 9, [12, 10, 7], [2, 2, 2], 41)
    records, total = {}, P.Stats()
    for pattern in P.PATTERNS:
        rec, st = [], P.Stats()
        solver, dev = TD._solver(str(tmp_path / pattern), monkeypatch, synth.TINY, synth.TINY_LM, deterministic=True,
                                 dropout_rate=0.3, dis_dropout_rate=0.3)
        csolver, _ = TC._solver(str(tmp_path / (pattern + "ctc")), monkeypatch, ctc_weight=0.3, deterministic=True)
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        P.empty_pool()
        with P.poisoned(pattern, st):
            ys_d = [torch.from_numpy(y).to(dev) for y in ys]
            rec.append((float(solver.judge_train_one_iteration(ys_d)["loss"]), TD._state(solver, solver.dis_opt)))
            assert P.poison_pool(pattern, st) > 0
            meta = solver.gen_train_one_iteration(torch.from_numpy(xs).to(dev), ilens, ys_d, torch.from_numpy(uxs).to(dev), uilens)
            rec.append((float(meta["loss"]), TD._state(solver, solver.gen_opt)))
            assert P.poison_pool(pattern, st) > 0
            loss = csolver.sup_train_one_iteration(*TC._sup_batch(dev), 1.0)
            csolver.flush()
            opt = csolver.gen_opt             # (the judge of this solver is not seeded and not stepped: the model and its Adam tensors)
            rec.append((float(loss), dict({n: p.detach().clone() for n, p in csolver.model.named_parameters()},
                                          **{"adam/" + k: getattr(opt, k).clone() for k in ("m", "v", "vmax") if getattr(opt, k, None) is not None})))
            _arena_zero_after_scope(dev, pattern)
        assert not hb.persist_aborted(dev)
        total.merge(st)
        records[pattern] = rec
    for pattern in ("nan", "huge"):
        for i, ((la, sa), (lb, sb)) in enumerate(zip(records["zero"], records[pattern])):
            assert np.isfinite(la) and la == lb, "iteration %d: loss %.9g under zero, %.9g under %s" % (i, la, lb, pattern)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), "iteration %d: %s differs between zero and %s" % (i, k, pattern)
    print("poison_coverage %-44s %s; 9 iterations; bit-identical" % ("judge, generator, ctc_weight 0.3 step (det)", total.line()))


# ------------------------------------------------------------------------------------------------- MWER, edit distance
def test_mwer_loss(hb):
    """ops.mwer_loss forward and backward at B = 3, K = 4 (test_mwer_gpu's grid case with holes in the list, L = 9, V = 65):
    its outputs and its workspace are torch.empty.  Ordered sums only: bit-identical; inside the allowance of
    test_mwer_gpu.test_kernels_against_float64 (mwer_ref.allowance against the float64 restatement).  (c): masked positions
    of dlogits and the unused slots of seq_logp / post / coef are +0.0 bit for bit."""
    import mwer_ref as R
    import ops
    import test_mwer_gpu as TM
    c = (3, 4, 9, 65, "normal", "random", "holes", "random")
    assert c in R.GRID
    case, r64, r32 = TM._refs(c)
    B, L = case["B"], case["L"]
    n = np.clip(case["npos"], 0, L)
    tokens, npos, err = (torch.from_numpy(case[k]).to(DEV) for k in ("tokens", "npos", "err"))

    def fn():
        z = torch.from_numpy(case["logits"]).to(DEV).requires_grad_()
        loss, parts = ops.mwer_loss(z, tokens, npos, err, case["scale"], n_utts=B)
        (loss * case["g"]).backward()
        return dict(loss=loss.reshape(1), risk=parts["risk"], post=parts["post"], seq_logp=parts["seq_logp"], coef=parts["coef"],
                    dlogits=z.grad)

    def gate(out, what):
        for name in TM.OUTPUTS:
            got = out[name].numpy().astype(np.float64).reshape(r64[name].shape)
            assert float(np.abs(got - r64[name]).max()) <= R.allowance(r64[name], r32[name]), "%s: %s" % (what, name)

    def zero(out, what):
        assert not out["dlogits"].numpy().view(np.uint32)[np.arange(L)[:, None] >= n[None, :]].any(), what
        for name in ("seq_logp", "post", "coef"):
            assert not out[name].numpy().view(np.uint32)[case["npos"] <= 0].any(), what + " " + name
    assert (case["npos"] <= 0).any() and (n < L).any()
    _sweep("mwer_loss B=3 K=4", fn, gate=gate, zero=zero)


def test_token_edit_distance(hb):
    """hb.edit_distance (its [3, N] int32 output is torch.empty: poisoned with 0 / 1) on pairs of the lengths around a wave
    and a block (0, 1, 63 .. 65, 129, 250), with skipped tokens, <EOS> cuts and totals: exactly the host's distances
    (test_cer_gpu._expect), the same under every pattern."""
    import test_cer_gpu as TE
    dev = torch.device(DEV)
    rs = np.random.RandomState(34)
    table = TE._table(34, dev)
    hyps, refs = [], []
    for a in (0, 1, 63, 64, 65, 129, 250):
        for b in (0, 1, 64, 129, 250):
            ref = rs.randint(TE.N_SKIP, TE.N_SKIP + 34, size=b)
            hyp = np.resize(ref, a).copy() if a and b else rs.randint(TE.N_SKIP, TE.N_SKIP + 34, size=a)
            change = rs.uniform(size=a) < 0.15
            hyp[change] = rs.randint(TE.N_SKIP, TE.N_SKIP + 34, size=int(change.sum()))
            hyps.append(TE._sprinkle(rs, hyp, [0, 1, 3]) + [TE.EOS] + rs.randint(0, 38, size=3).tolist())
            refs.append(TE._sprinkle(rs, ref, [0, 1, 2, 3]))
    want = TE._expect(hyps, refs, table)

    def fn():
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        dist, hyp_n, ref_n = TE._launch(hb, hyps, refs, table, dev, totals=totals)
        assert (dist, hyp_n, ref_n) == tuple(want) and totals.tolist() == [sum(want[0]), sum(want[2])]
        return dict(dist=torch.tensor(dist), totals=totals)
    _sweep("edit_distance (token) 35 pairs", fn)



# ------------------------------------------------------------------------------------------------- the operators whose parity tests are whole checks
def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.equal(a.cpu(), b.cpu())
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _under_patterns(name, check, verdict="inside the operator's own parity check"):
    """check() runs an operator AND its existing parity check (reference, gate and the documented padding - the -1 / -inf
    of unused slots, zeros behind a length - are that test's own, imported) -> its outputs or None.  Run under the three
    patterns; from the second run on, whatever the run before left in the pools (a DecBuffers lease among them) is poisoned
    where it lies and serves this run.  Outputs, where check returns them: bit-identical across the patterns (a)."""
    total, results = P.Stats(), []
    P.empty_pool()
    for i, pattern in enumerate(P.PATTERNS):
        st = P.Stats()
        if i:
            P.poison_pool(pattern, st)
        with P.poisoned(pattern, st):
            results.append(check())
            torch.cuda.synchronize()
        assert st.n_allocs > 0, "%s %s: nothing was poisoned - the case is vacuous" % (name, pattern)
        total.merge(st)
    for r, pattern in zip(results[1:], P.PATTERNS[1:]):
        assert _same(results[0], r), "%s: the outputs under %s differ from those under zero" % (name, pattern)
    print("poison_coverage %-44s %s; 3 runs; %s%s" % (name, total.line(), verdict,
                                                       "" if results[0] is None else ", bit-identical"))
    return total


DECODER_CASES = ["C10-T60-K1", "C16-T161-K10", "smooth-V36-C10-T60-K100", "smooth-V37-C10-T60-K100", "greedy-V37-C8-T128-K100"]


@pytest.mark.parametrize("name", DECODER_CASES)
def test_decoder_sequence(hb, name, monkeypatch):
    """ops.decoder_sequence forward and backward at B = 5, L = 3 / 4, width 512, with dropout, on every combination of the
    persistent and per-step kernels the case names (teacher-forced C10-T60-K1: persistent both ways; C16-T161-K10: per-step
    both ways; smooth V = 36: persistent backward; V = 37: per-step backward with dec_feedback_bwd; greedy V = 37) - the
    whole check of test_decoder_shapes_gpu against float64 under its limits.  hb.DecBuffers is some twenty torch.empty
    tensors: poisoned when allocated, and - the lease goes back to the pool after every backward - poisoned again where it
    lies between one pattern's forward and the next.  The float64 reference is computed once."""
    import ops
    import test_decoder_shapes_gpu as TDS
    case = [c.values[0] for c in TDS.TEACHER_CASES + TDS.FREE_CASES if c.values[0]["name"] == name]
    assert len(case) == 1, name
    case, cache, reference = case[0], {}, TDS._reference

    def once(c, x, dtype):
        key = (c["name"], dtype)
        if key not in cache:
            with torch.random.fork_rng():
                cache[key] = reference(c, x, dtype)
        return cache[key]
    monkeypatch.setattr(TDS, "_reference", once)
    seen = []

    def check():
        TDS._case(case)
        seen.append(sum(len(v) for k, v in ops._POOL.free.items() if k[0] == "dec"))
    total = _under_patterns("decoder_sequence " + name, check)
    assert seen[0] > 0 and total.pool_tensors > 0, "the DecBuffers lease was poisoned between two forwards"


def test_ctc_align_and_recognize_ctc(hb):
    """ops.ctc_align at V = 34, group block (back-pointers in LDS) and at the L = 200 case whose back-pointers go to the
    workspace, each through test_ctc_align_gpu's check against float64 (path -1 behind the length and in infeasible rows,
    first / last -1, score -inf); E2E.align / recognize_ctc through that module's model test."""
    import test_ctc_align_gpu as TA

    def fields(r):
        return tuple(getattr(r, k).cpu() for k in ("path", "score", "first", "last", "token_logp"))

    def grid():
        c = TA._case(34, "block", 1.0)
        r = TA._run(hb, c)
        TA._check(c, r, "poisoned V=34 block")
        return fields(r)

    def overflow():
        c = TA._overflow_case(hb)
        r = TA._run(hb, c)
        TA._check(c, r, "poisoned workspace back-pointers")
        return fields(r)
    _under_patterns("ctc_align V=34 block", grid)
    _under_patterns("ctc_align L=200 (workspace back-pointers)", overflow)
    _under_patterns("E2E.align + recognize_ctc", lambda: TA.test_model_align_and_recognize_ctc(hb))


def test_ctc_beam_plain_ngram_and_word_lm(hb):
    """ops.ctc_beam at ctc_beam_ref.grid_case(34, 4, 100, 1.0) - plain, with the n-gram LM and with the word LM inside - and at
    the EXTRA case (5, 16, 257, 50.0) whose 257 x 16 history entries exceed the 4096 of LDS and go to the workspace: the
    checks of test_ctc_beam_gpu / test_ngram_gpu / test_word_lm_gpu against their restatements (hyp padded with -1, hyp_len
    -1 and score -inf in unused slots are theirs)."""
    import ctc_beam_ref as R
    import ngram_ref as N
    import test_ctc_beam_gpu as TCB
    import test_ngram_gpu as TN
    import test_word_lm_gpu as TW
    import word_lm_ref as WR
    assert (5, 16, 257, 50.0) in R.EXTRA and 257 * 16 > 4096

    def plain(case):
        def check():
            TCB._check_case(*case, [0.0])
            z, lens = R.grid_case(*case)
            return TCB._search(z, lens, case[0], case[1])[:3]
        return check
    _under_patterns("ctc_beam plain V=34 K=4 T=100", plain((34, 4, 100, 1.0)))
    _under_patterns("ctc_beam plain V=5 K=16 T=257 (workspace hist)", plain((5, 16, 257, 50.0)))
    ng = [c for c in N.grid()[0] if tuple(c[:4]) == (34, 4, 100, 1.0)]
    wl = [c for c in WR.grid()[0] if tuple(c[:4]) == (34, 4, 100, 1.0)]
    assert ng and wl
    _under_patterns("ctc_beam n-gram V=34 K=4 T=100", lambda: TN._check_case(ng[0], [0.0]))
    _under_patterns("ctc_beam word-LM V=34 K=4 T=100", lambda: TW._check_case(wl[0], [0.0]))


def test_ctc_prefix_state_and_beam_search(hb):
    """hb.CtcPrefixState: the constructor's init and four chained score / advance steps (test_beam_ctc_gpu._kernel_case at
    V = 34, T' = 100, K = 4; lse, state, last and psi_prev are torch.empty).  hb.BeamSearch, whose tok_hist, bp_hist, fin and
    fin_score are torch.empty: select against a stable sort (first and last step), reorder as an exact permutation, and whole
    searches - every step's select and reorder, then the backtrack - against the float64 restatement at K = 4, B = 5."""
    import test_beam_ctc_gpu as TBC
    import test_beam_gpu as TB
    _under_patterns("CtcPrefixState init, 4 x score + advance", lambda: TBC._report("poisoned V=34 T'=100 K=4", TBC._kernel_case(hb, 34, 100, 4, 3.0)))
    _under_patterns("BeamSearch.select K=4 V=33", lambda: (TB.test_select_kernel_against_a_stable_sort(hb, 4, 33, False),
                                                         TB.test_select_kernel_against_a_stable_sort(hb, 4, 33, True))[0])
    _under_patterns("BeamSearch.reorder", lambda: TB.test_reorder_is_an_exact_permutation(hb))
    _under_patterns("BeamSearch select, reorder, backtrack K=4 B=5", lambda: TB.test_beams_against_the_float64_restatement(hb, 4, 320, 128, 30, 5))


def test_scoring(hb):
    """Word edit distance (segmentation, word identity, K hypotheses per reference with totals), ops.ngram_score and
    ops.word_lm_score against float64: the checks of test_wer_gpu, test_ngram_gpu and test_word_lm_gpu."""
    import test_ngram_gpu as TN
    import test_wer_gpu as TWER
    import test_word_lm_gpu as TW
    _under_patterns("word_edit_distance", lambda: (TWER.test_segmentation(hb), TWER.test_words_are_equal_only_when_their_tokens_are(hb),
                                                   TWER.test_k_hypotheses_per_reference_and_totals_over_two_launches(hb))[0], "exact")
    _under_patterns("ngram_score V=257 order 4", lambda: TN.test_ngram_score_against_float64(hb, 257, 4))
    _under_patterns("word_lm_score V=34 order 3", lambda: TW.test_word_lm_score_against_float64(hb, 34, 3))


def test_front_end(hb):
    """fbank (log), CMVN per utterance and deltas of order 2 through Frontend on four ragged waveforms (its buffers are
    torch.empty; zeros behind every length are that test's assertion); the resampler, the
    reverb and the noise mix through Frontend.run and the mix on its own (its float64 partial sums live in a torch.empty
    workspace): the checks of test_frontend_gpu, test_resample_gpu and test_augment_gpu against their restatements."""
    import test_augment_gpu as TAU
    import test_frontend_gpu as TF
    import test_resample_gpu as TR
    _under_patterns("Frontend fbank, CMVN, deltas 2, 4 ragged", lambda: TF.test_frontend_against_the_restatement(hb))
    _under_patterns("Frontend + resample", lambda: TR.test_frontend_run_with_factor_indices(hb))
    _under_patterns("Frontend + reverb + noise", lambda: TAU.test_frontend_composes_the_launches(hb, np.int16))
    _under_patterns("noise_mix", lambda: TAU.test_mix_parity(hb, np.float32, False))


def test_seeded_dropout_and_relu_of(hb):
    """The seeded dropout kernels (mask, in place, the relu-dropout backward) and the pad-fill gradient of rows_unpack with
    relu_of and a seeded mask: the checks of test_hip_parity.test_seeded_dropout_kernels and
    test_deterministic_gpu.test_pad_fill_grad_det."""
    import test_deterministic_gpu as TD
    import test_hip_parity as TP
    _under_patterns("seeded dropout p=0.3", lambda: TP.test_seeded_dropout_kernels(0.3))
    _under_patterns("rows_unpack_bwd relu_of + seeded mask", lambda: TD.test_pad_fill_grad_det(hb, 8, True, True))
