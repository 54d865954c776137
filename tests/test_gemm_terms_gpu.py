"""The GEMM kernels of csrc/gemm.hip, element by element, against the float64 sum of exactly the split-term products each
arithmetic keeps (tests/gemm_terms_ref.py: the model, the unit 2^-24 S, the fp32 yardstick Y, the rule max e <= 4 Y - no
other tolerance).  One test per kernel family over the four operand layouts and both bf16 arithmetics; every call first
asserts that the library plans the kernel the case names, so a change of launch policy fails here instead of moving the
coverage somewhere else.  Operands are views into NaN-filled buffers, outputs views into a buffer of sentinels whose
padding must survive.  Each check prints `gemm_parity <case> <kernel>: e_max, Y, ratio` (profiles/gemm_parity.txt)."""
import numpy as np
import pytest
import torch

import gemm_terms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _dev(x):
    return torch.tensor(np.asarray(x)).to(DEV)


def _views(c, batch=None):
    """The stored operands of a case on the GPU: (A view, B view, lda, ldb, sA, sB); batch: stacked buffers, 3-D views."""
    st = [R.storage(c, b) for b in range(batch or 1)]
    a_off, b_off = st[0][1], st[0][3]
    a = torch.from_numpy(np.stack([s[0] for s in st])).to(DEV)
    b = torch.from_numpy(np.stack([s[2] for s in st])).to(DEV)
    ar, ac = (c.K, c.M) if c.ta else (c.M, c.K)
    br, bc = (c.N, c.K) if c.tb else (c.K, c.N)
    av, bv = a[:, :ar, a_off:a_off + ac], b[:, :br, b_off:b_off + bc]
    for v in (av, bv):
        assert (v.data_ptr() % 16 != 0) == c.mis and (v.stride(1) % 2 == 1) == c.mis and not bool(torch.isnan(v).any())
    if batch is None:
        av, bv = av[0], bv[0]
    return av, bv, a.shape[2], b.shape[2], a.shape[1] * a.shape[2], b.shape[1] * b.shape[2]


def _product_case(hb, c):
    """One call of the case table: plan asserted, product run, padding and per-element parity checked."""
    M, N, K = c.M, c.N, c.K
    _, _, bias, base = R.operands(M, N, K)
    if c.entry == "batched":
        return _batched_case(hb, c)
    av, bv, lda, ldb, _, _ = _views(c)
    out, off = R.out_buffer(M, N, base if c.epi == "acc" else None, dense=c.epi == "drop")
    od = torch.from_numpy(out).to(DEV)
    view = od[:M, off:off + N]
    mask = None
    if c.entry == "side":
        queue = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert hb.gemm_side(av, bv, view, queue, c.mask, trans_a=c.ta, trans_b=c.tb, arith=c.mode)
        assert int(queue.item()) > 0
    else:
        R.assert_plan(c, hb.gemm_plan(M, N, K, **R.plan_kwargs(c, lda, ldb, od.shape[1])))
        drop = None
        if c.epi == "drop":
            drop = hb.SeededMask((M, N), R.DROP_P, DEV, seed=R.DROP_SEED)
            mask = drop.tensor().cpu().numpy()
            assert 0.1 < float((mask == 0).mean()) < 0.4
        hb.gemm(av, bv, trans_a=c.ta, trans_b=c.tb, bias=_dev(bias) if c.epi in ("bias", "bias_relu", "drop") else None,
                relu=c.epi in ("bias_relu", "drop"), out=view, accumulate=c.epi == "acc", split_k=c.split_k, arith=c.mode, drop=drop)
    got = od.cpu().numpy()
    assert R.padding_kept(got, M, N, off), "%s: the padding of the output lost its sentinel" % c.name
    R.check(c.name, c.kernel, got[:M, off:off + N], R.reference(M, N, K, c.arith, c.epi, 0, mask))


def _batched_case(hb, c):
    M, N, K, nb = c.M, c.N, c.K, c.batch
    av, bv, lda, ldb, sA, sB = _views(c, nb)
    bases = [R.operands(M, N, K, b)[3] for b in range(nb)]
    out, off = R.out_buffer(M, N, np.stack(bases) if c.epi == "acc" else None, batch=nb)
    od = torch.from_numpy(out).to(DEV)
    ldc, sC = od.shape[2], od.shape[1] * od.shape[2]
    R.assert_plan(c, hb.gemm_plan(M, N, K, **R.plan_kwargs(c, lda, ldb, ldc, sA, sB, sC)))
    hb.gemm_batched(av, bv, od[:, :, off:], c.ta, c.tb, M, N, K, lda, ldb, ldc, nb, sA, sB, sC, accumulate=c.epi == "acc",
                    arith=c.mode, split_k=c.split_k)
    got = od.cpu().numpy()
    assert R.padding_kept(got, M, N, off), "%s: the padding of the output lost its sentinel" % c.name
    for b in range(nb):
        R.check("%s[%d]" % (c.name, b), c.kernel, got[b, :M, off:off + N], R.reference(M, N, K, c.arith, c.epi, b))


def _family(hb, family, layout, arith):
    cases = R.family_cases(family, layout, arith)
    assert cases
    for c in cases:
        _product_case(hb, c)


_BOTH = [p for p in R.family_params("bf3_128")]


@pytest.mark.parametrize("layout,arith", R.family_params("f32"))
def test_f32_kernel(hb, layout, arith):
    """gemm_f32_kernel (the fp32-input MFMA): K tails 40 and 33 (K % 4 != 0), edge tiles in M and N, two tile rows."""
    _family(hb, "f32", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_bf3_kernel_128(hb, layout, arith):
    """gemm_bf3_kernel, 128 x 128 tiles (+narrow): every staging branch of tile_store_bf3 at TS = 128 (KC and both
    row-contiguous forms come with the layouts), K tail and K % 4 != 0, one interior tile with two K tiles, split_k = 3 at
    K = 96 (zero pass + atomics, atomics onto a base, late bias / ReLU pass), misaligned views with odd leading dimensions."""
    _family(hb, "bf3_128", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_bf3_kernel_64(hb, layout, arith):
    """gemm_bf3_kernel, 64 x 64 tiles (+small): the TS = 64 staging branches, K = 32 / 36 / 64, split_k = 2, a misaligned
    view, and the dropout epilogue (bias_act_kernel with the seeded mask) against the model times SeededMask.tensor()."""
    _family(hb, "bf3_64", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_wide_kernels(hb, layout, arith):
    """gemm_bf6w_kernel / gemm_bf3w_kernel (+wide, LDS-DMA): one stage at 64 x 64 x 32 (a clamped edge tile), two and three
    stages with edge tiles in M and N at 260 x 132, and the kernel's own K split at K = 1024 (rule only: no power left)."""
    _family(hb, "wide", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_bfs_kernel(hb, layout, arith):
    """gemm_bfs_kernel (+sp, one wave per SIMD): K = 64 unmasked (KT = false), masked K tails 36, 68, 92 (KT = true)."""
    _family(hb, "bfs", layout, arith)


@pytest.mark.parametrize("layout,arith", R.family_params("bfk"))
def test_bfk_kernel(hb, layout, arith):
    """gemm_bfk_kernel (K = 80, k-contiguous operands, the default policy): 1024 x 128 plain and with bias on the branch-free
    epilogue (PLAIN), with ReLU and accumulate on the guarded one; 1100 x 200 (edge tiles in M and N) guarded throughout."""
    _family(hb, "bfk", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_queue_instantiation(hb, layout, arith):
    """gemm_bf3_kernel<..., 64, QUEUE> through asr_gemm_side_f32 on all XCDs and on four, accumulating onto a non-zero out."""
    _family(hb, "queue", layout, arith)


@pytest.mark.parametrize("layout,arith", _BOTH)
def test_batched_entry(hb, layout, arith):
    """asr_gemm_f32 with batch = 2 and operand / output strides on the smallest shape of the 64 x 64, LDS-DMA and
    one-wave-per-SIMD kernels: each batch element has its own operands and its own model."""
    _family(hb, "batched", layout, arith)


@pytest.mark.parametrize("M,N,K,mt", R.SKINNY)
def test_skinny_kernel(hb, M, N, K, mt):
    """skinny_kernel<1> (M <= 32) and <2>: fp32 FMAs, so the model is the float64 product; plain, bias, accumulate."""
    c = R._case("f32", M, N, K, "NT", "f32")
    A, B, bias, base = R.operands(M, N, K)
    av, bv, _, _, _, _ = _views(c)
    for epi in ("plain", "bias", "acc"):
        out, off = R.out_buffer(M, N, base if epi == "acc" else None)
        od = torch.from_numpy(out).to(DEV)
        hb.gemm_skinny(av, bv, bias=_dev(bias) if epi == "bias" else None, out=od[:M, off:off + N],
                       accumulate=epi == "acc")
        got = od.cpu().numpy()
        assert R.padding_kept(got, M, N, off)
        R.check("skinny/%dx%dx%d/%s" % (M, N, K, epi), "skinny_kernel<%d>" % mt, got[:M, off:off + N], R.reference(M, N, K, "f32", epi))


@pytest.mark.parametrize("M,N,kernel", R.COLSUM)
def test_colsum_kernels(hb, M, N, kernel):
    """colsum4_kernel (N and ld multiples of four) and colsum_kernel (N = 130, two 512-row chunks), plain and accumulating."""
    for acc in (False, True):
        X, old, model, S, Y = R.colsum_reference(M, N, acc)
        buf, off = R.padded(X)
        xd = torch.from_numpy(buf).to(DEV)
        assert (kernel == "colsum4_kernel") == (N % 4 == 0 and buf.shape[1] % 4 == 0)
        out, _ = R.out_buffer(0, N + 5, dense=True)                  # one row of N + 5 sentinels, the sums go to [2, 2 + N)
        if acc:
            out[0, 2:2 + N] = old
        od = torch.from_numpy(out).to(DEV)
        hb.colsum(xd[:M, off:off + N], out=od[0, 2:2 + N], accumulate=acc)
        got = od.cpu().numpy()
        assert R.padding_kept(got, 1, N, 2)
        ref = R.Ref(model, S, Y, None, None, None, None, None, None)
        R.check("colsum/%dx%d/%s" % (M, N, "acc" if acc else "plain"), kernel, got[0, 2:2 + N], ref)
