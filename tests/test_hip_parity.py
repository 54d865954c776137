"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed golden
fixtures.  Tolerance: 1e-3 relative fp32 (BASELINE.json north_star); most checks are much tighter."""
import os

import numpy as np
import pytest
import torch

import synth
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-3


def _gpu():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _close(got, want, rtol=RTOL, atol=1e-5, what=""):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= atol + rtol * scale, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


def _load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


# ----------------------------------------------------------------------------------------- GEMMs
# Product arithmetics of asr_gemm_f32 (include/asr_hip.h) and the tolerance each is held to, relative to the largest
# output: the default bf16x6 (three-term split, six products) is fp32-equivalent and gets the fp32 tolerance.
GEMM_ARITH = [("bf16x6", 1e-5), ("f32", 1e-5), ("bf16x3", 3e-5)]
GEMM_ATOL = 1e-4
# the LSTM layer against the oracle: outputs, gradients (shared with tests/test_poison_gpu.py)
LSTM_Y_GATE = dict(rtol=1e-4, atol=1e-5)
LSTM_GRAD_GATE = dict(rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("arith,rtol", GEMM_ARITH)
@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (257, 130, 70), (33, 34, 9), (1000, 96, 513), (1, 1, 1), (7, 5, 3)])
def test_gemm_variants(ta, tb, M, N, K, arith, rtol):
    """asr_gemm_f32 in its four operand layouts, with epilogue / split-K / accumulate, in its three product arithmetics:
    bf16x6 (default: three bf16 terms per operand, six MFMA products, fp32-equivalent), the fp32-input MFMA, and bf16x3
    (two terms, three products, <= 2^-16 relative per product).  Tolerances relative to the largest output: 1e-5 for the
    first two, 3e-5 for bf16x3 - the parity gate is 1e-3."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    tol = dict(rtol=rtol, atol=GEMM_ATOL)
    with hb.arith(arith):
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
        _close(out, ref.float(), what="plain", **tol)
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, bias=bias.to(dev), relu=True)
        _close(out, torch.relu(ref + bias).float(), what="bias+relu", **tol)
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, split_k=3)
        _close(out, ref.float(), what="split-k", **tol)
        base = torch.randn(M, N, generator=g)
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, out=base.to(dev), accumulate=True)
        _close(out, (ref + base).float(), what="accumulate", **tol)
    # the arithmetic is an argument of the call, not process state: an explicit one wins over the host default
    with hb.arith("bf16x3"):
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, arith=arith)
    _close(out, ref.float(), what="explicit arith", **tol)


@pytest.mark.parametrize("arith,rtol", GEMM_ARITH)
@pytest.mark.parametrize("ta,tb,M,N,K", [(False, True, 25600, 4096, 80),      # layer-0 input-gate projection [T*B,80]x[80,8H]
                                         (True, False, 4096, 80, 25600),     # layer-0 dW_ih = dG^T X
                                         (False, False, 6400, 512, 4096),    # dX = dG W_ih (layer 2)
                                         (True, False, 512, 2048, 12800)])   # projection weight gradient
def test_gemm_step_shapes(ta, tb, M, N, K, arith, rtol):
    """The shapes of the cfg-2 train step with a thin dimension (K = 80, N = 80) or a long contraction (K = T*B), against a
    float64 product of the same fp32 inputs."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = ((A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())).float()
    out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, arith=arith)
    _close(out, ref, rtol=rtol, atol=1e-4, what="%dx%dx%d" % (M, N, K))


@pytest.mark.parametrize("ta,tb,M,N,K", [(False, True, 1024, 512, 4096), (True, False, 512, 2048, 12800),
                                         (False, False, 300, 200, 1030), (False, True, 257, 130, 70)])
def test_gemm_bf16x6_is_fp32_equivalent(ta, tb, M, N, K):
    """The default arithmetic against the exact fp32-input MFMA kernel, both measured against a float64 product of the
    same fp32 operands: the three-term split is lossless (a + b + c == x) and the dropped products are below 2^-24, so the
    error of bf16x6 must stay within 2x of the fp32 kernel's own (fp32 accumulation order is all that differs) - on the
    wide LDS-DMA kernel, on the 128 x 128 kernel, with and without a K split.  bf16x3 is measurably further away."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M + 3 * N + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    scale = float(ref.abs().max())

    def err(**kw):
        out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, **kw)
        return float((out.double().cpu() - ref).abs().max()) / scale
    e32 = err(arith="f32", split_k=1)
    for kw in (dict(arith="bf16x6"), dict(arith="bf16x6", split_k=1), dict(arith="bf16x6+narrow", split_k=1),
               dict(arith="bf16x6+wide", split_k=1), dict(arith="bf16x6+sp", split_k=1), dict(arith="bf16x6+sp"),
               dict(arith="bf16x6+small", split_k=1), dict(arith="bf16x6+small")):
        e6 = err(**kw)
        assert e6 <= 2.0 * e32 + 2e-8, "bf16x6 %s: error %.3g vs fp32 kernel %.3g" % (kw, e6, e32)
    e3 = err(arith="bf16x3", split_k=1)
    # (with K in the thousands the fp32 accumulation error itself grows, so the gap narrows: 2.4x at K = 12800)
    assert e3 > 1.5 * e32, "bf16x3 error %.3g is not measurably above fp32's %.3g: is it running the right kernel?" % (e3, e32)


def test_gemm_split_terms_are_lossless():
    """Operands whose low mantissa bits matter: x = 1 + k 2^-23 against y = 2^12 - sums whose fp32 value differs from a
    16-bit-significand evaluation in the leading digits.  bf16x6 reproduces the float64 product to fp32 rounding."""
    dev = _gpu()
    import hip_backend as hb
    K = 64
    k = torch.arange(1, 128 * K + 1, dtype=torch.float64).reshape(128, K)
    A = (1.0 + k * 2.0 ** -23).float()
    B = torch.where(torch.arange(K * 128).reshape(K, 128) % 2 == 0, 4096.0, -4096.0).float()
    ref = A.double() @ B.double()                  # the 1 * 4096 terms cancel pairwise: what is left lives in the low bits
    out6 = hb.gemm(A.to(dev), B.to(dev), arith="bf16x6", split_k=1).double().cpu()
    out32 = hb.gemm(A.to(dev), B.to(dev), arith="f32", split_k=1).double().cpu()
    assert float((out32 - ref).abs().max()) <= 1e-6 * 4096.0 * K
    assert float((out6 - ref).abs().max()) <= 1e-6 * 4096.0 * K, float((out6 - ref).abs().max())


@pytest.mark.parametrize("arith,rtol", [("bf16x6", 1e-5), ("bf16x3", 3e-5)])
@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(256, 128, 32), (256, 128, 64), (512, 256, 96), (256, 384, 4096), (1024, 128, 1024),
                                   (300, 80, 64), (1000, 200, 512), (64, 64, 32), (4096, 80, 3200), (3232, 1152, 2048),
                                   (2560, 512, 80), (260, 132, 100)])
def test_gemm_wide_tile(ta, tb, M, N, K, arith, rtol):
    """(Also "+small": the 64 x 64 tiles of the 128 x 128 kernel's code, the default for products whose large tiles would not fill the chip.)
    The 256 x 128 kernels - LDS-DMA (gemm_bf6w_kernel / gemm_bf3w_kernel: K % 32 == 0) and one wave per SIMD with the
    split once per workgroup (gemm_bfs_kernel, "+sp": also a masked K tail, K = 80 / 100) - of the bf16 arithmetics in
    the four operand layouts: 1, 2, 3 and many ring stages, their own K split (long K on few tiles), edge tiles in M and N
    (clamped DMA sources, guarded stores; the thin N = 80 weight gradient and the decoder's M = 3232), epilogue,
    accumulate, and the same call under the shipping policy and with the wide kernel off giving the same numbers.  An
    explicit split_k = 1 is an unsplit product on every path: two runs are bit-identical."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M * 5 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    base = torch.randn(M, N, generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    tol = dict(rtol=rtol, atol=1e-4)
    for mode in (arith + "+wide", arith + "+sp", arith, arith + "+narrow", arith + "+small"):
        with hb.arith(mode):
            out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
            _close(out, ref.float(), what="plain/%s" % mode, **tol)
            out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, bias=bias.to(dev), relu=True)
            _close(out, torch.relu(ref + bias).float(), what="bias+relu/%s" % mode, **tol)
            out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, bias=bias.to(dev), relu=True, split_k=1)
            _close(out, torch.relu(ref + bias).float(), what="bias+relu unsplit/%s" % mode, **tol)
            out = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, out=base.to(dev), accumulate=True)
            _close(out, (ref + base).float(), what="accumulate/%s" % mode, **tol)
            o1 = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, split_k=1)
            o2 = hb.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb, split_k=1)
            _close(o1, ref.float(), what="unsplit/%s" % mode, **tol)
            assert torch.equal(o1, o2), "split_k = 1 must be an unsplit, run-to-run identical product (%s)" % mode
    # row-strided operands and output (views of wider buffers)
    wideA = torch.randn((K, M + 64) if ta else (M, K + 64), generator=g).to(dev)
    Av = wideA[:, 32:32 + M] if ta else wideA[:, 32:32 + K]
    refv = (Av.cpu().double().t() if ta else Av.cpu().double()) @ (B.double().t() if tb else B.double())
    for flag in ("+wide", "+sp", "+small"):
        outw = torch.zeros(M, N + 32, device=dev)
        with hb.arith(arith + flag):
            hb.gemm(Av, B.to(dev), trans_a=ta, trans_b=tb, out=outw[:, 16:16 + N])
        _close(outw[:, 16:16 + N], refv.float(), what="strided" + flag, **tol)
        assert float(outw[:, :16].abs().max()) == 0.0 and float(outw[:, 16 + N:].abs().max()) == 0.0


@pytest.mark.parametrize("arith,rtol", [("bf16x6", 1e-5), ("bf16x3", 3e-5)])
@pytest.mark.parametrize("M,N", [(1024, 128), (1100, 200), (3000, 4000), (2048, 130), (1025, 257), (12800, 512)])
def test_gemm_short_k_weights_stationary(M, N, arith, rtol):
    """gemm_bfk_kernel (K = 80, k-contiguous operands: the layer-0 input projection x W_ih^T + b): the weight tile stays in
    registers, workgroups walk down the M tiles with the previous tile's stores under the current tile's MFMAs.  Interior
    shapes take the branch-free epilogue (bias only), the rest the guarded one (edge tiles in M and N, relu, accumulate);
    row-strided operands and output; batched.  Against a float64 product, and against the 128 x 128 kernel's numbers."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M + N)
    A, B = torch.randn(M, 80, generator=g), torch.randn(N, 80, generator=g)
    bias, base = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = A.double() @ B.double().t()
    tol = dict(rtol=rtol, atol=1e-4)
    with hb.arith(arith):
        _close(hb.gemm(A.to(dev), B.to(dev), trans_b=True), ref.float(), what="plain", **tol)
        _close(hb.gemm(A.to(dev), B.to(dev), trans_b=True, bias=bias.to(dev)), (ref + bias).float(), what="bias", **tol)
        _close(hb.gemm(A.to(dev), B.to(dev), trans_b=True, bias=bias.to(dev), relu=True), torch.relu(ref + bias).float(), what="bias+relu", **tol)
        _close(hb.gemm(A.to(dev), B.to(dev), trans_b=True, out=base.clone().to(dev), accumulate=True), (ref + base).float(), what="accumulate", **tol)
        o1 = hb.gemm(A.to(dev), B.to(dev), trans_b=True, bias=bias.to(dev))
        o2 = hb.gemm(A.to(dev), B.to(dev), trans_b=True, bias=bias.to(dev), arith=arith + "+narrow", split_k=1)
        _close(o1, o2, rtol=rtol, atol=1e-5, what="vs the 128 x 128 kernel")
        wideA = torch.randn(M, 96, generator=g).to(dev)
        wideB = torch.randn(N, 88, generator=g).to(dev)
        outw = torch.zeros(M, N + 32, device=dev)
        hb.gemm(wideA[:, 8:88], wideB[:, 4:84], trans_b=True, out=outw[:, 16:16 + N])
        refv = wideA[:, 8:88].cpu().double() @ wideB[:, 4:84].cpu().double().t()
        _close(outw[:, 16:16 + N], refv.float(), what="strided", **tol)
        assert float(outw[:, :16].abs().max()) == 0.0 and float(outw[:, 16 + N:].abs().max()) == 0.0
    if M <= 2048:
        Ab, Bb = torch.randn(2, M, 80, generator=g).to(dev), torch.randn(2, N, 80, generator=g).to(dev)
        C = torch.full((2, M, N), 3.0, device=dev)
        hb.gemm_batched(Ab, Bb, C, False, True, M, N, 80, 80, 80, N, 2, M * 80, N * 80, M * N, arith=arith)
        _close(C, torch.einsum("bmk,bnk->bmn", Ab.cpu().double(), Bb.cpu().double()).float(), what="batched", **tol)


@pytest.mark.parametrize("arith,rtol", [("bf16x6", 1e-5), ("bf16x3", 3e-5)])
def test_gemm_wide_tile_batched(arith, rtol):
    """The batched form (pointer + strides, one launch) through the 256 x 128 kernel: C[b] = A[:, b, :]^T B[:, b, :] with
    K % 32 == 0, edge tiles in M and N, batch folded into grid.y next to the kernel's own K split."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(2)
    L, Bn, Tp, Od = 2048, 3, 40, 72
    A = torch.randn(L, Bn, Tp, generator=g).to(dev)
    Bm = torch.randn(L, Bn, Od, generator=g).to(dev)
    want = torch.einsum("lbt,lbo->bto", A.cpu().double(), Bm.cpu().double()).float()
    for mode in (arith + "+wide", arith + "+sp", arith + "+narrow", arith + "+small"):
        C = torch.full((Bn, Tp, Od), 3.0, device=dev)
        hb.gemm_batched(A, Bm, C, True, False, Tp, Od, L, Bn * Tp, Bn * Od, Od, Bn, Tp, Od, Tp * Od, arith=mode)
        _close(C, want, rtol=rtol, atol=1e-4, what="batched/%s" % mode)


def test_gemm_strided_views_and_batched():
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(1)
    big = torch.randn(64, 100, generator=g).to(dev)
    W = torch.randn(48, 40, generator=g).to(dev)
    out = torch.zeros(64, 80, device=dev)
    hb.gemm(big[:, 20:60], W, trans_b=True, out=out[:, 16:64])
    _close(out[:, 16:64], big[:, 20:60].cpu() @ W.cpu().t(), rtol=1e-5, atol=1e-4)      # default arithmetic (bf16x6)
    assert float(out[:, :16].abs().max()) == 0.0
    # batched: C[b] = A[:, b, :]^T B[:, b, :]
    L, Bn, Tp, Od = 7, 3, 10, 12
    A = torch.randn(L, Bn, Tp, generator=g).to(dev)
    Bm = torch.randn(L, Bn, Od, generator=g).to(dev)
    C = torch.empty(Bn, Tp, Od, device=dev)
    hb.gemm_batched(A, Bm, C, True, False, Tp, Od, L, Bn * Tp, Bn * Od, Od, Bn, Tp, Od, Tp * Od)
    _close(C, torch.einsum("lbt,lbo->bto", A.cpu(), Bm.cpu()), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(32, 2048, 512), (3, 9, 32), (20, 34, 1024), (40, 100, 64)])
def test_gemm_skinny_and_colsum(M, N, K):
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(M + N + K)
    A, Bt, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    out = hb.gemm_skinny(A.to(dev), Bt.to(dev), bias=bias.to(dev))
    _close(out, A @ Bt.t() + bias, rtol=1e-5, atol=1e-4)
    acc = torch.randn(M, N, generator=g)
    out = hb.gemm_skinny(A.to(dev), Bt.to(dev), out=acc.to(dev), accumulate=True)
    _close(out, A @ Bt.t() + acc, rtol=1e-5, atol=1e-4)
    _close(hb.colsum(A.to(dev)), A.sum(0), rtol=1e-5, atol=1e-4)


# ----------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("T", [10, 11, 1])
def test_pyramid_concat(T):
    dev = _gpu()
    import ops
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, 3, 8, generator=g)
    mask = (torch.rand(T, 3, 8, generator=g) > 0.3).float() / 0.7
    for m in (None, mask):
        xr = x.clone().requires_grad_(True)
        ref = O.pair_concat((xr if m is None else xr * m).transpose(0, 1)).transpose(0, 1)
        xg = x.to(dev).requires_grad_(True)
        got = ops.pyramid_concat(xg, None if m is None else m.to(dev))
        _close(got, ref, rtol=0, atol=0)
        dy = torch.randn(ref.shape, generator=g)
        ref.backward(dy)
        got.backward(dy.to(dev))
        _close(xg.grad, xr.grad, rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------------------- LSTM layer
@pytest.mark.parametrize("ndir,B,T,I,H,lens", [
    (2, 3, 9, 8, 16, [9, 7, 4]), (1, 5, 6, 16, 32, [6, 6, 3, 2, 1]), (2, 33, 5, 12, 64, None),
    (2, 20, 7, 10, 48, None)])
def test_lstm_layer_fwd_bwd(ndir, B, T, I, H, lens):
    dev = _gpu()
    import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    if lens is None:
        lens = sorted([int(v) for v in torch.randint(1, T + 1, (B,), generator=g)], reverse=True)
        lens[0] = T
    x = torch.randn(B, T, I, generator=g)
    k = 1.0 / np.sqrt(H)
    prm = []
    for d in range(ndir):
        prm += [torch.empty(4 * H, I).uniform_(-k, k, generator=g), torch.empty(4 * H, H).uniform_(-k, k, generator=g),
                torch.empty(4 * H).uniform_(-k, k, generator=g), torch.empty(4 * H).uniform_(-k, k, generator=g)]
    cp = [p.clone().requires_grad_(True) for p in prm]
    xc = x.clone().requires_grad_(True)
    ref = torch.cat([O.lstm_direction(xc, lens, *cp[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(ndir)], 2)
    gp = [p.to(dev).requires_grad_(True) for p in prm]
    xg = x.to(dev).requires_grad_(True)
    got = ops.lstm_layer(xg.transpose(0, 1), torch.tensor(lens, dtype=torch.int32, device=dev), gp, ndir)
    _close(got.transpose(0, 1), ref, what="y", **LSTM_Y_GATE)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    got.backward(dy.transpose(0, 1).contiguous().to(dev))
    _close(xg.grad, xc.grad, what="dx", **LSTM_GRAD_GATE)
    for i, (a, b) in enumerate(zip(gp, cp)):
        _close(a.grad, b.grad, what="param %d" % i, **LSTM_GRAD_GATE)


# ----------------------------------------------------------------------------------------- full model
def _product(cfg, weights, ld, dev):
    import model as M
    net = M.E2E(labeldist=ld, **cfg).to(dev)
    missing = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    net.train()
    return net


def _grads(net):
    return {n: p.grad for n, p in net.named_parameters()}


def test_state_dict_keys_match_reference(golden_dir):
    dev = _gpu()
    net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), synth.labeldist(9, 12), dev)
    assert list(net.state_dict().keys()) == list(synth.e2e_weights(synth.TINY, 11).keys())
    assert len(net.state_dict()) == 43


def test_tiny_e2e_teacher_forced(golden_dir):
    dev = _gpu()
    g = _load(golden_dir, "tiny_e2e.npz")
    net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), g["labeldist"], dev)
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    enc_h, enc_lens = net.encoder(xs_d, ilens)
    assert enc_lens == g["enc_lens"].tolist()
    _close(enc_h, g["enc_h"], what="enc_h")
    np.random.seed(5)
    logits, lp, pred, ws = net(xs_d, ilens, ys_d, tf_rate=1.0)
    _close(logits, g["tf_logits"], what="logits"); _close(lp, g["tf_lp"], what="lp"); _close(ws, g["tf_ws"], what="ws")
    assert (pred.cpu().numpy() == g["tf_pred"]).all()
    loss = -lp.mean()
    _close(loss, g["tf_loss"], rtol=1e-5, what="loss")
    _close(net.mask_and_cal_loss(lp, ys_d), g["tf_masked_loss"], rtol=1e-5)
    net.zero_grad()
    loss.backward()
    for n, gr in _grads(net).items():
        _close(gr, g["grad/" + n], atol=1e-6, what="grad " + n)


def test_tiny_e2e_free_running_modes(golden_dir):
    dev = _gpu()
    g = _load(golden_dir, "tiny_e2e.npz")
    net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), g["labeldist"], dev)
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    np.random.seed(7)
    logits, lp, pred, _ = net(xs_d, ilens, ys_d, tf_rate=0.5)
    assert (pred.cpu().numpy() == g["ss_pred"]).all()
    _close(logits, g["ss_logits"], what="ss logits"); _close(lp, g["ss_lp"], what="ss lp")
    logits, lp, pred, ws = net(xs_d, ilens, ys=None, max_dec_timesteps=5)
    assert (pred.cpu().numpy() == g["gr_pred"]).all()
    _close(logits, g["gr_logits"], what="greedy logits"); _close(ws, g["gr_ws"], what="greedy ws")
    logits, lp, pred, _ = net(xs_d, ilens, ys=None, max_dec_timesteps=5, smooth=True, scaling=3.0,
                              label_smoothing=False)
    _close(logits, g["sm_logits"], what="smooth logits"); _close(lp, g["sm_lp"], what="smooth lp")
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, g["smgrad/" + n], atol=1e-6, what="smooth grad " + n)
    net.eval()
    np.random.seed(5)
    _, lp_eval, _, _ = net(xs_d, ilens, ys_d)
    _close(lp_eval, g["eval_lp"], what="eval lp")


@pytest.mark.parametrize("arith,rtol", [("bf16x6", 1e-4), ("f32", 1e-4), ("bf16x3", 5e-4)])
def test_tiny_optimizer_steps(golden_dir, arith, rtol):
    """Weights after 1 and 3 clip + Adam(amsgrad) steps vs the reference (solver.py:152-153,382-385), clip active and
    inactive.  Adam divides by sqrt(v): after the first steps an update is ~lr * sign(g), so tiny gradient differences
    show up amplified; the default bf16x6 products and the exact-fp32 products are held to 1e-4 of each tensor's scale,
    the non-default bf16x3 products to 5e-4 (gate: 1e-3)."""
    dev = _gpu()
    import hip_backend as hb
    from parallel import FlatAdam
    g = _load(golden_dir, "tiny_e2e.npz")
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    with hb.arith(arith):
        for clip, prefix, steps in ((5.0, "after", 3), (0.05, "clip", 1)):
            net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), g["labeldist"], dev)
            opt = FlatAdam(net, lr=5e-4, weight_decay=1e-6, amsgrad=True, max_grad_norm=clip)
            for step in range(steps):
                np.random.seed(100 + step)
                _, lp, _, _ = net(xs_d, ilens, ys_d, tf_rate=1.0)
                opt.zero_grad()
                (-lp.mean()).backward()
                gsq = opt.step()
                if prefix == "after":
                    _close(gsq.sqrt(), g["opt_gnorm%d" % step], rtol=1e-3)
                    if step in (0, 2):
                        for n, p in net.named_parameters():
                            _close(p, g["after%d/%s" % (step + 1, n)], rtol=rtol, atol=2e-6, what="after %s" % n)
                else:
                    for n, p in net.named_parameters():
                        _close(p, g["clip/" + n], rtol=rtol, atol=2e-6, what="clip %s" % n)


def _ref_adam_state(g):
    """tiny_opt.npz -> the dict torch.optim.Adam.state_dict() returned in the reference run (what `.opt` files hold)."""
    state = {}
    for k, v in g.items():
        if k.startswith("state/"):
            _, i, name = k.split("/")
            state.setdefault(int(i), {})[name] = torch.from_numpy(np.asarray(v))
    grp = dict(lr=float(g["group/lr"]), betas=tuple(float(b) for b in g["group/betas"]), eps=float(g["group/eps"]),
               weight_decay=float(g["group/weight_decay"]), amsgrad=bool(g["group/amsgrad"]),
               params=[int(i) for i in g["group/params"]])
    return dict(state=state, param_groups=[grp])


def test_resume_from_reference_adam_state(golden_dir):
    """a `.opt` written by the reference (torch.optim.Adam.state_dict() after step 1, solver.py:38-46)
    loads into FlatAdam; steps 2-3 from there land on the reference's weights after 3 steps."""
    dev = _gpu()
    from parallel import FlatAdam
    g = _load(golden_dir, "tiny_e2e.npz")
    o = _load(golden_dir, "tiny_opt.npz")
    after1 = {k[len("after1/"):]: v for k, v in o.items() if k.startswith("after1/")}
    weights = dict(synth.e2e_weights(synth.TINY, 11))
    for k in weights:                                  # incl. the duplicated attention keys
        base = k[len("decoder."):] if k.startswith("decoder.attention.") else k
        weights[k] = after1[base]
    net = _product(synth.TINY, weights, g["labeldist"], dev)
    assert [n for n, _ in net.named_parameters()] == [str(n) for n in o["param_order"]]
    opt = FlatAdam(net, lr=1.0, weight_decay=0.5, amsgrad=True, max_grad_norm=5.0)       # wrong on purpose: the file wins
    opt.load_state_dict(_ref_adam_state(o))
    assert opt.t == 1 and opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[0]["weight_decay"] == 1e-6
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    for step in (1, 2):
        np.random.seed(100 + step)
        _, lp, _, _ = net(xs_d, ilens, ys_d, tf_rate=1.0)
        _close(-lp.mean(), g["opt_loss%d" % step], rtol=1e-4, what="loss of step %d" % step)
        opt.zero_grad()
        (-lp.mean()).backward()
        opt.step()
    for n, p in net.named_parameters():
        _close(p, g["after3/" + n], rtol=5e-4, atol=2e-6, what="after3 %s" % n)
    # and back out: the state FlatAdam saves has torch.optim.Adam's schema (one entry per parameter, same fields)
    sd = opt.state_dict()
    assert sorted(sd["state"].keys()) == list(range(len(list(net.parameters()))))
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert float(sd["state"][0]["step"]) == 3.0


def test_cfg1_against_golden(golden_dir):
    dev = _gpu()
    g = _load(golden_dir, "cfg1.npz")
    net = _product(synth.CFG1, synth.e2e_weights(synth.CFG1, 21), synth.labeldist(34, 23), dev)
    xs, ilens, ys = synth.batch(80, 34, synth.CFG1_ILENS, synth.CFG1_YLENS, 22)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    np.random.seed(5)
    logits, lp, pred, ws = net(xs_d, ilens, ys_d)
    _close(logits, g["logits"], what="logits"); _close(lp, g["lp"], what="lp"); _close(ws, g["ws"], what="ws")
    loss = -lp.mean()
    _close(loss, g["loss"], rtol=1e-5)
    net.zero_grad()
    loss.backward()
    for n, p in net.named_parameters():
        flat = p.grad.detach().cpu().numpy().ravel()
        np.testing.assert_allclose(np.sqrt((flat.astype(np.float64) ** 2).sum()), g["gnorm/" + n], rtol=RTOL)
        scale = float(np.abs(flat).max())
        assert np.abs(flat[:16] - g["ghead/" + n]).max() <= RTOL * scale + 1e-7, n


def test_lm_against_golden(golden_dir):
    dev = _gpu()
    import model as M
    from parallel import FlatAdam
    g = _load(golden_dir, "tiny_lm.npz")
    w = synth.lm_weights(synth.TINY_LM, 31)

    def build():
        lm = M.LM(bos=1, eos=2, pad=0, labeldist=g["labeldist"], **synth.TINY_LM).to(dev)
        assert list(lm.state_dict().keys()) == list(w.keys())
        lm.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        lm.train()
        return lm

    lm = build()
    ys = [torch.from_numpy(g["ys%d" % i]).to(dev) for i in range(3)]
    lp, p, pred = lm(ys, discrete_input=True)
    _close(lp, g["d_lp"]); _close(p, g["d_p"])
    loss = -lm.mask_and_cal_sum(lp, ys)
    _close(loss, g["d_loss"], rtol=1e-5)
    _close(lm.mask_and_cal_sum(p, ys), g["d_avg_prob"], rtol=1e-5)
    lm.zero_grad()
    loss.backward()
    for n, q in lm.named_parameters():
        _close(q.grad, g["grad/" + n], atol=1e-6, what="lm grad " + n)
    lp, p, pred = lm(torch.from_numpy(g["c_ys"]).to(dev), discrete_input=False)
    _close(lp, g["c_lp"]); _close(p, g["c_p"])
    assert (pred.cpu().numpy() == g["c_pred"]).all()
    lm.eval()
    lp_e, _, _ = lm(ys, discrete_input=True)
    _close(lp_e, g["d_lp_eval"])
    lm2 = build()
    opt = FlatAdam(lm2, lr=2e-4, max_grad_norm=5.0)
    lp, _, _ = lm2(ys, discrete_input=True)
    opt.zero_grad()
    (-lm2.mask_and_cal_sum(lp, ys)).backward()
    opt.step()
    for n, q in lm2.named_parameters():
        _close(q, g["after1/" + n], rtol=1e-4, atol=2e-6, what="lm after " + n)


def test_ssl_loss_against_golden(golden_dir):
    dev = _gpu()
    import model as M
    g = _load(golden_dir, "tiny_ssl.npz")
    t = _load(golden_dir, "tiny_e2e.npz")
    net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), t["labeldist"], dev)
    lm = M.LM(bos=1, eos=2, pad=0, labeldist=_load(golden_dir, "tiny_lm.npz")["labeldist"], **synth.TINY_LM).to(dev)
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lm_weights(synth.TINY_LM, 31).items()})
    lm.train()
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    uxs, uilens, _ = synth.batch(8, 9, [12, 10, 7], [2, 2, 2], 41)
    uxs_d = torch.from_numpy(uxs).to(dev)
    _, u_lp, u_pred, _ = net(uxs_d, uilens, ys=None, sample=False, label_smoothing=False,
                             max_dec_timesteps=int(uxs_d.size(1) * float(g["proportion"])), smooth=True, scaling=3)
    assert (u_pred.cpu().numpy() == g["u_pred"]).all()
    _, lm_p, _ = lm(ys=u_pred, discrete_input=False)
    mask = (u_pred != 2).float()
    unsup = -torch.sum(lm_p * u_lp * mask) / torch.sum(mask)
    np.random.seed(9)
    _, l_lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, ys=[torch.from_numpy(y).to(dev) for y in ys], tf_rate=1.0)
    sup = -l_lp.mean()
    _close(sup, g["sup"], rtol=1e-5); _close(unsup, g["unsup"], rtol=1e-4)
    loss = sup + float(g["unsup_weight"]) * unsup
    net.zero_grad()
    loss.backward()
    for n, gr in _grads(net).items():
        _close(gr, g["grad/" + n], atol=1e-6, what="ssl grad " + n)


def test_oracle_parity_random_shapes():
    """HIP path vs the oracle on a second, larger random configuration (odd T, B not a multiple of 16)."""
    dev = _gpu()
    cfg = dict(input_dim=20, enc_hidden_dim=32, enc_n_layers=3, subsample=[2, 2, 1], dropout_rate=0.0,
               dec_hidden_dim=48, att_dim=32, conv_channels=4, conv_kernel_size=5, att_odim=32, embedding_dim=16,
               output_dim=12, ls_weight=0.1)
    ld = synth.labeldist(12, 3)
    w = synth.e2e_weights(cfg, 77)
    ilens = [37, 37, 30, 22, 21, 20, 9, 5, 5, 5, 4, 3, 3, 3, 3, 3, 2, 2, 1]
    xs, ilens, ys = synth.batch(20, 12, ilens, [max(2, l // 6) for l in ilens], 78)
    net = _product(cfg, w, ld, dev)
    np.random.seed(1)
    logits, lp, _, ws = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    sd = O.make_leaf_state(w)
    np.random.seed(1)
    rl, rlp, _, rws = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens,
                                    [torch.from_numpy(y) for y in ys])
    _close(logits, rl, what="logits"); _close(lp, rlp, what="lp"); _close(ws, rws, what="ws")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


def test_dropout_mask_injection(monkeypatch):
    """Dropout cannot match bitwise across RNGs: inject the SAME masks into the HIP path and the
    oracle and require forward + gradient parity (covers the fused-mask paths: pyramid kernel, the decoder's
    masked operand copy, masked dX epilogue)."""
    dev = _gpu()
    import model as M
    import hip_backend as hb
    import torch.nn.functional as F
    if not hb.USE_PACKED_ROWS:
        pytest.skip("the replay below maps the masks of the packed-row encoder (ASR_ENCODER_ROWS=padded is a measurement switch)")
    cfg = dict(input_dim=12, enc_hidden_dim=16, enc_n_layers=2, subsample=[2, 1], dropout_rate=0.4,
               dec_hidden_dim=32, att_dim=16, conv_channels=3, conv_kernel_size=4, att_odim=16, embedding_dim=16,
               output_dim=10, ls_weight=0.05)
    ld = synth.labeldist(10, 3)
    w = synth.e2e_weights(cfg, 55)
    ilens = [13, 11, 8, 5]
    xs, ilens, ys = synth.batch(12, 10, ilens, [3, 2, 2, 2], 56)
    gen = torch.Generator().manual_seed(9)
    recorded = []

    def fake_mask(shape, p, device):
        m = (torch.rand(*shape, generator=gen) >= p).float() / (1.0 - p)
        recorded.append(m)
        return m.to(device)

    monkeypatch.setattr(M, "_drop_mask", fake_mask)
    net = _product(cfg, w, ld, dev)
    np.random.seed(2)
    logits, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    net.zero_grad()
    (-lp.mean()).backward()
    # replay into the oracle: the encoder's masks cover the PACKED rows here (utterance b's frame t at row base[b] + t of its
    # layer, model.pBLSTM._forward_packed) and the padded batch-major tensor there; the frames behind an utterance are dead
    # in the encoder (ones) except in its output, whose mask is the one recorded after the last layer; the decoder mask is
    # one [L,B,O+E] block laid out (ctx|emb) here and a per-step [B,E+O] (emb|ctx) mask there
    O_, E_ = cfg["att_odim"], cfg["embedding_dim"]
    nl = cfg["enc_n_layers"]
    assert len(recorded) == 2 * nl + 2
    lay = net.encoder.enc2.last_layout

    def padded(m, layer, fill=None):
        out = torch.ones(len(ilens), int(lay.lens[layer].max()), m.shape[-1]) if fill is None else fill.clone()
        for b_ in range(len(ilens)):
            n_, r0 = int(lay.lens[layer][b_]), int(lay.base[layer][b_])
            out[b_, :n_] = m[r0:r0 + n_, 0]
        return out
    queue = []
    for li in range(nl):
        queue.append(padded(recorded[2 * li], li))
        queue.append(padded(recorded[2 * li + 1], li + 1, fill=recorded[2 * nl] if li == nl - 1 else None))
    xm = recorded[-1]
    queue += [torch.cat([xm[s][:, O_:], xm[s][:, :O_]], 1) for s in range(xm.shape[0])]

    def replay(x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        m = queue.pop(0)
        assert m.shape == x.shape, (m.shape, x.shape)
        return x * m

    monkeypatch.setattr(O.F, "dropout", replay)
    sd = O.make_leaf_state(w)
    np.random.seed(2)
    rl, rlp, _, _ = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens,
                                  [torch.from_numpy(y) for y in ys])
    assert not queue
    _close(logits, rl, what="dropout logits"); _close(lp, rlp, what="dropout lp")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="dropout grad " + n)


def test_sharded_equals_full_batch_on_gpu():
    """Exact-parity sharding on the HIP path: two strided shards padded to the global T_max / olength, local loss
    -sum/(B_global*olength); summed gradients == single-process gradients."""
    dev = _gpu()
    import model as M
    import parallel
    cfg = dict(synth.TINY)
    ld = synth.labeldist(9, 12)
    w = synth.e2e_weights(cfg, 11)
    ilens, ylens = [11, 10, 9, 6, 5, 3], [4, 2, 3, 2, 3, 2]
    xs, ilens, ys = synth.batch(8, 9, ilens, ylens, 13)
    net = _product(cfg, w, ld, dev)
    np.random.seed(4)
    _, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    net.zero_grad()
    (-lp.mean()).backward()
    full = {n: p.grad.clone() for n, p in net.named_parameters()}
    full_loss = float(-lp.mean())
    net.zero_grad()
    tot = 0.0
    for rank in range(2):
        xs_r, il_r, ys_r, info = parallel.shard_batch(xs, ilens, ys, rank, 2)
        tl = M.padded_lengths(info["t_max"], cfg["enc_n_layers"], cfg["subsample"])
        np.random.seed(4)
        _, lp_r, _, _ = net(torch.from_numpy(np.ascontiguousarray(xs_r)).to(dev), il_r,
                            [torch.from_numpy(y).to(dev) for y in ys_r], total_length=tl, olength=info["olength"])
        loss_r = parallel.local_loss(lp_r, info)
        loss_r.backward()                       # accumulates into .grad
        tot += float(loss_r)
    assert abs(tot - full_loss) < 1e-5 * abs(full_loss)
    for n, p in net.named_parameters():
        _close(p.grad, full[n], rtol=1e-4, atol=1e-6, what="sharded grad " + n)


def test_attloc_forward_standalone(golden_dir):
    """AttLoc.forward with the reference's signature against the two golden attention steps."""
    dev = _gpu()
    g = _load(golden_dir, "tiny_e2e.npz")
    net = _product(synth.TINY, synth.e2e_weights(synth.TINY, 11), g["labeldist"], dev)
    enc_h = torch.from_numpy(g["enc_h"]).to(dev)
    lens = g["enc_lens"].tolist()
    net.attention.reset()
    c0, w0 = net.attention(enc_h, lens, torch.from_numpy(g["att_z0"]).to(dev), None)
    c1, w1 = net.attention(enc_h, lens, torch.from_numpy(g["att_z1"]).to(dev), w0)
    net.attention.reset()
    _close(c0, g["att_c0"], what="c0"); _close(w0, g["att_w0"], what="w0")
    _close(c1, g["att_c1"], what="c1"); _close(w1, g["att_w1"], what="w1")


def test_long_utterances_cfg5_extent():
    """cfg-5's time extent (80 x 1600 frames -> T' = 200 encoder frames, 201-tap location conv) at small widths:
    exercises the T' > 128 / T' > 256-lane loops of the attention kernels and 1600-step recurrences against the oracle."""
    dev = _gpu()
    cfg = dict(input_dim=16, enc_hidden_dim=32, enc_n_layers=3, subsample=[2, 2, 2], dropout_rate=0.0,
               dec_hidden_dim=32, att_dim=32, conv_channels=10, conv_kernel_size=100, att_odim=32, embedding_dim=16,
               output_dim=12, ls_weight=0.05)
    ld = synth.labeldist(12, 5)
    w = synth.e2e_weights(cfg, 55)
    ilens = [1600, 1411, 977]
    xs, ilens, ys = synth.batch(16, 12, ilens, [9, 7, 5], 56)
    net = _product(cfg, w, ld, dev)
    np.random.seed(2)
    logits, lp, _, ws = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    assert ws.shape[-1] == 200
    sd = O.make_leaf_state(w)
    np.random.seed(2)
    rl, rlp, _, rws = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens,
                                    [torch.from_numpy(y) for y in ys])
    _close(logits, rl, what="logits"); _close(lp, rlp, what="lp"); _close(ws, rws, what="ws")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


@pytest.mark.parametrize("B,T", [(1, 7), (2, 1), (5, 2)])
def test_edge_shapes(B, T):
    """Single utterance, single frame, two frames: model vs oracle (forward + gradients)."""
    dev = _gpu()
    cfg = dict(synth.TINY)
    ld = synth.labeldist(9, 12)
    w = synth.e2e_weights(cfg, 11)
    ilens = sorted([max(1, T - i) for i in range(B)], reverse=True)
    xs, ilens, ys = synth.batch(8, 9, ilens, [2] * B, 90 + B)
    net = _product(cfg, w, ld, dev)
    np.random.seed(3)
    logits, lp, _, ws = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    sd = O.make_leaf_state(w)
    np.random.seed(3)
    rl, rlp, _, rws = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens,
                                    [torch.from_numpy(y) for y in ys])
    _close(logits, rl, what="logits"); _close(lp, rlp, what="lp"); _close(ws, rws, what="ws")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


@pytest.mark.parametrize("ndir,B,T,lens,H", [(2, 32, 9, None, 512), (2, 20, 6, None, 512), (1, 40, 5, None, 512),
                                              (2, 3, 4, [4, 2, 1], 512), (2, 48, 5, None, 320), (2, 7, 6, None, 128),
                                              (1, 70, 4, None, 256), (2, 16, 5, None, 512), (2, 12, 7, None, 320),
                                              (2, 17, 4, None, 256), (1, 30, 5, None, 128), (2, 8, 40, None, 512),
                                              (2, 32, 1, None, 512), (2, 9, 2, None, 512), (2, 32, 3, None, 256),
                                              (2, 32, 41, None, 512), (1, 64, 13, None, 128), (2, 33, 8, None, 512),
                                              (2, 64, 9, None, 512), (2, 96, 5, None, 512), (2, 70, 6, None, 512),
                                              (1, 128, 4, None, 512), (1, 150, 3, None, 512), (2, 256, 3, None, 512)])
def test_lstm_persistent_path(ndir, B, T, lens, H):
    """H in {128,256,320,512} takes the persistent XCD-local kernels (forward and backward); parity vs the oracle
    incl. ragged lengths, batches spanning several row blocks, and the group shapes (4 rows per XCD group up to
    4 * 8/ndir rows, 8 rows beyond; at H = 512 the forward takes 16 rows per group for every block of 16 * 8/ndir rows:
    B = 64, 96 = 64 + 32, 70 = 64 + 6, 256); the kernels must not have aborted."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    assert hb.USE_PERSIST
    I = 24
    g = torch.Generator().manual_seed(B * 10 + T)
    if lens is None:
        lens = sorted([int(v) for v in torch.randint(1, T + 1, (B,), generator=g)], reverse=True)
        lens[0] = T
    x = torch.randn(B, T, I, generator=g)
    k = 1.0 / np.sqrt(H)
    prm = []
    for d in range(ndir):
        prm += [torch.empty(4 * H, I).uniform_(-k, k, generator=g), torch.empty(4 * H, H).uniform_(-k, k, generator=g),
                torch.empty(4 * H).uniform_(-k, k, generator=g), torch.empty(4 * H).uniform_(-k, k, generator=g)]
    cp = [p.clone().requires_grad_(True) for p in prm]
    xc = x.clone().requires_grad_(True)
    ref = torch.cat([O.lstm_direction(xc, lens, *cp[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(ndir)], 2)
    gp = [p.to(dev).requires_grad_(True) for p in prm]
    xg = x.to(dev).requires_grad_(True)
    hb.LAUNCHES.clear()
    with hb.require_persistent():          # an ASR_E_SHAPE fallback to the per-step kernels raises
        got = ops.lstm_layer(xg.transpose(0, 1), torch.tensor(lens, dtype=torch.int32, device=dev), gp, ndir)
    assert not hb.persist_aborted(dev)
    _close(got.transpose(0, 1), ref, rtol=1e-4, atol=1e-5, what="y (persistent)")
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    with hb.require_persistent():
        got.backward(dy.transpose(0, 1).contiguous().to(dev))
    assert hb.LAUNCHES["lstm_fwd_persist"] == 1 and hb.LAUNCHES["lstm_bwd_persist"] == 1, dict(hb.LAUNCHES)
    assert hb.LAUNCHES["lstm_fwd_step"] == 0 and hb.LAUNCHES["lstm_bwd_step"] == 0, dict(hb.LAUNCHES)
    _close(xg.grad, xc.grad, what="dx", **LSTM_GRAD_GATE)
    for i, (a, b) in enumerate(zip(gp, cp)):
        _close(a.grad, b.grad, what="param %d" % i, **LSTM_GRAD_GATE)


def _packed_lstm_case(ndir, B, T, H, sub, lens=None, persistent=False, I=24):
    """ops.lstm_layer on PACKED rows (hb.RowLayout: utterance b = rows base[b] .. base[b] + ext[b] - 1, include/asr_hip.h)
    against the oracle's packed-sequence LSTM: outputs and input gradients row by row, zeros on every block's padding rows
    whatever the upstream gradient holds there, parameter gradients (dW_hh as ONE row-shifted product over all rows)."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    g = torch.Generator().manual_seed(B * 10 + T + H)
    if lens is None:
        lens = sorted([int(v) for v in torch.randint(1, T + 1, (B,), generator=g)], reverse=True)
        lens[0] = T
    x = torch.randn(B, T, I, generator=g)
    for b_, n_ in enumerate(lens):
        x[b_, n_:] = 0.0
    k = 1.0 / np.sqrt(H)
    prm = []
    for d in range(ndir):
        prm += [torch.empty(4 * H, I).uniform_(-k, k, generator=g), torch.empty(4 * H, H).uniform_(-k, k, generator=g),
                torch.empty(4 * H).uniform_(-k, k, generator=g), torch.empty(4 * H).uniform_(-k, k, generator=g)]
    cp = [p.clone().requires_grad_(True) for p in prm]
    xc = x.clone().requires_grad_(True)
    ref = torch.cat([O.lstm_direction(xc, lens, *cp[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(ndir)], 2)
    gp = [p.to(dev).requires_grad_(True) for p in prm]
    layout = hb.RowLayout(lens, [sub], dev)
    rows = hb.LayerRows(layout, 0)
    assert all(int(e) > n_ for e, n_ in zip(layout.ext[0], lens)) and rows.R == int(layout.ext[0].sum())
    xp = hb.rows_pack(x.to(dev), rows).requires_grad_(True)
    hb.LAUNCHES.clear()
    if persistent:
        with hb.require_persistent():
            got = ops.lstm_layer(xp, None, gp, ndir, rows=rows)
    else:
        got = ops.lstm_layer(xp, None, gp, ndir, rows=rows)
    gy = got.detach().cpu()
    dy = torch.randn(ref.shape, generator=g)
    dyp = torch.randn(rows.R, ndir * H, generator=g)               # noise on the padding rows: must not reach any gradient
    for b_, n_ in enumerate(lens):
        r0, e_ = int(layout.base[0][b_]), int(layout.ext[0][b_])
        _close(gy[r0:r0 + n_], ref[b_, :n_], what="y of utterance %d" % b_, **LSTM_Y_GATE)
        assert float(gy[r0 + n_:r0 + e_].abs().max()) == 0.0, "padding rows of a block hold zeros"
        dyp[r0:r0 + n_] = dy[b_, :n_]
    ref.backward(dy)
    if persistent:
        with hb.require_persistent():
            got.backward(dyp.to(dev))
        assert not hb.persist_aborted(dev)
        assert hb.LAUNCHES["lstm_fwd_persist"] == 1 and hb.LAUNCHES["lstm_bwd_persist"] == 1, dict(hb.LAUNCHES)
    else:
        got.backward(dyp.to(dev))
    gx = xp.grad.cpu()
    for b_, n_ in enumerate(lens):
        r0, e_ = int(layout.base[0][b_]), int(layout.ext[0][b_])
        _close(gx[r0:r0 + n_], xc.grad[b_, :n_], what="dx of utterance %d" % b_, **LSTM_GRAD_GATE)
        assert float(gx[r0 + n_:r0 + e_].abs().max()) == 0.0
    for i, (a, b) in enumerate(zip(gp, cp)):
        _close(a.grad, b.grad, what="param %d" % i, **LSTM_GRAD_GATE)


@pytest.mark.parametrize("ndir,B,T,H,sub,lens", [(2, 3, 9, 16, 1, [9, 7, 4]), (1, 5, 6, 32, 2, [6, 6, 3, 2, 1]), (2, 33, 5, 64, 2, None),
                                                  (2, 20, 7, 48, 1, None), (2, 4, 1, 16, 2, [1, 1, 1, 1]), (2, 6, 13, 16, 2, [13, 13, 2, 1, 1, 1])])
def test_lstm_layer_packed_rows_per_step_kernels(ndir, B, T, H, sub, lens):
    _packed_lstm_case(ndir, B, T, H, sub, lens)


@pytest.mark.parametrize("arith", ["bf16x6", "f32", "bf16x3"])
@pytest.mark.parametrize("ndir,B,T,H,sub,lens", [(2, 32, 9, 512, 2, None), (2, 20, 6, 512, 1, None), (1, 40, 5, 512, 2, None),
                                                  (2, 3, 4, 512, 2, [4, 2, 1]), (2, 48, 5, 320, 2, None), (2, 7, 6, 128, 1, None),
                                                  (1, 70, 4, 256, 2, None), (2, 8, 40, 512, 2, None), (2, 32, 1, 512, 2, None),
                                                  (2, 64, 9, 512, 2, None), (2, 96, 5, 512, 1, None), (2, 256, 3, 512, 2, None),
                                                  (2, 32, 41, 512, 2, [41, 41, 40, 37, 33] + [9] * 20 + [1] * 7)])
def test_lstm_layer_packed_rows_persistent_kernels(ndir, B, T, H, sub, lens, arith):
    """The persistent XCD-local kernels on packed rows: every row-group shape (4 / 8 / 16 rows), row blocks whose later
    blocks run fewer steps than the first (rowext_host), extreme raggedness (41 ... 1 frames in one group of eight)."""
    _gpu()
    import hip_backend as hb
    with hb.arith(arith):
        _packed_lstm_case(ndir, B, T, H, sub, lens, persistent=True)


@pytest.mark.parametrize("arith", ["bf16x3+gather", "bf16x6+gather"])
@pytest.mark.parametrize("ndir,B,T,H,sub,lens", [(2, 7, 6, 128, 1, None), (1, 70, 4, 256, 2, None), (2, 48, 5, 320, 2, None),
                                                  (2, 3, 4, 512, 2, [4, 2, 1])])
def test_lstm_layer_packed_rows_gathered_split_backward(ndir, B, T, H, sub, lens, arith):
    """The PACKED instantiations of the gathered-dG backward with split dh products (two and three terms), which only the
    `+gather` flag reaches on packed rows: 4-row groups with an incomplete last one, 8-row groups in two launches with a
    short last block, 10 units per CU, ragged lengths."""
    _gpu()
    import hip_backend as hb
    if arith == "bf16x6+gather" and H == 512:
        pytest.skip("the gathered-dG backward with three terms needs 171 KB of LDS at H = 512: the call declines")
    with hb.arith(arith):
        _packed_lstm_case(ndir, B, T, H, sub, lens, persistent=True)


@pytest.mark.parametrize("persistent,H", [(False, 16), (True, 512)])
def test_packed_rows_after_a_longer_batch_left_nan_in_the_shared_workspace(persistent, H):
    """The pooled LSTM workspace is shared by row CAPACITY, and the packed-row dW_hh product reads one row behind the matrix
    (against a zero padding row of the other operand).  A longer batch whose launch aborted leaves NaN there - the kernels
    poison their outputs on purpose - and 0 * NaN is NaN: _LstmLayer.backward zeroes that row when a longer batch has used
    the workspace.  Here: a long batch, its workspace filled with NaN behind its back, then a shorter batch of the same
    capacity class, checked against the oracle."""
    _gpu()
    import ops
    B = 8 if persistent else 3
    _packed_lstm_case(2, B, 9, H, 2, [9] * B, persistent=persistent)
    keys = [key for key in ops._POOL.free if key[0] == "lstm" and key[3] == B and key[4] == H]
    pooled = [ws for key in keys for ws in ops._POOL.free[key]]
    assert pooled, "the long batch's workspace went back to the pool"
    try:
        for ws in pooled:
            assert ws["rows_written"] > 0
            ws["gates_buf"][:ws["rows_written"] + 1].fill_(float("nan"))     # what a poisoned launch of that batch could have left
            ws["y_buf"][:ws["rows_written"] + 1].fill_(float("nan"))
            ws["c_buf"][:ws["rows_written"]].fill_(float("nan"))
        _packed_lstm_case(2, B, 5, H, 2, [5] * (B - 1) + [2], persistent=persistent)
    finally:
        for key in keys:                 # (other tests lease by the same keys: they get fresh workspaces)
            del ops._POOL.free[key]


def test_lstm_judge_width_packed_rows():
    """H = 640 (the judge LM's width) on packed rows: forward on the bf16 kernels, backward on its own exchanged-partials kernel."""
    _packed_lstm_case(1, 32, 11, 640, 1, None, persistent=True)


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "bf16x3+gather", "bf16x6+gather"])
@pytest.mark.parametrize("ndir,B,T,H", [(2, 32, 9, 512), (2, 7, 6, 128), (1, 40, 5, 256), (2, 12, 7, 320), (2, 64, 5, 512)])
def test_lstm_persistent_other_arithmetics(ndir, B, T, H, arith):
    """The persistent LSTM kernels that are not the default stay selectable (the `arith` argument of the C ABI) and
    correct: the exact-fp32 4x4x1 products of round 1, the two-term bf16x3 products of round 2, and - behind `+gather` -
    the split dh products of the gathered-dG backward.  That backward is one kernel, lstm_persist_bwd_kernel<H, NR, NT>:
    NT = 1 is the f32 column, NT = 2 / 3 the two / three split terms (three terms do not exist at H = 512)."""
    _gpu()
    import hip_backend as hb
    if arith == "bf16x6+gather" and H == 512:
        pytest.skip("the gathered-dG backward with three terms needs 171 KB of LDS at H = 512: the call declines")
    with hb.arith(arith):
        test_lstm_persistent_path(ndir, B, T, None, H)


@pytest.mark.parametrize("H,B,T,ndir", [(512, 32, 7, 2), (256, 9, 5, 2), (128, 40, 4, 1)])
def test_lstm_bwd_persist_forward_layout_weights(H, B, T, ndir):
    """asr_lstm_seq_bwd_persist_w (W_hh in the forward layout, no transposed copy) gives bit-identical dG, dW_hh and db
    to asr_lstm_seq_bwd_persist fed the transpose; with the exchanged-partials kernel off it declines (ASR_E_SHAPE)."""
    dev = _gpu()
    import hip_backend as hb
    lib = hb.load()
    g = torch.Generator().manual_seed(H + B + T)
    gact = (torch.rand(T, B, ndir, 4 * H, generator=g) * 0.8 + 0.1).to(dev)
    w = (torch.randn(ndir, 4 * H, H, generator=g) / np.sqrt(H)).to(dev)
    wT = w.transpose(1, 2).contiguous()
    lens = torch.tensor(sorted([int(v) for v in torch.randint(1, T + 1, (B,), generator=g)], reverse=True), dtype=torch.int32, device=dev)
    dy = (torch.randn(T, B, ndir * H, generator=g) * 0.1).to(dev)
    c = torch.randn(T, B, ndir * H, generator=g).to(dev)
    y = torch.tanh(torch.randn(T, B, ndir * H, generator=g)).to(dev)
    xch, ctrl = hb.persist_scratch(dev)
    outs = []
    for fn, wt in ((lib.asr_lstm_seq_bwd_persist, wT), (lib.asr_lstm_seq_bwd_persist_w, w)):
        gb = gact.clone()
        dw = torch.zeros(ndir, 4 * H, H, device=dev)
        db = torch.zeros(ndir * 4 * H, device=dev)
        rc = fn(T, B, B, H, ndir, hb.ptr(gb), hb.ptr(wt), hb.ptr(lens), None, None, None, hb.ptr(dy), hb.ptr(c), hb.ptr(y), hb.ptr(dw), hb.ptr(db),
                hb.c_p(xch.data_ptr()), hb.c_p(ctrl.data_ptr()), hb.current_arith(), hb.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert not hb.persist_aborted(dev)
        outs.append((gb, dw, db))
    assert torch.equal(outs[0][0], outs[1][0]), "dG differs"
    # dW_hh / db are sums of float atomics over the row groups: equal up to the order of those additions
    _close(outs[1][1], outs[0][1], rtol=1e-5, atol=1e-6, what="dW_hh")
    _close(outs[1][2], outs[0][2], rtol=1e-5, atol=1e-6, what="db")
    for declined in (hb.ARITH_F32, hb.ARITH_BF16X3 | hb.LSTM_BWD_GATHER):
        gb = gact.clone()
        rc = lib.asr_lstm_seq_bwd_persist_w(T, B, B, H, ndir, hb.ptr(gb), hb.ptr(w), hb.ptr(lens), None, None, None, hb.ptr(dy), hb.ptr(c), None, None,
                                            None, hb.c_p(xch.data_ptr()), hb.c_p(ctrl.data_ptr()), declined, hb.stream())
        assert rc == -2, rc


def test_arith_is_per_call_not_process_state():
    """Two streams, two arithmetics, interleaved launches: every result carries the error signature of the arithmetic its
    own call named (no process-global switch inside the library)."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(9)
    A, B = torch.randn(512, 2048, generator=g).to(dev), torch.randn(2048, 256, generator=g).to(dev)
    ref = A.double().cpu() @ B.double().cpu()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = {}
    for rep in range(4):
        for st, name in ((s1, "bf16x6"), (s2, "bf16x3")):
            with torch.cuda.stream(st):
                outs[(name, rep)] = hb.gemm(A, B, arith=name, split_k=1)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    err = {k: float((o.double().cpu() - ref).abs().max()) / scale for k, o in outs.items()}
    e32 = float((hb.gemm(A, B, arith="f32", split_k=1).double().cpu() - ref).abs().max()) / scale
    for (name, rep), o in outs.items():
        if name == "bf16x6":
            assert err[(name, rep)] <= 2.0 * e32 + 2e-8, (name, rep, err[(name, rep)], e32)
        else:
            assert 1.5 * e32 < err[(name, rep)] < 1e-4, (name, rep, err[(name, rep)], e32)
        assert torch.equal(o, outs[(name, 0)])


@pytest.mark.parametrize("B,T,ndir", [(32, 12, 1), (20, 7, 1), (8, 5, 2), (40, 3, 1), (64, 105, 1), (3, 40, 2), (16, 31, 2)])
def test_lstm_judge_width_h640(B, T, ndir):
    """H = 640 (the judge LM: config.yaml dis_hidden_dim, reference model.py:466-467): the forward recurrence runs on the
    persistent split-bf16 kernel (20 units per CU = 5 M tiles), the backward - since round 3 - on its own
    exchanged-partials kernel (lstm_persist_bwd_rs640_kernel: 80 local gate columns = two k-steps of 32 and one of 16, five
    unit quads per row); both against the oracle, and the counters say which kernels ran."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    H, I = 640, 256
    g = torch.Generator().manual_seed(B * 10 + T)
    lens = sorted([int(v) for v in torch.randint(1, T + 1, (B,), generator=g)], reverse=True)
    lens[0] = T
    x = torch.randn(B, T, I, generator=g)
    k = 1.0 / np.sqrt(H)
    prm = []
    for d in range(ndir):
        prm += [torch.empty(4 * H, I).uniform_(-k, k, generator=g), torch.empty(4 * H, H).uniform_(-k, k, generator=g),
                torch.empty(4 * H).uniform_(-k, k, generator=g), torch.empty(4 * H).uniform_(-k, k, generator=g)]
    cp = [p.clone().requires_grad_(True) for p in prm]
    xc = x.clone().requires_grad_(True)
    ref = torch.cat([O.lstm_direction(xc, lens, *cp[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(ndir)], 2)
    gp = [p.to(dev).requires_grad_(True) for p in prm]
    xg = x.to(dev).requires_grad_(True)
    hb.LAUNCHES.clear()
    got = ops.lstm_layer(xg.transpose(0, 1), torch.tensor(lens, dtype=torch.int32, device=dev), gp, ndir)
    assert not hb.persist_aborted(dev)
    _close(got.transpose(0, 1), ref, rtol=1e-4, atol=1e-5, what="y (H=640)")
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    got.backward(dy.transpose(0, 1).contiguous().to(dev))
    assert hb.LAUNCHES["lstm_fwd_persist"] == 1 and hb.LAUNCHES["lstm_bwd_persist"] == 1, dict(hb.LAUNCHES)
    assert not hb.persist_aborted(dev)
    _close(xg.grad, xc.grad, what="dx", **LSTM_GRAD_GATE)
    for i, (a, b) in enumerate(zip(gp, cp)):
        _close(a.grad, b.grad, what="param %d" % i, **LSTM_GRAD_GATE)


@pytest.mark.parametrize("dim,B,Tp,L,drop", [(512, 32, 100, 6, True), (512, 7, 37, 4, False), (320, 32, 100, 5, True),
                                             (512, 40, 100, 3, False), (512, 16, 96, 3, True), (320, 5, 9, 4, False),
                                             (512, 70, 100, 2, True), (512, 8, 200, 4, True), (512, 32, 128, 3, True),
                                             (512, 19, 256, 3, False), (320, 6, 150, 5, True)])
def test_decoder_persistent_path(dim, B, Tp, L, drop, K=100):
    """The persistent XCD-local decoder forward kernel (one launch for the whole teacher-forced sequence) against the
    per-step kernels on the same inputs: outputs and every gradient (the backward consumes the buffers it saved).
    The tiny/cfg-1 end-to-end tests hold the per-step kernels to the oracle; cfg-2 end to end covers this path."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    g = torch.Generator().manual_seed(13 + B + Tp)
    D = A = O = dim
    E, C, V = 128, 10, 34
    sc0 = 1.0 / np.sqrt(D)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=g) * sc).to(dev)

    base = dict(P=rnd(B, Tp, A, sc=0.5), Q=rnd(B, Tp, O, sc=0.5), emb_w=rnd(V, E, sc=0.5),
                w_ih=rnd(4 * D, E + O, sc=sc0), w_hh=rnd(4 * D, D, sc=sc0), b_ih=rnd(4 * D, sc=sc0),
                b_hh=rnd(4 * D, sc=sc0), wdec=rnd(A, D, sc=sc0), convw=rnd(C, 1, 1, 2 * K + 1, sc=0.1),
                watt=rnd(A, C, sc=0.3), gvec=rnd(1, A, sc=sc0), bo=rnd(O, sc=sc0), w_out=rnd(V, D + O, sc=sc0),
                b_out=rnd(V, sc=sc0))
    lens = torch.randint(max(1, Tp // 2), Tp + 1, (B,), generator=g)
    w0 = torch.zeros(B, Tp)
    for b in range(B):
        w0[b, :lens[b]] = 1.0 / float(lens[b])
    w0 = w0.to(dev)
    tokens = torch.randint(0, V, (B, L), generator=g).to(dev)
    xmask = ((torch.rand(L, B, O + E, generator=g) > 0.3).float() / 0.7).to(dev) if drop else None
    dlog = rnd(L, B, V)
    dws = rnd(L, B, Tp, sc=0.1)
    names = list(base.keys())

    def run(persist, persist_bwd=False):
        old = hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD
        hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = persist, persist_bwd
        try:
            par = {k: v.clone().requires_grad_(True) for k, v in base.items()}
            opts = dict(L=L, tokens=tokens, tf_flags=None, smooth=False, sample=False, scaling=2.0, xmask=xmask, bos=1)
            hb.LAUNCHES.clear()
            logits, ws, _pred = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"],
                                                     par["b_ih"], par["b_hh"], par["wdec"], par["convw"], par["watt"],
                                                     par["gvec"], par["bo"], par["w_out"], par["b_out"], w0, opts)
            ((logits * dlog).sum() + (ws * dws).sum()).backward()
            torch.cuda.synchronize()
            # the path that ran is the path that was asked for (a silent ASR_E_SHAPE fallback fails here)
            want = {"dec_fwd_persist" if persist else "dec_fwd_step": 1, "dec_bwd_persist" if persist_bwd else "dec_bwd_step": 1}
            assert dict(hb.LAUNCHES) == want, (dict(hb.LAUNCHES), want)
            return logits.detach(), ws.detach(), {k: par[k].grad.detach() for k in names}
        finally:
            hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = old

    lr, wr, gr = run(False)
    # (T' > 100 at 10 conv channels: both persistent kernels run in the 2-utterances-per-group geometry, T' <= 256)
    for mode in ((True, False), (False, True), (True, True)):      # persistent forward / backward / both
        lp, wpp, gp = run(*mode)
        assert not hb.persist_aborted(dev), mode
        assert torch.isfinite(lp).all()
        _close(lp, lr, rtol=2e-4, atol=2e-5, what="logits (persistent decoder %s)" % (mode,))
        _close(wpp, wr, rtol=2e-4, atol=2e-5, what="attention weights (persistent decoder %s)" % (mode,))
        for k in names:
            scale = float(gr[k].abs().max()) + 1e-12
            err = float((gp[k] - gr[k]).abs().max()) / scale
            assert err < 2e-4, (mode, k, err)


@pytest.mark.parametrize("B,Tp,K", [(8, 96, 2), (12, 60, 7), (8, 130, 30), (6, 104, 2)])
def test_decoder_persistent_conv_wider_than_reach(B, Tp, K):
    """T' > K + 1: frames further apart than the location conv reaches.  The conv-backward Toeplitz product of the
    persistent backward dropped the first taps of three of every four output frames - invisible while T' <= K + 1 (their
    operands are zero then), which was the case of every persistent-path test of round 1 (K = 100, T' <= 100); found when
    the T' <= 256 geometry arrived.  Same comparison as test_decoder_persistent_path, short conv kernels."""
    test_decoder_persistent_path(512, B, Tp, 3, True, K=K)


@pytest.mark.parametrize("V,ls", [(34, 0.05), (34, 0.0), (100, 0.1), (7, 0.3)])
def test_label_logprob_kernels(V, ls):
    """asr_label_logprob_fwd/bwd against log_softmax -> gather -> label smoothing in torch (model.py:354-366)."""
    dev = _gpu()
    import ops
    g = torch.Generator().manual_seed(V)
    L, B = 5, 7
    logits = (torch.randn(L, B, V, generator=g) * 3).to(dev).requires_grad_(True)
    idx = torch.randint(0, V, (L, B), generator=g).to(dev)
    dist = torch.rand(V, generator=g)
    dist = (dist / dist.sum()).to(dev)
    up = torch.randn(L, B, generator=g).to(dev)
    got = ops.label_logprob(logits, idx, dist if ls > 0 else None, ls)
    got.backward(up)
    g_got = logits.grad.clone()
    ref_in = logits.detach().clone().requires_grad_(True)
    lp = torch.log_softmax(ref_in, dim=2)
    ref = torch.gather(lp, 2, idx.unsqueeze(2)).squeeze(2)
    if ls > 0:
        ref = (1 - ls) * ref + ls * torch.sum(lp * dist, dim=2)
    ref.backward(up)
    _close(got, ref, rtol=1e-5, atol=1e-6, what="label log-probs")
    _close(g_got, ref_in.grad, rtol=1e-5, atol=1e-6, what="d(logits)")
    # the sum of all outputs times a constant (the training loss, solver.py:377) and the argmax from the same launch; the
    # gradient through that scalar alone is the gradient of the loss
    scale = -1.0 / (L * B)
    lg2 = logits.detach().clone().requires_grad_(True)
    out, total, amax = ops.label_logprob(lg2, idx, dist if ls > 0 else None, ls, with_sum=True, sum_scale=scale, with_argmax=True)
    _close(total, ref.detach().sum() * scale, rtol=1e-5, atol=1e-6, what="scaled sum")
    assert torch.equal(amax, logits.detach().argmax(-1))
    total.backward()
    ref_in.grad = None
    lp2 = torch.log_softmax(ref_in, dim=2)
    ref2 = torch.gather(lp2, 2, idx.unsqueeze(2)).squeeze(2)
    if ls > 0:
        ref2 = (1 - ls) * ref2 + ls * torch.sum(lp2 * dist, dim=2)
    (ref2.sum() * scale).backward()
    _close(lg2.grad, ref_in.grad, rtol=1e-5, atol=1e-7, what="d(logits) through the scaled sum")
    # both gradients at once
    lg3 = logits.detach().clone().requires_grad_(True)
    out3, total3 = ops.label_logprob(lg3, idx, dist if ls > 0 else None, ls, with_sum=True, sum_scale=scale)
    ((out3 * up).sum() + 2.0 * total3).backward()
    _close(lg3.grad, g_got + 2.0 * lg2.grad, rtol=1e-5, atol=1e-6, what="d(logits), both paths")


@pytest.mark.parametrize("drop", [False, True])
def test_dec_prepare_matches_torch(drop):
    """asr_dec_prepare_f32 (teacher-forced decoder input in one launch) against the torch ops it replaces: embedding
    gather of the transposed tokens, dropout mask on the embedding part, zero recurrent slots, zero last slab."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(11)
    L, B, D, O, E, V = 7, 5, 16, 12, 8, 11
    KX = D + O + E
    tokens = torch.randint(0, V, (B, L + 3), generator=g)[:, :L].to(dev)          # row-strided view
    emb = torch.randn(V, E, generator=g).to(dev)
    xmask = ((torch.rand(L, B, O + E, generator=g) > 0.3).float() / 0.7).to(dev) if drop else None
    X = torch.full((L + 1, B, KX), 7.0, device=dev)
    Xd = torch.full((L + 1, B, KX), 7.0, device=dev) if drop else None
    fed = torch.empty(L, B, dtype=torch.long, device=dev)
    hb.dec_prepare(tokens, emb, xmask, X, Xd, fed, L, B, D, O, E)
    want = torch.zeros(L + 1, B, KX, device=dev)
    want[:L, :, D + O:] = emb[tokens.t()]
    assert torch.equal(fed, tokens.t()) and torch.equal(X, want)
    if drop:
        wd = want.clone()
        wd[:L, :, D + O:] *= xmask[:, :, O:]
        assert torch.equal(Xd, wd)


def test_gather_sumsq_kernel():
    """asr_gather_sumsq_f32: the gradient gather of a one-process step (torch._foreach_copy_ into the flat buffer) with the
    sum of squares of clip_grad_norm_ (solver.py:384) taken on the way; more jobs than one launch carries, odd sizes, an
    unaligned source."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(17)
    sizes = [1, 3, 4, 5, 4096, 4097, 12345, 2048 * 512, 7] + [33] * 70
    srcs, offs, off = [], [], 0
    for i, n in enumerate(sizes):
        t = torch.randn(n + 1, generator=g).to(dev)
        srcs.append(t[1:] if i == 6 else t[:n])                       # one source that is not 16-byte aligned
        offs.append(off)
        off += (n + 3) // 4 * 4
    flat = torch.full((off,), 7.0, device=dev)
    acc = torch.zeros(1, device=dev)
    hb.gather_sumsq([s_.contiguous() if False else s_ for s_ in srcs], offs, flat, acc)
    want = 0.0
    for s_, o in zip(srcs, offs):
        assert torch.equal(flat[o:o + s_.numel()], s_)
        want += float((s_.double() ** 2).sum())
    assert abs(float(acc) - want) <= 1e-5 * want
    keep = flat.clone()
    hb.gather_sumsq(srcs[:3], offs[:3], flat, None)                    # without the norm
    assert torch.equal(flat, keep)


@pytest.mark.parametrize("rows,E,V,KX", [(3232, 128, 34, 1152), (37, 16, 12, 48), (5, 8, 140, 8), (640, 256, 64, 256)])
def test_embedding_grad_kernel(rows, E, V, KX):
    """asr_embedding_grad_f32 (autograd of nn.Embedding over the decoder's token-fed steps, model.py:337) against
    index_add_: row-strided gradient (the embedding columns of the dX buffer), -1 = a step that was not fed a token."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(rows + V)
    buf = torch.randn(rows, KX, generator=g).to(dev)
    grad = buf[:, KX - E:]
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[torch.rand(rows, generator=g) < 0.2] = -1
    tok = tok.to(dev)
    acc = torch.randn(V, E, generator=g).to(dev)
    want = acc.clone()
    fedmask = tok >= 0
    want.index_add_(0, tok[fedmask], grad[fedmask])
    assert hb.embedding_grad(tok, grad, acc)
    _close(acc, want, rtol=1e-5, atol=1e-5, what="embedding gradient")
    assert not hb.embedding_grad(tok, buf[:, 1:1 + E], acc.clone())          # unaligned rows: the caller's own path


@pytest.mark.parametrize("H,I,ndir", [(16, 12, 2), (128, 80, 2), (32, 32, 1)])
def test_lstm_pack_unpack_roundtrip(H, I, ndir):
    """asr_lstm_pack_f32 produces the gate-interleaved layout (row = unit*4 + gate) and asr_lstm_unpack_f32 inverts it."""
    dev = _gpu()
    import hip_backend as hb
    import ops
    g = torch.Generator().manual_seed(H + I)
    prm = []
    for _ in range(ndir):
        prm += [torch.randn(4 * H, I, generator=g).to(dev), torch.randn(4 * H, H, generator=g).to(dev),
                torch.randn(4 * H, generator=g).to(dev), torch.randn(4 * H, generator=g).to(dev)]
    w_ih = torch.empty(ndir * 4 * H, I, device=dev)
    w_hh = torch.empty(ndir, 4 * H, H, device=dev)
    bias = torch.empty(ndir * 4 * H, device=dev)
    hb.lstm_pack(prm, ndir, w_ih, w_hh, bias)
    perm = ops.gate_perm(H, dev)
    for d in range(ndir):
        assert torch.equal(w_ih[d * 4 * H:(d + 1) * 4 * H], prm[4 * d][perm])
        assert torch.equal(w_hh[d], prm[4 * d + 1][perm])
        assert torch.equal(bias[d * 4 * H:(d + 1) * 4 * H], (prm[4 * d + 2] + prm[4 * d + 3])[perm])
    g_ih, g_hh, g_b = hb.lstm_unpack(H, I, ndir, w_ih, w_hh, bias)
    for d in range(ndir):
        assert torch.equal(g_ih[d], prm[4 * d]) and torch.equal(g_hh[d], prm[4 * d + 1])
        assert torch.equal(g_b[d], prm[4 * d + 2] + prm[4 * d + 3])


@pytest.mark.parametrize("ndir,dims", [(2, [(16, 12), (16, 64), (16, 64)]), (1, [(20, 8), (20, 20)]),
                                       (2, [(8, 4), (8, 32), (8, 32), (8, 32), (8, 32)])])
def test_lstm_pack_multi_equals_per_layer(ndir, dims):
    """asr_lstm_pack_multi_f32 / asr_lstm_unpack_multi_f32: the layers of a stack (the encoder's three, the judge's two, and
    more than ASR_PACK_MAX_LAYERS) in one launch = asr_lstm_pack_f32 / asr_lstm_unpack2_f32 layer by layer; and through
    autograd (ops.lstm_pack) the gradients of interleaved-layout consumers come back in torch layout."""
    dev = _gpu()
    import hip_backend as hb
    import ops
    g = torch.Generator().manual_seed(len(dims) + ndir)
    layers = []
    for H, I in dims:
        prm = []
        for _ in range(ndir):
            prm += [torch.randn(4 * H, I, generator=g).to(dev), torch.randn(4 * H, H, generator=g).to(dev),
                    torch.randn(4 * H, generator=g).to(dev), torch.randn(4 * H, generator=g).to(dev)]
        layers.append(prm)
    outs = hb.lstm_pack_multi(layers, ndir)
    for (H, I), prm, (w_ih, w_hh, bias) in zip(dims, layers, outs):
        r_ih, r_hh, r_b = torch.empty_like(w_ih), torch.empty_like(w_hh), torch.empty_like(bias)
        hb.lstm_pack(prm, ndir, r_ih, r_hh, r_b)
        assert torch.equal(w_ih, r_ih) and torch.equal(w_hh, r_hh) and torch.equal(bias, r_b)
    grads = [tuple(torch.randn(t.shape, generator=g).to(dev) for t in out) for out in outs]
    grads[1] = (None, None, None)                       # a layer without gradients gets none
    back = hb.lstm_unpack_multi(grads, dims, ndir)
    assert back[1] is None
    for j, ((H, I), gr) in enumerate(zip(dims, grads)):
        if gr[0] is None:
            continue
        r_ih, r_hh, r_b, r_b2 = hb.lstm_unpack(H, I, ndir, gr[0], gr[1], gr[2], two_biases=True)
        for d in range(ndir):
            got = back[j][4 * d:4 * d + 4]
            assert torch.equal(got[0], r_ih[d]) and torch.equal(got[1], r_hh[d]) and torch.equal(got[2], r_b[d])
            assert torch.equal(got[3], r_b2[d]) and got[2].data_ptr() != got[3].data_ptr()
    # autograd: sum_j <c_j, pack(params)_j> differentiates to unpack(c)
    leaves = [[p.clone().requires_grad_(True) for p in prm] for prm in layers]
    packed = ops.lstm_pack(leaves, ndir)
    coef = [tuple(torch.randn(t.shape, generator=g).to(dev) for t in out) for out in packed]
    sum((c * t).sum() for cs, ts in zip(coef, packed) for c, t in zip(cs, ts)).backward()
    want = hb.lstm_unpack_multi(coef, dims, ndir)
    for prm, w in zip(leaves, want):
        for p, t in zip(prm, w):
            _close(p.grad, t, rtol=1e-6, atol=1e-6, what="d(param) through the pack node")


def test_cell_pack_unpack_roundtrip():
    dev = _gpu()
    import hip_backend as hb
    import ops
    D, O, E = 32, 16, 8
    g = torch.Generator().manual_seed(9)
    w_ih, w_hh = torch.randn(4 * D, E + O, generator=g).to(dev), torch.randn(4 * D, D, generator=g).to(dev)
    b_ih, b_hh = torch.randn(4 * D, generator=g).to(dev), torch.randn(4 * D, generator=g).to(dev)
    wcat, bcat = torch.empty(4 * D, D + O + E, device=dev), torch.empty(4 * D, device=dev)
    hb.cell_pack(w_ih, w_hh, b_ih, b_hh, D, O, E, wcat, bcat)
    perm = ops.gate_perm(D, dev)
    assert torch.equal(wcat, torch.cat([w_hh, w_ih[:, E:E + O], w_ih[:, :E]], 1)[perm])
    assert torch.equal(bcat, (b_ih + b_hh)[perm])
    dw_ih, dw_hh, db, db2 = hb.cell_unpack(wcat, bcat, D, O, E)
    assert torch.equal(dw_ih, w_ih) and torch.equal(dw_hh, w_hh) and torch.equal(db, b_ih + b_hh)
    assert torch.equal(db2, db) and db2.data_ptr() != db.data_ptr()


@pytest.mark.parametrize("D,O,E,A,C", [(32, 16, 8, 24, 3), (512, 512, 128, 512, 10), (20, 12, 4, 36, 5)])
def test_dec_pack_and_colsum_parts(D, O, E, A, C):
    """asr_dec_pack_f32 = asr_cell_pack_f32 + the transposed images wcatT / wdecT / wattT (tile transposes, ragged edges
    included); asr_colsum_parts_f32 = the sums over utterances of the decoder backward's three partial gradients."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(D + A)
    KX = D + O + E
    w_ih, w_hh = torch.randn(4 * D, E + O, generator=g).to(dev), torch.randn(4 * D, D, generator=g).to(dev)
    b_ih, b_hh = torch.randn(4 * D, generator=g).to(dev), torch.randn(4 * D, generator=g).to(dev)
    wdec, watt = torch.randn(A, D, generator=g).to(dev), torch.randn(A, C, generator=g).to(dev)
    ref_cat, ref_b = torch.empty(4 * D, KX, device=dev), torch.empty(4 * D, device=dev)
    hb.cell_pack(w_ih, w_hh, b_ih, b_hh, D, O, E, ref_cat, ref_b)
    wcat, bcat = torch.full((4 * D, KX), 9.0, device=dev), torch.full((4 * D,), 9.0, device=dev)
    wcatT, wdecT, wattT = torch.full((KX, 4 * D), 9.0, device=dev), torch.full((D, A), 9.0, device=dev), torch.full((C, A), 9.0, device=dev)
    hb.dec_pack(w_ih, w_hh, b_ih, b_hh, wdec, watt, D, O, E, A, C, wcat, bcat, wcatT, wdecT, wattT)
    assert torch.equal(wcat, ref_cat) and torch.equal(bcat, ref_b)
    assert torch.equal(wcatT, ref_cat.t()) and torch.equal(wdecT, wdec.t()) and torch.equal(wattT, watt.t())
    only = torch.full((C, A), 9.0, device=dev)                  # the forward-only form: no backward images
    hb.dec_pack(w_ih, w_hh, b_ih, b_hh, wdec, watt, D, O, E, A, C, wcat, bcat, None, None, only)
    assert torch.equal(only, watt.t())
    B = 7
    parts = [torch.randn(B, A, generator=g).to(dev), torch.randn(B, A, C, generator=g).to(dev),
             torch.randn(B, C, 2 * 3 + 1, generator=g).to(dev)]
    for got, p in zip(hb.colsum_parts(parts), parts):
        _close(got, p.sum(0), rtol=1e-6, atol=1e-6, what="column sums of a part")


@pytest.mark.parametrize("B,V,E,DO", [(32, 34, 128, 1024), (5, 7, 12, 40), (3, 100, 64, 640)])
def test_decoder_feedback_kernels(B, V, E, DO):
    """asr_dec_feedback_fwd/bwd (logits + argmax + next-step embedding; smooth-embedding backward) against the torch
    expressions of model.py:329-351 on strided step-input buffers, all four feed modes."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(5 + B + V)
    KX = DO + E
    X = torch.randn(2, B, KX, generator=g).to(dev)
    w_out = (torch.randn(V, DO, generator=g) / np.sqrt(DO)).to(dev)
    b_out = torch.randn(V, generator=g).to(dev)
    emb = torch.randn(V, E, generator=g).to(dev)
    mask = ((torch.rand(B, 7 + E, generator=g) > 0.3).float() / 0.7).to(dev)
    toks = torch.randint(0, V, (B, 3), generator=g).to(dev)
    ref_logits = X[0][:, :DO] @ w_out.t() + b_out
    ref_pred = ref_logits.argmax(-1)
    k = 3.0
    for mode in (hb.FEED_PREDICTED, hb.FEED_SMOOTH, hb.FEED_TEACHER, hb.FEED_NONE):
        Xn, Xd = X.clone(), torch.zeros_like(X)
        logits = torch.empty(B, V, device=dev)
        pred = torch.empty(B, dtype=torch.long, device=dev)
        fed = torch.full((B,), -7, dtype=torch.long, device=dev)
        probs = torch.empty(B, V, device=dev)
        last = mode == hb.FEED_NONE
        hb.dec_feedback_fwd(Xn[0][:, :DO], w_out, b_out, emb, logits, pred, mode, k,
                            tok=toks[:, 1] if mode == hb.FEED_TEACHER else None, fed=None if last else fed,
                            probs=probs if mode == hb.FEED_SMOOTH else None, x_emb_next=None if last else Xn[1][:, DO:],
                            xd_emb_next=None if last else Xd[1][:, DO:], mask=None if last else mask[:, 7:])
        _close(logits, ref_logits, rtol=1e-5, atol=1e-5, what="feedback logits")
        assert torch.equal(pred, ref_pred)
        assert torch.equal(Xn[1][:, :DO], X[1][:, :DO]) and torch.equal(Xn[0], X[0])
        if last:
            assert torch.equal(Xn[1], X[1])
            continue
        if mode == hb.FEED_SMOOTH:
            p = torch.softmax(ref_logits * k, -1)
            want, want_fed = p @ emb, torch.full((B,), -1, dtype=torch.long, device=dev)
            _close(probs, p, rtol=1e-5, atol=1e-6, what="feedback probs")
        else:
            want_fed = toks[:, 1] if mode == hb.FEED_TEACHER else ref_pred
            want = emb[want_fed]
        assert torch.equal(fed, want_fed)
        _close(Xn[1][:, DO:], want, rtol=1e-5, atol=1e-6, what="next embedding")
        _close(Xd[1][:, DO:], want * mask[:, 7:], rtol=1e-5, atol=1e-6, what="dropped next embedding")
    # backward of the smooth feedback
    G = torch.randn(B, KX, generator=g).to(dev)
    p = torch.softmax(ref_logits * k, -1)
    dlog0 = torch.randn(B, V, generator=g).to(dev)
    dp = G[:, DO:] @ emb.t()
    dl = k * p * (dp - (p * dp).sum(-1, keepdim=True))
    want_top = G[:, :DO] + dl @ w_out
    Gk, dlog = G.clone(), dlog0.clone()
    hb.dec_feedback_bwd(Gk[:, DO:], Gk[:, :DO], p.contiguous(), emb, w_out, k, dlog)
    _close(dlog, dlog0 + dl, rtol=1e-4, atol=1e-5, what="feedback dlogits")
    _close(Gk[:, :DO], want_top, rtol=1e-4, atol=1e-5, what="feedback d[z,c]")
    assert torch.equal(Gk[:, DO:], G[:, DO:])


@pytest.mark.parametrize("dim,B,Tp,L,drop,kind", [(512, 32, 100, 6, True, "smooth"), (512, 32, 100, 5, True, "greedy"),
                                                  (320, 7, 37, 5, False, "smooth"), (512, 9, 60, 6, True, "mixed"),
                                                  (512, 40, 100, 4, False, "greedy"), (320, 6, 50, 7, True, "smooth"),
                                                  (512, 5, 30, 1, True, "smooth"), (320, 8, 16, 2, False, "greedy"),
                                                  # T' > 100: the free-running kernel in the 2-rows-per-group geometry
                                                  (512, 9, 200, 6, False, "greedy"), (512, 12, 130, 5, True, "smooth"),
                                                  (320, 5, 256, 4, False, "smooth"), (512, 19, 200, 3, True, "greedy"),
                                                  (512, 8, 200, 7, True, "smooth"), (512, 21, 200, 4, False, "smooth"),
                                                  (320, 16, 150, 6, True, "smooth"),
                                                  # longer smooth sequences: the feedback path through many steps
                                                  (512, 32, 100, 12, True, "smooth"), (512, 7, 50, 9, False, "smooth"),
                                                  (320, 10, 64, 8, True, "smooth"),
                                                  # scheduled sampling at full batch, at the other width, in the wide geometry
                                                  (512, 32, 100, 6, True, "mixed"), (320, 6, 40, 6, False, "mixed"),
                                                  (512, 9, 150, 5, False, "mixed")])
def test_free_running_decode_fused_feedback(dim, B, Tp, L, drop, kind):
    """Free-running decoder sequences (smooth embedding with grad as in solver.py:460-495, greedy, scheduled sampling)
    with the fused per-step feedback kernel against the same steps through torch glue: outputs and every gradient.
    The tiny golden tests hold both to the reference's numbers at small shapes."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    g = torch.Generator().manual_seed(31 + B + Tp)
    D = A = O = dim
    E, C, K, V = 128, 10, 100, 34
    sc0 = 1.0 / np.sqrt(D)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=g) * sc).to(dev)

    base = dict(P=rnd(B, Tp, A, sc=0.5), Q=rnd(B, Tp, O, sc=0.5), emb_w=rnd(V, E, sc=0.5),
                w_ih=rnd(4 * D, E + O, sc=sc0), w_hh=rnd(4 * D, D, sc=sc0), b_ih=rnd(4 * D, sc=sc0),
                b_hh=rnd(4 * D, sc=sc0), wdec=rnd(A, D, sc=sc0), convw=rnd(C, 1, 1, 2 * K + 1, sc=0.1),
                watt=rnd(A, C, sc=0.3), gvec=rnd(1, A, sc=sc0), bo=rnd(O, sc=sc0), w_out=rnd(V, D + O, sc=0.3),
                b_out=rnd(V, sc=0.3))
    lens = torch.randint(max(1, Tp // 2), Tp + 1, (B,), generator=g)
    w0 = torch.zeros(B, Tp)
    for b in range(B):
        w0[b, :lens[b]] = 1.0 / float(lens[b])
    w0 = w0.to(dev)
    tokens = torch.randint(0, V, (B, L), generator=g).to(dev) if kind == "mixed" else None
    flags = [True, False, True, False, False, True][:L] if kind == "mixed" else None
    xmask = ((torch.rand(L, B, O + E, generator=g) > 0.3).float() / 0.7).to(dev) if drop else None
    dlog = rnd(L, B, V)
    dws = rnd(L, B, Tp, sc=0.1)
    names = list(base.keys())

    def run(fused, persist=False):
        old = hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD
        hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = fused, persist, persist
        try:
            par = {k: v.clone().requires_grad_(True) for k, v in base.items()}
            opts = dict(L=L, tokens=tokens, tf_flags=flags, smooth=kind == "smooth", smooth_scaling=3.0, sample=False,
                        scaling=2.0, xmask=xmask, bos=1, pooled=True)
            hb.LAUNCHES.clear()
            logits, ws, pred = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"],
                                                    par["b_ih"], par["b_hh"], par["wdec"], par["convw"], par["watt"],
                                                    par["gvec"], par["bo"], par["w_out"], par["b_out"], w0, opts)
            ((logits * dlog).sum() + (ws * dws).sum()).backward()
            torch.cuda.synchronize()
            if fused:
                assert hb.LAUNCHES["dec_free_persist" if persist else "dec_free_step"] == 1, (persist, dict(hb.LAUNCHES))
                assert hb.LAUNCHES["dec_free_step" if persist else "dec_free_persist"] == 0, (persist, dict(hb.LAUNCHES))
            if fused and kind == "mixed":
                # scheduled sampling: the host's per-step draws travel with the launch, both directions persistent
                assert hb.LAUNCHES["dec_bwd_persist" if persist else "dec_bwd_step"] == 1, (persist, dict(hb.LAUNCHES))
            if fused and kind == "smooth" and L > 1:
                # the backward of the smooth free-running sequence: persistent (feedback carried inside the kernel) in both
                # geometries (4 rows per group up to T' = 100, 2 rows per group up to T' = 256: cfg-5's T' = 200)
                want = "dec_bwd_persist" if persist else "dec_bwd_step"
                assert hb.LAUNCHES[want] == 1, (persist, Tp, dict(hb.LAUNCHES))
            return logits.detach(), ws.detach(), pred.clone(), {k: par[k].grad.detach() for k in names}
        finally:
            hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = old

    lr, wr, pr, gr = run(False)
    # per-step kernels + fused feedback kernel, then (sequences without teacher tokens) the whole sequence in the
    # persistent kernel with the feedback computed inside it
    for persist in (False, True):
        lf, wf, pf, gf = run(True, persist)
        assert not hb.persist_aborted(dev), persist
        assert torch.equal(pf, pr), "predictions differ (persist=%s)" % persist
        _close(lf, lr, rtol=2e-4, atol=2e-5, what="logits (fused feedback, %s, persist=%s)" % (kind, persist))
        _close(wf, wr, rtol=2e-4, atol=2e-5, what="attention weights (fused feedback, %s, persist=%s)" % (kind, persist))
        for k in names:
            scale = float(gr[k].abs().max()) + 1e-12
            err = float((gf[k] - gr[k]).abs().max()) / scale
            assert err < 2e-4, (kind, persist, k, err)


@pytest.mark.parametrize("p", [0.3, 0.5])
def test_seeded_dropout_kernels(p):
    """Counter-based dropout (dropout.hip, pyramid.hip *_seeded): the mask is a pure function of (seed, index); every
    consumer that regenerates it must agree with the materialised mask."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(21)
    m = hb.SeededMask((7, 6, 40), p, dev, seed=123456789012345)
    mask = m.tensor()
    assert mask.shape == (7, 6, 40)
    vals = torch.unique(mask).cpu().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1.0 / (1.0 - p)) < 1e-6
    big = hb.SeededMask((1 << 20,), p, dev, seed=987654321).tensor()
    assert abs(float((big > 0).float().mean()) - (1.0 - p)) < 5e-3
    assert not torch.equal(hb.SeededMask((7, 6, 40), p, dev, seed=5).tensor(), mask)
    assert torch.equal(hb.SeededMask((7, 6, 40), p, dev, seed=123456789012345).tensor(), mask)
    # in-place forward and the fused relu + dropout backward
    x = torch.randn(7, 6, 40, generator=g).to(dev)
    y = torch.relu(x) * mask
    got = hb.dropout_seeded_(torch.relu(x).contiguous(), m)
    assert torch.equal(got, y)
    gr = torch.randn(7, 6, 40, generator=g).to(dev)
    assert torch.equal(hb.relu_dropout_bwd(gr, y, m.seed, m.p), gr * mask * (y > 0).float())
    assert torch.equal(hb.relu_dropout_bwd(gr, torch.relu(x), 0, 0.0), gr * (x > 0).float())
    # pair-concat with the mask regenerated in flight, even and odd T
    for T in (7, 8):
        import ops
        xin = torch.randn(T, 6, 40, generator=g).to(dev)
        ms = hb.SeededMask((T, 6, 40), p, dev, seed=77 + T)
        mt = ms.tensor()
        a = xin.clone().requires_grad_(True)
        b = xin.clone().requires_grad_(True)
        ya, yb = ops.pyramid_concat(a, ms), ops.pyramid_concat(b, mt)
        assert torch.equal(ya, yb)
        go = torch.randn(ya.shape, generator=g).to(dev)
        ya.backward(go); yb.backward(go)
        assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("M,N,K", [(1368, 512, 2048), (5472, 512, 2048), (96, 64, 64), (2736, 512, 512)])
def test_gemm_with_dropout_epilogue(M, N, K):
    """asr_gemm_drop_f32: relu(x W^T + b) -> seeded dropout (model.py:93-95) as ONE call - the mask goes into the bias / ReLU
    pass of a product that was split over K, or into a pass of its own - equals the product followed by
    asr_dropout_seeded_f32 (same mask: a pure function of seed and element index), and ops.linear's backward regenerates it."""
    dev = _gpu()
    import hip_backend as hb
    import ops
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    m = hb.SeededMask((M, 1, N), 0.3, dev, seed=4242 + M)
    for split in (None, 1):
        got = hb.gemm(x, w, trans_b=True, bias=b, relu=True, drop=m, split_k=split)
        ref = hb.dropout_seeded_(hb.gemm(x, w, trans_b=True, bias=b, relu=True, split_k=split), m)
        _close(got, ref, rtol=1e-5, atol=1e-5, what="product with the dropout epilogue (split_k=%s)" % split)
        if split == 1:                                   # (no atomics: the same product bit for bit)
            assert torch.equal(got, ref)
    xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ya = ops.linear(xa, wa, ba, relu=True, drop=m)
    xb, wb, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yb = torch.relu(xb @ wb.t() + bb) * m.tensor().view(M, N)
    go = torch.randn(M, N, generator=g).to(dev)
    ya.backward(go); yb.backward(go)
    _close(ya, yb, rtol=1e-4, atol=1e-4, what="linear + relu + dropout")
    for a_, b_, nm in ((xa, xb, "dx"), (wa, wb, "dw"), (ba, bb, "db")):
        _close(a_.grad, b_.grad, rtol=2e-3, atol=2e-3 * float(b_.grad.abs().max()), what=nm)


def test_seeded_dropout_end_to_end_equals_explicit_masks(monkeypatch):
    """The whole model with dropout: seeded in-kernel masks against the same masks materialised and passed as tensors
    (the path the injected-mask oracle test pins)."""
    dev = _gpu()
    import model as M
    import hip_backend as hb
    cfg = dict(input_dim=12, enc_hidden_dim=16, enc_n_layers=2, subsample=[2, 2], dropout_rate=0.4,
               dec_hidden_dim=32, att_dim=16, conv_channels=3, conv_kernel_size=4, att_odim=16, embedding_dim=16,
               output_dim=10, ls_weight=0.05)
    ld = synth.labeldist(10, 3)
    w = synth.e2e_weights(cfg, 57)
    xs, ilens, ys = synth.batch(12, 10, [13, 11, 8, 5], [3, 2, 2, 2], 58)
    outs = []
    for explicit in (False, True):
        seeds = iter(range(1000, 1100))

        def mask(shape, p, device, explicit=explicit, seeds=seeds):
            sm = hb.SeededMask(shape, p, device, seed=next(seeds))
            return sm.tensor() if explicit else sm

        monkeypatch.setattr(M, "_drop_mask", mask)
        net = _product(cfg, w, ld, dev)
        np.random.seed(2)
        logits, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
        net.zero_grad()
        (-lp.mean()).backward()
        outs.append((logits.detach().clone(), {n: g_.clone() for n, g_ in _grads(net).items()}))
    _close(outs[0][0], outs[1][0], rtol=1e-6, atol=1e-7, what="seeded vs explicit logits")
    for n in outs[0][1]:
        _close(outs[0][1][n], outs[1][1][n], rtol=1e-5, atol=1e-7, what="seeded vs explicit grad " + n)


@pytest.mark.parametrize("eos_bias", [0.0, 1.5, 30.0])
def test_greedy_decode_early_stop(eos_bias):
    """Decoding without autograd may stop a group of 4 utterances once all of them have emitted <EOS>:
    up to and including each utterance's first <EOS> the predictions equal those of the full-length decode, and the
    CER path (utils.remove_pad_eos) sees identical hypotheses."""
    dev = _gpu()
    import hip_backend as hb
    from utils import remove_pad_eos
    cfg = dict(input_dim=16, enc_hidden_dim=128, enc_n_layers=1, subsample=[2], dropout_rate=0.0, dec_hidden_dim=320,
               att_dim=320, conv_channels=10, conv_kernel_size=20, att_odim=320, embedding_dim=128, output_dim=12,
               ls_weight=0.0)
    w = synth.e2e_weights(cfg, 71)
    w["decoder.output_layer.bias"] = w["decoder.output_layer.bias"].copy()
    w["decoder.output_layer.bias"][2] += eos_bias
    net = _product(cfg, w, synth.labeldist(12, 3), dev).eval()
    xs, ilens, _ = synth.batch(16, 12, [40, 37, 33, 30, 28, 25, 21, 18, 12], [3] * 9, 72)
    xs_d = torch.from_numpy(xs).to(dev)
    outs = {}
    for stop in (False, True):
        old = hb.DECODE_EARLY_STOP
        hb.DECODE_EARLY_STOP = stop
        try:
            with torch.no_grad():
                _, _, pred, _ = net(xs_d, ilens, ys=None, max_dec_timesteps=25)
            assert not hb.persist_aborted(dev)
            outs[stop] = pred.cpu().numpy()
        finally:
            hb.DECODE_EARLY_STOP = old
    full, early = outs[False], outs[True]
    assert full.shape == early.shape == (9, 25)
    assert remove_pad_eos(full.tolist(), eos=2) == remove_pad_eos(early.tolist(), eos=2)
    for b in range(9):
        hit = np.where(full[b] == 2)[0]
        upto = int(hit[0]) + 1 if len(hit) else 25
        assert (full[b, :upto] == early[b, :upto]).all(), b
    if eos_bias >= 30.0:
        assert (early == 2).all()
    if eos_bias == 0.0:
        assert (full == early).all() or (full == 2).any()


# ------------------------------------------------------------------------------ round 3: pins the verdict asked for
def test_free_running_persistent_decoder_against_oracle_d512():
    """The kernel cfg-4 and validation actually run - dec_persist_fwd_kernel<512,512,512,128,FB=true>, free-running with
    the smooth-embedding feedback computed inside the kernel - directly against the oracle's Decoder.forward
    (model.py:296-367, ys=None, smooth=True) at D = A = O = 512, B = 32, T' = 100, 20 steps: logits, log-probs, the
    hypothesis, attention weights, and the gradients of a loss over log-probs and attention weights with respect to the
    encoder output and every decoder / attention parameter."""
    dev = _gpu()
    import hip_backend as hb
    import model as M
    cfg = dict(synth.CFG2)
    B, Tp, L = 32, 100, 20
    w = synth.e2e_weights(cfg, 123)
    g = torch.Generator().manual_seed(17)
    enc = (torch.randn(B, Tp, cfg["enc_hidden_dim"], generator=g) * 0.5)
    enc_lens = sorted([int(v) for v in torch.randint(Tp // 2, Tp + 1, (B,), generator=g)], reverse=True)
    enc_lens[0] = Tp
    r_lp = torch.randn(B, L, generator=g)
    r_ws = torch.randn(B, L, Tp, generator=g) * 0.1
    # ---- oracle (CPU)
    sd = O.make_leaf_state(w)
    enc_c = enc.clone().requires_grad_(True)
    lg_o, lp_o, pred_o, ws_o = O.decoder_forward(sd, enc_c, enc_lens, ys=None, max_dec_timesteps=L, smooth=True, scaling=3.0,
                                                 label_smoothing=False)
    names = [n for n in O.unique_param_names(sd) if n.startswith(("attention.", "decoder."))]
    loss_o = (lp_o * r_lp).sum() + (ws_o * r_ws).sum()
    grads_o = torch.autograd.grad(loss_o, [enc_c] + [sd[n] for n in names])
    # ---- product (GPU), persistent kernel required
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 5), **cfg).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    net.train()
    enc_g = enc.to(dev).requires_grad_(True)
    hb.persist_clear_abort(dev)
    hb.LAUNCHES.clear()
    with hb.require_persistent():
        lg, lp, pred, ws = net.decoder(enc_g, enc_lens, ys=None, max_dec_timesteps=L, smooth=True, scaling=3.0,
                                       label_smoothing=False)
    assert hb.LAUNCHES["dec_free_persist"] == 1, dict(hb.LAUNCHES)
    assert not hb.persist_aborted(dev)
    assert torch.equal(pred.cpu(), pred_o), "hypotheses differ"
    _close(lg, lg_o, rtol=2e-4, atol=2e-5, what="logits")
    _close(lp, lp_o, rtol=2e-4, atol=2e-5, what="log-probs")
    _close(ws, ws_o, rtol=2e-4, atol=2e-6, what="attention weights")
    net.zero_grad()
    ((lp * r_lp.to(dev)).sum() + (ws * r_ws.to(dev)).sum()).backward()
    _close(enc_g.grad, grads_o[0], rtol=1e-3, atol=1e-6, what="d enc_h")
    got = dict(net.named_parameters())
    for n, gr in zip(names, grads_o[1:]):
        _close(got[n].grad, gr, rtol=1e-3, atol=1e-6, what="grad " + n)


def test_scheduled_sampling_persistent_decoder_against_oracle_d512():
    """Scheduled sampling (Decoder.forward with ys and tf_rate < 1, model.py:324-351: one numpy draw per step decides between
    the teacher's token and the model's own argmax) on the persistent kernels in both directions, against the oracle at
    D = A = O = 512, B = 32, T' = 100 with the same numpy stream: logits, log-probs, predictions, attention weights and
    every gradient.  Until round 3 this mode ran on the per-step kernels."""
    dev = _gpu()
    import hip_backend as hb
    import model as M
    cfg = dict(synth.CFG2)
    B, Tp = 32, 100
    w = synth.e2e_weights(cfg, 77)
    g = torch.Generator().manual_seed(29)
    enc = (torch.randn(B, Tp, cfg["enc_hidden_dim"], generator=g) * 0.5)
    enc_lens = sorted([int(v) for v in torch.randint(Tp // 2, Tp + 1, (B,), generator=g)], reverse=True)
    enc_lens[0] = Tp
    ys = [torch.randint(3, cfg["output_dim"], (int(n),), generator=g) for n in torch.randint(8, 17, (B,), generator=g)]
    L = max(len(y) for y in ys) + 1
    r_lp = torch.randn(B, L, generator=g)
    r_ws = torch.randn(B, L, Tp, generator=g) * 0.1
    sd = O.make_leaf_state(w)
    enc_c = enc.clone().requires_grad_(True)
    np.random.seed(5)
    lg_o, lp_o, pred_o, ws_o = O.decoder_forward(sd, enc_c, enc_lens, ys=ys, tf_rate=0.5, label_smoothing=False)
    names = [n for n in O.unique_param_names(sd) if n.startswith(("attention.", "decoder."))]
    loss_o = (lp_o * r_lp).sum() + (ws_o * r_ws).sum()
    grads_o = torch.autograd.grad(loss_o, [enc_c] + [sd[n] for n in names])
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 5), **cfg).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    net.train()
    net.decoder.dropout_rate = 0.0
    enc_g = enc.to(dev).requires_grad_(True)
    hb.persist_clear_abort(dev)
    hb.LAUNCHES.clear()
    np.random.seed(5)
    with hb.require_persistent():
        lg, lp, pred, ws = net.decoder(enc_g, enc_lens, ys=[y.to(dev) for y in ys], tf_rate=0.5, label_smoothing=False)
        assert hb.LAUNCHES["dec_free_persist"] == 1, dict(hb.LAUNCHES)
        assert torch.equal(pred.cpu(), pred_o), "predictions differ"
        _close(lg, lg_o, rtol=2e-4, atol=2e-5, what="logits")
        _close(lp, lp_o, rtol=2e-4, atol=2e-5, what="log-probs")
        _close(ws, ws_o, rtol=2e-4, atol=2e-6, what="attention weights")
        net.zero_grad()
        ((lp * r_lp.to(dev)).sum() + (ws * r_ws.to(dev)).sum()).backward()
    assert hb.LAUNCHES["dec_bwd_persist"] == 1, dict(hb.LAUNCHES)
    assert not hb.persist_aborted(dev)
    _close(enc_g.grad, grads_o[0], rtol=1e-3, atol=1e-6, what="d enc_h")
    got = dict(net.named_parameters())
    for n, gr in zip(names, grads_o[1:]):
        _close(got[n].grad, gr, rtol=1e-3, atol=1e-6, what="grad " + n)


def test_thirty_optimizer_steps_track_the_oracle():
    """Drift proxy for "CER within 0.3 abs after equal steps" while WSJ is absent: 30 clip + Adam(amsgrad) steps at the
    cfg-1 model shape (1x128 encoder, 320 decoder, B = 4, T = 200) on the GPU under the bench's default arithmetic against
    the oracle's trajectory on the CPU from the same weights and batches: the loss of every step and the final weights.
    Adam normalises every update to ~lr, so a gradient error of relative size e moves a weight by ~e * lr per step (and
    elements whose gradient sits at the fp32 noise floor by more); asserted: every step's loss within the 1e-3 parity
    gate (observed ~1e-6) and, after 30 steps, every weight tensor within 10 % of the largest distance any of its elements
    has travelled (observed: printed)."""
    dev = _gpu()
    import hip_backend as hb
    import model as M
    from parallel import FlatAdam
    cfg = dict(synth.CFG1)
    ld = synth.labeldist(cfg["output_dim"], 23)
    w0 = synth.e2e_weights(cfg, 21)
    steps = 30
    batches = [synth.batch(cfg["input_dim"], cfg["output_dim"], synth.CFG1_ILENS, synth.CFG1_YLENS, 500 + i) for i in range(3)]
    # ---- oracle trajectory
    sd = O.make_leaf_state(w0)
    names = O.unique_param_names(sd)
    opt_o = O.AdamAmsgrad(names, lr=5e-4, weight_decay=1e-6)
    mcfg = dict(cfg, labeldist=ld)
    losses_o = []
    for s in range(steps):
        xs, ilens, ys = batches[s % 3]
        np.random.seed(100 + s)
        out = O.sup_train_step(sd, mcfg, opt_o, torch.from_numpy(xs), ilens, [torch.from_numpy(y) for y in ys], max_grad_norm=5.0)
        losses_o.append(float(out[0] if isinstance(out, (tuple, list)) else out))
    # ---- product trajectory (default arithmetic)
    assert hb.arith_name() == "bf16x6"
    net = M.E2E(labeldist=ld, **cfg).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w0.items()})
    net.train()
    opt = FlatAdam(net, lr=5e-4, weight_decay=1e-6, amsgrad=True, max_grad_norm=5.0)
    losses = []
    for s in range(steps):
        xs, ilens, ys = batches[s % 3]
        np.random.seed(100 + s)
        _, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys], tf_rate=1.0)
        loss = -lp.mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    for s, (a, b) in enumerate(zip(losses, losses_o)):
        assert abs(a - b) <= 1e-3 * abs(b), "loss of step %d: %.7f vs oracle %.7f" % (s, a, b)
    worst = 0.0
    for n, p in net.named_parameters():
        start = torch.from_numpy(w0[n])
        want = sd[n].detach()
        travelled = float((want - start).abs().max())
        err = float((p.detach().cpu() - want).abs().max())
        worst = max(worst, err / max(travelled, 1e-12))
        assert err <= 0.10 * travelled + 1e-7, (n, err, travelled)
    worst_loss = max(abs(a - b) / abs(b) for a, b in zip(losses, losses_o))
    print("30 steps: last loss %.6f (oracle %.6f), worst loss error %.2e, worst weight error %.3f %% of the distance travelled"
          % (losses[-1], losses_o[-1], worst_loss, 100 * worst))


def test_decoder_and_lm_forward_step_methods():
    """The thin per-step methods of the reference's class surface (Decoder.forward_step / zero_state, model.py:276-294;
    LM.forward_step / zero_state, model.py:486-490,534-542) against the fused sequence paths the fixtures pin: driving
    the loop by hand reproduces Decoder.forward's teacher-forced logits and LM.forward's log-probabilities."""
    dev = _gpu()
    import model as M
    cfg = dict(synth.TINY)
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
    net.eval()
    xs, ilens, ys = synth.batch(cfg["input_dim"], cfg["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    with torch.no_grad():
        enc_h, enc_lens = net.encoder(xs_d, ilens)
        logits, _, _, ws = net.decoder(enc_h, enc_lens, ys_d, tf_rate=1.0)
        dec = net.decoder
        tok_in = dec._label_matrices(ys_d)[0]
        z, cst = dec.zero_state(enc_h), dec.zero_state(enc_h)
        c, w = dec.zero_state(enc_h, dim=dec.att_odim), None
        assert z.shape == (len(ys), cfg["dec_hidden_dim"]) and c.shape == (len(ys), cfg["att_odim"])
        dec.attention.reset()
        for s in range(tok_in.size(1)):
            logit, z, cst, c, w = dec.forward_step(dec.embedding(tok_in[:, s]), z, cst, c, w, enc_h, enc_lens)
            _close(logit, logits[:, s], rtol=2e-4, atol=2e-5, what="forward_step logits, step %d" % s)
            _close(w, ws[:, s], rtol=2e-4, atol=2e-6, what="forward_step attention weights, step %d" % s)
    lcfg = dict(synth.TINY_LM)
    lm = M.LM(bos=1, eos=2, pad=0, labeldist=synth.labeldist(lcfg["output_dim"], 32), **lcfg).to(dev)
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lm_weights(lcfg, 31).items()})
    lm.eval()
    dense = torch.randint(3, lcfg["output_dim"], (3, 7), generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        lp, _, _ = lm(dense, discrete_input=False)
        inp = torch.cat([torch.full((3, 1), 1, dtype=torch.long, device=dev), dense[:, :-1]], dim=1)
        zs = cs = None
        assert lm.zero_state(dense).shape == (lcfg["n_layers"], 3, lcfg["hidden_dim"])
        for s in range(7):
            logit, zs, cs = lm.forward_step(lm.embedding(inp[:, s]).unsqueeze(1), zs, cs)
            step_lp = torch.log_softmax(logit, dim=-1).gather(1, dense[:, s:s + 1]).squeeze(1)
            _close(step_lp, lp[:, s], rtol=2e-4, atol=2e-5, what="LM.forward_step log-prob, step %d" % s)
        samples = lm.decode(n_samples=3, sample=False, max_dec_timesteps=5)
        assert samples.shape == (3, 5)


def _rccl_child(out_path):
    """Fresh process, no GPU call before init_process_group: backend nccl (= RCCL on ROCm), world_size 1."""
    import os, sys, json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "semi-supervised-asr_amd"), os.path.join(root, "tests", "golden")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    torch.cuda.set_device(0)
    import numpy as np
    import synth, parallel, model as M
    from parallel import FlatAdam
    dev = torch.device("cuda", 0)
    cfg = dict(synth.TINY)
    res = {}
    parallel.FlatBuffers.BUCKET_FLOATS = 700         # tiny model: several buckets
    for tag in ("collective", "overlapped", "plain"):
        net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).to(dev)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
        net.train()
        opt = FlatAdam(net, lr=5e-4, weight_decay=1e-6, amsgrad=True, max_grad_norm=5.0,
                       overlap="force" if tag == "overlapped" else False)
        xs, ilens, ys = synth.batch(cfg["input_dim"], cfg["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
        np.random.seed(5)
        _, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
        opt.zero_grad()
        (-lp.mean()).backward()
        if tag == "collective":
            opt.buf.set_aux([1.5, 2.5])
            opt.buf.collect()
            dist.all_reduce(opt.buf.flat_g, op=dist.ReduceOp.SUM)        # THE collective of a data-parallel step, on RCCL
            res["aux"] = opt.buf.aux[:2].tolist()
            res["backend"] = dist.get_backend()
            opt.apply()
        elif tag == "overlapped":
            # the data-parallel default: bucket all-reduces issued by post-accumulate hooks from inside the backward pass
            # (async RCCL collectives on slices of the flat buffer), awaited in reduce(); aux scalars in their own collective
            assert opt.buf.overlap and len(opt.buf.buckets) >= 3 and opt.buf._issued >= 1, (opt.buf.overlap, opt.buf._issued)
            opt.buf.set_aux([1.5, 2.5])
            opt.reduce()
            res["aux_overlapped"] = opt.buf.aux[:2].tolist()
            opt.apply()
        else:
            opt.step()
        res[tag] = [float(p.detach().double().abs().sum()) for p in net.parameters()]
    with open(out_path, "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


def test_rccl_allreduce_of_the_flat_gradient_buffer(tmp_path):
    """RCCL touched on hardware (world_size 1 is all a one-GPU box allows): a freshly spawned child initialises the `nccl`
    backend before any other GPU call, pushes the flat gradient buffer (+ aux scalars) through dist.all_reduce - once as ONE
    collective, once as the overlapped bucket exchange of a data-parallel step (async collectives issued from autograd hooks)
    - and applies the fused clip + Adam; the weights equal those of the non-distributed step."""
    _gpu()
    import json
    import subprocess
    import sys
    out = os.path.join(str(tmp_path), "rccl.json")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.join(here, "golden"), os.path.dirname(here), os.path.join(os.path.dirname(here), "semi-supervised-asr_amd")]
    code = "import sys; sys.path[:0] = %r; import test_hip_parity as t; t._rccl_child(%r)" % (paths, out)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert res["backend"] == "nccl" and res["aux"] == [1.5, 2.5] and res["aux_overlapped"] == [1.5, 2.5]
    for tag in ("collective", "overlapped"):
        for a, b in zip(res[tag], res["plain"]):
            assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (tag, a, b)


# ----------------------------------------------------------------------------------------------------------------------
# The kernels' OWN abort path (csrc/persist.h: a bounded spin expires -> raise_abort -> NaN poison -> every other workgroup
# drains), run for real instead of the host writing the latch: the FAULT instantiations of the persistent LSTM / decoder
# forward kernels (ASR_DEBUG_FAULT in `arith`; asr_dec_seq_fwd_persist_fault) - slice 1 of group 0 stops publishing after its
# first step and every wait gives up after 4 096 attempts.


def _timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def test_lstm_kernel_raises_its_own_abort_and_the_next_launch_is_clean():
    dev = _gpu()
    import hip_backend as hb
    H, B, T, ndir = 512, 32, 24, 2
    g = torch.Generator().manual_seed(5)
    gates0 = (torch.randn(T, B, ndir, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(ndir, 4 * H, H, generator=g) / np.sqrt(H)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)

    def run():
        gts, y, c = gates0.clone(), torch.empty(T, B, ndir * H, device=dev), torch.empty(T, B, ndir * H, device=dev)
        with hb.require_persistent():
            hb.lstm_seq_fwd(gts, whh, lens, y, c)
        return y
    hb.persist_clear_abort(dev)
    want = run()
    torch.cuda.synchronize()
    assert not hb.persist_aborted(dev) and torch.isfinite(want).all()
    with hb.arith("bf16x6+fault"):
        got, ms = _timed_ms(run)
    ctrl = hb.persist_scratch(dev)[1].cpu().tolist()
    assert ms < 100.0, "the bounded spins of the armed launch expire in milliseconds, got %.1f ms" % ms
    assert ctrl[0] == 1 and ctrl[1] == 1, "latch + code of the forward hand-off's wait (code 1), got %s" % ctrl[:2]
    assert ctrl[16 + 8] == 1 and ctrl[16 + 9] == 1, "per-launch abort word + code"
    assert hb.persist_aborted(dev) and hb.persist_abort_code(dev) == 1
    # group 0 = (direction 0, rows 0..7): the waves whose K range holds the silent producer's units give up at step 2 and
    # poison what they produce from there on; the other waves of the group sample the abort word every 16th step and poison
    # from then on.  The other groups do not depend on group 0: they may have finished - with valid numbers - before it gave up
    assert torch.isnan(got[2, :8, :H]).any(), "the stalled group produces NaN from the step behind the silent producer"
    assert torch.isnan(got[T - 1, :8, :H]).all()
    hb.persist_clear_abort(dev)
    again = run()
    torch.cuda.synchronize()
    assert not hb.persist_aborted(dev)
    assert torch.equal(again, want), "the next clean launch on the same scratch is bit-identical to the one before the fault"


def test_decoder_kernel_raises_its_own_abort_and_the_next_launch_is_clean():
    dev = _gpu()
    import ops
    import hip_backend as hb
    g = torch.Generator().manual_seed(21)
    D = A = O = 512
    E, C, V, K, B, Tp, L = 128, 10, 34, 100, 8, 40, 10

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=g) * sc).to(dev)
    sc0 = 1.0 / np.sqrt(D)
    par = dict(P=rnd(B, Tp, A, sc=0.5), Q=rnd(B, Tp, O, sc=0.5), emb_w=rnd(V, E, sc=0.5), w_ih=rnd(4 * D, E + O, sc=sc0),
               w_hh=rnd(4 * D, D, sc=sc0), b_ih=rnd(4 * D, sc=sc0), b_hh=rnd(4 * D, sc=sc0), wdec=rnd(A, D, sc=sc0),
               convw=rnd(C, 1, 1, 2 * K + 1, sc=0.1), watt=rnd(A, C, sc=0.3), gvec=rnd(1, A, sc=sc0), bo=rnd(O, sc=sc0),
               w_out=rnd(V, D + O, sc=sc0), b_out=rnd(V, sc=sc0))
    w0 = torch.full((B, Tp), 1.0 / Tp, device=dev)
    tokens = torch.randint(0, V, (B, L), generator=g).to(dev)

    def run():
        opts = dict(L=L, tokens=tokens, tf_flags=None, smooth=False, sample=False, scaling=2.0, xmask=None, bos=1)
        with torch.no_grad(), hb.require_persistent():
            logits, ws, _ = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"], par["b_ih"],
                                                 par["b_hh"], par["wdec"], par["convw"], par["watt"], par["gvec"], par["bo"],
                                                 par["w_out"], par["b_out"], w0, opts)
        return logits, ws
    hb.persist_clear_abort(dev)
    want_l, want_w = run()
    torch.cuda.synchronize()
    assert not hb.persist_aborted(dev) and torch.isfinite(want_l).all()
    try:
        hb.DEC_FAULT[0] = True
        (got_l, got_w), ms = _timed_ms(run)
    finally:
        hb.DEC_FAULT[0] = False
    ctrl = hb.persist_scratch(dev)[1].cpu().tolist()
    assert ms < 100.0, "got %.1f ms" % ms
    assert ctrl[0] == 1 and ctrl[1] in (11, 12, 14, 16, 17), "latch + the code of a decoder-forward wait, got %s" % ctrl[:2]
    assert ctrl[16 + 8] == 1
    assert torch.isnan(got_l[L - 1, :4]).all(), "the stalled group's utterances (rows 0..3) end in NaN"
    hb.persist_clear_abort(dev)
    again_l, again_w = run()
    torch.cuda.synchronize()
    assert not hb.persist_aborted(dev)
    assert torch.equal(again_w, want_w), "the kernel's own outputs are bit-identical to those before the fault"
    _close(again_l, want_l, rtol=1e-5, atol=1e-6, what="logits after the fault")     # (a split-K product: atomics, run-to-run order)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_labels", [False, True])
def test_sampled_decoding_with_injected_draws(monkeypatch, with_labels):
    """sample=True (model.py:347-351: Categorical(logits).sample() instead of argmax) cannot match across RNGs, so - like
    the dropout masks - the DRAWS are injected: both sides turn the same pre-drawn uniforms into tokens through the inverse
    CDF of their own probabilities.  Free-running sampling (ys=None) and scheduled sampling whose non-teacher steps feed the
    SAMPLED token (ys given, tf_rate 0.5): predictions, log-probabilities, attention and every gradient against the oracle."""
    dev = _gpu()
    cfg = dict(synth.TINY)
    ld = synth.labeldist(9, 12)
    w = synth.e2e_weights(cfg, 11)
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    steps = 6
    draws = torch.rand(64, len(ilens), generator=torch.Generator().manual_seed(77))
    state = {"k": 0}

    def inverse_cdf(self, sample_shape=torch.Size()):
        u = draws[state["k"]].to(self.probs.device)
        state["k"] += 1
        cdf = torch.cumsum(self.probs.double(), dim=-1)
        return (cdf < u.double().unsqueeze(-1)).sum(-1).clamp(max=self.probs.shape[-1] - 1)

    monkeypatch.setattr(torch.distributions.Categorical, "sample", inverse_cdf)
    net = _product(cfg, w, ld, dev)
    kw = dict(sample=True, max_dec_timesteps=steps, tf_rate=0.5 if with_labels else 1.0)
    state["k"] = 0
    np.random.seed(4)
    _, lp, pred, ws = net(torch.from_numpy(xs).to(dev), ilens,
                          [torch.from_numpy(y).to(dev) for y in ys] if with_labels else None, **kw)
    used = state["k"]
    sd = O.make_leaf_state(w)
    state["k"] = 0
    np.random.seed(4)
    _, rlp, rpred, rws = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens,
                                       [torch.from_numpy(y) for y in ys] if with_labels else None, **kw)
    assert used == state["k"] == pred.shape[1], "one draw per decoder step on both sides"
    assert torch.equal(pred.cpu(), rpred), "the sampled hypotheses agree token for token"
    _close(lp, rlp, what="log-probs of the sampled hypothesis"); _close(ws, rws, what="attention weights")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


def test_greedy_decoding_with_a_large_vocabulary():
    """V > 128 is outside the fused feedback kernels (their logits tile) and V > 64 outside the persistent free-running
    kernel: greedy decoding then runs on the per-step kernels + torch glue (ops._DecoderSeq) - against the oracle."""
    dev = _gpu()
    cfg = dict(synth.TINY, output_dim=140)
    ld = synth.labeldist(140, 12)
    w = synth.e2e_weights(cfg, 17)
    xs, ilens, _ = synth.batch(8, 140, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    net = _product(cfg, w, ld, dev)
    _, lp, pred, ws = net(torch.from_numpy(xs).to(dev), ilens, None, max_dec_timesteps=5)
    sd = O.make_leaf_state(w)
    _, rlp, rpred, rws = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens, None, max_dec_timesteps=5)
    assert torch.equal(pred.cpu(), rpred)
    _close(lp, rlp, what="lp"); _close(ws, rws, what="ws")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    for n, gr in _grads(net).items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


def test_embedding_gradient_with_a_table_larger_than_lds():
    """asr_embedding_grad_f32 folds its rows into an LDS table [V][E] and declines tables over 64 KB (ASR_E_SHAPE on the C side;
    hip_backend.embedding_grad returns False before calling it): ops._DecoderSeq then takes index_add_.  V * E = 300 * 64
    floats = 76.8 KB - teacher-forced gradients against the oracle, the embedding's among them."""
    dev = _gpu()
    cfg = dict(synth.TINY, output_dim=300, embedding_dim=64)
    assert cfg["output_dim"] * cfg["embedding_dim"] * 4 > 65536
    ld = synth.labeldist(300, 12)
    w = synth.e2e_weights(cfg, 19)
    xs, ilens, ys = synth.batch(8, 300, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    net = _product(cfg, w, ld, dev)
    np.random.seed(3)
    _, lp, _, _ = net(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys])
    sd = O.make_leaf_state(w)
    np.random.seed(3)
    _, rlp, _, _ = O.e2e_forward(sd, dict(cfg, labeldist=ld), torch.from_numpy(xs), ilens, [torch.from_numpy(y) for y in ys])
    _close(lp, rlp, what="lp")
    names = O.unique_param_names(sd)
    rg = dict(zip(names, torch.autograd.grad(-rlp.mean(), [sd[n] for n in names])))
    net.zero_grad()
    (-lp.mean()).backward()
    got = _grads(net)
    assert float(got["decoder.embedding.weight"].abs().max()) > 0
    for n, gr in got.items():
        _close(gr, rg[n], atol=1e-6, what="grad " + n)


class _ExactAllocation(object):
    """`numel` floats from hipMalloc itself (ctypes on libamdhip64: not torch's caching allocator, which rounds a request up
    and parks it inside a larger segment), exposed to torch through __cuda_array_interface__: the tensor's last element is
    the allocation's last."""

    _hip = None

    def __init__(self, shape):
        import ctypes
        if _ExactAllocation._hip is None:
            _ExactAllocation._hip = ctypes.CDLL("libamdhip64.so")
        self.shape = tuple(int(v) for v in shape)
        n = 1
        for v in self.shape:
            n *= v
        self.ptr = ctypes.c_void_p()
        rc = self._hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(4 * n))
        assert rc == 0 and self.ptr.value, "hipMalloc(%d) -> %d" % (4 * n, rc)
        self.__cuda_array_interface__ = dict(shape=self.shape, typestr="<f4", data=(int(self.ptr.value), False), version=2, strides=None)

    def tensor(self, values=None):
        t = torch.as_tensor(self, device="cuda")
        assert t.data_ptr() == self.ptr.value
        if values is not None:
            t.copy_(values)
        return t

    def free(self):
        if self.ptr.value:
            torch.cuda.synchronize()
            self._hip.hipFree(self.ptr)
            self.ptr.value = None


@pytest.mark.parametrize("case", ["bfk_m_tail", "bfs_k_tail_tn", "bfs_k_tail_nt", "bfs_m_tail"])
def test_gemm_operands_flush_against_the_end_of_an_allocation(case):
    """gemm_bfk_kernel's M tiles and the masked K tail of gemm_bfs_kernel used to carry their tile offset in the
    buffer instruction's SGPR offset, which the hardware's range check does not see - a fetch behind the operand.  Operands
    from exact-size hipMalloc allocations (the operand's last byte is the allocation's last), M % 128 != 0 or K % 32 != 0:
    the products against float64, with nothing behind the operands that a stray fetch could lean on.  (The static half of
    this guard - no buffer load of these kernels has an SGPR offset - is tests/test_isa_guard_cpu.py.)"""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(11)
    if case == "bfk_m_tail":                 # layer-0 input projection: [M, 80] x [8H, 80]^T, M % 128 = 37
        M, N, K, ta, tb, mode = 10021, 4096, 80, False, True, "bf16x6"
    elif case == "bfs_k_tail_tn":            # weight gradient over packed rows: dG^T x, K = rows, K % 32 = 4
        M, N, K, ta, tb, mode = 4096, 512, 10916, True, False, "bf16x6"
    elif case == "bfs_k_tail_nt":            # k-contiguous operands with a masked tail
        M, N, K, ta, tb, mode = 1000, 1024, 2084, False, True, "bf16x6+sp"
    else:                                    # M % 256 = 148: edge tile rows clamped
        M, N, K, ta, tb, mode = 10900, 512, 2048, False, True, "bf16x6"
    a_shape = (K, M) if ta else (M, K)
    b_shape = (N, K) if tb else (K, N)
    A, B = torch.randn(*a_shape, generator=g), torch.randn(*b_shape, generator=g)
    allocs = [_ExactAllocation(a_shape), _ExactAllocation(b_shape), _ExactAllocation((M, N))]
    try:
        At, Bt, Ct = allocs[0].tensor(A), allocs[1].tensor(B), allocs[2].tensor(torch.zeros(M, N))
        with hb.arith(mode):
            hb.gemm(At, Bt, trans_a=ta, trans_b=tb, out=Ct)
        ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
        _close(Ct, ref.float(), rtol=1e-5, atol=1e-4 * float(K) ** 0.5, what=case)
    finally:
        for a in allocs:
            a.free()


@pytest.mark.parametrize("arith,rtol", [("bf16x6", 1e-5), ("bf16x3", 3e-5)])
@pytest.mark.parametrize("mask", [0xff, 0xf0, 0x01, 0xaa])
def test_gemm_side_on_a_subset_of_the_xcds(mask, arith, rtol):
    """asr_gemm_side_f32: the 64 x 64 queue instantiation that runs beside the persistent kernels of a small batch, restricted
    to the XCDs of `mask` - every (tile, K slice) is computed exactly once wherever the hardware places the workgroups (one
    XCD, four, all eight), the K slices and an initial C add up, edges in M, N and a K tail are guarded; transposed operands;
    the batched row-shifted form of dW_hh.  Against float64."""
    dev = _gpu()
    import hip_backend as hb
    g = torch.Generator().manual_seed(mask)
    tol = dict(rtol=rtol)
    for (ta, tb, M, N, K) in ((True, False, 1024, 512, 5248), (True, False, 100, 70, 333), (False, True, 200, 130, 96),
                              (False, False, 64, 64, 2048), (True, True, 130, 64, 40)):
        A = torch.randn(*((K, M) if ta else (M, K)), generator=g)
        B = torch.randn(*((N, K) if tb else (K, N)), generator=g)
        C0 = torch.randn(M, N, generator=g)
        out = C0.clone().to(dev)
        queue = torch.zeros(1, dtype=torch.int32, device=dev)
        with hb.arith(arith):
            assert hb.gemm_side(A.to(dev), B.to(dev), out, queue, mask, trans_a=ta, trans_b=tb)
        ref = C0.double() + (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
        _close(out, ref.float(), atol=1e-4 * float(K) ** 0.5, what="%s%s %dx%dx%d mask %#x" % ("T" if ta else "N", "T" if tb else "N", M, N, K, mask), **tol)
        assert int(queue.item()) > 0
    # dW_hh of a bidirectional layer over packed rows: batch over the directions, K = R rows, operands shifted by one row
    H, R = 64, 520
    dG = torch.randn(R + 1, 2, 4 * H, generator=g)
    y = torch.randn(R + 1, 2 * H, generator=g)
    dG[R], y[R] = 0.0, 0.0
    out = torch.zeros(2, 4 * H, H, device=dev)
    queue = torch.zeros(1, dtype=torch.int32, device=dev)
    ldg, ldy = 2 * 4 * H, 2 * H
    with hb.arith(arith):
        assert hb.gemm_side_batched(dG.to(dev), y.to(dev), out, queue, mask, True, False, 4 * H, H, R, ldg, ldy, H, 2,
                                    4 * H - ldg, ldy + H, 4 * H * H, a_off=ldg, b_off=0)
    ref = torch.stack([dG[1:, 0].double().t() @ y[:R, :H].double(), dG[:R, 1].double().t() @ y[1:, H:].double()])
    _close(out, ref.float(), atol=1e-4 * float(R) ** 0.5, what="batched dW_hh mask %#x" % mask, **tol)
    with hb.arith("f32"):
        assert hb.gemm_side(A.to(dev), B.to(dev), torch.zeros(M, N, device=dev), queue.zero_(), mask, trans_a=ta, trans_b=tb) is False


def test_weight_gradients_beside_the_chains_equal_the_main_stream_ones():
    """A batch of <= 8 utterances: the encoder's weight-gradient products run on a side stream, on the XCDs the persistent
    kernels leave idle (ops._SideStream, asr_gemm_side_f32), joined when the backward pass ends.  The 3 x 512 model (persistent
    kernels on) at B = 8: every gradient equals the one of the same pass with the side stream switched off (the K slices meet
    in atomics on both paths: equal to rounding, not to the bit), the side stream was used, and reading .grad right behind
    backward() needs no synchronisation of the caller's.  Twice the same model in ONE graph (the semi-supervised step's two
    passes): a weight with two gradients on their way keeps its products on the main stream."""
    dev = _gpu()
    import ops
    import hip_backend as hb
    cfg = dict(synth.CFG2)
    ld = synth.labeldist(cfg["output_dim"], 5)
    w = synth.e2e_weights(cfg, 99)
    net = _product(cfg, w, ld, dev)
    xs, ilens, ys = synth.ragged_batch(8, 320, cfg["input_dim"], cfg["output_dim"], 77)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    assert hb.idle_xcd_mask(8) == 0xF0 and hb.idle_xcd_mask(9) == 0 and hb.idle_xcd_mask(0) == 0

    def grads(side, passes=1):
        ops._SIDE.enabled = side
        before = ops._SIDE.launches
        net.zero_grad()
        np.random.seed(4)
        loss = 0.0
        for _ in range(passes):
            _, lp, _, _ = net(xs_d, ilens, ys_d)
            loss = loss - lp.mean()
        with hb.require_persistent():
            loss.backward()
        out = {n: g_.clone() for n, g_ in _grads(net).items()}          # (no synchronize: the join is the engine's)
        return out, ops._SIDE.launches - before

    try:
        on, used = grads(True)
        off, unused = grads(False)
        assert used >= 3 and unused == 0, (used, unused)      # layers 1, 2 (dW_ih + dW_hh each), the layer-0 projection
        for n in off:
            _close(on[n], off[n], rtol=2e-5, atol=1e-7, what="side vs main: " + n)
        two, used2 = grads(True, passes=2)
        ref2, _ = grads(False, passes=2)
        assert 0 < used2, used2
        for n in ref2:
            _close(two[n], ref2[n], rtol=2e-5, atol=1e-7, what="two passes, side vs main: " + n)
    finally:
        ops._SIDE.enabled = True
    assert not hb.persist_aborted(dev)


def test_side_stream_survives_a_backward_pass_that_raised():
    """ops._SideStream registers its join with the autograd engine per backward PASS.  A pass that raises half way (here: in
    the backward of encoder layer 1, with the products of layer 2 queued) never runs that join; the next pass must drop what
    it left, register its own join and deliver complete gradients."""
    dev = _gpu()
    import ops
    cfg = dict(synth.CFG2)
    ld = synth.labeldist(cfg["output_dim"], 5)
    net = _product(cfg, synth.e2e_weights(cfg, 99), ld, dev)
    xs, ilens, ys = synth.ragged_batch(8, 320, cfg["input_dim"], cfg["output_dim"], 78)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]

    def run():
        net.zero_grad()
        np.random.seed(4)
        _, lp, _, _ = net(xs_d, ilens, ys_d)
        (-lp.mean()).backward()
        return {n: g_.clone() for n, g_ in _grads(net).items()}

    real = ops._LstmLayer.backward
    state = {"calls": 0}

    def exploding(ctx, dy):
        state["calls"] += 1
        if state["calls"] == 2:                      # the second LSTM layer of the pass (layer 1): products of layer 2 are queued
            raise RuntimeError("boom")
        return real(ctx, dy)

    want = run()
    ops._LstmLayer.backward = staticmethod(exploding)
    try:
        with pytest.raises(RuntimeError, match="boom"):
            run()
    finally:
        ops._LstmLayer.backward = staticmethod(real)
    assert ops._SIDE.active is not None and ops._SIDE.deferred, "the failed pass left its state behind (what this test is about)"
    got = run()
    assert ops._SIDE.active is None and not ops._SIDE.deferred
    for n in want:
        _close(got[n], want[n], rtol=2e-5, atol=1e-7, what="after a failed pass: " + n)
