"""Bit-level record of the GEMM kernels (csrc/gemm.hip):

    python tools/gemm_bits.py dump OUT.npz         fixed-seed inputs through every kernel family, layout and epilogue -> all outputs
    python tools/gemm_bits.py compare A.npz B.npz  exit 1 unless both hold the same arrays, equal as raw 32-bit words

Run `dump` in two checkouts (each in its own process) and `compare` anywhere: with split_k = 1 no product uses atomics, so the
kernels promise the same bits in every run and a change that is meant to keep behaviour must compare equal.  Only hb.gemm and
hb.gemm_batched are used; the family is forced with the arith suffixes (+narrow, +small, +wide, +sp) under both bf16 arithmetics,
and `dump` prints which kernels the plans named, so that a family nobody reached shows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARITHS = ["f32"] + [b + s for b in ("bf16x6", "bf16x3") for s in ("", "+narrow", "+small", "+wide", "+sp")]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
EPILOGUES = [("plain", False, False, False), ("bias", True, False, False), ("bias_relu", True, True, False),
             ("acc", False, False, True), ("acc_bias_relu", True, True, True)]
# the smallest shapes that reach each path: interior with one K tile; a wide interior tile with three / five ring stages (the
# Full loop); edges in M and N; 64 x 64; guarded loads
SHAPES = [(128, 128, 32), (256, 128, 96), (512, 256, 160), (257, 130, 64), (64, 64, 32), (33, 34, 9)]
SP_ONLY = [(260, 132, 100)]                     # edge with a masked K tail
BFK = [(1024, 128, 80), (1100, 200, 80)]        # short K, NT: every tile interior / guarded


def dump(path):
    import torch
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    dev, out, kernels = torch.device("cuda"), {}, set()
    rng = np.random.RandomState(20241019)

    def rand(*shape):
        return torch.from_numpy(rng.randn(*shape).astype(np.float32)).to(dev)

    def keep(name, t):
        out[name] = t.detach().cpu().contiguous().numpy().view(np.uint32)

    def run(M, N, K, ariths, layouts):
        ops = {False: (rand(M, K), rand(K, N)), True: (rand(K, M), rand(N, K))}
        bias, c0 = rand(N), rand(M, N)
        for ar in ariths:
            for ta, tb in layouts:
                A, B = ops[ta][0], ops[tb][1]
                for ename, use_bias, relu, acc in EPILOGUES:
                    C = c0.clone()
                    hb.gemm(A, B, trans_a=ta, trans_b=tb, bias=bias if use_bias else None, relu=relu, out=C, accumulate=acc, split_k=1,
                            arith=ar)
                    keep("%dx%dx%d_%s_%s%s_%s" % (M, N, K, ar, "T" if ta else "N", "T" if tb else "N", ename), C)
                    kernels.add(hb.gemm_plan(M, N, K, ta, tb, bias=use_bias, relu=relu, accumulate=acc, split_k=1, arith=ar).get("kernel", "refused"))

    for M, N, K in SHAPES:
        run(M, N, K, ARITHS, LAYOUTS)
    for M, N, K in SP_ONLY:
        run(M, N, K, ["bf16x6+sp", "bf16x3+sp"], LAYOUTS)
    for M, N, K in BFK:
        run(M, N, K, ["bf16x6", "bf16x3"], [(False, True)])
    # one batched call, transA: batch element b is A[b] [K][M], B[b] [K][N] -> out[b] [M][N]
    L, Bn, Tp, Od = 64, 3, 40, 72
    A, B, c0 = rand(Bn, L, Tp), rand(Bn, L, Od), rand(Bn, Tp, Od)
    for ar in ("f32", "bf16x6", "bf16x3"):
        for acc in (False, True):
            C = c0.clone()
            hb.gemm_batched(A, B, C, True, False, Tp, Od, L, Tp, Od, Od, Bn, L * Tp, L * Od, Tp * Od, accumulate=acc, arith=ar, split_k=1)
            keep("batched_%s_acc%d" % (ar, acc), C)
    # row-strided views of A and C: the padding columns of the output buffer stay zero
    M, N, K, pad = 257, 130, 64, 8
    Af, B, bias = rand(M, K + pad), rand(K, N), rand(N)
    for ar in ("f32", "bf16x6", "bf16x3", "bf16x6+sp"):
        Cf = torch.zeros(M, N + pad, device=dev)
        hb.gemm(Af[:, :K], B, bias=bias, relu=True, out=Cf[:, :N], split_k=1, arith=ar)
        assert not bool(Cf[:, N:].any()), "strided_%s wrote into the padding columns" % ar
        keep("strided_%s" % ar, Cf)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("gemm_bits: %d arrays -> %s" % (len(out), path))
    print("kernels planned (%d):\n  %s" % (len(kernels), "\n  ".join(sorted(kernels))))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    groups = {}
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)
        g = groups.setdefault("_".join(k.split("_")[:2]), [0, 0])          # shape_arith
        g[0] += 1
        g[1] += int(x.size)
        if not same:
            bad.append(k)
            print("%-60s %-10s DIFFER" % (k, "x".join(map(str, x.shape))))
    for name, (n, words) in sorted(groups.items()):
        print("%-34s %3d arrays %9d words  %s" % (name, n, words, "PASS" if not any(k == name or k.startswith(name + "_") for k in bad) else "DIFFER"))
    print("%d arrays: %s" % (len(a.files), "PASS, every array equal word for word" if not bad else "FAIL (%s)" % ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
