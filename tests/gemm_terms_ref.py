"""CPU model of the GEMM kernels of csrc/gemm.hip, term by term, and the rule their outputs are held to.  numpy only, no GPU.

The split-bf16 kernels do not compute A B: they compute a fixed sum of products of bf16 TERMS of the fp32 operands
(gemm.hip, "split-bf16 product" and "Three-term split").  The terms are emulated here bit for bit, their products are
formed in float64, and a kernel's output is compared with the sum of exactly the products it keeps:

    f32      A B
    bf16x6   T00 + T01 + T10 + T02 + T20 + T11      T[p][q] = term_p(A) term_q(B), terms (a, b, c) of split3
    bf16x3   T00 + T01 + T10                        terms (hi, lo) of split2

Unit.  Element (m, n) is measured in units of 2^-24 S[m, n], S = |A| |B| (+ |bias| + |base| where the call has them): the
quantity every worst-case bound of an fp32 sum of these terms is written in, whatever the order of the sum.  Where S == 0
the output must equal the model exactly.

Yardstick.  No tolerance is written down.  Y of a case is the largest error, in the same unit, of a plain fp32 product of
the same operands (K outer-product adds, one k after another, then the fp32 epilogue) against their float64 product.  A
kernel passes when max e <= FACTOR * Y: another summation order of the same terms, no more (FACTOR = 4 as in
tests/test_ctc_gpu.py).  tests/test_gemm_terms_cpu.py proves that a lost or doubled cross product fails this rule on every
case flagged `terms`; the cases with a longer K can only assert the rule and say so in their name ("rule_only").

Operands: randn times a power of two per row of A and per column of B (2^-6 .. 2^6), so that rows far below the largest
output are checked like the others; stored in NaN-filled buffers with a leading dimension larger than the extent and a row
of NaN behind the last; outputs are views into a buffer filled with a sentinel bit pattern that the padding must keep."""
import collections
import functools

import numpy as np

UNIT = 2.0 ** -24
FACTOR = 4.0
SENTINEL = 0x7fc5a5a5                      # a quiet NaN with a payload: an element nobody wrote fails as NaN
LAYOUTS = (("NT", False, True), ("NN", False, False), ("TN", True, False), ("TT", True, True))
KEPT = {"bf16x6": ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)), "bf16x3": ((0, 0), (0, 1), (1, 0))}
EPILOGUES = ("plain", "bias", "bias_relu", "acc")
DROP_P, DROP_SEED = 0.25, 20261


# ------------------------------------------------------------------------------------------------ split emulation
def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bf16_rne(x):
    """fp32 -> the nearest bf16 value (ties to even), as an fp32 array with 16 zero low bits (finite inputs, no overflow)."""
    u = _f32(x).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def is_bf16(x):
    return bool(((_f32(x).view(np.uint32) & np.uint32(0xffff)) == 0).all())


def split3(x):
    """bfn_split2<3>: a = bf16(x), b = bf16(x - a), c = x - a - b; c is a bf16 value and a + b + c == x exactly."""
    x = _f32(x)
    a = bf16_rne(x)
    r = x - a                              # exact in fp32
    b = bf16_rne(r)
    c = r - b                              # exact, at most 8 significand bits
    assert is_bf16(c), "the third term of the split does not fit bf16"
    assert (a.astype(np.float64) + b.astype(np.float64) + c.astype(np.float64) == x.astype(np.float64)).all()
    assert ((x.astype(np.float64) - a) == r).all() and ((r.astype(np.float64) - b) == c).all()
    return a, b, c


def split2(x):
    """bfn_split2<2>: hi = the upper 16 bits of the word, lo = bf16(x - hi) rounded to nearest."""
    x = _f32(x)
    hi = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = x - hi                             # exact
    assert ((x.astype(np.float64) - hi) == r).all()
    return hi, bf16_rne(r)


def terms_of(arith, x):
    return split3(x) if arith == "bf16x6" else split2(x)


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(M, N, K, b=0):
    """The logical operands of a case, the same under every layout and arithmetic: A [M, K], B [K, N], bias [N], base [M, N]."""
    rs = np.random.RandomState(1000003 * M + 1009 * N + 7 * K + 7919 * b)
    ra = 2.0 ** rs.randint(-6, 7, size=M)
    cb = 2.0 ** rs.randint(-6, 7, size=N)
    A = _f32(rs.randn(M, K) * ra[:, None])
    B = _f32(rs.randn(K, N) * cb[None, :])
    bias = _f32(rs.randn(N) * cb * np.sqrt(K))
    base = _f32(rs.randn(M, N) * ra[:, None] * cb[None, :] * np.sqrt(K))
    for x in (A, B, bias, base):
        x.setflags(write=False)
    return A, B, bias, base


def padded(x, misaligned=False):
    """x [rows, cols] inside a NaN-filled buffer -> (buffer, column offset): leading dimension larger than cols (a
    multiple of four and a 16-byte aligned view; misaligned: an odd one and a view that starts at element 1), one row of NaN behind."""
    rows, cols = x.shape
    if misaligned:
        ld, off = cols + 3 + (cols % 2), 1
        assert ld % 2 == 1
    else:
        ld, off = (cols + 3) // 4 * 4 + 4, 0
    buf = np.full((rows + 1, ld), np.nan, dtype=np.float32)
    buf[:rows, off:off + cols] = x
    return buf, off


def out_buffer(M, N, base=None, dense=False, batch=None):
    """An output buffer of sentinels, [M + 1, N + 5] (dense: ld = N), whose view [:M, 2 : 2 + N] holds `base` where given."""
    ldc, off = (N, 0) if dense else (N + 5, 2)
    shape = (M + 1, ldc) if batch is None else (batch, M + 1, ldc)
    buf = np.full(shape, SENTINEL, dtype=np.uint32).view(np.float32)
    if base is not None:
        buf[..., :M, off:off + N] = base
    return buf, off


def padding_kept(buf, M, N, off):
    """True when everything outside the view [..., :M, off : off + N] still holds the sentinel."""
    u = np.ascontiguousarray(buf).view(np.uint32).copy()
    u[..., :M, off:off + N] = SENTINEL
    return bool((u == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ model and rule
def seq_product_f32(A, B):
    """The yardstick's product: K float32 outer-product adds, one k after another."""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc += np.multiply.outer(A[:, k], B[k, :])
    return acc


def epilogue(v, epi, bias, base, mask=None):
    """(v + bias) + base, ReLU, mask - in the dtype of v (float64: the model; float32: the yardstick)."""
    dt = v.dtype
    if epi in ("bias", "bias_relu", "drop"):
        v = v + bias.astype(dt)[None, :]
    if epi == "acc":
        v = v + base.astype(dt)
    if epi in ("bias_relu", "drop"):
        v = np.maximum(v, dt.type(0))
    if epi == "drop":
        v = v * mask.astype(dt)
    return v


def scale_of(S0, epi, bias, base, mask=None):
    S = S0.copy()
    if epi in ("bias", "bias_relu", "drop"):
        S += np.abs(bias.astype(np.float64))[None, :]
    if epi == "acc":
        S += np.abs(base.astype(np.float64))
    if epi == "drop":
        S *= mask.astype(np.float64)
    return S


@functools.lru_cache(maxsize=32)
def products(M, N, K, b=0):
    """Everything of a shape that does not depend on layout or epilogue: the float64 product, S0, the fp32 yardstick
    product and the float64 term products of both splits."""
    A, B, _, _ = operands(M, N, K, b)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    out = dict(P=A64 @ B64, S0=np.abs(A64) @ np.abs(B64), seq=seq_product_f32(A, B))
    for arith in ("bf16x6", "bf16x3"):
        ta = [t.astype(np.float64) for t in terms_of(arith, A)]
        tb = [t.astype(np.float64) for t in terms_of(arith, B)]
        out[arith] = {pq: ta[pq[0]] @ tb[pq[1]] for pq in KEPT[arith]}
    return out


Ref = collections.namedtuple("Ref", "model S Y prod terms bias base epi mask")


def reference(M, N, K, arith, epi, b=0, mask=None):
    """The model of one call in float64, its scale S and its yardstick Y.  `prod` is the model before the epilogue and
    `terms` its kept products (None for f32): what the power test takes away or adds."""
    _, _, bias, base = operands(M, N, K, b)
    pr = products(M, N, K, b)
    terms = pr.get(arith)
    prod = pr["P"] if terms is None else sum(terms[pq] for pq in KEPT[arith])
    S = scale_of(pr["S0"], epi, bias, base, mask)
    Y = error(epilogue(pr["seq"], epi, bias, base, mask), epilogue(pr["P"], epi, bias, base, mask), S)
    return Ref(epilogue(prod, epi, bias, base, mask), S, Y, prod, terms, bias, base, epi, mask)


def remodel(ref, prod):
    """The model of `ref` with another product under the same epilogue (the power test's mutated models)."""
    return epilogue(prod, ref.epi, ref.bias, ref.base, ref.mask)


def error(got, model, S):
    """max over the elements of |got - model| / (2^-24 S); inf where got is not finite or differs from the model at S == 0."""
    got = np.asarray(got)
    if got.shape != model.shape or not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got.astype(np.float64) - model)
    z = S == 0
    if z.any() and (d[z] != 0).any():
        return float("inf")
    if z.all():
        return 0.0
    return float((d[~z] / (UNIT * S[~z])).max())


def passes(got, model, S, Y):
    return error(got, model, S) <= FACTOR * Y


def check(case, kernel, got, ref):
    """Print the case's line and assert the rule."""
    e = error(got, ref.model, ref.S)
    print("gemm_parity %s %s: e_max %.3f, Y %.3f, ratio %.3f" % (case, kernel, e, ref.Y, e / ref.Y if ref.Y > 0 else float("inf")))
    assert e <= FACTOR * ref.Y, "%s on %s: e_max %.3f units of 2^-24 S, above %g x the fp32 yardstick's %.3f" % (case, kernel, e, FACTOR, ref.Y)
    return e


# ------------------------------------------------------------------------------------------------ column sums
def colsum_reference(M, N, accumulate):
    """X [M, N] (the A operand of shape (M, 1, N) by another name), the float64 column sums (+ the old value), S and Y."""
    rs = np.random.RandomState(31 * M + N)
    X = _f32(rs.randn(M, N) * 2.0 ** rs.randint(-6, 7, size=N)[None, :])
    old = _f32(rs.randn(N) * np.sqrt(M) * np.abs(X).max(0))
    X64 = X.astype(np.float64)
    model, S = X64.sum(0), np.abs(X64).sum(0)
    seq = np.zeros(N, dtype=np.float32)
    for m in range(M):
        seq += X[m]
    if accumulate:
        model, S, seq = model + old, S + np.abs(old.astype(np.float64)), seq + old
    return X, old, model, S, error(seq, model, S)


# ------------------------------------------------------------------------------------------------ the case table
class Case(collections.namedtuple("Case", "family entry M N K layout arith flag epi split_k mis batch mask terms kernel plan")):
    """family: the row of the table below; entry: gemm / batched / side / skinny; layout: a name of LAYOUTS; arith + flag:
    what the call passes; epi: plain / bias / bias_relu / acc / drop; split_k: None (the library's), 1, n; mis: operands
    misaligned with an odd ld; batch; mask: the XCD mask of the side entry; terms: the power test covers it; kernel: the
    product kernel the call must run, in the short form of tools/isa_guard.py; plan: the other plan fields it must show."""

    @property
    def ta(self):
        return dict((n, a) for n, a, _ in LAYOUTS)[self.layout]

    @property
    def tb(self):
        return dict((n, b) for n, _, b in LAYOUTS)[self.layout]

    @property
    def mode(self):
        return self.arith + self.flag

    @property
    def name(self):
        parts = [self.family, "%dx%dx%d" % (self.M, self.N, self.K), self.layout, self.arith, self.epi]
        if self.split_k is not None:
            parts.append("sk%d" % self.split_k)
        if self.mis:
            parts.append("mis")
        if self.batch > 1:
            parts.append("b%d" % self.batch)
        if self.mask is not None:
            parts.append("x%02x" % self.mask)
        if not self.terms and self.arith != "f32":
            parts.append("rule_only")
        return "/".join(parts)


def _tf(*v):
    return ",".join(("true" if x else "false") if isinstance(x, bool) else str(x) for x in v)


POWER_MAX_K = 96          # a lost third-order product is 21+ units at K <= 128 against 4 Y = 13-16, 15 against 19.5 at K = 256


def _case(family, M, N, K, layout, arith, flag="", epi="plain", split_k=None, mis=False, batch=1, mask=None, entry="gemm", **plan):
    ta, tb = dict((n, (a, b)) for n, a, b in LAYOUTS)[layout]
    akc, bkc = not ta, tb
    nt = 3 if arith == "bf16x6" else 2
    kernel = {"f32": lambda: "gemm_f32_kernel<%s>" % _tf(akc, bkc),
              "bf3_128": lambda: "gemm_bf3_kernel<%s>" % _tf(akc, bkc, nt, 128, False),
              "bf3_64": lambda: "gemm_bf3_kernel<%s>" % _tf(akc, bkc, nt, 64, False),
              "queue": lambda: "gemm_bf3_kernel<%s>" % _tf(akc, bkc, nt, 64, True),
              "wide": lambda: "gemm_bf%dw_kernel<%s>" % (6 if nt == 3 else 3, _tf(akc, bkc)),
              "bfs": lambda: "gemm_bfs_kernel<%s>" % _tf(akc, bkc, nt, bool(plan.get("kt"))),
              "bfk": lambda: "gemm_bfk_kernel<%s>" % _tf(nt, 5, bool(plan.get("plain")))}[family]()
    terms = arith != "f32" and K <= POWER_MAX_K
    return Case(family, entry, M, N, K, layout, arith, flag, epi, split_k, mis, batch, mask, terms, kernel, tuple(sorted(plan.items())))


def _with_epilogues(family, shapes, layout, arith, flag="", **plan):
    return [_case(family, M, N, K, layout, arith, flag, epi, **plan) for (M, N, K) in shapes for epi in EPILOGUES]


def family_cases(family, layout="NT", arith="bf16x6"):
    """The cases of one family under one layout and arithmetic (the parameters of one GPU test)."""
    c = []
    if family == "f32":
        c += _with_epilogues("f32", [(70, 66, 40), (130, 129, 33)], layout, "f32", split_k=1)
    elif family == "bf3_128":
        f = "+narrow"
        c += _with_epilogues(family, [(130, 129, 40), (130, 129, 33), (128, 128, 64)], layout, arith, f, split_k=1)
        # K = 96 in three slices: zero pass + atomics, atomics onto the base, and the late bias / ReLU pass
        c.append(_case(family, 130, 129, 96, layout, arith, f, "plain", split_k=3, zero_pass=1, behind=()))
        c.append(_case(family, 130, 129, 96, layout, arith, f, "acc", split_k=3, zero_pass=0, behind=()))
        c.append(_case(family, 130, 129, 96, layout, arith, f, "bias_relu", split_k=3, zero_pass=1, behind=("epilogue",)))
        # odd leading dimensions and views that start at element 1: every load guarded
        c.append(_case(family, 130, 129, 33, layout, arith, f, "bias_relu", mis=True, split_k=1))
        c.append(_case(family, 130, 129, 40, layout, arith, f, "acc", mis=True, split_k=1))
    elif family == "bf3_64":
        f = "+small"
        c += _with_epilogues(family, [(70, 66, 32), (70, 66, 36), (70, 66, 64)], layout, arith, f, split_k=1)
        c.append(_case(family, 70, 66, 64, layout, arith, f, "plain", split_k=2, zero_pass=1, behind=()))
        c.append(_case(family, 70, 66, 64, layout, arith, f, "bias_relu", split_k=2, zero_pass=1, behind=("epilogue",)))
        c.append(_case(family, 70, 66, 36, layout, arith, f, "bias", mis=True, split_k=1))
        c.append(_case(family, 70, 66, 32, layout, arith, f, "drop", split_k=1, behind=("dropout",)))
    elif family == "wide":
        f = "+wide"
        c += _with_epilogues(family, [(64, 64, 32), (260, 132, 64), (260, 132, 96)], layout, arith, f, split_k=1)
        # the kernel's own K split (the library's choice, asserted > 1), zero pass, atomics, the late pass
        c.append(_case(family, 260, 132, 1024, layout, arith, f, "plain", split_k_above=1, zero_pass=1, behind=()))
        c.append(_case(family, 260, 132, 1024, layout, arith, f, "bias_relu", split_k_above=1, zero_pass=1, behind=("epilogue",)))
    elif family == "bfs":
        f = "+sp"
        c += _with_epilogues(family, [(260, 132, 64)], layout, arith, f, split_k=1, kt=0)
        c += _with_epilogues(family, [(260, 132, 36), (260, 132, 68), (260, 132, 92)], layout, arith, f, split_k=1, kt=1)
    elif family == "bfk":
        assert layout == "NT", "gemm_bfk_kernel takes k-contiguous operands only"
        for epi in EPILOGUES:
            c.append(_case(family, 1024, 128, 80, layout, arith, "", epi, plain=int(epi in ("plain", "bias"))))
            c.append(_case(family, 1100, 200, 80, layout, arith, "", epi, plain=0))
    elif family == "queue":
        for mask in (0xff, 0x0f):
            c.append(_case(family, 70, 66, 64, layout, arith, "", "acc", mask=mask, entry="side"))
    elif family == "batched":
        c.append(_case("bf3_64", 70, 66, 32, layout, arith, "+small", "plain", batch=2, entry="batched", split_k=1))
        c.append(_case("bf3_64", 70, 66, 32, layout, arith, "+small", "acc", batch=2, entry="batched", split_k=1))
        c.append(_case("wide", 64, 64, 32, layout, arith, "+wide", "plain", batch=2, entry="batched", split_k=1))
        c.append(_case("wide", 64, 64, 32, layout, arith, "+wide", "acc", batch=2, entry="batched", split_k=1))
        c.append(_case("bfs", 260, 132, 36, layout, arith, "+sp", "plain", batch=2, entry="batched", split_k=1, kt=1))
        c.append(_case("bfs", 260, 132, 36, layout, arith, "+sp", "acc", batch=2, entry="batched", split_k=1, kt=1))
    else:
        raise KeyError(family)
    return c


FAMILIES = ("f32", "bf3_128", "bf3_64", "wide", "bfs", "bfk", "queue", "batched")
ARITHS = ("bf16x6", "bf16x3")
SKINNY = ((3, 9, 32, 1), (20, 34, 96, 1), (40, 34, 96, 2))          # M, N, K, the MT of skinny_kernel<MT>
COLSUM = ((33, 64, "colsum4_kernel"), (600, 130, "colsum_kernel"))


def family_params(family):
    """(layout, arith) pairs a family is parametrised over."""
    if family == "f32":
        return [(n, "f32") for n, _, _ in LAYOUTS]
    if family == "bfk":
        return [("NT", a) for a in ARITHS]
    return [(n, a) for n, _, _ in LAYOUTS for a in ARITHS]


def all_cases():
    return [c for fam in FAMILIES for (layout, arith) in family_params(fam) for c in family_cases(fam, layout, arith)]


def plan_kwargs(c, lda, ldb, ldc, sA=0, sB=0, sC=0):
    """The arguments of hip_backend.gemm_plan for a case whose buffers have these leading dimensions and strides."""
    return dict(trans_a=c.ta, trans_b=c.tb, lda=lda, ldb=ldb, ldc=ldc, batch=c.batch, sA=sA, sB=sB, sC=sC,
                bias=c.epi in ("bias", "bias_relu", "drop"), relu=c.epi in ("bias_relu", "drop"), accumulate=c.epi == "acc",
                drop=c.epi == "drop", split_k=c.split_k, arith=c.mode, misaligned=3 if c.mis else 0)


def assert_plan(c, p):
    """The plan of a case's call names the kernel of the case table and shows the fields the case pins."""
    assert p["rc"] == 0, (c.name, p)
    assert p["kernel"] == c.kernel, "%s: planned %s, the case is about %s" % (c.name, p["kernel"], c.kernel)
    want = dict(c.plan)
    if "split_k_above" in want:
        assert p["split_k"] > want.pop("split_k_above"), (c.name, p["split_k"])
    elif c.split_k is not None:
        assert p["split_k"] == c.split_k, (c.name, p["split_k"])
    for k, v in want.items():
        got = tuple(p[k]) if isinstance(p[k], list) else p[k]
        assert got == v, "%s: plan field %s is %r, the case pins %r" % (c.name, k, got, v)
    names = [l[0] for l in p["launches"]]
    assert ("zero_rows_kernel" in names) == bool(p["zero_pass"]) and ("bias_act_kernel" in names) == bool(p["behind"])


def storage(c, b=0):
    """The operands of a case as stored: (A buffer, offset, B buffer, offset), op(A) = A or A^T as the layout says."""
    A, B, _, _ = operands(c.M, c.N, c.K, b)
    a_buf, a_off = padded(A.T if c.ta else A, c.mis)
    b_buf, b_off = padded(B.T if c.tb else B, c.mis)
    return a_buf, a_off, b_buf, b_off
