"""The proof of the GEMM checker (tests/gemm_terms_ref.py) itself, without a GPU: the model and the yardstick pass the rule
on every case of the table, a lost or doubled cross product fails it on every case flagged `terms`, the usual kernel
mistakes (a transposed tile, a row one place off, NaN from the padding, an element never written) fail it, the bf16x3
model is far from the float64 product, and the library plans for every case the kernel the case table names."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_terms_ref as R  # noqa: E402


def _cpu_mask(M, N):
    """A stand-in for SeededMask.tensor() where there is no GPU: keep / (1 - p) with its own generator."""
    keep = np.random.RandomState(M + N).rand(M, N) >= R.DROP_P
    return (keep / (1.0 - R.DROP_P)).astype(np.float32)


def _unique(cases):
    """One case per (shape, arithmetic, epilogue): the reference does not depend on layout, flag, split or entry."""
    seen = {}
    for c in cases:
        seen.setdefault((c.M, c.N, c.K, c.arith, c.epi), c)
    return sorted(seen.values(), key=lambda c: (c.M, c.N, c.K, c.arith, c.epi))


def _reference(c, b=0):
    return R.reference(c.M, c.N, c.K, c.arith, c.epi, b, _cpu_mask(c.M, c.N) if c.epi == "drop" else None)


CASES = R.all_cases()
UNIQUE = _unique(CASES)


def test_split_emulation_is_exact():
    rs = np.random.RandomState(0)
    x = np.concatenate([(rs.randn(20000) * 2.0 ** rs.randint(-12, 13, size=20000)).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23,
                                  1.0 + 3 * 2.0 ** -9, 255.0 / 256, 4096.0, -3.0 * 2.0 ** -20], dtype=np.float32),
                        rs.randint(0x30000000, 0x50000000, size=20000).astype(np.uint32).view(np.float32)])
    # round to nearest even on 16 dropped bits, against the definition
    a = R.bf16_rne(x)
    assert R.is_bf16(a)
    ulp = np.abs(((a.view(np.uint32) & np.uint32(0xff800000)).view(np.float32)).astype(np.float64)) * 2.0 ** -7
    d = np.abs(x.astype(np.float64) - a)
    assert (d <= ulp / 2).all()
    tie = d == ulp / 2
    assert tie.any() and ((a[tie & (x != 0)].view(np.uint32) >> np.uint32(16)) & np.uint32(1) == 0).all()
    a, b, c = R.split3(x)                                  # (asserts a + b + c == x and that c is a bf16 value)
    assert R.is_bf16(a) and R.is_bf16(b) and R.is_bf16(c)
    nz = x != 0
    assert (np.abs(b[nz]) <= 2.0 ** -8 * np.abs(x[nz])).all() and (np.abs(c[nz]) <= 2.0 ** -16 * np.abs(x[nz])).all()
    hi, lo = R.split2(x)
    assert (hi.view(np.uint32) == (x.view(np.uint32) & np.uint32(0xffff0000))).all() and R.is_bf16(lo)
    assert (np.abs(x.astype(np.float64) - hi - lo)[nz] <= 2.0 ** -16 * np.abs(x[nz])).all()
    assert (np.abs(hi) <= np.abs(x)).all()                 # truncation, not rounding: hi never exceeds x


def test_operands_cover_small_rows_and_sit_in_nan():
    c = R.family_cases("bf3_128", "TN", "bf16x6")[0]
    A, B, bias, base = R.operands(c.M, c.N, c.K)
    rows = np.abs(A).max(1)
    assert rows.max() / rows.min() > 2.0 ** 8 and np.abs(B).max(0).max() / np.abs(B).max(0).min() > 2.0 ** 8
    a_buf, a_off, b_buf, b_off = R.storage(c)
    assert a_buf.shape[0] == c.K + 1 and a_buf.shape[1] > c.M and a_buf.shape[1] % 4 == 0 and a_off == 0
    assert np.isnan(a_buf[c.K]).all() and np.isnan(a_buf[:, c.M:]).all() and (a_buf[:c.K, :c.M] == A.T).all()
    assert (b_buf[:c.K, :c.N] == B).all() and np.isnan(b_buf[:, c.N:]).all()
    m = [x for x in R.family_cases("bf3_128", "NT", "bf16x3") if x.mis][0]
    a_buf, a_off, b_buf, b_off = R.storage(m)
    assert a_buf.shape[1] % 2 == 1 and b_buf.shape[1] % 2 == 1 and a_off == 1 and b_off == 1 and np.isnan(a_buf[:, 0]).all()
    out, off = R.out_buffer(c.M, c.N, base)
    assert R.padding_kept(out, c.M, c.N, off) and (out[:c.M, off:off + c.N] == base).all()
    out[c.M, 0] = 0.0
    assert not R.padding_kept(out, c.M, c.N, off)
    out, off = R.out_buffer(c.M, c.N)
    assert R.error(out[:c.M, off:off + c.N], np.zeros((c.M, c.N)), np.ones((c.M, c.N))) == float("inf")    # nobody wrote it


def test_the_model_and_the_yardstick_pass_on_every_case():
    assert len(UNIQUE) >= 60
    for c in UNIQUE:
        for b in range(c.batch):
            r = _reference(c, b)
            assert 0.5 < r.Y < 16.0, (c.name, r.Y)                       # an fp32 sum of K terms, K <= 1024
            e = R.error(r.model.astype(np.float32), r.model, r.S)
            # (half an ulp is up to 2^-24 |model|, and |model| <= S up to the 2^-16 of the bf16x3 split)
            assert e <= 1.0 + 2.0 ** -15 and R.passes(r.model.astype(np.float32), r.model, r.S, r.Y), (c.name, e)
            yard = R.epilogue(R.products(c.M, c.N, c.K, b)["seq"], c.epi, r.bias, r.base, r.mask)
            if c.arith == "f32":
                assert R.error(yard, r.model, r.S) == r.Y
            elif c.arith == "bf16x6":                                     # fp32-equivalent: the yardstick passes its model too
                assert R.passes(yard, r.model, r.S, r.Y), (c.name, R.error(yard, r.model, r.S), r.Y)


def test_a_lost_or_doubled_cross_product_fails_on_every_terms_case():
    flagged = [c for c in UNIQUE if c.terms]
    assert flagged and all(c.K <= R.POWER_MAX_K for c in flagged)
    assert all(c.terms == (c.K <= R.POWER_MAX_K) for c in CASES if c.arith != "f32")
    assert all(("rule_only" in c.name) == (not c.terms and c.arith != "f32") for c in CASES)
    weakest = {}
    for c in flagged:
        r = _reference(c)
        for pq in R.KEPT[c.arith][1:]:
            for sign, what in ((-1.0, "lost"), (1.0, "doubled")):
                got = R.remodel(r, r.prod + sign * r.terms[pq]).astype(np.float32)
                e = R.error(got, r.model, r.S)
                assert e > R.FACTOR * r.Y, "%s: T%d%d %s gives e_max %.2f, inside %g x Y = %.2f" % (c.name, pq[0], pq[1], what, e, R.FACTOR, R.FACTOR * r.Y)
                weakest[c.K] = min(weakest.get(c.K, 1e30), e / (R.FACTOR * r.Y))
    print("gemm_parity power: smallest e_max / (4 Y) of a lost or doubled product, by K: %s" % sorted(weakest.items()))


@pytest.mark.parametrize("arith", ["f32", "bf16x6", "bf16x3"])
def test_kernel_mistakes_fail(arith):
    for (M, N, K) in ((130, 129, 40), (70, 66, 64)):
        r = R.reference(M, N, K, arith, "bias")
        good = r.model.astype(np.float32)
        assert R.passes(good, r.model, r.S, r.Y)
        t = good.copy()                                   # a 32 x 32 tile written transposed
        t[32:64, 0:32] = good[32:64, 0:32].T
        assert not R.passes(t, r.model, r.S, r.Y)
        s = good.copy()                                   # a row one place off
        s[17, 1:] = good[17, :-1]
        assert not R.passes(s, r.model, r.S, r.Y)
        s = good.copy()
        s[5:7] = good[[6, 5]]
        assert not R.passes(s, r.model, r.S, r.Y)
        # one k too many, read from the gap behind a row of A: the NaN of the padding reaches row 3
        A, B, bias, _ = R.operands(M, N, K)
        a_buf, a_off = R.padded(A)
        leak = good.copy()
        leak[3] += a_buf[3, a_off + K] * B[0]
        assert np.isnan(leak[3]).all() and not R.passes(leak, r.model, r.S, r.Y)
        one = good.copy()                                 # a single element, a hundred units off, in the smallest row
        m = int(np.argmin(r.S.max(1)))
        one[m, 7] += np.float32(100 * R.UNIT * r.S[m, 7])
        assert not R.passes(one, r.model, r.S, r.Y)
        assert R.error(good[:, :-1], r.model, r.S) == float("inf")


def test_zero_scale_elements_must_be_exact():
    model, S = np.array([[0.0, 1.0]]), np.array([[0.0, 1.0]])
    assert R.error(np.array([[0.0, 1.0]], dtype=np.float32), model, S) == 0.0
    assert R.error(np.array([[1e-30, 1.0]], dtype=np.float32), model, S) == float("inf")
    # a dropped element has S == 0: anything but zero fails
    c = [x for x in CASES if x.epi == "drop"][0]
    r = _reference(c)
    got = r.model.astype(np.float32)
    assert (r.mask == 0).any() and R.passes(got, r.model, r.S, r.Y)
    m, n = np.argwhere(r.mask == 0)[0]
    got[m, n] = np.float32(1e-20)
    assert not R.passes(got, r.model, r.S, r.Y)


def test_the_bf16x3_model_is_not_the_float64_product():
    """bf16x3 drops lo lo' and the rounding of lo: its model sits tens to hundreds of units from A B, so a kernel that passes
    against this model is held to its own arithmetic, and one that computed something better or worse would not pass."""
    dist = []
    for c in UNIQUE:
        if c.arith != "bf16x3" or c.epi != "plain":
            continue
        r = _reference(c)
        P = R.products(c.M, c.N, c.K)["P"]
        e = R.error(P.astype(np.float32), r.model, r.S)
        assert e > R.FACTOR * r.Y, (c.name, e, r.Y)
        x6 = R.reference(c.M, c.N, c.K, "bf16x6", "plain").model
        assert R.error(x6.astype(np.float32), r.model, r.S) > R.FACTOR * r.Y
        dist.append(e)
    assert len(dist) >= 8
    print("gemm_parity bf16x3 model: %.0f .. %.0f units from the float64 product" % (min(dist), max(dist)))


def test_column_sum_yardstick():
    for (M, N, _) in R.COLSUM:
        for acc in (False, True):
            X, old, model, S, Y = R.colsum_reference(M, N, acc)
            assert 0.0 < Y < 16.0 and R.passes(model.astype(np.float32), model, S, Y)
            bad = model.astype(np.float32)
            bad[1:] = bad[:-1].copy()
            assert not R.passes(bad, model, S, Y)
            assert not R.passes((model - X[-1]).astype(np.float32), model, S, Y)        # the last row left out


# ------------------------------------------------------------------------------------------------ plans (the library, no device)
@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend
    return hip_backend


def _plan_of(hb, c):
    a_buf, _, b_buf, _ = R.storage(c)
    out, _ = R.out_buffer(c.M, c.N, dense=c.epi == "drop")
    st = (a_buf.size, b_buf.size, out.size) if c.batch > 1 else (0, 0, 0)
    return hb.gemm_plan(c.M, c.N, c.K, **R.plan_kwargs(c, a_buf.shape[1], b_buf.shape[1], out.shape[-1], *st))


def test_every_case_plans_the_kernel_it_names(hb):
    planned = set()
    for c in CASES:
        if c.entry == "side":                  # asr_gemm_side_f32 has one kernel and no plan: the launch is the assertion
            planned.add(c.kernel)
            continue
        p = _plan_of(hb, c)
        R.assert_plan(c, p)
        planned.update(l[0] for l in p["launches"])
    lay = [R._tf(not ta, tb) for _, ta, tb in R.LAYOUTS]
    want = {"zero_rows_kernel", "bias_act_kernel"}
    want |= {"gemm_f32_kernel<%s>" % l for l in lay}
    want |= {"gemm_bf3_kernel<%s,%d,%d,%s>" % (l, nt, ts, q) for l in lay for nt in (2, 3) for ts, q in ((128, "false"), (64, "false"), (64, "true"))}
    want |= {"gemm_bf%dw_kernel<%s>" % (w, l) for l in lay for w in (3, 6)}
    want |= {"gemm_bfs_kernel<%s,%d,%s>" % (l, nt, kt) for l in lay for nt in (2, 3) for kt in ("true", "false")}
    want |= {"gemm_bfk_kernel<%d,5,%s>" % (nt, pl) for nt in (2, 3) for pl in ("true", "false")}
    assert want <= planned, sorted(want - planned)
    assert set(mt for _, _, _, mt in R.SKINNY) == {1, 2} and set(k for _, _, k in R.COLSUM) == {"colsum_kernel", "colsum4_kernel"}


def test_the_plans_show_what_the_cases_are_about(hb):
    by = lambda **kw: [c for c in CASES if all(getattr(c, k) == v for k, v in kw.items())]
    p = _plan_of(hb, by(family="bf3_128", K=96, epi="bias_relu", layout="NT", arith="bf16x6")[0])
    assert [l[0].split("<")[0] for l in p["launches"]] == ["zero_rows_kernel", "gemm_bf3_kernel", "bias_act_kernel"] and p["grid"][1] == 3
    p = _plan_of(hb, by(family="bf3_128", K=96, epi="acc", layout="NT", arith="bf16x6")[0])
    assert len(p["launches"]) == 1 and p["grid"][1] == 3
    for c in by(family="wide", K=1024):
        assert _plan_of(hb, c)["split_k"] > 1 and "rule_only" in c.name
    assert _plan_of(hb, by(family="bfk", M=1024, epi="bias", arith="bf16x3")[0])["plain"] == 1
    assert all(_plan_of(hb, c)["plain"] == 0 for c in by(family="bfk", M=1100))
    assert all(_plan_of(hb, c)["kt"] == (c.K != 64) for c in by(family="bfs"))
    assert all(_plan_of(hb, c)["behind"] == ["dropout"] for c in by(epi="drop"))
    # the misaligned cases plan the same kernel as the aligned ones; what differs is the load path inside it (MatView.vec)
    assert by(family="bf3_128", mis=True) and by(family="bf3_64", mis=True)
    assert set(c.batch for c in by(entry="batched")) == {2} and set(c.family for c in by(entry="batched")) == {"bf3_64", "wide", "bfs"}
