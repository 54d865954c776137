"""Which kernel, grid and K split asr_gemm_f32 / asr_gemm_drop_f32 choose for a call, pinned without a GPU.

tests/golden/gemm_plan.json.gz (a gzipped JSON text, one call per line) lists calls and the launches each one caused on the GPU, in order (kernel in the short form of
tools/isa_guard.py, grid in workgroups, threads per workgroup), read from a rocprofv3 kernel trace by
tools/gemm_plan_trace.py.  hip_backend.gemm_plan - the library's own plan_gemm, which needs no device - must name the same
launches for every row.  A change of the kernel-selection policy rewrites the table on purpose."""
import json
import os
import sys
import ctypes
import gzip

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

F32, X6, X3 = 0, 1, 2
NARROW, WIDE, SP, SMALL, ZEROED = 0x100, 0x200, 0x800, 0x1000, 0x2000
TILE_FLAGS = NARROW | WIDE | SP | SMALL
E_SHAPE = -2


@pytest.fixture(scope="module")
def table():
    entry.build()
    d = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json.gz"), "rt"))
    names = d["columns"]
    return [dict(zip(names, row)) for row in d["cases"]]


def _plan(c):
    import hip_backend as hb
    return hb.gemm_plan(c["M"], c["N"], c["K"], bool(c["ta"]), bool(c["tb"]), lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"],
                        batch=c["batch"], sA=c["sA"], sB=c["sB"], sC=c["sC"], bias=bool(c["bias"]), relu=bool(c["relu"]),
                        accumulate=bool(c["acc"]), drop=bool(c["drop"]), split_k=c["split_k"], arith=c["arith"], misaligned=c["mis"])


def _product(c):
    """The product launch of a row: the one that is neither the zero pass nor the pass behind."""
    ks = [l for l in c["launches"] if l[0].startswith("gemm_")]
    assert len(ks) == 1, c
    return ks[0]


def _family(c):
    """-> bfk / bfs / wide / 128 / 64 / f32 of a row's product kernel."""
    k = _product(c)[0]
    if k.startswith("gemm_bf3_kernel"):
        return k[:-1].split(",")[3]
    return {"gemm_bfk": "bfk", "gemm_bfs": "bfs", "gemm_bf6w": "wide", "gemm_bf3w": "wide", "gemm_f32": "f32"}[k.split("_kernel")[0]]


def test_plan_reproduces_every_traced_launch(table):
    bad = []
    for c in table:
        p = _plan(c)
        got = [[k, list(g), b] for k, g, b in p["launches"]]
        if p["rc"] != c["rc"] or got != c["launches"]:
            bad.append((c, p["rc"], got))
    assert not bad, "%d of %d calls planned differently from the trace, first: %s" % (len(bad), len(table), bad[0])


def test_table_covers_the_step_calls_and_the_gemm_tests(table):
    srcs = set(s for c in table for s in c["src"].split(","))
    assert {"cfg2", "cfg5", "variants", "step_shapes", "fp32_equivalent", "wide_tile", "short_k", "wide_tile_batched",
            "strided_batched", "threshold", "dropout"} <= srcs
    n = lambda s: sum(1 for c in table if s in c["src"].split(","))
    assert n("cfg2") >= 10 and n("cfg5") >= 10
    # test_gemm_variants: 6 shapes x 4 layouts x 3 arithmetics x (plain, bias + relu, split_k = 3, accumulate)
    assert n("variants") == 6 * 4 * 3 * 4
    assert n("step_shapes") == 4 * 3
    # test_gemm_wide_tile: 12 shapes x 4 layouts x 2 arithmetics x (5 modes x 5 calls + 3 strided calls)
    assert n("wide_tile") == 12 * 4 * 2 * (5 * 5 + 3)
    # test_gemm_short_k_weights_stationary: 6 shapes x 2 arithmetics x 6 calls + the batched call of the four M <= 2048
    assert n("short_k") == 6 * 2 * 6 + 4 * 2
    assert n("wide_tile_batched") == 2 * 4 and n("strided_batched") == 2
    assert any(c["batch"] > 1 for c in table if "cfg2" in c["src"].split(","))


def test_every_family_by_default_and_by_flag_under_both_bf16_arithmetics(table):
    ok = [c for c in table if c["rc"] == 0]
    for ar in (X6, X3):
        default = set(_family(c) for c in ok if c["arith"] & ~ZEROED == ar)
        assert default == {"bfk", "bfs", "wide", "128", "64"}, (ar, default)
        for flag, fam in ((SP, "bfs"), (WIDE, "wide"), (NARROW, "128"), (SMALL, "64")):
            assert any(_family(c) == fam for c in ok if c["arith"] & (0xff | TILE_FLAGS) == ar | flag), (ar, fam)
        wide_name = "gemm_bf6w_kernel" if ar == X6 else "gemm_bf3w_kernel"
        assert any(_product(c)[0].startswith(wide_name) for c in ok if c["arith"] & 0xff == ar)
    assert set(_family(c) for c in ok if c["arith"] & 0xff == F32) == {"f32"}


def _row(table, ar, ta, tb, M, N, K, flags=0, **kw):
    want = dict(ta=ta, tb=tb, M=M, N=N, K=K, arith=ar | flags, bias=0, relu=0, acc=0, split_k=0, mis=0, drop=0, batch=1,
                lda=M if ta else K, ldb=K if tb else N, ldc=N)
    want.update(kw)
    rows = [c for c in table if all(c[k] == v for k, v in want.items())]
    assert len(rows) == 1, (want, len(rows))
    return rows[0]


@pytest.mark.parametrize("ar,nt", [(X6, 3), (X3, 2)])
def test_both_sides_of_each_threshold(table, ar, nt):
    row = lambda *a, **kw: _row(table, ar, *a, **kw)
    kernel = lambda *a, **kw: _product(row(*a, **kw))[0]
    kinds = lambda *a, **kw: [l[0].split("<")[0] for l in row(*a, **kw)["launches"]]
    wide = "gemm_bf6w_kernel" if nt == 3 else "gemm_bf3w_kernel"
    # K = 80, k-contiguous operands: the weights-stationary kernel, branch-free epilogue for interior shapes only
    assert kernel(0, 1, 1024, 128, 80) == "gemm_bfk_kernel<%d,5,true>" % nt
    assert kernel(0, 1, 1100, 200, 80) == "gemm_bfk_kernel<%d,5,false>" % nt
    for M, N, kw in ((1024, 128, dict(flags=NARROW)), (1100, 200, dict(flags=NARROW)), (1000, 128, {}), (1024, 120, {}),
                     (1024, 128, dict(split_k=3)), (1024, 128, dict(lda=82)), (1024, 128, dict(mis=2))):
        assert not kernel(0, 1, M, N, 80, **kw).startswith("gemm_bfk"), (M, N, kw)
    # 256 x 128 tiles x K tiles >= 5 000: one wave per SIMD; below, 128 x 128 tiles, unsplit
    assert kernel(0, 1, 4096, 2048, 640) == "gemm_bfs_kernel<true,true,%d,false>" % nt
    c = row(0, 1, 4096, 2048, 608)
    assert c["launches"] == [["gemm_bf3_kernel<true,true,%d,128,false>" % nt, [32 * 16, 1, 1], 256]]
    assert kernel(0, 1, 4096, 2048, 2052) == "gemm_bfs_kernel<true,true,%d,true>" % nt        # a long K with a tail pays
    # row-contiguous operands, K >= 1024: the LDS-DMA kernel with its own split; at most 256 large tiles after the split: 64 x 64
    c = row(1, 0, 1280, 1024, 1024)
    assert _product(c)[0] == wide + "<false,false>" and _product(c)[1][1] > 1 and c["launches"][0][0] == "zero_rows_kernel"
    assert kernel(1, 0, 1024, 1024, 1024) == "gemm_bf3_kernel<false,false,%d,64,false>" % nt
    # epilogue and accumulate: never split; a split product with an epilogue: zero pass, product, late epilogue
    for z in (0, ZEROED):
        c = row(0, 1, 1368, 512, 2048, flags=z, bias=1, relu=1, acc=1)
        assert len(c["launches"]) == 1 and c["launches"][0][1][1] == 1
        got = kinds(0, 1, 1368, 512, 2048, flags=z, bias=1, relu=1)
        assert got[-1] == "bias_act_kernel" and (got[0] == "zero_rows_kernel") == (z == 0) and len(got) == (3 if z == 0 else 2)
        got = kinds(0, 1, 300, 200, 1030, flags=z, bias=1, split_k=3)
        assert got[-1] == "bias_act_kernel" and (got[0] == "zero_rows_kernel") == (z == 0)
        assert _product(row(0, 1, 300, 200, 1030, flags=z, split_k=3))[1][1] == 3
        assert row(0, 1, 300, 200, 1030, flags=z, split_k=1)["launches"][0][1][1] == 1
        assert len(row(0, 1, 300, 200, 1030, flags=z, split_k=1)["launches"]) == 1
    assert row(0, 1, 300, 200, 1030, bias=1, acc=1, split_k=3)["rc"] == E_SHAPE
    # a masked K tail on the one-wave-per-SIMD kernel
    assert kernel(0, 1, 260, 132, 100, flags=SP) == "gemm_bfs_kernel<true,true,%d,true>" % nt
    # a misaligned pointer or ld % 4 != 0 falls off every wide path
    for kw in (dict(mis=1), dict(mis=2), dict(lda=642)):
        assert kernel(0, 1, 4096, 2048, 640, **kw).startswith("gemm_bf3_kernel"), kw
    assert kernel(1, 0, 1280, 1024, 1024, ldb=1026).startswith("gemm_bf3_kernel")


def _plan_child(rows):
    """In a child process: the plans of `rows` as JSON on stdout (the parent built the library)."""
    print(json.dumps([_plan(c) for c in rows]))


def test_the_plan_does_not_read_the_environment(table):
    """plan_gemm is a function of its arguments.  Three environment variables, read once per process (hence a fresh child),
    used to move its thresholds and force the wide kernels' K split; with all three set, one row each that lands on 64 x 64
    tiles, 128 x 128 tiles, the LDS-DMA kernel (split), the one-wave-per-SIMD kernel and the K = 80 kernel plans as the table has it."""
    import subprocess
    rows = [_row(table, X6, 1, 0, 1024, 1024, 1024), _row(table, X6, 0, 1, 4096, 2048, 608), _row(table, X6, 0, 1, 1368, 512, 2048),
            _row(table, X6, 0, 1, 4096, 2048, 640), _row(table, X6, 0, 1, 1024, 128, 80)]
    assert [_family(c) for c in rows] == ["64", "128", "wide", "bfs", "bfk"]
    assert _product(rows[2])[1][1] not in (1, 4)          # (a forced split of 4 would show)
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, ROOT, os.path.join(ROOT, "semi-supervised-asr_amd")]
    code = "import sys; sys.path[:0] = %r; import test_gemm_plan_cpu as t; t._plan_child(%r)" % (paths, rows)
    env = dict(os.environ, ASR_GEMM_SMALL_MAX="0", ASR_GEMM_SP_MIN="0", ASR_GEMM_WIDE_SK="4")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    plans = json.loads(r.stdout.strip().splitlines()[-1])
    for c, p in zip(rows, plans):
        assert p["rc"] == c["rc"] and [[k, list(g), b] for k, g, b in p["launches"]] == c["launches"], (c, p)


def test_f32_arithmetic_has_one_kernel(table):
    assert _product(_row(table, F32, 0, 1, 4096, 2048, 640))[0] == "gemm_f32_kernel<true,true>"
    assert _product(_row(table, F32, 1, 0, 1280, 1024, 1024, flags=WIDE))[0] == "gemm_f32_kernel<false,false>"
    assert _product(_row(table, F32, 0, 1, 1024, 128, 80))[0] == "gemm_f32_kernel<true,true>"


def test_the_flags_do_what_they_say(table):
    """The answer to "is it running the right kernel?" of test_gemm_bf16x6_is_fp32_equivalent and test_gemm_wide_tile: for each
    of their shapes +wide plans the LDS-DMA kernel where K % 32 == 0 and the shape conforms (operands of at least 64 rows
    and columns, row-contiguous ones in multiples of four), +sp the one-wave-per-SIMD kernel (also K % 4 == 0 above 32),
    +small 64 x 64 tiles, +narrow 128 x 128 tiles."""
    rows = [c for c in table if set(c["src"].split(",")) & {"wide_tile", "fp32_equivalent"} and c["arith"] & 0xff != F32]
    seen = set()
    for c in rows:
        fam, flag = _family(c), c["arith"] & TILE_FLAGS
        M, N, K, akc, bkc = c["M"], c["N"], c["K"], not c["ta"], bool(c["tb"])
        conforms = M >= 64 and N >= 64 and (akc or M % 4 == 0) and (bkc or N % 4 == 0)
        if flag == WIDE:
            assert (fam == "wide") == (conforms and K % 32 == 0), c
        elif flag == SP:
            assert (fam == "bfs") == (conforms and (K % 32 == 0 or (K % 4 == 0 and K > 32))), c
        elif flag == SMALL:
            assert fam == "64", c
        elif flag == NARROW:
            assert fam == "128", c
        seen.add((flag, fam))
    assert {(WIDE, "wide"), (SP, "bfs"), (SMALL, "64"), (NARROW, "128")} <= seen
    shapes = set((c["M"], c["N"], c["K"]) for c in rows)
    assert len(shapes) == 12 + 4


def test_grid_y_above_65535_is_refused():
    entry.build()
    import hip_backend as hb
    assert hb.gemm_plan(64, 64, 64, batch=65535, sA=4096, sB=4096, sC=4096, split_k=1)["rc"] == 0
    assert hb.gemm_plan(64, 64, 64, batch=65536, sA=4096, sB=4096, sC=4096, split_k=1)["rc"] == E_SHAPE
    assert hb.gemm_plan(64, 64, 64, batch=70000, sA=4096, sB=4096, sC=4096)["rc"] == E_SHAPE
    assert hb.gemm_plan(64, 64, 4096, batch=30000, sA=4096, sB=4096, sC=4096, split_k=3, arith="bf16x6+narrow")["rc"] == E_SHAPE
    assert hb.gemm_plan(1024, 128, 80, trans_b=True, batch=70000, sA=1024 * 80, sB=128 * 80, sC=1024 * 128)["rc"] == E_SHAPE
    # the side entry returns before any launch: the pointers are never read
    lib = hb.load()
    fake = ctypes.c_void_p(1 << 20)
    side = lambda batch, M, N, mask: lib.asr_gemm_side_f32(0, 1, M, N, 64, fake, 64, fake, 64, fake, N, batch, 4096, 4096, 4096,
                                                           hb.ARITH_BF16X6, mask, fake, None)
    assert side(70000, 64, 64, 0xff) == E_SHAPE
    # 10 000 tiles x 60 000: 6e8 tickets (allowed), but on one XCD the masked launch is 80 008 x 60 000 workgroups > 2^32
    assert side(60000, 6400, 6400, 0x01) == E_SHAPE
