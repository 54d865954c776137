"""The launches asr_gemm_f32 / asr_gemm_drop_f32 cause, read from a rocprofv3 kernel trace: tests/golden/gemm_plan.json.gz
(gzip of a JSON text with one call per line: `zdiff` of two tables reads per call).

The table pins which kernel, grid and block every product of the case list takes; tests/test_gemm_plan_cpu.py holds
hip_backend.gemm_plan to it without a GPU.  It is written from a trace of the library as it stood BEFORE a change and
compared with a trace of the changed library; a policy change rewrites it on purpose.

    CFG=cfg2 GS_RECORD=CFG2.json python tools/gemm_shapes.py                # GPU: the asr_gemm_f32 calls of a step (and CFG=cfg5)
    python tools/gemm_plan_trace.py cases --steps cfg2=CFG2.json cfg5=CFG5.json --out CASES.json
    rocprofv3 --kernel-trace -M --output-format csv -d DIR -o t -- \
        python tools/gemm_plan_trace.py run --cases CASES.json --lib LIB.so --rc RC.json      # GPU, one process
    python tools/gemm_plan_trace.py table --cases CASES.json --rc RC.json --trace DIR --out TABLE.json
    python tools/gemm_plan_trace.py families [TABLE.json]                   # which kernel each step call takes (hb.gemm_plan)

`--cases` also takes a finished table (the golden file): run + table then reproduce it from another library.
A sentinel launch (colsum_kernel) separates the cases in the trace, so a zero pass in front of a product and a bias /
ReLU / dropout pass behind it are attributed to their call.  rocprofv3 reports grids in work-items; they are converted to
workgroups here, once."""
import argparse, collections, csv, ctypes, glob, gzip, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, ROOT + '/semi-supervised-asr_amd', ROOT + '/tests/golden', ROOT + '/tools']
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'gemm_plan.json.gz')
COLUMNS = ('ta', 'tb', 'M', 'N', 'K', 'lda', 'ldb', 'ldc', 'batch', 'sA', 'sB', 'sC', 'bias', 'relu', 'acc', 'split_k', 'arith', 'mis',
           'drop', 'src')
SENTINEL = 'colsum_kernel'
F32, X6, X3 = 0, 1, 2
NARROW, WIDE, SP, SMALL, ZEROED = 0x100, 0x200, 0x800, 0x1000, 0x2000
FLAGS = {'narrow': NARROW, 'wide': WIDE, 'sp': SP, 'small': SMALL, 'zeroed': ZEROED, 'f32': F32, 'bf16x6': X6, 'bf16x3': X3}
LAYOUTS = ((0, 1), (0, 0), (1, 0), (1, 1))


def code(mode):
    c = 0
    for part in mode.split('+'):
        c |= FLAGS[part]
    return c


def call(ta, tb, M, N, K, mode, src, lda=None, ldb=None, ldc=None, batch=1, sA=0, sB=0, sC=0, bias=0, relu=0, acc=0, split_k=0,
         mis=0, drop=0):
    return (int(ta), int(tb), M, N, K, lda or (M if ta else K), ldb or (K if tb else N), ldc or N, batch, sA, sB, sC, bias, relu,
            acc, split_k, code(mode), mis, drop, src)


def static_cases():
    """The calls of the GEMM tests of tests/test_hip_parity.py, the thresholds of the policy from both sides, and every
    kernel family by default and by flag under both bf16 arithmetics."""
    cs = []
    for ar in ('bf16x6', 'f32', 'bf16x3'):                                                     # test_gemm_variants
        for ta, tb in LAYOUTS:
            for M, N, K in ((128, 128, 32), (257, 130, 70), (33, 34, 9), (1000, 96, 513), (1, 1, 1), (7, 5, 3)):
                cs += [call(ta, tb, M, N, K, ar, 'variants'), call(ta, tb, M, N, K, ar, 'variants', bias=1, relu=1),
                       call(ta, tb, M, N, K, ar, 'variants', split_k=3), call(ta, tb, M, N, K, ar, 'variants', acc=1)]
        for ta, tb, M, N, K in ((0, 1, 25600, 4096, 80), (1, 0, 4096, 80, 25600), (0, 0, 6400, 512, 4096), (1, 0, 512, 2048, 12800)):
            cs.append(call(ta, tb, M, N, K, ar, 'step_shapes'))                                 # test_gemm_step_shapes
    for ta, tb, M, N, K in ((0, 1, 1024, 512, 4096), (1, 0, 512, 2048, 12800), (0, 0, 300, 200, 1030), (0, 1, 257, 130, 70)):
        cs.append(call(ta, tb, M, N, K, 'f32', 'fp32_equivalent', split_k=1))                   # test_gemm_bf16x6_is_fp32_equivalent
        for ar in ('bf16x6', 'bf16x3'):                                                        # (every flag under both arithmetics)
            cs.append(call(ta, tb, M, N, K, ar, 'fp32_equivalent'))
            cs.append(call(ta, tb, M, N, K, ar, 'fp32_equivalent', split_k=1))
            for f in ('+narrow', '+wide', '+sp', '+small'):
                cs.append(call(ta, tb, M, N, K, ar + f, 'fp32_equivalent', split_k=1))
                cs.append(call(ta, tb, M, N, K, ar + f, 'fp32_equivalent'))
    for ar in ('bf16x6', 'bf16x3'):
        for ta, tb in LAYOUTS:                                                                  # test_gemm_wide_tile
            for M, N, K in ((256, 128, 32), (256, 128, 64), (512, 256, 96), (256, 384, 4096), (1024, 128, 1024), (300, 80, 64),
                            (1000, 200, 512), (64, 64, 32), (4096, 80, 3200), (3232, 1152, 2048), (2560, 512, 80), (260, 132, 100)):
                for mode in (ar + '+wide', ar + '+sp', ar, ar + '+narrow', ar + '+small'):
                    cs += [call(ta, tb, M, N, K, mode, 'wide_tile'), call(ta, tb, M, N, K, mode, 'wide_tile', bias=1, relu=1),
                           call(ta, tb, M, N, K, mode, 'wide_tile', bias=1, relu=1, split_k=1),
                           call(ta, tb, M, N, K, mode, 'wide_tile', acc=1), call(ta, tb, M, N, K, mode, 'wide_tile', split_k=1)]
                for f in ('+wide', '+sp', '+small'):                                            # (views of wider buffers)
                    cs.append(call(ta, tb, M, N, K, ar + f, 'wide_tile', lda=(M if ta else K) + 64, ldc=N + 32))
        for M, N in ((1024, 128), (1100, 200), (3000, 4000), (2048, 130), (1025, 257), (12800, 512)):
            kw = dict(src='short_k')                                                            # test_gemm_short_k_weights_stationary
            cs += [call(0, 1, M, N, 80, ar, **kw), call(0, 1, M, N, 80, ar, bias=1, **kw), call(0, 1, M, N, 80, ar, bias=1, relu=1, **kw),
                   call(0, 1, M, N, 80, ar, acc=1, **kw), call(0, 1, M, N, 80, ar + '+narrow', bias=1, split_k=1, **kw),
                   call(0, 1, M, N, 80, ar, lda=96, ldb=88, ldc=N + 32, **kw)]
            if M <= 2048:
                cs.append(call(0, 1, M, N, 80, ar, batch=2, sA=M * 80, sB=N * 80, sC=M * N, **kw))
        for f in ('+wide', '+sp', '+narrow', '+small'):                                         # test_gemm_wide_tile_batched
            cs.append(call(1, 0, 40, 72, 2048, ar + f, 'wide_tile_batched', lda=120, ldb=216, ldc=72, batch=3, sA=40, sB=72, sC=2880))
        # ---- the thresholds of the policy, from both sides
        kw = dict(src='threshold')
        cs += [call(0, 1, 1024, 128, 80, ar, **kw), call(0, 1, 1100, 200, 80, ar, **kw),        # bfk plain / guarded / excluded
               call(0, 1, 1024, 128, 80, ar + '+narrow', **kw), call(0, 1, 1100, 200, 80, ar + '+narrow', **kw),
               call(0, 1, 1024, 128, 80, ar, split_k=3, **kw), call(0, 1, 1000, 128, 80, ar, **kw), call(0, 1, 1024, 120, 80, ar, **kw),
               call(0, 1, 4096, 2048, 640, ar, **kw), call(0, 1, 4096, 2048, 608, ar, **kw),   # bfs: 5120 / 4864 units
               call(1, 0, 1280, 1024, 1024, ar, **kw), call(1, 0, 1024, 1024, 1024, ar, **kw), # LDS-DMA kernel / 64 x 64 tiles
               call(1, 0, 1280, 1024, 992, ar, **kw), call(0, 1, 1280, 1024, 1024, ar, **kw),
               call(0, 1, 260, 132, 100, ar + '+sp', **kw), call(0, 1, 260, 132, 100, ar + '+sp', bias=1, **kw),   # masked K tail
               call(0, 1, 4096, 2048, 2052, ar, **kw)]                                          # (a long K with a tail pays)
        for z in ('', '+zeroed'):
            cs += [call(0, 1, 1368, 512, 2048, ar + z, bias=1, relu=1, acc=1, **kw),            # epilogue and accumulate: unsplit
                   call(0, 1, 1368, 512, 2048, ar + z, bias=1, relu=1, **kw),                   # split with a late epilogue
                   call(0, 1, 1368, 512, 2048, ar + z, **kw), call(0, 1, 1368, 512, 2048, ar + z, acc=1, **kw),
                   call(0, 1, 1000, 200, 4096, ar + z + '+narrow', bias=1, **kw), call(0, 1, 1000, 200, 4096, ar + z + '+narrow', **kw),
                   call(0, 1, 300, 200, 1030, ar + z, bias=1, split_k=3, **kw), call(0, 1, 300, 200, 1030, ar + z, split_k=3, **kw),
                   call(0, 1, 300, 200, 1030, ar + z, split_k=1, **kw)]
        cs += [call(0, 1, 300, 200, 1030, ar, bias=1, acc=1, split_k=3, **kw),                  # refused: ASR_E_SHAPE
               call(0, 1, 300, 200, 40, ar, bias=1, split_k=3, **kw),                           # split_k above the K tiles
               call(0, 1, 4096, 2048, 640, ar, mis=1, **kw), call(0, 1, 4096, 2048, 640, ar, mis=2, **kw),        # misaligned A / B
               call(0, 1, 4096, 2048, 640, ar, lda=642, **kw), call(1, 0, 1280, 1024, 1024, ar, ldb=1026, **kw),  # ld % 4 != 0
               call(0, 1, 1024, 128, 80, ar, lda=82, **kw), call(0, 1, 1024, 128, 80, ar, mis=2, **kw)]
        for M, N, K in ((1368, 512, 2048), (5472, 512, 2048), (96, 64, 64), (2736, 512, 512)):  # test_gemm_with_dropout_epilogue
            for sk in (0, 1):
                cs.append(call(0, 1, M, N, K, ar, 'dropout', bias=1, relu=1, split_k=sk, drop=1))
        cs.append(call(0, 1, 1024, 128, 80, ar, 'dropout', bias=1, drop=1))
    cs += [call(0, 1, 64, 48, 40, 'bf16x6', 'strided_batched', lda=100, ldc=80),               # test_gemm_strided_views_and_batched
           call(1, 0, 10, 12, 7, 'bf16x6', 'strided_batched', lda=30, ldb=36, ldc=12, batch=3, sA=10, sB=12, sC=120),
           call(0, 1, 4096, 2048, 640, 'f32', 'threshold'), call(1, 0, 1280, 1024, 1024, 'f32+wide', 'threshold'),
           call(0, 1, 1024, 128, 80, 'f32', 'threshold'), call(0, 1, 300, 200, 1030, 'f32', 'threshold', bias=1, split_k=3)]
    return cs


def merge(cases):
    """Identical calls once, in first-seen order, with every source that makes them."""
    seen = collections.OrderedDict()
    for c in cases:
        srcs = seen.setdefault(tuple(c[:-1]), [])
        if c[-1] not in srcs:
            srcs.append(c[-1])
    return [list(k) + [','.join(v)] for k, v in seen.items()]


def load(path):
    return json.load(gzip.open(path, 'rt') if path.endswith('.gz') else open(path))


def load_cases(path):
    d = load(path)
    assert tuple(d['columns'][:len(COLUMNS)]) == COLUMNS, d['columns']
    return [r[:len(COLUMNS)] for r in d['cases']]


def cmd_cases(args):
    cs = static_cases()
    for name, path in (s.split('=') for s in args.steps):              # (gemm_shapes.py records COLUMNS up to 'mis')
        cs += [tuple(c) + (0, name) for c in json.load(open(path))]
    cs = merge(cs)
    json.dump(dict(columns=COLUMNS, cases=cs), open(args.out, 'w'))
    print('%d cases' % len(cs))


def extent(rows, cols, ld, batch, stride):
    """-> (elements before the base pointer, elements from it) a strided batch of [rows][cols] matrices touches."""
    span = (rows - 1) * ld + cols
    back = (batch - 1) * -stride if stride < 0 else 0
    return back, span + ((batch - 1) * stride if stride > 0 else 0)


def cmd_run(args):
    import torch
    cases = load_cases(args.cases)
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    c_i, c_i64, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.asr_gemm_f32.argtypes = [c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_i, c_i, c_i64, c_i64, c_i64,
                                 c_i, c_i, c_p]
    lib.asr_gemm_drop_f32.argtypes = [c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_i, c_i,
                                      ctypes.c_uint64, ctypes.c_float, c_p]
    lib.asr_colsum_f32.argtypes = [c_i64, c_i64, c_p, c_i64, c_p, c_i, c_p]
    need = [0, 0, 0, 0]
    geo = []
    for ta, tb, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, bias, relu, acc, sk, ar, mis, drop, src in cases:
        ext = (extent(K if ta else M, M if ta else K, lda, batch, sA), extent(N if tb else K, K if tb else N, ldb, batch, sB),
               extent(M, N, ldc, batch, sC))
        assert (lda >= (M if ta else K) or (K if ta else M) == 1) and (ldb >= (K if tb else N) or (N if tb else K) == 1)
        assert (ldc >= N or M == 1) and batch * max(sk, 1) <= 65535
        geo.append([e[0] for e in ext])
        for i, e in enumerate(ext):
            need[i] = max(need[i], e[0] + e[1])
        need[3] = max(need[3], N)
    dev = torch.device('cuda')
    pools = [torch.zeros(n + 64, device=dev) for n in need]              # (+ 64: room for the one-element misalignment)
    assert all(p.data_ptr() % 16 == 0 for p in pools)
    torch.cuda.synchronize()
    sentinel = lambda: lib.asr_colsum_f32(1, 1, pools[3].data_ptr(), 1, pools[3].data_ptr() + 64, 1, None)
    rcs = []
    assert sentinel() == 0
    for c, back in zip(cases, geo):
        ta, tb, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, bias, relu, acc, sk, ar, mis, drop, src = c
        A, B, C = (pools[i].data_ptr() + 4 * (back[i] + ((mis >> i) & 1)) for i in range(3))
        bp = pools[3].data_ptr() if bias else None
        if drop:
            assert batch == 1 and not acc
            rc = lib.asr_gemm_drop_f32(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bp, relu, sk, ar, 4242, 0.3, None)
        else:
            rc = lib.asr_gemm_f32(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bp, relu, acc, batch, sA, sB, sC, sk, ar, None)
        rcs.append(rc)
        if rc > 0:                                                        # a HIP error: nothing more is launched
            break
        assert sentinel() == 0
    torch.cuda.synchronize()
    json.dump(rcs, open(args.rc, 'w'))
    print('%d of %d cases run, %d refused' % (len(rcs), len(cases), sum(1 for r in rcs if r < 0)))
    return 0 if len(rcs) == len(cases) and all(r <= 0 for r in rcs) else 1


def kernel_name(name):
    """rocprofv3's kernel name (mangled with -M, else demangled) -> the short form of tools/isa_guard.py."""
    if name.endswith('.kd'):
        name = name[:-3]
    m = re.match(r'_ZN12_GLOBAL__N_1(\d+)', name)
    if m:                                                                # (short_name is for templates: a plain kernel is its identifier)
        import isa_guard
        base = name[m.end():m.end() + int(m.group(1))]
        return isa_guard.short_name(name) if name[m.end() + len(base)] == 'I' else base
    name = re.sub(r'^void ', '', name).replace('(anonymous namespace)::', '')
    name = re.sub(r'\((?!.*>).*$', '', name)                             # the argument list behind the template arguments
    return name.replace(' ', '')


def read_trace(trace_dir):
    """-> [(kernel, [grid in workgroups], threads per workgroup)] in dispatch order."""
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r['Dispatch_Id']))
    out = []
    for r in rows:
        wg = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        grid = [int(r['Grid_Size_' + a]) for a in 'XYZ']
        assert all(g % w == 0 for g, w in zip(grid, wg)), r
        out.append((kernel_name(r['Kernel_Name']), [g // w for g, w in zip(grid, wg)], wg[0] * wg[1] * wg[2]))
    return out


def cmd_table(args):
    cases, rcs = load_cases(args.cases), json.load(open(args.rc))
    segs, cur = [], None
    for k in read_trace(args.trace):
        if k[0] == SENTINEL:
            cur = []
            segs.append(cur)
        elif cur is not None:                                            # (what ran before the first sentinel: the allocator's fills)
            cur.append(list(k))
    assert len(segs) == len(cases) + 1 and not segs[-1] and len(rcs) == len(cases), (len(segs), len(cases), len(rcs))
    raw = open(args.out, 'wb')
    with raw, (gzip.GzipFile(fileobj=raw, mode='wb', mtime=0) if args.out.endswith('.gz') else raw) as f:
        write = lambda t: f.write(t.encode())
        write('{"columns": %s,\n "cases": [\n' % json.dumps(list(COLUMNS) + ['rc', 'launches']))
        write(',\n'.join('  ' + json.dumps(c + [rc, seg], separators=(',', ':')) for c, rc, seg in zip(cases, rcs, segs)))
        write('\n ]}\n')
    print('%d cases, %d launches' % (len(cases), sum(len(s) for s in segs)))


def cmd_families(args):
    import hip_backend as hb
    d = load(args.table)
    col = {n: i for i, n in enumerate(d['columns'])}
    seen = set()
    for name in ('cfg2', 'cfg5'):
        agg = collections.OrderedDict()
        for r in d['cases']:
            if name in r[col['src']].split(','):
                kw = {k: r[col[k]] for k in ('lda', 'ldb', 'ldc', 'batch', 'sA', 'sB', 'sC', 'split_k', 'arith')}
                p = hb.gemm_plan(r[col['M']], r[col['N']], r[col['K']], bool(r[col['ta']]), bool(r[col['tb']]), bias=bool(r[col['bias']]),
                                 relu=bool(r[col['relu']]), accumulate=bool(r[col['acc']]), misaligned=r[col['mis']], **kw)
                agg.setdefault((p['kernel'], p['tile']), []).append('%s%s %dx%dx%d%s' % ('T' if r[col['ta']] else 'N', 'T' if r[col['tb']] else 'N',
                               r[col['M']], r[col['N']], r[col['K']], ' x%d' % r[col['batch']] if r[col['batch']] > 1 else ''))
        for (k, tile), shapes in agg.items():
            seen.add((k.split('<')[0], tile))
            print('%s  %-40s tile %-3d %s' % (name, k, tile, ', '.join(shapes)))
    print('selected by a step call:', sorted(seen))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('cases'); p.add_argument('--steps', nargs='*', default=[]); p.add_argument('--out', required=True)
    p = sub.add_parser('run'); p.add_argument('--cases', default=GOLDEN); p.add_argument('--lib', required=True); p.add_argument('--rc', required=True)
    p = sub.add_parser('table'); p.add_argument('--cases', default=GOLDEN); p.add_argument('--rc', required=True)
    p.add_argument('--trace', required=True); p.add_argument('--out', required=True)
    p = sub.add_parser('families'); p.add_argument('table', nargs='?', default=GOLDEN)
    a = ap.parse_args()
    sys.exit({'cases': cmd_cases, 'run': cmd_run, 'table': cmd_table, 'families': cmd_families}[a.cmd](a) or 0)
