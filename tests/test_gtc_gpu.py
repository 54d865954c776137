"""The graph CTC loss on the GPU (csrc/gtc.hip) against its torch restatement (tests/gtc_ref.py) in float64, the
identities with ops.ctc_loss, then E2E.gtc_nll and the Solver's pseudo-label step.

Tolerance of the kernel cases: none is written down here.  Every case also runs the restatement in float32 on the same
inputs; per element the kernel's error against float64 may be at most 4 x the float32 restatement's worst error (another
summation order inside the log-sum-exps, no more), with a floor of 8 fp32 ulps of the tensor's largest magnitude where the
float32 error is about zero - test_ctc_gpu's rule.  Each case prints a `gtc_parity` line with its two ratios
(profiles/gtc_parity.txt holds one run).

The dispatch boundaries are the header's (include/asr_hip.h, "Graph CTC", max_nodes): one wave per utterance up to 64 nodes,
a node per thread up to 256, nodes strided over 256 threads beyond.  Every group holds the small rows (T' = 1, one node, tries
with K in {1, 2, 8}, a sausage with skips, random sparse graphs with arc weights in [-3, 0], an unreachable node, one token on
every node, no blank at all, two rows sharing a graph) and its own node counts: 64 | 65, 256 and an in-degree of 79 | 257
and 600 (a thread strides three times).  Exactly one row per case has no path: a lattice with too few frames (V = 5, 34,
257) or a row with 0 frames (V = 2, 65)."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import gtc_ref as R
import poison as P
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")

VOCABS = (2, 5, 34, 65, 257)
GROUPS = ("wave", "block", "strided")
SCALES = (1.0, 8.0)


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _random_graph(rs, N, V, no_blank=False, one_token=None, hub=False):
    """A sparse graph: a chain 0 -> 1 -> .. with a self-loop on most nodes and two random arcs out of every node, weights in
    [-3, 0]; node N // 2 (N >= 4) has no arc into it and no start weight - unreachable, though arcs leave it; with hub every
    node has an arc into node 1 (an in-degree of N - 1)."""
    import gtc
    lo = 1 if no_blank else 0
    lab = [int(one_token)] * N if one_token is not None else [int(v) for v in rs.randint(lo, V, size=N)]
    dead = N // 2 if N >= 4 else -1
    arcs = {}
    for n in range(N):
        if n == 0 or rs.uniform() < 0.7:
            arcs[(n, n)] = 0
        nxt = n + 2 if n + 1 == dead else n + 1
        if nxt < N:
            arcs[(n, nxt)] = 0
        for m in rs.randint(0, N, size=2):
            arcs[(n, int(m))] = 0
        if hub:
            arcs[(n, 1)] = 0
    rows = [(m, n, float(rs.uniform(-3, 0))) for (m, n) in sorted(arcs) if n != dead]
    rs.shuffle(rows)
    start = [float(rs.uniform(-1, 0)) if n < 3 and n != dead else -INF for n in range(N)]
    fin = [float(rs.uniform(-1, 0)) if (n % 2 == 0 or n == N - 1) else -INF for n in range(N)]
    return gtc.Graph(V, lab, start, fin, rows)


def _labels(rs, V, n):
    return [int(v) for v in rs.randint(1, V, size=n)]


def _need(labels):
    """labels + adjacent equal labels: the frames the shortest CTC path takes"""
    return len(labels) + sum(1 for x, y in zip(labels, labels[1:]) if x == y)


def _lattice(rs, V, L):
    """(frames, the CTC lattice) of L random labels, three frames above what the shortest path takes"""
    import gtc
    y = _labels(rs, V, L)
    return _need(y) + 3, gtc.Graph.ctc(y, V)


def _rows(V, group, seed):
    """(frames, graph) per row; row 5 is the infeasible one."""
    import gtc
    rs = np.random.RandomState(seed)
    a = int(rs.randint(1, V))
    b = a % (V - 1) + 1 if V > 2 else a
    shared = _random_graph(rs, 9, V)
    hyps8 = [[a], [a, b], [a, b, a], [b], [b, a], [a, a], [], [a, b, b]]
    sausage = [[(a, -0.2), (b, -1.1)], [(None, -0.4), (b, -0.9)], [(a, -0.3), (None, -1.5)], [(b, -0.1), (a, -2.0)]]
    if V in (2, 65):
        bad = (0, gtc.Graph.ctc([a], V))                                   # no frame: no path, whatever the graph
    else:
        bad = (3, gtc.Graph.ctc([a, a, b], V))                             # 3 labels + 1 repeat need 4 frames
    rows = [(1, gtc.Graph(V, [0], [0.0], [0.0], [(0, 0, 0.0)])),           # one node, T' = 1
            (1, gtc.Graph.ctc([a], V)),
            (7, shared),
            (6, gtc.Graph.from_nbest([[a, b]], [-0.5], V)),                # K = 1
            (5, gtc.Graph.from_nbest([[a, b], [a]], [-0.3, -1.4], V)),     # K = 2, a shared prefix
            bad,
            (9, gtc.Graph.from_nbest(hyps8, [float(w) for w in rs.uniform(-3, 0, size=8)], V)),   # K = 8
            (8, gtc.Graph.from_confusion(sausage, V)),
            (11, shared),                                                  # two rows, one graph
            (13, _random_graph(rs, 13, V, one_token=a)),                   # the longest run of the sorted node list
            (6, _random_graph(rs, 17, V, no_blank=True)),
            _lattice(rs, V, 2)]
    if group == "wave":
        rows.append((5, _random_graph(rs, 64, V)))
    elif group == "block":
        rows += [_lattice(rs, V, 32),                                      # 65 nodes
                 (5, _random_graph(rs, 256, V)),
                 (4, _random_graph(rs, 80, V, hub=True))]                  # an in-degree of 79
    else:
        rows += [_lattice(rs, V, 128),                                     # 257 nodes
                 (6, _random_graph(rs, 600, V)),                           # a thread owns three nodes
                 (4, _random_graph(rs, 80, V, hub=True))]
    return rows


_CASES = {}


def _reference(z, lens, graphs, g):
    out = {}
    for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
        zz = z.to(dt).clone().requires_grad_()
        nll, _ = R.gtc_nll(zz, lens, graphs, zero_infinity=True)
        (nll * g.to(dt)).sum().backward()
        out[name] = (nll.detach().double(), zz.grad.double())
    return out


def _case(V, group, scale, extra=0):
    """Inputs and the CPU results (float64 checker, float32 yardstick) of one case, computed once and left unchanged.
    extra: frames behind the longest row."""
    key = (V, group, scale, extra)
    if key in _CASES:
        return _CASES[key]
    rows = _rows(V, group, 100 + V)
    rs = np.random.RandomState(7 * V + len(group))
    B, T = len(rows), max(t for t, _ in rows)
    z = torch.from_numpy((scale * rs.normal(0, 1, size=(B, T, V))).astype(np.float32))
    if extra:
        z, T = torch.cat([z, torch.zeros(B, extra, V)], 1), T + extra
    lens = [t for t, _ in rows]
    for i, t in enumerate(lens):
        z[i, t:] = 0.0
    graphs = [g for _, g in rows]
    g = torch.from_numpy(rs.uniform(-2, 2, size=B).astype(np.float32))
    g[1], g[-1] = 0.0, 1.0
    out = dict(z=z, lens=lens, graphs=graphs, g=g, B=B, T=T, V=V)
    out.update(_reference(z, lens, graphs, g))
    _, out["feasible"] = R.gtc_nll(z.double(), lens, graphs, zero_infinity=False)
    # exactly one row is infeasible, under the reference alone, before the GPU runs
    assert int((~out["feasible"]).sum()) == 1 and not bool(out["feasible"][5])
    assert bool(torch.isfinite(out["ref"][0]).all()) and bool(torch.isfinite(out["ref"][1]).all())
    assert float(out["ref"][0][5]) == 0.0 and bool((out["ref"][1][5] == 0).all())
    _CASES[key] = out
    return out


def _batch(c, rows):
    """The rows' graphs as one GraphBatch: a graph object that several rows name appears once in the table."""
    import gtc
    uniq, index = [], []
    for i in rows:
        g = c["graphs"][i]
        at = [k for k, u in enumerate(uniq) if u is g]
        if not at:
            uniq.append(g)
            at = [len(uniq) - 1]
        index.append(at[0])
    return gtc.GraphBatch(uniq, index)


def _run(hb, c, zero_infinity=True, rows=None, extra_cols=3):
    """ops.gtc_loss on the case (or on its `rows`, in that order): the logits are a [B, T, V] view of a [B, T, V + 3] buffer
    (ld = V + 3) whose padding - the frames behind every length and the three extra columns - is NaN."""
    import ops
    rows = list(range(c["B"])) if rows is None else list(rows)
    T, V = c["T"], c["V"]
    buf = torch.full((len(rows), T, V + extra_cols), float("nan"))
    for r, i in enumerate(rows):
        buf[r, :c["lens"][i], :V] = c["z"][i, :c["lens"][i]]
    buf = buf.to(DEV).requires_grad_()
    nll = ops.gtc_loss(buf[:, :, :V], hb.to_device_i32([c["lens"][i] for i in rows], DEV), _batch(c, rows), zero_infinity)
    nll.backward(c["g"][rows].to(DEV))
    return nll.detach().cpu(), buf.grad.cpu()


def _allowance(f32, ref, other32=0.0):
    err32 = max(float((f32 - ref).abs().max()), other32)
    floor = 8.0 * float(np.spacing(np.float32(ref.abs().max())))
    return max(4.0 * err32, floor), err32


def _check(c, nll, grad, rows, what, ref=None, other32=(0.0, 0.0)):
    V = c["V"]
    for i, t in enumerate(c["lens"]):
        assert bool((grad[i, t:] == 0).all()), "%s: row %d has a gradient behind its %d frames" % (what, i, t)
    assert bool((grad[:, :, V:] == 0).all())
    assert bool(torch.isfinite(nll[rows]).all()) and bool(torch.isfinite(grad[rows]).all()), what
    ref_n, ref_g = c["ref"] if ref is None else ref
    f32_n, f32_g = c["f32"]
    allow_n, e32n = _allowance(f32_n[rows], c["ref"][0][rows], other32[0])
    allow_g, e32g = _allowance(f32_g[rows], c["ref"][1][rows], other32[1])
    err_n = float((nll[rows].double() - ref_n[rows]).abs().max())
    err_g = float((grad[rows][:, :, :V].double() - ref_g[rows]).abs().max())
    print("gtc_parity %s: nll err %.3g (f32 cpu %.3g, allowed %.3g, ratio %.3f)  grad err %.3g (f32 cpu %.3g, allowed "
          "%.3g, ratio %.3f)  max|nll| %.4g" % (what, err_n, e32n, allow_n, err_n / allow_n, err_g, e32g, allow_g,
                                                err_g / allow_g, float(c["ref"][0][rows].abs().max())))
    assert err_n <= allow_n, "%s: nll error %.3g above %.3g" % (what, err_n, allow_n)
    assert err_g <= allow_g, "%s: gradient error %.3g above %.3g" % (what, err_g, allow_g)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("V", VOCABS)
def test_kernel_against_float64(hb, V, group, scale):
    """Every row of every case, no element left out: nll and gradient per element within the allowance; the infeasible row
    has loss 0 and gradient 0 under zero_infinity; ld = V + 3; NaN behind every length and in the padding columns; upstream
    gradients of both signs and an exact 0."""
    c = _case(V, group, scale)
    nll, grad = _run(hb, c)
    bad = int((~c["feasible"]).nonzero()[0])
    assert float(nll[bad]) == 0.0 and bool((grad[bad] == 0).all())
    _check(c, nll, grad, torch.arange(c["B"]), "V=%d %s x%g" % (V, group, scale))


@pytest.mark.parametrize("V,group", [(34, "block"), (2, "wave"), (65, "strided")])
def test_infeasible_without_zero_infinity(hb, V, group):
    """zero_infinity off: +inf for the row without a path (too few frames at V = 34, no frame at V = 2 and 65), a zero
    gradient for it all the same, every other row as before."""
    c = _case(V, group, 1.0)
    nll, grad = _run(hb, c, zero_infinity=False)
    bad = ~c["feasible"]
    assert bool(torch.isinf(nll[bad]).all()) and bool((nll[bad] > 0).all()) and bool((grad[bad] == 0).all())
    _check(c, nll, grad, c["feasible"].nonzero().flatten(), "V=%d %s, zero_infinity off" % (V, group))


@pytest.mark.parametrize("group", GROUPS)
def test_time_axis_past_every_row(hb, group):
    """T = max(t) + 5: the same allowance, zeros behind every length, and the bits of the run at T = max(t)."""
    c, short = _case(34, group, 1.0, extra=5), _case(34, group, 1.0)
    assert c["T"] == short["T"] + 5 and torch.equal(c["z"][:, :short["T"]], short["z"])
    nll, grad = _run(hb, c)
    assert grad.shape[1] == c["T"]
    _check(c, nll, grad, torch.arange(c["B"]), "V=34 %s T+5" % group)
    nll0, grad0 = _run(hb, short)
    assert torch.equal(nll, nll0), "nll differs from the run at T = max(t)"
    assert torch.equal(grad[:, :short["T"]], grad0), "the gradient differs from the run at T = max(t)"
    assert bool((grad[:, short["T"]:] == 0).all())


# ------------------------------------------------------------------------------------------------ identities
def _ctc_case(V, lens_labels, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    B, T = len(lens_labels), max(t for t, _ in lens_labels)
    z = torch.from_numpy((scale * rs.normal(0, 1, size=(B, T, V))).astype(np.float32))
    lens = [t for t, _ in lens_labels]
    for i, t in enumerate(lens):
        z[i, t:] = 0.0
    g = torch.from_numpy(rs.uniform(-2, 2, size=B).astype(np.float32))
    g[0] = 0.0
    return z, lens, [y for _, y in lens_labels], g


def _gpu_ctc(hb, z, lens, labels, g=None):
    """ops.ctc_loss on the rows -> (nll, gradient) on the host, or nll [B] on the device with autograd when g is None"""
    import ops
    zz = z.to(DEV).requires_grad_()
    ys = torch.tensor([v for y in labels for v in y], dtype=torch.long, device=DEV)
    nll = ops.ctc_loss(zz, hb.to_device_i32(lens, DEV), ys, [len(y) for y in labels], True)
    if g is None:
        return nll, zz
    nll.backward(g.to(DEV))
    return nll.detach().cpu(), zz.grad.cpu()


@pytest.mark.parametrize("group", GROUPS)
def test_ctc_lattices_are_the_ctc_loss(hb, group):
    """Graph.ctc against ops.ctc_loss on the same rows (one of them infeasible, one without labels), by the rule of the kernel
    cases.  Two kernels are compared, each with a float32 yardstick of its own - the restatement here, torch's float32 CPU
    ctc_loss for ops.ctc_loss (test_ctc_gpu) - and "the float32 reference's own error" is the larger of the two, as in
    test_ctc_star_gpu.test_closed_rows_are_the_ctc_loss.  No bits are promised."""
    import gtc
    import ops
    import torch.nn.functional as F
    V = 34
    rs = np.random.RandomState(5)
    top = dict(wave=31, block=127, strided=140)[group]
    long = _labels(rs, V, top)
    lens_labels = [(1, []), (9, _labels(rs, V, 4)), (3, [7, 7, 7]), (12, [3, 3, 4, 4]), (_need(long) + 2, long),
                   (20, _labels(rs, V, 7))]
    z, lens, labels, g = _ctc_case(V, lens_labels, 17)
    graphs = [gtc.Graph.ctc(y, V) for y in labels]
    want_n, want_g = _gpu_ctc(hb, z, lens, labels, g)
    zz = z.to(DEV).requires_grad_()
    nll = ops.gtc_loss(zz, hb.to_device_i32(lens, DEV), gtc.GraphBatch(graphs, range(len(graphs))), True)
    nll.backward(g.to(DEV))
    assert float(nll.detach()[2]) == 0.0 and float(want_n[2]) == 0.0
    yard = []
    ys = torch.tensor([v for y in labels for v in y], dtype=torch.long)
    for dt in (torch.float64, torch.float32):
        zc = z.to(dt).clone().requires_grad_()
        t_nll = F.ctc_loss(F.log_softmax(zc, -1).transpose(0, 1), ys, torch.tensor(lens), torch.tensor([len(y) for y in labels]),
                           blank=0, reduction="none", zero_infinity=True)
        (t_nll * g.to(dt)).sum().backward()
        yard.append((t_nll.detach().double(), zc.grad.double()))
    other32 = tuple(float((yard[1][k] - yard[0][k]).abs().max()) for k in (0, 1))
    c = dict(V=V, lens=lens, B=len(lens), T=z.shape[1])
    c.update(_reference(z, lens, graphs, g))
    _check(c, nll.detach().cpu(), zz.grad.cpu(), torch.arange(len(lens)), "V=34 %s Graph.ctc vs ops.ctc_loss" % group,
           ref=(want_n.double(), want_g.double()), other32=other32)


@pytest.mark.parametrize("K", [1, 2, 8])
def test_nbest_tries_are_the_composition_of_ctc_losses(hb, K):
    """from_nbest against -logsumexp_k (log w_k - nll_k) composed from K ops.ctc_loss calls with autograd, value and gradient,
    by the rule of the kernel cases.  Two float32 kernels are compared there, each with a yardstick of its own - the
    restatement on the trie, and the same composition from torch's float32 CPU ctc_loss - and "the float32 reference's own
    error" is the larger of the two, as in test_ctc_lattices_are_the_ctc_loss; then the trie alone against float64."""
    import gtc
    import ops
    import torch.nn.functional as F
    V, B, T = 34, 4, 14
    rs = np.random.RandomState(40 + K)
    lists = []
    for b in range(B):
        stem = _labels(rs, V, 3)
        hyps = [stem[:int(rs.randint(0, 4))] + _labels(rs, V, int(rs.randint(0, 4))) for _ in range(K)]
        if K == 8:
            hyps[3], hyps[5] = list(hyps[0]), []                          # a duplicate and the empty hypothesis
        lists.append((hyps, [float(w) for w in rs.uniform(-3, 0, size=K)]))
    z, lens, _, g = _ctc_case(V, [(T - b, []) for b in range(B)], 50 + K)
    graphs = [gtc.Graph.from_nbest(h, w, V) for h, w in lists]
    zz = z.to(DEV).requires_grad_()
    nll = ops.gtc_loss(zz, hb.to_device_i32(lens, DEV), gtc.GraphBatch(graphs, range(B)), True)
    nll.backward(g.to(DEV))
    zc = z.to(DEV).requires_grad_()
    lens_dev = hb.to_device_i32(lens, DEV)
    terms = []
    for k in range(K):
        ys = torch.tensor([v for h, _ in lists for v in h[k]], dtype=torch.long, device=DEV)
        nk = ops.ctc_loss(zc, lens_dev, ys, [len(h[k]) for h, _ in lists], False)
        terms.append(torch.tensor([w[k] for _, w in lists], device=DEV) - nk)
    want = -torch.logsumexp(torch.stack(terms, 1), 1)
    want.backward(g.to(DEV))
    # the composition's own float32 yardstick: the same composition from torch's CPU ctc_loss, float32 against float64
    yard = []
    for dt in (torch.float64, torch.float32):
        zt = z.to(dt).clone().requires_grad_()
        x = F.log_softmax(zt, -1).transpose(0, 1)
        tk = []
        for k in range(K):
            ys = torch.tensor([v for h, _ in lists for v in h[k]], dtype=torch.long)
            nk = F.ctc_loss(x, ys, torch.tensor(lens), torch.tensor([len(h[k]) for h, _ in lists]), blank=0, reduction="none")
            tk.append(torch.tensor([w[k] for _, w in lists], dtype=dt) - nk)
        comp = -torch.logsumexp(torch.stack(tk, 1), 1)
        (comp * g.to(dt)).sum().backward()
        yard.append((comp.detach().double(), zt.grad.double()))
    other32 = tuple(float((yard[1][k] - yard[0][k]).abs().max()) for k in (0, 1))
    c = dict(V=V, lens=lens, B=B, T=z.shape[1])
    c.update(_reference(z, lens, graphs, g))
    _check(c, nll.detach().cpu(), zz.grad.cpu(), torch.arange(B), "V=34 K=%d from_nbest vs %d ops.ctc_loss" % (K, K),
           ref=(want.detach().cpu().double(), zc.grad.cpu().double()), other32=other32)
    _check(c, nll.detach().cpu(), zz.grad.cpu(), torch.arange(B), "V=34 K=%d from_nbest" % K)


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("det", [False, True])
def test_bit_reproducible(hb, det):
    c = _case(257, "strided", 1.0)
    with hb.deterministic(det):
        first, second = _run(hb, c), _run(hb, c)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1]) and not bool(torch.isnan(first[1]).any())


def test_batch_invariance(hb):
    """A row's nll and gradient have the same bits alone (its own max_nodes: another kernel for most rows), at another batch
    position (reversed order), and - the rows of the one-wave group - beside rows with larger graphs."""
    c = _case(34, "strided", 1.0)
    B = c["B"]
    nll, grad = _run(hb, c)
    rev = list(range(B))[::-1]
    nll_r, grad_r = _run(hb, c, rows=rev)
    for r, i in enumerate(rev):
        assert torch.equal(nll_r[r], nll[i]) and torch.equal(grad_r[r], grad[i]), "moved: row %d" % i
    for i in range(B):
        n1, g1 = _run(hb, c, rows=[i])
        assert torch.equal(n1[0], nll[i]) and torch.equal(g1[0], grad[i]), "alone: row %d" % i
    small = [i for i in range(B) if c["graphs"][i].N <= 64]
    assert len(small) >= 10 and max(c["graphs"][i].N for i in range(B)) > 512
    n2, g2 = _run(hb, c, rows=small)                                       # the one-wave kernel
    for r, i in enumerate(small):
        assert torch.equal(n2[r], nll[i]) and torch.equal(g2[r], grad[i]), "beside larger graphs: row %d" % i
    print("gtc_parity batch invariance V=34 strided: %d rows alone, moved, beside larger graphs: bit-identical" % B)


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_outputs_and_workspace(hb, pattern):
    """torch.empty & co (nll, dlogits, a fresh workspace) filled with the pattern, then the pooled workspace a LARGER call
    left behind poisoned where it lay: the bits of the clean run."""
    import ops
    c, big = _case(34, "block", 1.0), _case(34, "strided", 1.0)
    P.empty_pool()
    want = _run(hb, c)
    try:
        for variant in ("fresh", "leftover"):
            st = P.Stats()
            P.empty_pool()
            if variant == "leftover":
                _run(hb, big)
                assert any(k[0] == "gtc" and v for k, v in ops._POOL.free.items())
                assert P.poison_pool(pattern, st) > 0
            with P.poisoned(pattern, st):
                got = _run(hb, c)
            assert st.total > 0
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (variant, pattern)
    finally:
        P.empty_pool()


def test_backward_twice_raises(hb):
    import ops
    c = _case(5, "wave", 1.0)
    z = c["z"].to(DEV).requires_grad_()
    nll = ops.gtc_loss(z, hb.to_device_i32(c["lens"], DEV), _batch(c, range(c["B"])), True)
    nll.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        nll.sum().backward()


def test_refused_shapes(hb):
    import gtc
    import ops
    with pytest.raises(hb.UnsupportedShape):
        hb.gtc_ws_bytes(1, 4, 5, hb.GTC_MAX_NODES + 1)
    with pytest.raises(hb.UnsupportedShape):
        hb.gtc_ws_bytes(1, 4, 1, 3)
    z = torch.zeros(2, 4, 5, device=DEV)
    two = hb.to_device_i32([4, 4], DEV)
    g = gtc.Graph.ctc([1, 2], 5)
    with pytest.raises(ValueError):
        ops.gtc_loss(z, two, gtc.Graph.ctc([1], 6))                         # another vocabulary
    with pytest.raises(ValueError):
        ops.gtc_loss(z, two, gtc.GraphBatch([g], [0]))                      # one row listed, two in the call
    with pytest.raises(ValueError):
        ops.gtc_loss(z, two, [g, g])
    # the workspace: 4-byte aligned and at least gtc_ws_bytes, checked before anything is launched
    need = hb.gtc_ws_bytes(2, 4, 5, g.N)
    raw = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    nll, dz, up = torch.zeros(2, device=DEV), torch.zeros(2, 4, 5, device=DEV), torch.ones(2, device=DEV)
    table = g.to(DEV)
    before = dict(hb.LAUNCHES)
    for ws, nbytes in ((raw[1:], need), (raw[:need], need - 4)):
        with pytest.raises(RuntimeError):
            hb.gtc_loss_fwd(z, 5, two, table, True, nll, ws, ws_bytes=nbytes)
        with pytest.raises(RuntimeError):
            hb.gtc_loss_bwd(z, 5, two, table, True, up, ws, dz, 5, ws_bytes=nbytes)
    assert dict(hb.LAUNCHES) == before
    hb.gtc_loss_fwd(z, 5, two, table, True, nll, raw[:need])
    assert bool(torch.isfinite(nll).all())


# ------------------------------------------------------------------------------------------------ the model
TINY_ILENS = [23, 17, 12]                            # 6, 5 and 3 encoder frames


def _tiny(seed=21, **kw):
    import model as M
    torch.manual_seed(seed)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw).to(DEV)
    weights = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    res = net.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys and all(k.startswith("ctc_lo.") for k in res.missing_keys)
    net.train()
    xs, ilens, _ = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], TINY_ILENS, [4, 3, 2], 13)
    return net, torch.from_numpy(xs).to(DEV), ilens


def test_gradient_into_the_head_and_the_encoder(hb):
    """E2E.gtc_nll: d enc_h, d ctc_lo.weight, d ctc_lo.bias of the mean against the float64 restatement applied to the model's
    own enc_h, 1e-3 of each tensor's max (the head's fp32 product against float64); and through the encoder itself
    the gradient reaches its first layer.  Without the head: ValueError."""
    import gtc
    net, xs, ilens = _tiny(ctc_weight=0.3)
    V = synth.TINY["output_dim"]
    graphs = [gtc.Graph.from_nbest([[3, 4], [3], [5, 4]], [-0.4, -1.5, -2.0], V), gtc.Graph.ctc([6, 6], V),
              gtc.Graph.from_confusion([[(3, -0.1), (4, -2.0)], [(None, -0.7), (5, -0.6)]], V)]
    batch = gtc.GraphBatch(graphs, range(3))
    enc_h, _ = net.encoder(xs, ilens)
    e = enc_h.detach().clone().requires_grad_()
    net.zero_grad()
    (net.gtc_nll(e, batch).sum() / 3).backward()
    lens = net.encoder.enc2.last_lens_dev.cpu().tolist()
    e64 = enc_h.detach().double().cpu().requires_grad_()
    w64 = net.ctc_lo.weight.detach().double().cpu().requires_grad_()
    b64 = net.ctc_lo.bias.detach().double().cpu().requires_grad_()
    ref, feasible = R.gtc_nll(e64 @ w64.t() + b64, lens, graphs)
    assert bool(feasible.all())
    (ref.sum() / 3).backward()
    for name, got, want in (("enc_h", e.grad, e64.grad), ("ctc_lo.weight", net.ctc_lo.weight.grad, w64.grad),
                            ("ctc_lo.bias", net.ctc_lo.bias.grad, b64.grad)):
        err, top = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        print("gtc head %s: err %.3g of max %.3g" % (name, err, top))
        assert top > 0 and err <= 1e-3 * top, name
    net.zero_grad()
    enc_h, _ = net.encoder(xs, ilens)
    net.gtc_nll(enc_h, batch).sum().backward()
    first = next(p for n, p in net.named_parameters() if n.startswith("encoder."))
    assert first.grad is not None and float(first.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        plain = _tiny()[0]
        plain.gtc_nll(enc_h.detach(), batch)


def _solver(root, monkeypatch, **over):
    """The tiny Solver of tests/test_ctc_gpu.py with seeded weights; the CTC head from a seeded torch generator."""
    import yaml
    from dataset import synthetic_utterances
    from solver import Solver
    t, l = synth.TINY, synth.TINY_LM
    nv = t["output_dim"]
    vocab = {s: i for i, s in enumerate(["<PAD>", "<BOS>", "<EOS>"] + ["s%d" % i for i in range(nv - 5)] + ["<space>", "<NOISE>"])}
    os.makedirs(root, exist_ok=True)
    for name, n, seed in (("train", 12, 1), ("dev", 4, 2)):
        with open(os.path.join(root, name + ".pkl"), "wb") as f:
            pickle.dump(synthetic_utterances(n, t["input_dim"], nv, 24, seed), f)
    with open(os.path.join(root, "vocab_dict.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(root, "non_lang_syms.pkl"), "wb") as f:
        pickle.dump(["<NOISE>", "<PAD>", "<BOS>", "<EOS>"], f)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "semi-supervised-asr_amd", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(logdir=os.path.join(root, "log"), model_dir=root, model_name="m", load_model_path=os.path.join(root, "m"),
               load_judge_path=os.path.join(root, "m"), dataset_root_dir=root, vocab_path=os.path.join(root, "vocab_dict.pkl"),
               non_lang_syms_path=os.path.join(root, "non_lang_syms.pkl"), labeled_set="train", unlabeled_speech_set="train",
               unlabeled_text_set="train", dev_set="dev", test_set="dev", max_dec_timesteps=8, batch_size=4,
               input_dim=t["input_dim"], enc_hidden_dim=t["enc_hidden_dim"], enc_n_layers=t["enc_n_layers"],
               subsample=t["subsample"], dropout_rate=0.0, dec_hidden_dim=t["dec_hidden_dim"], att_dim=t["att_dim"],
               conv_channels=t["conv_channels"], conv_kernel_size=t["conv_kernel_size"], att_odim=t["att_odim"],
               embedding_dim=t["embedding_dim"], ls_weight=t["ls_weight"], dis_embedding_dim=l["embedding_dim"],
               dis_hidden_dim=l["hidden_dim"], dis_dropout_rate=0.0, dis_layers=l["n_layers"], d_learning_rate=2e-4,
               learning_rate=5e-4, weight_decay=1e-6, max_grad_norm=5, min_feature_length=1, add_gaussian=False)
    cfg.update(over)
    monkeypatch.chdir(root)
    solver = Solver(cfg)
    dev = next(solver.model.parameters()).device
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        wm = synth.e2e_weights(t, 11)
        for k, v in solver.model.state_dict().items():
            v.copy_(torch.from_numpy(wm[k]) if k in wm else torch.empty(v.shape).uniform_(-0.25, 0.25, generator=gen))
    solver.model.decoder.labeldist = synth.labeldist(nv, 12)
    solver.model.decoder.vlabeldist = torch.from_numpy(np.asarray(solver.model.decoder.labeldist, dtype=np.float32)).to(dev)
    solver.model.decoder._dist_dev = {}
    solver.model.train()
    return solver, dev


def _sup_batch(dev):
    xs, ilens, ys = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    return torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys]


def test_pseudo_train_step(hb, tmp_path, monkeypatch):
    """Solver.pseudo_train_one_iteration on the tiny configuration, deterministic mode: the step's loss is pseudo_weight times
    the mean over the rows of -logsumexp_k (log w_k - ops.ctc_loss of hypothesis k), composed here from the same n-best list
    on the same weights - within 32 fp32 ulps of the largest nll involved (two float32 loss kernels, each within its own 8 ulp
    floor, and the sums; test_ctc_gpu.test_joint_value's allowance) - and the parameters move."""
    import gtc
    import ops
    K, weight, temp = 4, 0.5, 0.7
    solver, dev = _solver(str(tmp_path / "s"), monkeypatch, ctc_weight=0.3, deterministic=True, pseudo_beam=K,
                          pseudo_weight=weight, pseudo_temperature=temp)
    xs, ilens, _ = _sup_batch(dev)
    net = solver.model
    B = len(ilens)
    with hb.deterministic():
        _, ids, logw = solver.pseudo_graphs(xs, ilens, K, temp)
        assert net.training and all(1 <= len(u) <= K for u in ids)
        for b in range(B):
            live = logw[b, :len(ids[b])]
            assert abs(float(np.exp(live).sum()) - 1.0) <= 1e-12 and bool(np.isinf(logw[b, len(ids[b]):]).all())
        with torch.no_grad():
            enc_h, _ = net.encoder(xs, ilens)
            logits = ops.linear(enc_h.reshape(-1, enc_h.shape[2]), net.ctc_lo.weight, net.ctc_lo.bias).view(B, enc_h.shape[1], -1)
            rows, top = [], 0.0
            for b in range(B):
                terms = []
                for k, h in enumerate(ids[b]):
                    nk = ops.ctc_loss(logits[b:b + 1], net.encoder.enc2.last_lens_dev[b:b + 1],
                                      torch.tensor(h if h else [1], dtype=torch.long, device=dev)[:len(h)], [len(h)], False)
                    terms.append(float(logw[b, k]) - float(nk))
                    top = max(top, abs(float(nk)))
                rows.append(-float(torch.logsumexp(torch.tensor(terms, dtype=torch.float64), 0)))
        want = weight * sum(rows) / B
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        launches = dict(hb.LAUNCHES)
        loss, mean = solver.pseudo_train_one_iteration(xs, ilens)
        solver.flush()
    assert solver.last_pseudo["ids"] == ids and np.array_equal(solver.last_pseudo["log_weights"], logw)
    assert hb.LAUNCHES["gtc_loss"] == launches.get("gtc_loss", 0) + 1
    assert hb.LAUNCHES["gtc_loss_bwd"] == launches.get("gtc_loss_bwd", 0) + 1
    print("gtc pseudo step: loss %.7f, composed %.7f, largest nll %.4g" % (float(loss), want, top))
    assert np.isfinite(float(loss)) and abs(float(loss) - weight * float(mean)) <= 4 * 2.0 ** -23 * abs(float(loss))
    assert abs(float(loss) - want) <= 32 * 2.0 ** -23 * max(top, abs(want))
    moved = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "ctc_lo.weight" in moved and any(n.startswith("encoder.") for n in moved)
    assert not hb.persist_aborted(dev)


def test_pseudo_keys_absent_is_todays_step(hb, tmp_path, monkeypatch):
    """Without pseudo_beam - and with it, as long as no pseudo step runs - a supervised step has the launches and the loss
    bits it has always had (deterministic mode), and no graph CTC kernel runs."""
    seen = []
    for run, over in enumerate((dict(), dict(pseudo_beam=4, pseudo_weight=0.5))):
        solver, dev = _solver(str(tmp_path / ("run%d" % run)), monkeypatch, ctc_weight=0.3, deterministic=True, **over)
        hb.persist_clear_abort(dev)
        np.random.seed(4)
        xs, ilens, ys = _sup_batch(dev)
        before = dict(hb.LAUNCHES)
        loss = solver.sup_train_one_iteration(xs, ilens, ys, 1.0)
        solver.flush()
        delta = {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
        seen.append((delta, np.float32(float(loss))))
    assert seen[0][0] == seen[1][0] and not any(k.startswith("gtc") for k in seen[0][0])
    assert seen[0][0].get("ctc_loss") == 1
    assert seen[0][1].tobytes() == seen[1][1].tobytes()
