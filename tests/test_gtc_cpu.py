"""Graph CTC without a GPU: the torch restatement (tests/gtc_ref.py) against a brute-force enumeration of every node sequence,
the graph builders of gtc.py against what they promise (torch's ctc_loss, the n-best composition, the enumeration of a
confusion network's choices), their validation and canonical order, the C ABI's declarations, and the Solver's refusals."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gtc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def gtc():
    import __graft_entry__ as entry
    entry._ensure_paths()
    import gtc
    return gtc


def _ctc(z, labels):
    """float64 CTC nll of one row z [T, V] (no labels: the all-blank path)"""
    x = F.log_softmax(z, -1)
    if not labels:
        return float(-x[:, 0].sum())
    return float(F.ctc_loss(x.unsqueeze(1), torch.tensor([labels]), torch.tensor([z.shape[0]]), torch.tensor([len(labels)]),
                            blank=0, reduction="none", zero_infinity=False))


def _nll(z, g):
    return float(R.gtc_nll(z.unsqueeze(0), [z.shape[0]], [g], zero_infinity=False)[0])


def _lse(terms):
    m = max(terms)
    return m if m == -INF else m + math.log(sum(math.exp(t - m) for t in terms))


def _close(a, b, tol=1e-11):
    return (a == b) or abs(a - b) <= tol * max(1.0, abs(b))


def test_reference_equals_brute_force_enumeration(gtc):
    """Random graphs with N <= 4 nodes and T <= 4 frames, V = 3: every node sequence enumerated.  -inf start and final
    weights, missing self-loops, unreachable nodes and graphs without any path (+inf on both sides) are all drawn."""
    rs = np.random.RandomState(3)
    seen_inf = n = 0
    for trial in range(120):
        N, T = int(rs.randint(1, 5)), int(rs.randint(1, 5))
        lab = rs.randint(0, 3, size=N)
        start = [float(rs.uniform(-2, 0)) if rs.uniform() < 0.6 else -INF for _ in range(N)]
        fin = [float(rs.uniform(-2, 0)) if rs.uniform() < 0.6 else -INF for _ in range(N)]
        arcs = [(m, k, float(rs.uniform(-3, 0))) for m in range(N) for k in range(N) if rs.uniform() < 0.5]
        g = gtc.Graph(3, lab, start, fin, arcs)
        z = torch.from_numpy(rs.normal(0, 2, size=(T, 3)))
        want = R.brute_force(F.log_softmax(z, -1).numpy(), g)
        got = _nll(z, g)
        assert _close(got, want), (trial, got, want)
        seen_inf += want == INF
        n += 1
    assert 5 <= seen_inf <= n - 60


def test_ctc_lattice_is_torch_ctc_loss(gtc):
    rs = np.random.RandomState(4)
    for labels, T in (([], 1), ([], 5), ([2], 1), ([1, 2, 3], 3), ([2, 2], 3), ([1, 1, 2, 2, 4], 9), ([3, 1, 3, 1], 12)):
        g = gtc.Graph.ctc(labels, 5)
        assert g.N == 2 * len(labels) + 1
        z = torch.from_numpy(rs.normal(0, 2, size=(T, 5)))
        assert _close(_nll(z, g), _ctc(z, labels)), labels
    z = torch.from_numpy(rs.normal(0, 1, size=(2, 5)))
    assert _nll(z, gtc.Graph.ctc([2, 2], 5)) == INF                        # 2 labels + 1 repeat need 3 frames
    zero, feasible = R.gtc_nll(z.unsqueeze(0), [2], [gtc.Graph.ctc([2, 2], 5)], zero_infinity=True)
    assert float(zero) == 0.0 and not bool(feasible)


def test_nbest_tree_is_the_weighted_sum_of_ctc_losses(gtc):
    """A duplicate hypothesis, the empty one, one that is a prefix of another, equal neighbours across a trie arc."""
    rs = np.random.RandomState(5)
    hyps = [[1, 2], [1], [1, 2], [], [3, 3, 1], [1, 2, 2], [4]]
    logw = [-0.3, -1.2, -2.0, -0.7, -1.5, -0.1, -INF]
    g = gtc.Graph.from_nbest(hyps, logw, 5)
    assert g.N == 2 * 7 + 1              # the root's blank and 7 trie nodes: 1, 1 2, 1 2 2, 3, 3 3, 3 3 1, 4
    for T in (1, 2, 4, 7):
        z = torch.from_numpy(rs.normal(0, 2, size=(T, 5)))
        want = -_lse([w - _ctc(z, h) if _need(h) <= T else -INF for h, w in zip(hyps, logw)])
        assert _close(_nll(z, g), want), T
    one = gtc.Graph.from_nbest([[2, 2]], [0.0], 5)
    z = torch.from_numpy(rs.normal(0, 2, size=(5, 5)))
    assert _close(_nll(z, one), _ctc(z, [2, 2]))


def _need(labels):
    return max(1, len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b))


def test_confusion_network_is_the_sum_over_its_choices(gtc):
    """A skippable position, two adjacent positions offering the same token, a position offering one token twice, skips at
    both ends, and a network whose every position can be skipped."""
    rs = np.random.RandomState(6)
    nets = [[[(1, -0.2), (2, -1.0)], [(None, -0.5), (2, -0.9)], [(2, -0.1), (3, -0.4), (None, -2.0)]],
            [[(None, -0.3), (1, -0.6)], [(1, -0.2)], [(1, -0.4), (1, -1.4)], [(None, -0.1), (4, -0.8)]],
            [[(None, -0.3), (1, -0.6)], [(None, -0.2), (None, -1.0), (2, -0.5)]],
            [[(3, 0.0)]], []]
    for slots in nets:
        g = gtc.Graph.from_confusion(slots, 5)
        assert g.N == len(slots) + 1 + sum(1 for s in slots for c, _ in s if c is not None)
        for T in (1, 3, 6):
            z = torch.from_numpy(rs.normal(0, 2, size=(T, 5)))
            terms = []
            for choice in itertools.product(*slots):
                toks = [c for c, _ in choice if c is not None]
                terms.append(sum(w for _, w in choice) - _ctc(z, toks) if _need(toks) <= T else -INF)
            want = -_lse(terms)
            assert _close(_nll(z, g), want), (slots, T)


def test_validation(gtc):
    ok = dict(V=5, lab=[0, 1], start=[0.0, -INF], fin=[-INF, 0.0], arcs=[(0, 0, 0.0), (0, 1, -1.0)])
    gtc.Graph(**ok)
    for bad in (dict(lab=[0, 5]), dict(lab=[0, -1]), dict(V=1), dict(lab=[]), dict(start=[0.0]), dict(fin=[0.0, float("nan")]),
                dict(start=[INF, 0.0]), dict(arcs=[(0, 1, -1.0), (0, 1, -2.0)]), dict(arcs=[(0, 2, 0.0)]),
                dict(arcs=[(0, 1, -INF)]), dict(arcs=[(0, 1, float("nan"))]), dict(lab=[0] * (gtc.MAX_NODES + 1))):
        with pytest.raises(ValueError):
            gtc.Graph(**dict(ok, **bad))
    with pytest.raises(ValueError):                                            # the arc limit
        gtc.Graph(5, [0] * 300, [0.0] * 300, [0.0] * 300, [(m, n, 0.0) for m in range(300) for n in range(300)][:gtc.MAX_ARCS + 1])
    with pytest.raises(ValueError):
        gtc.Graph.ctc([1, 5], 5)
    with pytest.raises(ValueError):
        gtc.Graph.ctc([1] * 1024, 5)                                           # 2049 nodes
    with pytest.raises(ValueError):
        gtc.Graph.from_nbest([[1, 0]], [0.0], 5)
    with pytest.raises(ValueError):
        gtc.Graph.from_nbest([[1]], [0.0, 0.0], 5)
    with pytest.raises(ValueError):
        gtc.Graph.from_nbest([[1]], [float("nan")], 5)
    with pytest.raises(ValueError):
        gtc.Graph.from_confusion([[(7, 0.0)]], 5)
    with pytest.raises(ValueError):
        gtc.Graph.from_confusion([[]], 5)
    g = gtc.Graph(**ok)
    for bad in ((None, [0]), ([g], [1]), ([g], [-1]), ([g], []), ([g, gtc.Graph.ctc([1], 6)], [0, 1])):
        with pytest.raises(ValueError):
            gtc.GraphBatch(bad[0] or [], bad[1]).compile()
    assert gtc.MAX_NODES == 2047


def test_nbest_weights(gtc):
    score = np.array([[-1.0, -2.0, -INF, -4.0], [-3.0, -INF, -INF, -INF], [-INF] * 4])
    hyp_len = np.array([[2, 0, -1, 3], [1, -1, -1, -1], [-1] * 4])
    w = gtc.nbest_weights(score, hyp_len, 0.5)
    live = np.array([-0.5, -1.0, -2.0])
    assert np.allclose(w[0, [0, 1, 3]], live - np.log(np.exp(live).sum()), atol=1e-14) and w[0, 2] == -INF
    assert w[1, 0] == 0.0 and np.isinf(w[1, 1:]).all() and np.isinf(w[2]).all()
    assert np.allclose(gtc.nbest_weights(score, hyp_len, 0.0)[0, [0, 1, 3]], -math.log(3))
    with pytest.raises(ValueError):
        gtc.nbest_weights(score, hyp_len, -1.0)


def test_canonical_arc_order(gtc):
    """Two insertion orders of the same arcs give equal tables, and the table is what the header says: arcs by destination
    with ascending sources, by source with ascending destinations, nodes sorted by (token, node) with run heads."""
    rs = np.random.RandomState(8)
    N, V = 11, 4
    lab = rs.randint(0, V, size=N)
    arcs = [(m, n, float(rs.uniform(-3, 0))) for m in range(N) for n in range(N) if rs.uniform() < 0.3]
    start, fin = list(rs.uniform(-1, 0, size=N)), list(rs.uniform(-1, 0, size=N))
    a = gtc.Graph(V, lab, start, fin, arcs).compile()
    shuffled = [arcs[i] for i in rs.permutation(len(arcs))]
    b = gtc.Graph(V, lab, start, fin, shuffled).compile()
    for name in gtc.GraphTable.FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert getattr(a, name).dtype in (np.int32, np.float32)
    W = np.full((N, N), -INF)
    for m, n, w in arcs:
        W[m, n] = np.float32(w)
    for n in range(N):
        src = a.in_src[a.in_ptr[n]:a.in_ptr[n + 1]]
        assert list(src) == sorted(src) == [m for m in range(N) if W[m, n] > -INF]
        assert np.array_equal(a.in_w[a.in_ptr[n]:a.in_ptr[n + 1]], W[src, n].astype(np.float32))
        dst = a.out_dst[a.out_ptr[n]:a.out_ptr[n + 1]]
        assert list(dst) == sorted(dst) == [k for k in range(N) if W[n, k] > -INF]
        assert np.array_equal(a.out_w[a.out_ptr[n]:a.out_ptr[n + 1]], W[n, dst].astype(np.float32))
    assert list(a.order) == sorted(range(N), key=lambda n: (lab[n], n))
    for k in range(V):
        e = int(a.head[0, k])
        first, count = e >> gtc.HEAD_SHIFT, e & ((1 << gtc.HEAD_SHIFT) - 1)
        assert count == int((lab == k).sum()) and (count == 0 or all(lab[a.order[first + j]] == k for j in range(count)))
    # a batch: node offsets, arc pointers continuing across graphs, one head row per graph
    other = gtc.Graph.ctc([1, 2], V)
    t = gtc.GraphBatch([gtc.Graph(V, lab, start, fin, arcs), other], [1, 0, 1]).compile()
    assert list(t.node_off) == [0, N, N + 5] and t.max_nodes == N and t.A == len(arcs) + other.A
    assert int(t.in_ptr[N]) == len(arcs) and int(t.in_ptr[-1]) == t.A and t.head.shape == (2, V)
    assert list(t.graph_of) == [1, 0, 1]


def test_abi_declares_the_three_entries():
    """include/asr_hip.h declares asr_gtc_ws_bytes / _loss_fwd / _loss_bwd under "Graph CTC", hip_backend.EXPORTS holds them, the
    library exports them, the version is 8 and the limits are the header's."""
    import __graft_entry__ as entry
    entry.build()
    import gtc
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_gtc_\w+)\s*\(", header, flags=re.M))
    want = {"asr_gtc_ws_bytes", "asr_gtc_loss_fwd", "asr_gtc_loss_bwd"}
    assert declared == want and "Graph CTC" in header
    assert want <= set(hb.EXPORTS)
    lib = hb.load()
    assert all(hasattr(lib, n) for n in want)
    assert re.search(r"^#define ASR_ABI_VERSION 8\s*$", header, flags=re.M)
    nodes = int(re.search(r"^#define ASR_GTC_MAX_NODES (\d+)", header, flags=re.M).group(1))
    arcs = int(re.search(r"^#define ASR_GTC_MAX_ARCS (\d+)", header, flags=re.M).group(1))
    assert nodes == hb.GTC_MAX_NODES == gtc.MAX_NODES == 2 * hb.CTC_MAX_LABELS + 1 == 2047
    assert arcs == hb.GTC_MAX_ARCS == gtc.MAX_ARCS
    B, T, V, N = 3, 7, 5, 9
    assert hb.gtc_ws_bytes(B, T, V, N) >= 4 * (B * T * (N + 1) + B)          # plain integers, no GPU
    with pytest.raises(hb.UnsupportedShape):
        hb.gtc_ws_bytes(B, T, V, nodes + 1)
    with pytest.raises(hb.UnsupportedShape):
        hb.gtc_ws_bytes(B, T, 1, N)
    fields = [n for n, _ in hb.GtcGraphs._fields_]
    struct = re.search(r"typedef struct \{([^}]*)\} asr_gtc_graphs_t;", header).group(1)
    assert fields == re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", struct))


def test_solver_refuses_what_cannot_hold():
    """The pseudo-labelling keys: off when absent; ValueError without the CTC head, under data parallelism, for a beam
    outside 2..16, a negative weight, a pseudo key without pseudo_beam, an n-gram weight without ngram_lm, word_lm."""
    import __graft_entry__ as entry
    entry._ensure_paths()
    from solver import Solver
    assert Solver.pseudo_config({}) is None and Solver.pseudo_config(dict(ngram_weight=0.5)) is None
    assert Solver.pseudo_config(dict(pseudo_beam=4)) == (4, 1.0, 1.0, 1, None)
    assert Solver.pseudo_config(dict(pseudo_beam=8, pseudo_temperature=0.5, pseudo_weight=0.3, pseudo_epochs=2, ngram_lm="lm.arpa",
                                     ngram_weight=0.4)) == (8, 0.5, 0.3, 2, ("lm.arpa", 0.4, 0.0))
    with pytest.raises(ValueError):
        Solver.pseudo_config(dict(pseudo_beam=4), has_ctc_head=False)
    with pytest.raises(ValueError):
        Solver.pseudo_config(dict(pseudo_beam=4), world=2)
    for bad in (dict(pseudo_beam=1), dict(pseudo_beam=17), dict(pseudo_beam=4, pseudo_weight=-1.0),
                dict(pseudo_beam=4, pseudo_temperature=-0.5), dict(pseudo_beam=4, pseudo_epochs=0), dict(pseudo_weight=0.5),
                dict(pseudo_epochs=2), dict(pseudo_beam=4, ngram_weight=0.5), dict(pseudo_beam=4, ngram_bonus=0.1),
                dict(pseudo_beam=4, word_lm="w.arpa")):
        with pytest.raises(ValueError):
            Solver.pseudo_config(bad)
