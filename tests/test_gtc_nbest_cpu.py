"""The n-best graph builder without a GPU: its numpy reference (tests/gtc_nbest_ref.py) against the host path
of Solver.pseudo_graphs where every row fits, the admission rule, the C ABI's declarations and exports, and the Solver's new
key."""
import os
import re

import numpy as np
import pytest

import gtc
import gtc_nbest_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"asr_nbest_gtc_bytes", "asr_nbest_gtc_f32"}


def _pseudo_graphs_construction(hyp, hyp_len, score, V, temperature):
    """What Solver.pseudo_graphs does behind its host read, line for line: the lists of the kept slots, score / hyp_len
    arrays padded with -inf / -1, gtc.nbest_weights, from_nbest over the live slots, the empty hypothesis otherwise."""
    B, K = hyp_len.shape
    ids = [[[int(v) for v in hyp[b, k, :hyp_len[b, k]]] for k in range(K) if hyp_len[b, k] >= 0] for b in range(B)]
    scores = [[float(score[b, k]) for k in range(K) if hyp_len[b, k] >= 0] for b in range(B)]
    sc = np.full((B, K), -np.inf)
    hl = np.full((B, K), -1, dtype=np.int64)
    for b in range(B):
        n = len(ids[b])
        sc[b, :n] = scores[b]
        hl[b, :n] = [len(h) for h in ids[b]]
    logw = gtc.nbest_weights(sc, hl, temperature)
    graphs = []
    for b in range(B):
        live = [k for k in range(len(ids[b])) if logw[b, k] > -np.inf]
        if live:
            graphs.append(gtc.Graph.from_nbest([ids[b][k] for k in live], [logw[b, k] for k in live], V))
        else:
            graphs.append(gtc.Graph.from_nbest([[]], [0.0], V))
    return gtc.GraphBatch(graphs, range(B)).compile()


@pytest.mark.parametrize("temperature", [0.0, 0.7, 3.0])
def test_reference_is_the_host_path_where_every_row_fits(temperature):
    """Lists as the search leaves them (the dead slots behind the live ones), small enough to fit: the reference's table is
    the table of pseudo_graphs' construction, every field, exactly."""
    rs = np.random.RandomState(3)
    B, K, L, V = 7, 8, 9, 5
    hyp, hyp_len, score = NR.random_lists(rs, B, K, L, V, dead=0.0)
    for b in range(B):                                         # dead slots trail, one row has none alive
        n = int(rs.randint(1, K + 1)) if b else 0
        hyp[b, n:], hyp_len[b, n:], score[b, n:] = -1, -1, -np.inf
    ref = NR.reference(hyp, hyp_len, score, V, temperature)
    assert not ref.dropped.any()
    want = _pseudo_graphs_construction(hyp, hyp_len, score, V, temperature)
    for name in gtc.GraphTable.FIELDS:
        assert np.array_equal(getattr(ref.table, name), getattr(want, name)), name
    assert (ref.table.max_nodes, ref.table.max_arcs) == (want.max_nodes, want.max_arcs)
    assert ref.graphs[0].N == 1 and float(ref.graphs[0].fin[0]) == 0.0


def test_admission_keeps_every_graph_within_the_limit():
    """K = 16 long hypotheses with little in common pass 1023 trie nodes: the reference admits a prefix of the live list,
    drops the rest, stays within 2047 nodes and renormalises the weights over what it kept."""
    rs = np.random.RandomState(5)
    B, K, L, V = 6, 16, 90, 40
    hyp, hyp_len, score = NR.random_lists(rs, B, K, L, V, dead=0.1, dup=0.1)
    hyp_len[0, :] = np.where(hyp_len[0] >= 0, L, -1)           # a row that certainly overflows
    hyp[0] = rs.randint(1, V, size=(K, L))
    ref = NR.reference(hyp, hyp_len, score, V, 1.0)
    assert ref.dropped[0] > 0
    for b in range(B):
        live = (hyp_len[b] >= 0) & (score[b] > -np.inf)
        assert ref.graphs[b].N <= gtc.MAX_NODES
        assert int(ref.dropped[b]) == int(live.sum()) - int(ref.admitted[b].sum())
        kept = np.nonzero(ref.admitted[b])[0]
        lost = np.nonzero(live & ~ref.admitted[b])[0]
        assert not len(lost) or not len(kept) or kept.max() < lost.min()        # a suffix of the list only
        assert bool(np.isinf(ref.log_weights[b, ~ref.admitted[b]]).all())
        if len(kept):
            assert abs(float(np.exp(ref.log_weights[b, kept]).sum()) - 1.0) <= 1e-12
    # the smallest overflow: 16 x 65 distinct first tokens = 1040 trie nodes; and exactly 1023 beside it
    hyp = rs.randint(1, 18, size=(2, 16, 65)).astype(np.int32)
    hyp[:, :, 0] = np.arange(1, 17)
    hyp_len = np.full((2, 16), 65, dtype=np.int32)
    hyp_len[1, 15] = NR.MAX_TRIE - 15 * 65
    ref = NR.reference(hyp, hyp_len, -np.arange(32, dtype=np.float32).reshape(2, 16), 18, 1.0)
    assert list(ref.dropped) == [1, 0] and ref.graphs[0].N == 2 * 15 * 65 + 1 and ref.graphs[1].N == gtc.MAX_NODES


def test_abi_declares_and_exports_the_entries():
    """include/asr_hip.h declares the two entries beside "Graph CTC" without a version change, hip_backend.EXPORTS holds
    them, build()'s library exports them, and the capacities are the header's bounds, from plain integers."""
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_nbest_gtc_\w+)\s*\(", header, flags=re.M))
    assert declared == ENTRIES and "the n-best graph builder" in header
    assert re.search(r"^#define ASR_ABI_VERSION 8\s*$", header, flags=re.M)
    assert ENTRIES <= set(hb.EXPORTS)
    lib = hb.load()
    assert all(hasattr(lib, n) for n in ENTRIES)
    assert hb.gtc_nbest_bytes(32, 8, 100, 34) == (1601, 3 * 1601, 8 * 32)
    assert hb.gtc_nbest_bytes(3, 16, 65, 5)[:2] == (hb.GTC_MAX_NODES, 3 * hb.GTC_MAX_NODES)
    assert hb.gtc_nbest_bytes(1, 1, 1, 2)[:2] == (3, 9)
    for bad in ((1, 17, 4, 5), (1, 4, 4, 1)):
        with pytest.raises(hb.UnsupportedShape):
            hb.gtc_nbest_bytes(*bad)
    with pytest.raises(RuntimeError):
        hb.gtc_nbest_bytes(1, 4, 0, 5)


def test_solver_key():
    """pseudo_graphs_on_gpu belongs to pseudo_beam: ValueError without it from the accessor and from pseudo_config; absent or
    false is off; pseudo_config's tuple is what it was, with and without the key."""
    from solver import Solver
    assert Solver.pseudo_graphs_on_gpu({}) is False
    assert Solver.pseudo_graphs_on_gpu(dict(pseudo_beam=4)) is False
    assert Solver.pseudo_graphs_on_gpu(dict(pseudo_beam=4, pseudo_graphs_on_gpu=False)) is False
    assert Solver.pseudo_graphs_on_gpu(dict(pseudo_beam=4, pseudo_graphs_on_gpu=True)) is True
    for bad in (dict(pseudo_graphs_on_gpu=True), dict(pseudo_graphs_on_gpu=False)):
        with pytest.raises(ValueError):
            Solver.pseudo_graphs_on_gpu(bad)
        with pytest.raises(ValueError):
            Solver.pseudo_config(bad)
    assert Solver.pseudo_config({}) is None
    assert Solver.pseudo_config(dict(pseudo_beam=4)) == (4, 1.0, 1.0, 1, None)
    assert Solver.pseudo_config(dict(pseudo_beam=4, pseudo_graphs_on_gpu=True)) == (4, 1.0, 1.0, 1, None)
    assert Solver.pseudo_config(dict(pseudo_beam=8, pseudo_temperature=0.5, pseudo_weight=0.3, pseudo_epochs=2)) == (8, 0.5, 0.3, 2, None)


def test_device_table_holds_only_host_numbers():
    """gtc.DeviceGraphTable on host tensors: its sizes are the capacities, none of them read from an array."""
    t = gtc.DeviceGraphTable(5, 3, 49, 147, "cpu")
    assert (t.G, t.NN, t.A, t.max_nodes, t.max_arcs) == (3, 147, 441, 49, 147)
    assert t.in_ptr.numel() == 148 and t.in_src.numel() == 441 and tuple(t.head.shape) == (3, 5) and t.graph_of.numel() == 3
    assert t.to("cpu") is t and t.rows(3) is t.graph_of
    with pytest.raises(ValueError):
        t.rows(2)
    with pytest.raises(ValueError):
        t.to("cuda")
