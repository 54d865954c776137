"""Contextual biasing on the host (context.py): the graph compile against a brute-force longest-suffix matcher,
the definition on hand cases, the device arrays against the dense automaton, the declared exports, the refusals of the Python
layer, and the cap on undecided utterances of the GPU grid (tests/test_context_gpu.py), from the restatements alone."""
import os

import numpy as np
import pytest

import context_ref as C

from context import ContextBatch, ContextGraph


def _state_of(g, seq):
    s = 0
    for c in seq:
        s = g.next_state(s, c)
    return s


@pytest.mark.parametrize("V,space", [(4, None), (6, None), (6, 5), (9, 8)])
def test_the_compile_against_a_brute_force_matcher(V, space):
    """Every sequence of up to 6 tokens (sampled where there are too many): the state is the node of the longest suffix that
    is a trie path, the bias the definition's; shared prefixes, a phrase that is a prefix of another, one that is a suffix
    of another's prefix, single tokens and repeated tokens are in every set."""
    for seed in range(6):
        phrases, boosts = C.random_phrases(V, 5, 100 * V + seed, space)
        g = ContextGraph(phrases, boosts, V=V, word_start_only=space)
        node = {p: i for i, p in enumerate(g.paths)}
        assert len(node) == g.n_trie and g.N == g.n_trie + (space is not None)
        rs = np.random.RandomState(seed)
        seqs = [tuple(int(c) for c in rs.randint(1, V, size=rs.randint(0, 9))) for _ in range(300)]
        seqs += [tuple(p) + tuple(q) for p in phrases[:4] for q in phrases[:4]] + [tuple(p[:-1]) + (1,) for p in phrases]
        for seq in seqs:
            want = C.brute_state(phrases, seq, space)
            got = _state_of(g, seq)
            assert got == (g.inside if want is None else node[want]), (phrases, seq, want, got)
            assert g.score(seq) == pytest.approx(C.brute_score(phrases, boosts, seq, space), abs=1e-9), (phrases, boosts, seq)
            assert sum(g.token_scores(seq)) == pytest.approx(g.score(seq), abs=1e-12) and len(g.token_scores(seq)) == len(seq) + 1


def test_the_definition_on_hand_cases():
    A, B, Cc, D, X = 1, 2, 3, 4, 5
    g = ContextGraph([[A, B, Cc]], boost=1.5, V=7)
    assert g.score([A, B, Cc]) == 4.5 and g.score([X, A, B, Cc, X]) == 4.5          # completion keeps its credit
    assert g.token_scores([A, B, Cc, X]) == [1.5, 1.5, 1.5, 0.0, 0.0]
    assert g.score([A, B, X]) == 0.0 and g.token_scores([A, B, X]) == [1.5, 1.5, -3.0, 0.0]      # a failed partial nets zero
    assert g.score([A, B]) == 0.0 and g.token_scores([A, B]) == [1.5, 1.5, -3.0]                  # ... at the end as well
    # fail-over to a shorter live match: "a b x" and "b c d" - after "a b", c continues "b c"
    g = ContextGraph([[A, B, X], [B, Cc, D]], boost=2.0, V=7)
    assert g.token_scores([A, B, Cc, D]) == [2.0, 2.0, 0.0, 2.0, 0.0] and g.score([A, B, Cc, D]) == 6.0
    assert g.score([A, B, Cc, X]) == 0.0
    # a phrase that is a prefix of another keeps what it completed; the longer one adds its own tokens
    g = ContextGraph([[A, B], [A, B, Cc, D]], boost=1.0, V=7)
    assert g.score([A, B]) == 2.0 and g.score([A, B, Cc]) == 2.0 and g.score([A, B, Cc, D]) == 4.0
    assert g.token_scores([A, B, Cc, X]) == [1.0, 1.0, 1.0, -1.0, 0.0]
    # only the longest match is credited: "b c" ends strictly inside the live "a b c d"
    g = ContextGraph([[A, B, Cc, D], [B, Cc]], boost=1.0, V=7)
    assert g.score([A, B, Cc, X]) == 0.0 and g.score([X, B, Cc, X]) == 2.0 and g.score([A, B, Cc, D]) == 4.0
    # a shared arc with two boosts: the larger wins, whatever the order of the list
    for order in ((0, 1), (1, 0)):
        ph, bo = [[A, B], [A, Cc]], [0.5, 2.0]
        g = ContextGraph([ph[i] for i in order], [bo[i] for i in order], V=7)
        assert g.score([A, B]) == 2.5 and g.score([A, Cc]) == 4.0


def test_word_start_only_blocks_art_inside_smart():
    vocab = {s: i + 1 for i, s in enumerate("smart")}                                       # s m a r t
    vocab["_"] = 6
    spell = lambda w: [vocab[ch] for ch in w]                                               # noqa: E731
    free = ContextGraph([spell("art")], boost=1.0, V=7)
    word = ContextGraph([spell("art")], boost=1.0, V=7, word_start_only=vocab["_"])
    assert free.score(spell("smart")) == 3.0 and word.score(spell("smart")) == 0.0
    assert word.score(spell("art")) == 3.0 and word.score(spell("sm_art")) == 3.0 and word.score(spell("art_s")) == 3.0
    assert word.score(spell("a_art")) == 3.0 and word.score(spell("aart")) == 0.0 and word.score(spell("ar_t")) == 0.0
    assert word.N == free.N + 1 and word.compile().R == 2 and free.compile().R == 1
    two = ContextGraph([spell("a_rt"), spell("rt")], boost=1.0, V=7, word_start_only=vocab["_"])
    assert two.score(spell("a_rt")) == 4.0 and two.score(spell("a_rs")) == 0.0 and two.score(spell("sa_rt")) == 2.0


@pytest.mark.parametrize("V,space", [(5, None), (34, 33)])
def test_the_device_arrays_give_the_dense_automaton(V, space):
    graphs = [ContextGraph(*C.random_phrases(V, 10, 7 + i, space if i else None), V=V, word_start_only=space if i else None)
              for i in range(3)]
    batch = ContextBatch(graphs, [0, 2, -1, 1])
    t = batch.compile()
    assert (t.G, t.N, t.R) == (3, sum(g.N for g in graphs), sum(g.rows.shape[0] for g in graphs))
    assert t.arc_off[0] == 0 and t.arc_off[-1] == t.A == len(t.arc_tok) == len(t.arc_next) and (np.diff(t.arc_off) >= 0).all()
    for s in range(t.N):
        toks = t.arc_tok[t.arc_off[s]:t.arc_off[s + 1]]
        assert (np.diff(toks) > 0).all() and ((toks >= 1) & (toks < V)).all()
    nxt = C.dense(t)
    n0 = 0
    for g, root in zip(graphs, t.root):
        assert root == n0
        assert np.array_equal(nxt[n0:n0 + g.N, 1:], g.dense()[:, 1:] + n0)
        assert np.array_equal(t.credit[n0:n0 + g.N], g.credit.astype(np.float32))
        assert np.array_equal(t.pending[n0:n0 + g.N], g.pending.astype(np.float32))
        for s in range(0, g.N, 3):
            for c in range(1, V):
                assert t.next_state(n0 + s, c) == g.next_state(s, c) + n0
        n0 += g.N
    assert V < 30 or t.A < t.N * (V - 1) / 4, "the sparse form is not sparse"      # (four tokens hardly leave a default)
    assert t.graph_of.tolist() == [0, 2, -1, 1] and graphs[0].compile().graph_of is None
    # the host walk over the table is the graph's score, to float32's rounding of the credits
    rs = np.random.RandomState(3)
    for _ in range(50):
        seq = [int(c) for c in rs.randint(1, V, size=rs.randint(0, 12))]
        got, per = C.walk(t, int(t.root[1]), seq, np.float64, nxt)
        assert got == pytest.approx(graphs[1].score(seq), abs=1e-5) and len(per) == len(seq)
    assert C.walk(t, -1, [1, 2], np.float64)[0] == 0.0


def test_from_text(tmp_path):
    vocab = {"<PAD>": 0, "a": 1, "b": 2, "c": 3, "<space>": 4, "7": 5}
    g = ContextGraph.from_text(["a b c 2.5", "", "# a comment", "b c", "c 7", "c 7 0.5"], vocab, boost=1.5)
    assert g.phrases == [(1, 2, 3), (2, 3), (3, 5), (3, 5)] and g.boosts == [2.5, 1.5, 1.5, 0.5] and g.V == 6
    path = os.path.join(str(tmp_path), "phrases.txt")
    with open(path, "w") as f:
        f.write("a b\nb <space> c 3\n")
    g = ContextGraph.from_text(path, vocab, V=8, word_start_only=4)
    assert g.phrases == [(1, 2), (2, 4, 3)] and g.boosts == [1.0, 3.0] and g.V == 8 and g.space == 4
    with pytest.raises(ValueError, match="not in the vocabulary"):
        ContextGraph.from_text(["a z"], vocab)


def test_the_exports_are_declared():
    import hip_backend as hb
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "asr_hip.h")) as f:
        header = f.read()
    for name in ("asr_context_score_f32", "asr_ctc_beam_ctx_f32"):
        assert name in hb.EXPORTS and ("int %s(" % name) in header
    fields = [n for n, _ in hb.ContextTable._fields_]
    assert fields == ["V", "N", "G", "R", "A", "arc_off", "arc_tok", "arc_next", "drow", "dflt", "credit", "pending", "root"]
    at = header.index("} asr_context_t;")
    body = header[header.rindex("typedef struct {", 0, at):at]
    assert [body.index(n) for n in fields] == sorted(body.index(n) for n in fields)


def test_refusals_of_the_python_layer():
    import torch
    import ops
    from solver import Solver
    for bad in (dict(phrases=[]), dict(phrases=[[]]), dict(phrases=[[0, 1]]), dict(phrases=[[5]]), dict(phrases=[[1]], boost=0.0),
                dict(phrases=[[1]], boost=float("inf")), dict(phrases=[[1]], boost=[1.0, 2.0]), dict(phrases=[[1]], word_start_only=5),
                dict(phrases=[[1]], V=None)):
        with pytest.raises(ValueError):
            ContextGraph(**dict(dict(V=5), **bad))
    g5, g6 = ContextGraph([[1, 2]], V=5), ContextGraph([[1, 2]], V=6)
    for graphs, rows in (([], [0]), ([g5], []), ([g5], [1]), ([g5], [-2]), ([g5, "x"], [0])):
        with pytest.raises(ValueError):
            ContextBatch(graphs, rows)
    with pytest.raises(ValueError, match="tokens"):
        ContextBatch([g5, g6], [0, 1]).compile()
    assert ContextBatch([g5], [0, -1]).score(1, [1, 2]) == 0.0 and ContextBatch([g5], [0, -1]).score(0, [1, 2]) == 2.0
    with pytest.raises(ValueError, match="word LM"):                 # (refused before anything touches a device)
        ops.ctc_beam(torch.zeros(1, 2, 5), torch.zeros(1, dtype=torch.int32), 2, word_lm=object(), context=g5)
    # Solver: context_bias only where the CTC prefix beam search runs
    sub = dict(phrases="p.txt")
    assert Solver.context_config({}, False, False) is None
    assert Solver.context_config(dict(context_bias=sub), True, False) is sub
    assert Solver.context_config(dict(context_bias=sub, ngram_lm="x"), False, True) is sub
    for cfg, tp, cb in ((dict(context_bias=sub), False, False), (dict(context_bias=dict(boost=2.0)), True, False),
                        (dict(context_bias=dict(sub, bonus=1.0)), True, False), (dict(context_bias=sub, word_lm="w.arpa"), False, True),
                        (dict(context_bias="p.txt"), True, False)):
        with pytest.raises(ValueError, match="context_bias"):
            Solver.context_config(cfg, tp, cb)


@pytest.mark.parametrize("V", C.GRID_V)
@pytest.mark.parametrize("K", C.GRID_K)
def test_the_gpu_grid_decides_enough_utterances(V, K):
    """The cap of tests/test_context_gpu.py: of the utterances of one parametrisation at most 1 in 10 may be left undecided
    (a float64 selection margin inside the allowance) - asserted here from the restatements alone."""
    cases = [c for c in C.grid()[0] if c[0] == V and c[1] == K]
    assert len(cases) == 6 and {c[4] for c in cases} == {False, True} and {c[2] for c in cases} == set(C.GRID_T)
    verdicts = [v for c in cases for v in C.judge(c)]
    undecided = sum(not v["decisive"] for v in verdicts)
    assert undecided <= C.UNDECIDED_CAP * len(verdicts), (V, K, undecided, len(verdicts))
    with_graph = [v for c in cases for b, v in enumerate(C.judge(c)) if b < 2 and C.GRAPH_OF[c[6]][b] >= 0]
    moved = sum(float(np.abs(v["ref"]["ctx"]).max()) > 0 for v in with_graph)
    assert moved >= len(with_graph) // 2, "the phrase lists hardly touch the grid's hypotheses"


def test_the_switch_cases_decide_enough_utterances():
    cases = C.grid()[1]
    assert [c[0] * c[1] > 1024 for c in cases[:2]] == [False, True] and [c[2] * c[1] > 4096 for c in cases[2:]] == [False, True]
    verdicts = [v for c in cases for v in C.judge(c)]
    assert sum(not v["decisive"] for v in verdicts) <= C.UNDECIDED_CAP * len(verdicts)
