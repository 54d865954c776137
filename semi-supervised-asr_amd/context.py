"""Contextual biasing: per-utterance phrase lists that nudge the CTC prefix beam search (csrc/ctc_beam.hip)
towards their phrases, and what the scoring kernel (csrc/context.hip) walks.  numpy only; nothing of the GPU path is imported
here (the .to methods import torch where they are called).

  ContextGraph(phrases, boost=1.0, V=..., word_start_only=None)   phrases as lists of token ids
  ContextGraph.from_text(lines, vocab, ...)                       one phrase per line, an optional trailing boost
  g.score(ids) / g.token_scores(ids)                              the definition below, float64
  g.compile() -> ContextTable                                     the sparse device form; g.to(device) uploads it once
  ContextBatch(graphs, graph_of)                                  several graphs in one table, graph_of[b] in -1 .. G-1 per
                                                                  utterance (-1: no biasing for that row)

The definition.  A phrase is a non-empty row of token ids (no blank) with a per-token boost b > 0 in log units.  Over the trie
of the phrases, next(s, c) is the Aho-Corasick goto function with the failure links resolved (the state after c is the
longest suffix of the tokens so far that is a path of the trie), and for a node s
    credit[s]   the sum of the token boosts on the trie path to s, counted from the nearest proper ancestor that ends a
                phrase (exclusive), from the root if there is none
    pending[s]  0 if s ends a phrase, credit[s] otherwise
    delta(s, c) = credit[next(s, c)] - pending[s]          final(s) = -pending[s]
The bias of a token sequence is the sum of its deltas in token order from the root, plus final of the last state: a function
of the token sequence only.  Along a trie arc the delta is the token's own boost; a completed phrase keeps what it earned; a
partial match that fails gives back exactly what it had been lent.  ONLY THE LONGEST MATCH IS CREDITED: a phrase that ends
strictly inside a longer live match is not credited unless that match is its own node (with "a b c d" and "b c" listed,
"a b c x" earns nothing: the state after "a b c" is the node of "a b c", not of "b c").  Where two phrases share an arc and give
it different boosts the larger boost wins.
word_start_only=<space id> (for character models): a phrase may begin only at the start of the sequence or right after
<space>.  On the host that is one extra state per graph ("inside a word, no match") that returns to the root on <space>, and
failure links that only keep suffixes which begin at a word start."""
import math
import os

import numpy as np


class ContextTable(object):
    """The sparse device form of one or several graphs (csrc/context.h).  N states, G graphs, R default rows, A arcs:
        arc_off int32 [N + 1], arc_tok int32 [A] ascending inside a state, arc_next int32 [A]   the transitions of state s
                                          that differ from its default row
        drow int32 [N], dflt int32 [R, V]     the default row of state s: next(s, c) = dflt[drow[s], c] where no arc lists c
        credit, pending float32 [N]           (credit64 / pending64: the float64 values they were rounded from, host only)
        root int32 [G]                        the root of graph g; graph_of int32 [B] or None (every row: graph 0)
    On the host these are numpy arrays, after .to(device) device tensors (arc_tok / arc_next hold one unused element when
    A = 0: no tensor is empty)."""
    FIELDS = ("arc_off", "arc_tok", "arc_next", "drow", "dflt", "credit", "pending", "root")

    def __init__(self, V, arc_off, arc_tok, arc_next, drow, dflt, credit, pending, root, graph_of=None, credit64=None,
                 pending64=None):
        self.V, self.N, self.G, self.R, self.A = int(V), int(len(drow)), int(len(root)), int(dflt.shape[0]), int(arc_off[-1])
        self.arc_off, self.arc_tok, self.arc_next, self.drow, self.dflt = arc_off, arc_tok, arc_next, drow, dflt
        self.credit, self.pending, self.root, self.graph_of = credit, pending, root, graph_of
        self.credit64, self.pending64 = credit64, pending64
        self._rows = {}

    def next_state(self, s, c):
        """next(s, c) through the sparse form, as csrc/context.h's step finds it (host arrays only)."""
        lo, hi = int(self.arc_off[s]), int(self.arc_off[s + 1])
        i = lo + int(np.searchsorted(self.arc_tok[lo:hi], c))
        if i < hi and int(self.arc_tok[i]) == c:
            return int(self.arc_next[i])
        return int(self.dflt[self.drow[s], c])

    def to(self, device):
        import torch
        t = ContextTable.__new__(ContextTable)
        t.__dict__.update(self.__dict__)
        t._rows = {}
        for name in self.FIELDS + ("graph_of",):
            a = getattr(self, name)
            if a is None:
                continue
            if not isinstance(a, torch.Tensor):
                a = np.ascontiguousarray(a)
                if a.size == 0:
                    a = np.zeros(1, dtype=a.dtype)
                a = torch.from_numpy(a)
            setattr(t, name, a.to(device))
        t.credit64 = t.pending64 = None
        return t

    def rows(self, B):
        """graph_of for a call over B rows (device form): the batch's own, or graph 0 for every row."""
        import torch
        if self.graph_of is not None:
            if int(self.graph_of.numel()) != int(B):
                raise ValueError("context: the batch lists a graph for %d utterances, the call has %d" % (self.graph_of.numel(), B))
            return self.graph_of
        if B not in self._rows:
            self._rows[B] = torch.zeros(int(B), dtype=torch.int32, device=self.root.device)
        return self._rows[B]


class ContextGraph(object):
    """One phrase list.  phrases: rows of token ids in 1 .. V-1; boost: one per-token boost for all, or one per phrase."""

    def __init__(self, phrases, boost=1.0, V=None, word_start_only=None):
        if V is None:
            raise ValueError("context: V, the number of tokens of the model, is required")
        self.V = int(V)
        self.space = None if word_start_only is None or word_start_only is False else int(word_start_only)
        if self.V < 2:
            raise ValueError("context: V = %d (at least the blank and one token)" % self.V)
        if self.space is not None and not 0 < self.space < self.V:
            raise ValueError("context: word_start_only = %d is not a token of 1 .. %d" % (self.space, self.V - 1))
        self.phrases = [tuple(int(c) for c in p) for p in phrases]
        boosts = [float(boost)] * len(self.phrases) if np.isscalar(boost) else [float(b) for b in boost]
        if len(boosts) != len(self.phrases):
            raise ValueError("context: %d boosts for %d phrases" % (len(boosts), len(self.phrases)))
        if not self.phrases:
            raise ValueError("context: an empty phrase list (leave the context out instead)")
        for p, b in zip(self.phrases, boosts):
            if not p or any(not 0 < c < self.V for c in p):
                raise ValueError("context: the phrase %r is empty or holds an id outside 1 .. %d (0 is the blank)" % (p, self.V - 1))
            if not (b > 0.0 and math.isfinite(b)):
                raise ValueError("context: the boost of %r must be positive and finite, got %r" % (p, b))
        self.boosts = boosts
        self._build()
        self._table = None
        self._device = {}

    @classmethod
    def from_text(cls, lines, vocab, boost=1.0, V=None, word_start_only=None):
        """lines: a file name, or an iterable of lines - one phrase per line as symbols of vocab ({symbol: id}) separated by
        blanks, with an optional trailing number: the per-token boost of that phrase.  Empty lines and lines that begin
        with # are skipped; a symbol outside the vocabulary is a ValueError that names it."""
        if isinstance(lines, (str, os.PathLike)):
            with open(os.fspath(lines), "r", encoding="utf-8") as f:
                lines = f.read().splitlines()
        phrases, boosts = [], []
        for raw in lines:
            f = raw.split()
            if not f or f[0].startswith("#"):
                continue
            b = float(boost)
            if len(f) > 1 and f[-1] not in vocab:
                try:
                    b = float(f[-1])
                except ValueError:
                    raise ValueError("context: the symbol %r of the phrase %r is not in the vocabulary" % (f[-1], raw))
                f = f[:-1]
            for s in f:
                if s not in vocab:
                    raise ValueError("context: the symbol %r of the phrase %r is not in the vocabulary" % (s, raw))
            phrases.append([int(vocab[s]) for s in f])
            boosts.append(b)
        V = max(int(i) for i in vocab.values()) + 1 if V is None else int(V)
        return cls(phrases, boost=boosts, V=V, word_start_only=word_start_only)

    # ---------------------------------------------------------------------------------------------------------- the graph
    def _build(self):
        """States: 0 the root, then the trie nodes breadth first (children in token order), then - with word_start_only -
        the "inside a word" state.  Every state gets a default row and the transitions that differ from it: those of its
        failure state, its own children written over them."""
        kids, arc, ends = [{}], [0.0], [False]
        for p, b in zip(self.phrases, self.boosts):
            node = 0
            for c in p:
                if c not in kids[node]:
                    kids[node][c] = len(kids)
                    kids.append({})
                    arc.append(b)
                    ends.append(False)
                node = kids[node][c]
                arc[node] = max(arc[node], b)                          # a shared arc: the larger boost wins
            ends[node] = True
        # breadth-first numbering
        order, parent = [0], {0: (None, None)}
        for s in order:
            for c in sorted(kids[s]):
                parent[kids[s][c]] = (s, c)
                order.append(kids[s][c])
        number = {s: i for i, s in enumerate(order)}
        n_trie = len(order)
        wso = self.space is not None
        N = n_trie + (1 if wso else 0)
        inside = n_trie if wso else None                               # the state "inside a word, no match"
        V = self.V
        rows = np.zeros((2 if wso else 1, V), dtype=np.int64)
        if wso:
            rows[0, :] = inside
            rows[0, self.space] = 0
            rows[1, :] = inside
            rows[1, self.space] = 0
        for c, k in kids[0].items():
            rows[0, c] = number[k]
        rows[:, 0] = 0
        drow = np.zeros(N, dtype=np.int64)
        if wso:
            drow[inside] = 1
        sparse = [dict() for _ in range(N)]
        credit, pending = np.zeros(N), np.zeros(N)

        def goto(s, c):
            return sparse[s].get(c, int(rows[drow[s], c]))
        fail = {}                                                      # a state after the states its failure chain visits
        for s in order[1:]:
            i = number[s]
            par, c = parent[s]
            pi = number[par]
            if par == 0:                                               # the empty suffix: a word start only behind <space>
                f = 0 if not wso or c == self.space else inside
            else:
                f = goto(fail[pi], c)
            fail[i] = f
            drow[i] = drow[f]
            d = dict(sparse[f])
            for cc, k in kids[s].items():
                d[cc] = number[k]
            sparse[i] = {cc: k for cc, k in d.items() if k != int(rows[drow[i], cc])}
            credit[i] = arc[s] + (0.0 if par == 0 or ends[par] else credit[pi])
            pending[i] = 0.0 if ends[s] else credit[i]
        self.fail = fail
        self.N, self.n_trie, self.inside = N, n_trie, inside
        self.rows, self.drow, self.sparse = rows, drow, sparse
        self.credit, self.pending = credit, pending
        self.ends = np.array([ends[s] for s in order] + ([False] if wso else []))
        self.paths = []
        for s in order:                                                # the token path of every trie state (for the tests)
            p = []
            while s != 0:
                s, c = parent[s]
                p.append(c)
            self.paths.append(tuple(reversed(p)))

    def next_state(self, s, c):
        return self.sparse[s].get(int(c), int(self.rows[self.drow[s], int(c)]))

    def dense(self):
        """-> next int64 [N, V], the whole goto function (column 0, the blank, keeps the state)."""
        nxt = np.empty((self.N, self.V), dtype=np.int64)
        for s in range(self.N):
            nxt[s] = self.rows[self.drow[s]]
            for c, k in self.sparse[s].items():
                nxt[s, c] = k
        nxt[:, 0] = np.arange(self.N)
        return nxt

    def token_scores(self, ids):
        """-> the float64 delta of every token of ids from the root, and final of the last state behind them."""
        s, out = 0, []
        for c in ids:
            c = int(c)
            if not 0 < c < self.V:
                raise ValueError("context: the id %d is not a token of 1 .. %d" % (c, self.V - 1))
            n = self.next_state(s, c)
            out.append(float(self.credit[n] - self.pending[s]))
            s = n
        out.append(float(-self.pending[s]))
        return out

    def score(self, ids):
        total = 0.0
        for v in self.token_scores(ids):
            total += v
        return total

    def compile(self):
        """-> ContextTable, computed once; validated here (the kernels trust the table)."""
        if self._table is None:
            self._table = _concat([self], None)
        return self._table

    def to(self, device):
        """The compiled table on `device`, uploaded once per device."""
        key = str(device)
        if key not in self._device:
            self._device[key] = self.compile().to(device)
        return self._device[key]


def _concat(graphs, graph_of):
    V = graphs[0].V
    for g in graphs:
        if g.V != V:
            raise ValueError("context: the graphs of one batch are over %d and %d tokens" % (V, g.V))
    arc_off, arc_tok, arc_next, drow, dflt, credit, pending, root = [0], [], [], [], [], [], [], []
    n0 = r0 = 0
    for g in graphs:
        root.append(n0)
        for s in range(g.N):
            for c in sorted(g.sparse[s]):
                arc_tok.append(c)
                arc_next.append(g.sparse[s][c] + n0)
            arc_off.append(len(arc_tok))
        drow.append(g.drow + r0)
        dflt.append(g.rows + n0)
        credit.append(g.credit)
        pending.append(g.pending)
        n0 += g.N
        r0 += g.rows.shape[0]
    if n0 >= 2 ** 31 or r0 * V >= 2 ** 31 or len(arc_tok) >= 2 ** 31:
        raise ValueError("context: %d states, %d default rows x %d tokens, %d arcs: each must stay below 2**31"
                         % (n0, r0, V, len(arc_tok)))
    credit64, pending64 = np.concatenate(credit), np.concatenate(pending)
    t = ContextTable(V, np.array(arc_off, dtype=np.int32), np.array(arc_tok, dtype=np.int32), np.array(arc_next, dtype=np.int32),
                     np.concatenate(drow).astype(np.int32), np.concatenate(dflt, axis=0).astype(np.int32),
                     credit64.astype(np.float32), pending64.astype(np.float32), np.array(root, dtype=np.int32),
                     graph_of=graph_of, credit64=credit64, pending64=pending64)
    if t.dflt.min() < 0 or t.dflt.max() >= t.N or (t.A and (t.arc_next.min() < 0 or t.arc_next.max() >= t.N)) or \
            (t.A and (t.arc_tok.min() < 1 or t.arc_tok.max() >= V)) or not np.isfinite(t.credit).all():
        raise ValueError("context: the table holds a state or a token outside its range, or a credit that is not finite")
    return t


class ContextBatch(object):
    """Several graphs in one table and the graph of every utterance: graph_of[b] in 0 .. G-1, or -1 - no biasing for that
    row (bias 0, the state never moves)."""

    def __init__(self, graphs, graph_of):
        self.graphs = list(graphs)
        if not self.graphs or not all(isinstance(g, ContextGraph) for g in self.graphs):
            raise ValueError("context: a batch needs at least one ContextGraph")
        self.graph_of = np.array([int(i) for i in graph_of], dtype=np.int32)
        if self.graph_of.ndim != 1 or self.graph_of.size == 0:
            raise ValueError("context: graph_of lists one graph per utterance")
        if self.graph_of.min() < -1 or self.graph_of.max() >= len(self.graphs):
            raise ValueError("context: graph_of holds an index outside -1 .. %d" % (len(self.graphs) - 1))
        self.V = self.graphs[0].V
        self._table = None
        self._device = {}

    def score(self, b, ids):
        g = int(self.graph_of[b])
        return 0.0 if g < 0 else self.graphs[g].score(ids)

    def compile(self):
        if self._table is None:
            self._table = _concat(self.graphs, self.graph_of)
        return self._table

    def to(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = self.compile().to(device)
        return self._device[key]
