"""Graph CTC (GTC; Moritz et al. 2021): label graphs for ops.gtc_loss (csrc/gtc.hip), built, validated and
compiled on the host.  numpy only; nothing of the GPU path is imported here (the .to methods import torch where they are
called).

  Graph(V, lab, start, fin, arcs)              any graph: node tokens, start / final weights, arcs (m, n, w)
  Graph.ctc(labels, V)                         the plain CTC lattice, 2 L + 1 nodes
  Graph.from_nbest(hyps, log_weights, V)       an n-best list as a prefix tree with a weight per hypothesis
  Graph.from_confusion(slots, V)               a confusion network (alternatives per position, skips) as a sausage
  g.compile() -> GraphTable                    the device form; g.to(device) uploads it once per device
  GraphBatch(graphs, graph_of)                 several graphs in one table, graph_of[b] in 0 .. G-1 per utterance
  nbest_weights(score, hyp_len, temperature)   the log weights of a ranked list from the scores of the search
  DeviceGraphTable                             the table ops.gtc_nbest_graphs builds on the device: sized by
                                               bounds, never read back

The definition (include/asr_hip.h, "Graph CTC").  Node n carries a token lab[n] in [0, V) (0 = blank), a start weight and a
final weight (finite or -inf); an arc (m -> n, w) a finite weight.  Self-loops are ordinary arcs and are never implied; there
are no parallel arcs.  With x[t][v] the frame's log-softmax and T the row's frame count a path n_0 .. n_{T-1} along arcs scores
    start[n_0] + sum_t x[t][lab[n_t]] + sum_{t >= 1} w(n_{t-1}, n_t) + fin[n_{T-1}]
and nll = -logsumexp over all paths: a path sum, not a normalised probability.  No gradient flows to the weights."""
import math

import numpy as np

MAX_NODES = 2047        # ASR_GTC_MAX_NODES
MAX_ARCS = 65536        # ASR_GTC_MAX_ARCS
HEAD_SHIFT = 12         # head entry = (first index in the sorted node list << 12) | run length


def _logaddexp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(min(a, b) - m))


class GraphTable(object):
    """The device form of one or several graphs (asr_gtc_graphs_t).  G graphs concatenated, NN nodes and A arcs in all:
        node_off int32 [G + 1]                         the nodes of graph g; arcs name nodes by their index inside the graph
        lab int32 [NN], start, fin float32 [NN]
        in_ptr int32 [NN + 1], in_src int32 [A], in_w float32 [A]      arcs by destination, sources ascending
        out_ptr int32 [NN + 1], out_dst int32 [A], out_w float32 [A]   arcs by source, destinations ascending
        order int32 [NN]                               per graph its nodes sorted by (token, node)
        head int32 [G, V]                              (first index in order << 12) | run length; 0: no node carries the token
        graph_of int32 [B] or None (every row: graph 0)
    On the host these are numpy arrays, after .to(device) device tensors (the arc arrays hold one unused element when A = 0:
    no tensor is empty)."""
    FIELDS = ("node_off", "lab", "start", "fin", "in_ptr", "in_src", "in_w", "out_ptr", "out_dst", "out_w", "order", "head")

    def __init__(self, V, max_nodes, max_arcs, graph_of=None, **arrays):
        self.V, self.max_nodes, self.max_arcs, self.graph_of = int(V), int(max_nodes), int(max_arcs), graph_of
        for name in self.FIELDS:
            setattr(self, name, arrays[name])
        self.G, self.NN, self.A = int(len(self.node_off)) - 1, int(len(self.lab)), int(self.in_ptr[-1])
        self._rows = {}

    def to(self, device):
        import torch
        t = GraphTable.__new__(GraphTable)
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
        return t

    def rows(self, B):
        """graph_of for a call over B rows (device form): the batch's own, or graph 0 for every row."""
        import torch
        if self.graph_of is not None:
            if int(self.graph_of.numel()) != int(B):
                raise ValueError("gtc: the batch lists a graph for %d utterances, the call has %d" % (self.graph_of.numel(), B))
            return self.graph_of
        if self.G != 1:
            raise ValueError("gtc: a table of %d graphs needs graph_of" % self.G)
        if B not in self._rows:
            self._rows[B] = torch.zeros(int(B), dtype=torch.int32, device=self.lab.device)
        return self._rows[B]


class DeviceGraphTable(GraphTable):
    """A table the device built (ops.gtc_nbest_graphs, csrc/gtc_nbest.hip): one graph per row, graph_of the
    identity.  The tensors are sized by bounds - cap_nodes nodes and cap_arcs arcs per row - and only the device knows how
    much of them is written: NN and A here are those CAPACITIES (B cap_nodes, B cap_arcs), max_nodes and max_arcs the per-row
    bounds the loss kernels dispatch by, and nothing in this class or behind it reads a device value.  Everything behind
    node_off[B] nodes and in_ptr[node_off[B]] arcs is undefined.  dropped int32 [B] (live slots lost to the node limit) and
    log_weights float64 [B, K] (-inf in dead and dropped slots) stay on the device."""

    def __init__(self, V, B, cap_nodes, cap_arcs, device):
        import torch
        self.V, self.G, self.max_nodes, self.max_arcs = int(V), int(B), int(cap_nodes), int(cap_arcs)
        self.cap_nodes, self.cap_arcs = self.max_nodes, self.max_arcs
        self.NN, self.A = self.G * self.cap_nodes, self.G * self.cap_arcs
        i32, f32 = torch.int32, torch.float32
        sizes = dict(node_off=(self.G + 1, i32), lab=(self.NN, i32), start=(self.NN, f32), fin=(self.NN, f32),
                     in_ptr=(self.NN + 1, i32), in_src=(self.A, i32), in_w=(self.A, f32), out_ptr=(self.NN + 1, i32),
                     out_dst=(self.A, i32), out_w=(self.A, f32), order=(self.NN, i32), head=(self.G * self.V, i32))
        for name in self.FIELDS:
            setattr(self, name, torch.empty(sizes[name][0], device=device, dtype=sizes[name][1]))
        self.head = self.head.view(self.G, self.V)
        self.graph_of = torch.empty(self.G, device=device, dtype=i32)
        self.dropped = self.log_weights = None
        self._rows = {}

    def to(self, device):
        import torch
        want = torch.device(device)
        if want.type != self.lab.device.type or (want.index is not None and want.index != self.lab.device.index):
            raise ValueError("gtc: a table built on %s cannot serve %s" % (self.lab.device, device))
        return self


class Graph(object):
    """One label graph.  lab: the token of every node; start, fin: a weight per node, finite or -inf; arcs: (m, n, w) rows
    in any order.  The arcs are kept sorted by (source, destination), so the device sums are a function of the graph and
    not of the insertion order.  ValueError for whatever the kernels would have to trust."""

    def __init__(self, V, lab, start, fin, arcs):
        self.V = int(V)
        if self.V < 2:
            raise ValueError("gtc: V = %d (at least the blank and one token)" % self.V)
        self.lab = np.array([int(c) for c in lab], dtype=np.int64).reshape(-1)
        self.N = N = int(self.lab.size)
        if not 1 <= N <= MAX_NODES:
            raise ValueError("gtc: %d nodes, a graph has 1 .. %d" % (N, MAX_NODES))
        if self.lab.min() < 0 or self.lab.max() >= self.V:
            raise ValueError("gtc: a node carries a token outside 0 .. %d" % (self.V - 1))
        self.start = np.array(start, dtype=np.float64).reshape(-1)
        self.fin = np.array(fin, dtype=np.float64).reshape(-1)
        for name, a in (("start", self.start), ("final", self.fin)):
            if a.size != N:
                raise ValueError("gtc: %d %s weights for %d nodes" % (a.size, name, N))
            if np.isnan(a).any() or (a == np.inf).any():
                raise ValueError("gtc: a %s weight is NaN or +inf (finite or -inf)" % name)
        rows = [(int(m), int(n), float(w)) for m, n, w in arcs]
        if len(rows) > MAX_ARCS:
            raise ValueError("gtc: %d arcs, a graph has at most %d" % (len(rows), MAX_ARCS))
        rows.sort(key=lambda r: (r[0], r[1]))
        self.src = np.array([r[0] for r in rows], dtype=np.int64)
        self.dst = np.array([r[1] for r in rows], dtype=np.int64)
        self.w = np.array([r[2] for r in rows], dtype=np.float64)
        self.A = len(rows)
        if self.A:
            if min(self.src.min(), self.dst.min()) < 0 or max(self.src.max(), self.dst.max()) >= N:
                raise ValueError("gtc: an arc names a node outside 0 .. %d" % (N - 1))
            if not np.isfinite(self.w).all():
                raise ValueError("gtc: an arc weight is not finite")
            key = self.src * N + self.dst
            if (key[1:] == key[:-1]).any():
                i = int(np.nonzero(key[1:] == key[:-1])[0][0])
                raise ValueError("gtc: parallel arcs %d -> %d (join their weights by logaddexp)" % (self.src[i], self.dst[i]))
        self._table = None
        self._device = {}

    # ------------------------------------------------------------------------------------------------------- builders
    @classmethod
    def ctc(cls, labels, V):
        """The plain CTC lattice of `labels` (ids in 1 .. V-1): nodes 0 .. 2L, blanks at the even ones, weight 0 everywhere -
        its value is the CTC negative log-likelihood."""
        labels = [int(c) for c in labels]
        if any(not 0 < c < int(V) for c in labels):
            raise ValueError("gtc: a label outside 1 .. %d (0 is the blank)" % (int(V) - 1))
        L = len(labels)
        N = 2 * L + 1
        lab = [0 if s % 2 == 0 else labels[s // 2] for s in range(N)]
        start = [0.0 if s < 2 else -math.inf for s in range(N)]
        fin = [0.0 if s >= N - 2 else -math.inf for s in range(N)]
        arcs = []
        for s in range(N):
            arcs.append((s, s, 0.0))
            if s >= 1:
                arcs.append((s - 1, s, 0.0))
            if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2]:
                arcs.append((s - 2, s, 0.0))
        return cls(V, lab, start, fin, arcs)

    @classmethod
    def from_nbest(cls, hyps, log_weights, V):
        """An n-best list as a prefix tree: hyps are id lists (ids in 1 .. V-1; an empty list is allowed), log_weights one log
        weight per hypothesis (finite or -inf).  Duplicates are merged, their weights joined by logaddexp.  Node 0 is the
        root's blank; trie node u (breadth first, children in token order, u = 1, 2, ..) gives the token node 2u - 1 and the
        blank node 2u.  Arcs l_u -> l_u, l_u -> b_u, b_u -> b_u, and for each child c of u: b_u -> l_c, and l_u -> l_c where
        the tokens differ; start weight 0 on the root blank and the root's children; final weight log w_k on l_u and b_u of
        the node where hypothesis k ends.  Paths are in bijection with (hypothesis, CTC alignment) pairs, so
        nll = -logsumexp_k (log w_k - nll_ctc(y_k))."""
        hyps = [tuple(int(c) for c in h) for h in hyps]
        logw = [float(w) for w in log_weights]
        if not hyps or len(hyps) != len(logw):
            raise ValueError("gtc: %d hypotheses with %d weights (at least one, one weight each)" % (len(hyps), len(logw)))
        for h, w in zip(hyps, logw):
            if any(not 0 < c < int(V) for c in h):
                raise ValueError("gtc: the hypothesis %r holds an id outside 1 .. %d (0 is the blank)" % (h, int(V) - 1))
            if w != w or w == math.inf:
                raise ValueError("gtc: the log weight of %r is %r (finite or -inf)" % (h, w))
        kids, tok, end = [{}], [0], [-math.inf]
        for h, w in zip(hyps, logw):
            node = 0
            for c in h:
                if c not in kids[node]:
                    kids[node][c] = len(kids)
                    kids.append({})
                    tok.append(c)
                    end.append(-math.inf)
                node = kids[node][c]
            end[node] = _logaddexp(end[node], w)
        order = [0]
        for s in order:
            order.extend(kids[s][c] for c in sorted(kids[s]))
        number = {s: i for i, s in enumerate(order)}
        if 2 * len(order) - 1 > MAX_NODES:
            raise ValueError("gtc: the prefix tree has %d nodes, a graph at most %d" % (2 * len(order) - 1, MAX_NODES))

        def l_(s):
            return 2 * number[s] - 1

        def b_(s):
            return 2 * number[s]
        N = 2 * len(order) - 1
        lab, start, fin, arcs = [0] * N, [-math.inf] * N, [-math.inf] * N, []
        start[0] = 0.0
        for s in order:
            fin[b_(s)] = end[s]
            arcs.append((b_(s), b_(s), 0.0))
            if s != 0:
                lab[l_(s)] = tok[s]
                fin[l_(s)] = end[s]
                arcs.append((l_(s), l_(s), 0.0))
                arcs.append((l_(s), b_(s), 0.0))
            for c, k in kids[s].items():
                arcs.append((b_(s), l_(k), 0.0))
                if s == 0:
                    start[l_(k)] = 0.0
                elif tok[s] != c:
                    arcs.append((l_(s), l_(k), 0.0))
        return cls(V, lab, start, fin, arcs)

    @classmethod
    def from_confusion(cls, slots, V):
        """A confusion network: slots is a list of positions, each a list of (token or None, log weight) alternatives; None
        means "skip this position" (several skips of a position join by logaddexp).  One blank node per boundary (P + 1 of
        them, node p for the boundary in front of position p), then one node per token alternative in slot order.  A token of
        position p goes to itself and to the blank of boundary p + 1; that blank, and the token itself where the tokens
        differ, go to the token nodes of every later position reachable over skippable positions, the skip weights and the
        alternative's own weight on the arc.  Start weights reach the positions in front of which everything can be skipped,
        final weights carry the skips behind.  The value is -logsumexp over all choice sequences of (the sum of the chosen
        weights - nll_ctc(the tokens of the choice))."""
        P = len(slots)
        skip, toks = [], []
        for p, slot in enumerate(slots):
            s, ts = -math.inf, []
            if not slot:
                raise ValueError("gtc: position %d of the confusion network offers nothing" % p)
            for c, w in slot:
                w = float(w)
                if not math.isfinite(w):
                    raise ValueError("gtc: the log weight %r at position %d is not finite" % (w, p))
                if c is None:
                    s = _logaddexp(s, w)
                else:
                    if not 0 < int(c) < int(V):
                        raise ValueError("gtc: the token %r at position %d is outside 1 .. %d" % (c, p, int(V) - 1))
                    ts.append((int(c), w))
            skip.append(s)
            toks.append(ts)
        N = P + 1 + sum(len(ts) for ts in toks)
        if N > MAX_NODES:
            raise ValueError("gtc: the confusion network has %d nodes, a graph at most %d" % (N, MAX_NODES))
        node, n = [], P + 1
        for ts in toks:
            node.append(list(range(n, n + len(ts))))
            n += len(ts)
        lab, start, fin, arcs = [0] * N, [-math.inf] * N, [-math.inf] * N, []
        tail = [0.0] * (P + 1)                                  # the skips of positions p .. P-1, -inf where one cannot be skipped
        for p in range(P - 1, -1, -1):
            tail[p] = tail[p + 1] + skip[p] if skip[p] > -math.inf and tail[p + 1] > -math.inf else -math.inf

        def reach(p):
            """(q, the skips of positions p .. q-1) for every position q >= p that can follow boundary p"""
            acc, q = 0.0, p
            while q < P:
                yield q, acc
                if skip[q] == -math.inf:
                    return
                acc += skip[q]
                q += 1
        start[0], fin[0] = 0.0, tail[0]
        for q, acc in reach(0):
            for (c, w), k in zip(toks[q], node[q]):
                start[k] = acc + w
        for p in range(P + 1):
            arcs.append((p, p, 0.0))
            if p >= 1:
                fin[p] = tail[p]
        for p in range(P):
            for (c, w), k in zip(toks[p], node[p]):
                lab[k], fin[k] = c, tail[p + 1]
                arcs.append((k, k, 0.0))
                arcs.append((k, p + 1, 0.0))
        for p in range(P):                                      # out of boundary p's blank and of position p-1's tokens
            for q, acc in reach(p):
                for (c, w), k in zip(toks[q], node[q]):
                    arcs.append((p, k, acc + w))
                    for (c0, _), k0 in (zip(toks[p - 1], node[p - 1]) if p >= 1 else ()):
                        if c0 != c:
                            arcs.append((k0, k, acc + w))
        return cls(V, lab, start, fin, arcs)

    # ----------------------------------------------------------------------------------------------------- device form
    def dense(self):
        """-> (W float64 [N, N] with W[m, n] the weight of m -> n and -inf where there is no arc)."""
        W = np.full((self.N, self.N), -np.inf)
        W[self.src, self.dst] = self.w
        return W

    def compile(self):
        """-> GraphTable, computed once."""
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
            raise ValueError("gtc: the graphs of one batch are over %d and %d tokens" % (V, g.V))
    node_off, in_ptr, out_ptr = [0], [0], [0]
    lab, start, fin, in_src, in_w, out_dst, out_w, order, head = [], [], [], [], [], [], [], [], []
    a0 = 0
    for g in graphs:
        node_off.append(node_off[-1] + g.N)
        lab.append(g.lab)
        start.append(g.start)
        fin.append(g.fin)
        # arcs are sorted by (source, destination): the out lists as they stand, the in lists by a stable sort on the destination
        by_dst = np.argsort(g.dst, kind="stable")
        out_dst.append(g.dst)
        out_w.append(g.w)
        in_src.append(g.src[by_dst])
        in_w.append(g.w[by_dst])
        out_ptr.extend((a0 + np.cumsum(np.bincount(g.src, minlength=g.N))).tolist())
        in_ptr.extend((a0 + np.cumsum(np.bincount(g.dst, minlength=g.N))).tolist())
        a0 += g.A
        o = np.argsort(g.lab, kind="stable")
        order.append(o)
        h = np.zeros(V, dtype=np.int64)
        sorted_lab = g.lab[o]
        first = np.searchsorted(sorted_lab, np.arange(V), side="left")
        count = np.searchsorted(sorted_lab, np.arange(V), side="right") - first
        h[count > 0] = (first[count > 0] << HEAD_SHIFT) | count[count > 0]
        head.append(h)
    if node_off[-1] >= 2 ** 31 or a0 >= 2 ** 31 or len(graphs) * V >= 2 ** 31:
        raise ValueError("gtc: %d nodes, %d arcs, %d graphs x %d tokens: each must stay below 2**31"
                         % (node_off[-1], a0, len(graphs), V))
    i32, f32 = np.int32, np.float32
    return GraphTable(V, max(g.N for g in graphs), max(g.A for g in graphs), graph_of=graph_of,
                      node_off=np.array(node_off, dtype=i32), lab=np.concatenate(lab).astype(i32),
                      start=np.concatenate(start).astype(f32), fin=np.concatenate(fin).astype(f32),
                      in_ptr=np.array(in_ptr, dtype=i32), in_src=np.concatenate(in_src).astype(i32),
                      in_w=np.concatenate(in_w).astype(f32), out_ptr=np.array(out_ptr, dtype=i32),
                      out_dst=np.concatenate(out_dst).astype(i32), out_w=np.concatenate(out_w).astype(f32),
                      order=np.concatenate(order).astype(i32), head=np.stack(head).astype(i32))


class GraphBatch(object):
    """Several graphs in one table and the graph of every utterance: graph_of[b] in 0 .. G-1; rows may share a graph."""

    def __init__(self, graphs, graph_of):
        self.graphs = list(graphs)
        if not self.graphs or not all(isinstance(g, Graph) for g in self.graphs):
            raise ValueError("gtc: a batch needs at least one Graph")
        self.graph_of = np.array([int(i) for i in graph_of], dtype=np.int32)
        if self.graph_of.ndim != 1 or self.graph_of.size == 0:
            raise ValueError("gtc: graph_of lists one graph per utterance")
        if self.graph_of.min() < 0 or self.graph_of.max() >= len(self.graphs):
            raise ValueError("gtc: graph_of holds an index outside 0 .. %d" % (len(self.graphs) - 1))
        self.V = self.graphs[0].V
        self._table = None
        self._device = {}

    def compile(self):
        if self._table is None:
            self._table = _concat(self.graphs, self.graph_of)
        return self._table

    def to(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = self.compile().to(device)
        return self._device[key]


def nbest_weights(score, hyp_len, temperature=1.0):
    """The log weights of a ranked n-best list: per row the log-softmax of temperature * score over the row's live slots
    (hyp_len >= 0 and a score above -inf); -inf in the others.  score, hyp_len: [B, K] arrays as ops.ctc_beam returns them
    (read to the host).  -> float64 [B, K].  temperature 0 weighs the live hypotheses equally; a row without a live slot
    keeps -inf throughout."""
    score = np.asarray(score, dtype=np.float64)
    live = (np.asarray(hyp_len) >= 0) & (score > -np.inf)
    t = float(temperature)
    if not (t >= 0.0 and math.isfinite(t)):
        raise ValueError("gtc: the temperature must be finite and >= 0, got %r" % (temperature,))
    if score.ndim != 2 or live.shape != score.shape:
        raise ValueError("gtc: score and hyp_len are [B, K] arrays of one shape")
    s = np.where(live, t * np.where(live, score, 0.0), -np.inf)
    out = np.full(score.shape, -np.inf)
    for b in range(score.shape[0]):
        if live[b].any():
            m = s[b].max()
            out[b] = s[b] - (m + math.log(np.exp(s[b] - m).sum()))
    return out
