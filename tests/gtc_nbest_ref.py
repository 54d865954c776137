"""The reference of the device-side n-best graph builder (csrc/gtc_nbest.hip), in numpy and on the host's own
graph code: the admission rule, gtc.nbest_weights over the admitted slots, gtc.Graph.from_nbest per row and gtc._concat.

    admit(hyp, hyp_len, score)                       -> (admitted bool [B, K], dropped int [B])
    reference(hyp, hyp_len, score, V, temperature)   -> Ref: .table (gtc.GraphTable, numpy), .graphs, .batch (GraphBatch),
                                                        .log_weights float64 [B, K], .dropped, .admitted, .lists

The admission rule is stated here with a set of prefixes, not with the kernels' table of longest common prefixes: a slot is
live iff hyp_len >= 0 and score > -inf; live hypotheses are admitted in slot order while the prefix tree stays within
MAX_TRIE = 1023 nodes beyond the root; the first that does not fit and every live slot behind it are dropped."""
import numpy as np

import gtc

MAX_TRIE = (gtc.MAX_NODES - 1) // 2


def admit(hyp, hyp_len, score):
    hyp, hyp_len, score = np.asarray(hyp), np.asarray(hyp_len), np.asarray(score, dtype=np.float64)
    B, K = hyp_len.shape
    admitted, dropped = np.zeros((B, K), dtype=bool), np.zeros(B, dtype=np.int64)
    for b in range(B):
        prefixes, stop = set(), False
        for k in range(K):
            if not (hyp_len[b, k] >= 0 and score[b, k] > -np.inf):
                continue
            if not stop:
                h = tuple(int(c) for c in hyp[b, k, :hyp_len[b, k]])
                new = {h[:n] for n in range(1, len(h) + 1)} - prefixes
                if len(prefixes) + len(new) > MAX_TRIE:
                    stop = True
                else:
                    prefixes |= new
                    admitted[b, k] = True
            if stop:
                dropped[b] += 1
    return admitted, dropped


class Ref(object):
    pass


def reference(hyp, hyp_len, score, V, temperature=1.0):
    hyp, hyp_len, score = np.asarray(hyp), np.asarray(hyp_len), np.asarray(score, dtype=np.float32)
    B, K = hyp_len.shape
    r = Ref()
    r.admitted, r.dropped = admit(hyp, hyp_len, score)
    r.log_weights = gtc.nbest_weights(score.astype(np.float64), np.where(r.admitted, hyp_len, -1), temperature)
    r.graphs, r.lists = [], []
    for b in range(B):
        ks = [k for k in range(K) if r.admitted[b, k]]
        if ks:
            hyps, ws = [[int(c) for c in hyp[b, k, :hyp_len[b, k]]] for k in ks], [float(r.log_weights[b, k]) for k in ks]
        else:                                                   # no slot left: the empty hypothesis at weight 0
            hyps, ws = [[]], [0.0]
        r.lists.append((hyps, ws))
        r.graphs.append(gtc.Graph.from_nbest(hyps, ws, V))
    r.batch = gtc.GraphBatch(r.graphs, range(B))
    r.table = gtc._concat(r.graphs, np.arange(B, dtype=np.int32))
    return r


INT_FIELDS = ("lab", "in_ptr", "in_src", "out_ptr", "out_dst", "order")


def extents(table):
    """name -> the written extent of every array of a table with NN nodes and A arcs"""
    NN, A = int(table.node_off[-1]), int(table.in_ptr[int(table.node_off[-1])])
    ext = dict(node_off=len(table.node_off), lab=NN, start=NN, fin=NN, in_ptr=NN + 1, out_ptr=NN + 1, in_src=A, in_w=A,
               out_dst=A, out_w=A, order=NN)
    return ext


def random_lists(rs, B, K, L, V, dead=0.15, dup=0.2, share=1.0):
    """Random n-best lists in the layout of ops.ctc_beam: tokens in 1 .. V-1 (a small V shares prefixes deeply), -1 padding,
    dead slots (hyp_len -1, score -inf) anywhere, duplicates, lengths 0 .. L; a hypothesis keeps up to `share` of its length
    from the row's common stem."""
    hyp = np.full((B, K, L), -1, dtype=np.int32)
    hyp_len = np.full((B, K), -1, dtype=np.int32)
    score = np.full((B, K), -np.inf, dtype=np.float32)
    for b in range(B):
        stem = rs.randint(1, V, size=L)
        for k in range(K):
            if rs.rand() < dead:
                continue
            n = int(rs.randint(0, L + 1))
            if k and rs.rand() < dup and hyp_len[b, k - 1] >= 0:
                n, h = int(hyp_len[b, k - 1]), hyp[b, k - 1, :hyp_len[b, k - 1]].copy()
            else:
                keep = int(rs.randint(0, int(n * share) + 1))
                h = np.concatenate([stem[:keep], rs.randint(1, V, size=n - keep)])
            hyp[b, k, :n], hyp_len[b, k] = h, n
            score[b, k] = -abs(rs.normal(0, 3))
    return hyp, hyp_len, score
