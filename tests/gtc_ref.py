"""The graph CTC loss (include/asr_hip.h, "Graph CTC") restated in torch: the yardstick of csrc/gtc.hip.

A graph is anything with  lab (N tokens), start, fin (N weights, finite or -inf)  and  dense() -> W [N, N] with W[m, n] the
weight of the arc m -> n and -inf where there is none.  With x = z - logsumexp_v z a path n_0 .. n_{T-1} scores

    start[n_0] + sum_t x[t][lab[n_t]] + sum_{t >= 1} W[n_{t-1}, n_t] + fin[n_{T-1}]

and nll = -logsumexp over all paths.  One row at a time, a log-space forward over the dense transition matrix; the arithmetic
runs in the dtype of the logits (float64: the checker; float32: the yardstick of the allowance) and the gradient comes from
autograd.  Dead nodes are -inf, and every log-sum-exp is a masked sum about a detached, finite maximum (ctc_star_ref's:
torch.logsumexp over all -inf inputs returns a NaN gradient, this one an exact zero).  Nothing here imports the package."""
import itertools
import math

import numpy as np
import torch


def _mlse(a, dim):
    """log-sum-exp along dim where -inf is a dead entry: -inf (with a zero gradient) when every entry is dead."""
    m = a.detach().amax(dim, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.exp(a - m).sum(dim)
    ok = s > 0
    val = m.squeeze(dim) + torch.log(torch.where(ok, s, torch.ones_like(s)))
    return torch.where(ok, val, torch.full_like(val, float("-inf")))


def gtc_nll(z, lens, graphs, zero_infinity=True):
    """z [B, T, V] (float64 or float32; may require grad: frames behind lens[b] get a zero gradient whatever they hold),
    lens per utterance, graphs one per utterance -> (nll [B] in z's dtype, feasible: bool [B]).  A row with no path of finite
    score, or with no frame, has nll +inf, or 0 with zero_infinity; its gradient is zero either way (the infeasible value
    is a constant)."""
    B, T, V = z.shape
    dt = z.dtype
    out, feasible = [], []
    for b in range(B):
        g, n = graphs[b], int(lens[b])
        if n < 1:
            out.append(torch.tensor(float("inf"), dtype=dt))
            continue
        zb = z[b, :n]
        x = zb - torch.logsumexp(zb, -1, keepdim=True)
        lab = torch.as_tensor(np.asarray(g.lab), dtype=torch.long)
        emit = x[:, lab]                                                     # [n, N]
        W = torch.as_tensor(np.asarray(g.dense()), dtype=dt)
        alpha = torch.as_tensor(np.asarray(g.start), dtype=dt) + emit[0]
        for t in range(1, n):
            alpha = _mlse(alpha.unsqueeze(1) + W, 0) + emit[t]
        out.append(-_mlse(alpha + torch.as_tensor(np.asarray(g.fin), dtype=dt), 0))
    raw = torch.stack(out)
    feasible = torch.isfinite(raw.detach())
    dead = torch.zeros_like(raw) if zero_infinity else torch.full_like(raw, float("inf"))
    return torch.where(feasible, raw, dead), feasible


def brute_force(x, g):
    """-logsumexp over every node sequence of the graph, enumerated (float64; x [T, V] log-probabilities as nested lists or
    an array).  For graphs of a few nodes and frames only."""
    x = np.asarray(x, dtype=np.float64)
    T, N, W = x.shape[0], len(g.lab), np.asarray(g.dense(), dtype=np.float64)
    total = -math.inf
    for path in itertools.product(range(N), repeat=T):
        s = float(g.start[path[0]]) + float(g.fin[path[-1]])
        for t, n in enumerate(path):
            s += x[t, int(g.lab[n])]
            if t:
                s += W[path[t - 1], n]
        if s > -math.inf:
            total = s if total == -math.inf else max(total, s) + math.log1p(math.exp(-abs(total - s)))
    return -total
