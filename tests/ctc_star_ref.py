"""The star CTC loss (include/asr_hip.h, "Star CTC") restated in torch: the yardstick of csrc/ctc_star.hip.

For labels l_1 .. l_L the lattice has S = 3 L + 2 states - b_0, s_0, then (l_g, b_g, s_g) for g = 1 .. L:

    emission    b_g: x[t][0]      l_g: x[t][l_g]      s_g: nb[t] + penalty
                x = z - logsumexp_v z,   nb[t] = logsumexp_{v >= 1} z[t][v] - logsumexp_v z[t][v]   (a direct log-sum-exp)
    b_g comes from b_g, s_g, and l_g if g >= 1
    s_g comes from s_g, b_g, and l_g if g >= 1
    l_g comes from l_g, b_{g-1}, s_{g-1}, and l_{g-1} if g >= 2 and l_g != l_{g-1}
    frame 0 sits in b_0, s_0 or l_1; the path ends in l_L, b_L or s_L (L = 0: b_0 or s_0)
    nll = -logsumexp over all state paths of the summed emissions

The whole batch advances one frame per step over a padded predecessor table [B, Smax, 4]; the arithmetic runs in the dtype of
the logits (float64: the checker; float32: the yardstick of the allowance) and the gradient comes from autograd.  Dead states
are -inf, and every log-sum-exp is a masked sum about a detached, finite maximum: torch.logsumexp over all -inf inputs returns
a NaN gradient, this one returns an exact zero.  Nothing here imports the package: `states` and `predecessors` are the
definition, and the brute-force enumeration of tests/test_ctc_star_cpu.py reads them."""
import torch

BLANK, LABEL, STAR = "b", "l", "s"


def states(labels):
    """[(kind, g)] in the order of the definition: b_0, s_0, then l_g, b_g, s_g for g = 1 .. L."""
    out = [(BLANK, 0), (STAR, 0)]
    for g in range(1, len(labels) + 1):
        out += [(LABEL, g), (BLANK, g), (STAR, g)]
    return out


def predecessors(labels, kind, g):
    """The states a path may come from into (kind, g), one frame earlier."""
    if kind == BLANK:
        return [(BLANK, g), (STAR, g)] + ([(LABEL, g)] if g >= 1 else [])
    if kind == STAR:
        return [(STAR, g), (BLANK, g)] + ([(LABEL, g)] if g >= 1 else [])
    pre = [(LABEL, g), (BLANK, g - 1), (STAR, g - 1)]
    if g >= 2 and labels[g - 1] != labels[g - 2]:
        pre.append((LABEL, g - 1))
    return pre


def initial(labels):
    return [(BLANK, 0), (STAR, 0)] + ([(LABEL, 1)] if labels else [])


def final(labels):
    L = len(labels)
    return ([(LABEL, L)] if L else []) + [(BLANK, L), (STAR, L)]


def needs_frames(labels):
    """labels + adjacent equal labels: the frames the shortest path takes (at least one: no frame, no path)."""
    return max(1, len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b))


def _mlse(a, dim):
    """log-sum-exp along dim where -inf is a dead entry: -inf (with a zero gradient) when every entry is dead."""
    m = a.detach().amax(dim, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.exp(a - m).sum(dim)
    ok = s > 0
    val = m.squeeze(dim) + torch.log(torch.where(ok, s, torch.ones_like(s)))
    return torch.where(ok, val, torch.full_like(val, float("-inf")))


def star_ctc_nll(z, lens, labels, penalty, zero_infinity=True):
    """z [B, T, V] (float64 or float32; may require grad: frames behind lens[b] get a zero gradient, whatever they hold as
    long as it is finite), lens and labels per utterance (host lists), penalty one float per utterance (<= 0 or -inf) ->
    (nll [B] in z's dtype, feasible: bool [B]).  An infeasible row - fewer frames than labels + adjacent equal labels, no
    frame at all, a label outside [1, V) - has nll +inf, or 0 (zero gradient) with zero_infinity."""
    B, T, V = z.shape
    dt, ninf = z.dtype, float("-inf")
    Smax = max(3 * len(y) + 2 for y in labels)
    idx = torch.zeros(B, Smax, dtype=torch.long)             # the vocabulary entry a state emits (stars: replaced below)
    star = torch.zeros(B, Smax, dtype=torch.bool)
    pred = torch.full((B, Smax, 4), Smax, dtype=torch.long)  # Smax: the dead column of the padded alpha
    init = torch.zeros(B, Smax, dtype=torch.bool)
    fin = torch.zeros(B, Smax, dtype=torch.bool)
    legal = torch.ones(B, dtype=torch.bool)
    for b, y in enumerate(labels):
        y = [int(v) for v in y]
        if any(v < 1 or v >= V for v in y) or int(lens[b]) < 1:
            legal[b] = False
            continue
        st = states(y)
        at = {s: i for i, s in enumerate(st)}
        for i, (kind, g) in enumerate(st):
            idx[b, i] = y[g - 1] if kind == LABEL else 0
            star[b, i] = kind == STAR
            for j, q in enumerate(predecessors(y, kind, g)):
                pred[b, i, j] = at[q]
        for s in initial(y):
            init[b, at[s]] = True
        for s in final(y):
            fin[b, at[s]] = True
    lse = torch.logsumexp(z, -1)
    x = z - lse.unsqueeze(-1)
    nb = torch.logsumexp(z[:, :, 1:], -1) - lse                                     # [B, T]
    pen = torch.tensor([float(p) for p in penalty], dtype=dt)
    emit = x.gather(2, idx.unsqueeze(1).expand(B, T, Smax))
    emit = torch.where(star.unsqueeze(1), (nb + pen.unsqueeze(1)).unsqueeze(-1).expand(B, T, Smax), emit)
    dead = torch.full((B, Smax), ninf, dtype=dt)
    lens_t = torch.tensor([int(n) for n in lens])
    alpha = torch.where(init, emit[:, 0], dead)
    for t in range(1, T):
        padded = torch.cat([alpha, dead[:, :1]], 1)
        came = padded.gather(1, pred.reshape(B, Smax * 4)).reshape(B, Smax, 4)
        new = _mlse(came, 2) + emit[:, t]
        alpha = torch.where((lens_t > t).unsqueeze(1), new, alpha)
    total = _mlse(torch.where(fin & legal.unsqueeze(1), alpha, dead), 1)
    raw = -total
    feasible = torch.isfinite(raw.detach())
    if zero_infinity:
        raw = torch.where(feasible, raw, torch.zeros_like(raw))
    return raw, feasible
