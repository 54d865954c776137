"""A numpy restatement of CTC forced alignment and best-path decoding (csrc/ctc_align.hip), parametrised by the
dtype of the logits it is given: float64 is the checker, float32 the yardstick of the device's rounding.  Blank = 0.

  align(logits, labels)   the Viterbi recurrence over the extended labels l' = (0, l_1, 0, ..., l_L, 0) with the contract's
                          tie rule (a predecessor replaces the current best only when strictly greater, tried in the order
                          stay, s-1, s-2; at the end S-1 unless S-2 is strictly greater), the backtrace, the spans and token
                          sums, and the runner-up gap
  best_path(logits)       frame argmax (NaN never wins, ties to the lowest index), repeats collapsed, blanks dropped
"""
import numpy as np

BLANK = 0


def log_probs(logits):
    """[T, V] raw logits of the valid frames -> x[t][v] = logits[t][v] - logsumexp_v logits[t], in the dtype of `logits`."""
    z = np.asarray(logits)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True, dtype=z.dtype)))).astype(z.dtype)


def collapse(tokens):
    """Frame tokens -> labels: repeats collapsed, then blanks dropped."""
    out, prev = [], None
    for t in tokens:
        t = int(t)
        if t != BLANK and t != prev:
            out.append(t)
        prev = t
    return out


def _extended(labels):
    ext = np.zeros(2 * len(labels) + 1, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(len(ext), dtype=bool)                    # s odd, s >= 3 and l'_s != l'_{s-2}
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, skip


def _shift(a, n):
    out = np.full_like(a, -np.inf)
    out[n:] = a[:len(a) - n]
    return out


def infeasible(T, L):
    return dict(feasible=False, score=-np.inf, path=np.full(T, -1, dtype=np.int64), states=None,
                first=np.full(L, -1, dtype=np.int64), last=np.full(L, -1, dtype=np.int64),
                token_logp=np.full(L, -np.inf), gap=np.inf)


def align(logits, labels, with_gap=True):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's), labels a list of ints -> dict(feasible, score,
    path [T] (the token per frame), states [T], first / last [L], token_logp [L], gap).  gap: with g the backward
    max-scores, score - max over the cells (t, s) NOT on the best path of (v + g)[t][s] - the score difference to the best
    path that differs anywhere (+inf: there is no other path)."""
    z = np.asarray(logits)
    T, V = z.shape
    L = len(labels)
    if T == 0 or any(not 1 <= int(k) < V for k in labels):
        return infeasible(T, L)
    dt = z.dtype
    x = log_probs(z)
    ext, skip = _extended([int(k) for k in labels])
    S = len(ext)
    e = x[:, ext]                                              # [T, S] emissions of the states
    v = np.full((T, S), -np.inf, dtype=dt)
    choice = np.zeros((T, S), dtype=np.int8)
    v[0, :2] = e[0, :2]
    for t in range(1, T):
        a0, a1, a2 = v[t - 1], _shift(v[t - 1], 1), np.where(skip, _shift(v[t - 1], 2), -np.inf).astype(dt)
        best, c = a0.copy(), np.zeros(S, dtype=np.int8)
        m = a1 > best
        best[m], c[m] = a1[m], 1
        m = a2 > best
        best[m], c[m] = a2[m], 2
        v[t], choice[t] = (best + e[t]).astype(dt), c
    s = S - 2 if S > 1 and v[T - 1, S - 2] > v[T - 1, S - 1] else S - 1
    score = v[T - 1, s]
    if not score > -np.inf:
        return infeasible(T, L)
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, 0, -1):
        states[t] = s
        s -= int(choice[t, s])
    states[0] = s
    path = ext[states]
    first, last = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    for t in range(T):
        if states[t] & 1:
            i = states[t] >> 1
            if first[i] < 0:
                first[i] = t
            last[i] = t
    out = dict(feasible=True, score=score, path=path, states=states, first=first, last=last,
               token_logp=token_sums(x, labels, first, last), gap=np.inf)
    if with_gap:
        g = np.full((T, S), -np.inf, dtype=dt)
        g[T - 1, max(S - 2, 0):] = 0
        for t in range(T - 2, -1, -1):
            n = g[t + 1] + e[t + 1]                            # entering state s' at frame t + 1
            n1, n2 = np.full(S, -np.inf, dtype=dt), np.full(S, -np.inf, dtype=dt)
            n1[:-1] = n[1:]
            n2[:-2] = np.where(skip[2:], n[2:], -np.inf)
            g[t] = np.maximum(n, np.maximum(n1, n2))
        through = (v + g).astype(np.float64)
        through[np.arange(T), states] = -np.inf
        out["gap"] = float(score) - float(through.max()) if through.size else np.inf
    return out


def token_sums(x, labels, first, last):
    """token_logp[i] = sum_{t = first_i .. last_i} x[t][l_i], added one frame after the other in x's dtype."""
    out = np.zeros(len(labels), dtype=x.dtype)
    for i, k in enumerate(labels):
        acc = x.dtype.type(0)
        for t in range(int(first[i]), int(last[i]) + 1):
            acc = x.dtype.type(acc + x[t, int(k)])
        out[i] = acc
    return out


def path_score(x, path):
    """The score of a frame path under log-probabilities x [T, V], frame after frame in x's dtype."""
    acc = x.dtype.type(0)
    for t, k in enumerate(path):
        acc = x.dtype.type(acc + x[t, int(k)])
    return acc


def best_path(logits):
    """logits [T, V] of the valid frames -> (frame_tok [T], ids): NaN never wins, ties go to the lowest index (a frame
    without any number above -inf gives 0)."""
    z = np.asarray(logits)
    if z.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), []
    frame_tok = np.where(np.isnan(z), -np.inf, z).argmax(axis=-1)
    return frame_tok, collapse(frame_tok)
