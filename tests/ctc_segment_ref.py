"""A numpy restatement of CTC segmentation (csrc/ctc_segment.hip), parametrised by the dtype of the logits it is
given like tests/ctc_align_ref.py, whose conventions, recurrence and tie rule it shares: float64 is the checker, float32 the
yardstick of the device's rounding.  Blank = 0.

  segment(logits, utt_labels, free_ends, window)   the Viterbi alignment of the concatenated utterances; with free ends the
                          emission of state 0 and of state S - 1 is 0 at every frame and their frames are -2 in the path.
                          Everything the kernel gives - path, score, first / last, token_logp, and per utterance begin, end,
                          logp, conf - plus the states, fx[t] = x[t][token of frame t] and the runner-up gap, computed with the
                          same (free-end) emissions
  utt_stats(fx, begin, end, window)   the sum and the windowed minimum mean of one utterance, frame after frame
"""
import numpy as np

import ctc_align_ref as R

OUTSIDE = -2


def utt_stats(fx, begin, end, window):
    """-> (logp, conf) of the frames begin .. end: the sum in ascending order; the minimum over the consecutive blocks of
    `window` frames from begin (the last may be shorter) of the block's sum (ascending) divided once by its count."""
    dt = fx.dtype.type
    acc = dt(0)
    for t in range(begin, end + 1):
        acc = dt(acc + fx[t])
    conf = dt(np.inf)
    t0 = begin
    while t0 <= end:
        n = min(window, end - t0 + 1)
        blk = dt(0)
        for t in range(t0, t0 + n):
            blk = dt(blk + fx[t])
        mean = dt(blk / dt(n))
        if mean < conf:
            conf = mean
        t0 += n
    return acc, conf


def infeasible(T, utt_labels):
    L, N = sum(len(u) for u in utt_labels), len(utt_labels)
    out = R.infeasible(T, L)
    out.update(utt_begin=np.full(N, -1, dtype=np.int64), utt_end=np.full(N, -1, dtype=np.int64), utt_logp=np.full(N, -np.inf),
               utt_conf=np.full(N, -np.inf), fx=None)
    return out


def segment(logits, utt_labels, free_ends=True, window=30, with_gap=True):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's), utt_labels a list of label lists (the recording's
    utterances) -> dict(feasible, score, path [T], states [T], first / last / token_logp [L], utt_begin / utt_end / utt_logp
    / utt_conf [N], fx [T], gap).  gap as in ctc_align_ref.align, with the emissions of this call."""
    assert window >= 1
    z = np.asarray(logits)
    T, V = z.shape
    labels = [int(k) for u in utt_labels for k in u]
    L, N = len(labels), len(utt_labels)
    if T == 0 or any(not 1 <= k < V for k in labels):
        return infeasible(T, utt_labels)
    dt = z.dtype
    x = R.log_probs(z)
    ext, skip = R._extended(labels)
    S = len(ext)

    def emit(t):
        e = x[t, ext]
        if free_ends:
            e[0] = 0
            e[S - 1] = 0
        return e

    choice = np.zeros((T, S), dtype=np.int8)
    keep = np.full((T, S), -np.inf, dtype=dt) if with_gap else None
    v = np.full(S, -np.inf, dtype=dt)
    v[:2] = emit(0)[:2]
    if with_gap:
        keep[0] = v
    for t in range(1, T):
        a0, a1, a2 = v, R._shift(v, 1), np.where(skip, R._shift(v, 2), -np.inf).astype(dt)
        best, c = a0.copy(), np.zeros(S, dtype=np.int8)
        m = a1 > best
        best[m], c[m] = a1[m], 1
        m = a2 > best
        best[m], c[m] = a2[m], 2
        v, choice[t] = (best + emit(t)).astype(dt), c
        if with_gap:
            keep[t] = v
    s = S - 2 if S > 1 and v[S - 2] > v[S - 1] else S - 1
    score = v[s]
    if not score > -np.inf:
        return infeasible(T, utt_labels)
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, 0, -1):
        states[t] = s
        s -= int(choice[t, s])
    states[0] = s
    tokens = ext[states]
    path = tokens.copy()
    if free_ends:
        path[(states == 0) | (states == S - 1)] = OUTSIDE
    first, last = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    odd = np.nonzero(states & 1)[0]
    for t in odd:
        i = states[t] >> 1
        if first[i] < 0:
            first[i] = t
        last[i] = t
    fx = x[np.arange(T), tokens]
    out = dict(feasible=True, score=score, path=path, states=states, first=first, last=last,
               token_logp=R.token_sums(x, labels, first, last), fx=fx, gap=np.inf)
    out.update(utterances(fx, first, last, [len(u) for u in utt_labels], window))
    if with_gap:
        g = np.full(S, -np.inf, dtype=dt)
        g[max(S - 2, 0):] = 0
        through = np.full((T, S), -np.inf)
        through[T - 1] = keep[T - 1] + g
        for t in range(T - 2, -1, -1):
            n = g + emit(t + 1)                                # entering state s' at frame t + 1
            n1, n2 = np.full(S, -np.inf, dtype=dt), np.full(S, -np.inf, dtype=dt)
            n1[:-1] = n[1:]
            n2[:-2] = np.where(skip[2:], n[2:], -np.inf)
            g = np.maximum(n, np.maximum(n1, n2))
            through[t] = keep[t] + g
        through[np.arange(T), states] = -np.inf
        out["gap"] = float(score) - float(through.max()) if through.size else np.inf
    return out


def utterances(fx, first, last, counts, window):
    """The per-utterance fields from the frame log-probabilities and the labels' spans; no labels: -1 / -1 / 0 / 0."""
    N = len(counts)
    begin, end = np.full(N, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    logp, conf = np.zeros(N, dtype=fx.dtype), np.zeros(N, dtype=fx.dtype)
    o = 0
    for u, n in enumerate(counts):
        if n:
            begin[u], end[u] = first[o], last[o + n - 1]
            logp[u], conf[u] = utt_stats(fx, int(begin[u]), int(end[u]), window)
        o += n
    return dict(utt_begin=begin, utt_end=end, utt_logp=logp, utt_conf=conf)
