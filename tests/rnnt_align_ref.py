"""Restatements of the transducer forced alignment (csrc/rnnt_align.hip) that need no GPU.

    viterbi          numpy, in the dtype asked for: float64 is the reference; float32 - the same recurrence in the kernel's
                     operation order (lse = max + log(sum exp(z - max)), lp = z - lse, candidate = v + lp, the label arc taken
                     only when STRICTLY greater) - is the yardstick of the allowance
    brute_force      every alignment path enumerated
    allowance        the project's usual one: max(4 x the float32 restatement's error, 8 x 2^-24 x the tensor's scale)
    utterance, case  the inputs of the GPU grid, made here so that the CPU test can hold that every case is decisive
    decisive         whether the float64 path of every utterance of a case is beyond the reach of float32 rounding

One utterance at a time: logits [T, U + 1, V] over the utterance's own lattice, labels [U] in [1, V), blank = 0."""
import functools
import itertools

import numpy as np

import rnnt_ref

SMALL = ((1, 0), (1, 1), (7, 0), (2, 6), (5, 3))
LARGE = ((64, 63), (65, 64), (130, 129), (3, 257))
VOCABS = (3, 34, 65)
# every lattice alone, and in a ragged batch of five
BATCHES = (SMALL, LARGE + ((5, 3),))
GRID = tuple(((lat,), V) for V in VOCABS for lat in SMALL + LARGE) + tuple((lats, V) for V in VOCABS for lats in BATCHES)

# (T, U, V) -> the seed of the utterance's logits and labels where seed 0 leaves a grid case undecided
# (tests/test_rnnt_align_cpu.py holds that every case is decisive with these)
SEEDS = {(130, 129, 65): 1}            # seed 0: gap 0.00429 against 2 x 0.00213 in the batch - decided by a hair's breadth


def emissions(logits, labels, dt):
    """-> (lp_0 [T, U + 1], lp_{y_{u+1}} [T, U + 1] with -inf at u = U)."""
    z = np.asarray(logits).astype(dt)
    T, U1, _ = z.shape
    lse = rnnt_ref._lse_rows(z, dt)
    lb = (z[:, :, 0] - lse).astype(dt)
    ly = np.full((T, U1), -np.inf, dt)
    for u in range(U1 - 1):
        ly[:, u] = z[:, u, int(labels[u])] - lse[:, u]
    return lb, ly


def viterbi(logits, labels, dt=np.float64):
    """-> dict(score, emit_frame [U], token_logp [U], frame_labels [T], blank_logp [T], gap): the best alignment of one
    utterance.  A tie goes to the blank predecessor (t - 1, u).  gap: the smallest |difference| of the two candidates over
    the nodes of the returned path that have two predecessors (inf: none has)."""
    lb, ly = emissions(logits, labels, dt)
    T, U1 = lb.shape
    U = U1 - 1
    v = np.zeros((T, U1), dt)
    from_label = np.zeros((T, U1), bool)
    diff = np.full((T, U1), np.inf)
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            if t == 0:
                v[t, u], from_label[t, u] = dt(v[t, u - 1] + ly[t, u - 1]), True
            elif u == 0:
                v[t, u] = dt(v[t - 1, u] + lb[t - 1, u])
            else:
                cb, cy = dt(v[t - 1, u] + lb[t - 1, u]), dt(v[t, u - 1] + ly[t, u - 1])
                from_label[t, u] = cy > cb
                v[t, u] = cy if cy > cb else cb
                diff[t, u] = abs(float(cy) - float(cb))
    emit = np.zeros(U, np.int32)
    frame_labels = np.zeros(T, np.int32)
    t, u, gap = T - 1, U, np.inf
    frame_labels[t] = u
    while t > 0 or u > 0:
        gap = min(gap, diff[t, u])
        if from_label[t, u]:
            emit[u - 1] = t
            u -= 1
        else:
            t -= 1
            frame_labels[t] = u
    return dict(score=dt(v[T - 1, U] + lb[T - 1, U]), emit_frame=emit,
                token_logp=np.asarray([ly[emit[i], i] for i in range(U)], dt), frame_labels=frame_labels,
                blank_logp=np.asarray([lb[t, frame_labels[t]] for t in range(T)], dt), gap=float(gap))


def brute_force(logits, labels):
    """-> (the best score, the emit frames of a best path, the number of paths that attain it), float64, every path
    enumerated: T - 1 blanks and U labels in any order, then the closing blank."""
    lb, ly = emissions(logits, labels, np.float64)
    T, U1 = lb.shape
    U = U1 - 1
    best, best_emit, n_best = -np.inf, None, 0
    for where in itertools.combinations(range(T - 1 + U), U):       # the moves that emit a label
        t = u = 0
        s, emit = 0.0, []
        for m in range(T - 1 + U):
            if m in where:
                s += ly[t, u]
                emit.append(t)
                u += 1
            else:
                s += lb[t, u]
                t += 1
        s += lb[T - 1, U]
        if s > best:
            best, best_emit, n_best = s, emit, 1
        elif s == best:
            n_best += 1
    return best, best_emit, n_best


def allowance(f32, ref):
    f32, ref = np.asarray(f32, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    err32 = float(np.abs(f32 - ref).max()) if ref.size else 0.0
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return max(4.0 * err32, 8.0 * 2.0 ** -24 * scale)


@functools.lru_cache(maxsize=None)
def utterance(T, U, V, seed=None):
    """Logits uniform in (-3, 3) [T, U + 1, V] float32 and labels uniform in [1, V), with the float64 and the float32
    restatement, computed once (the grid's cases share them: a row alone and the same row in a batch have the same inputs)."""
    seed = SEEDS.get((T, U, V), 0) if seed is None else seed
    rs = np.random.RandomState(5000 + 131 * seed + 7 * V + 3 * T + U)
    z = rs.uniform(-3, 3, (T, U + 1, V)).astype(np.float32)
    y = rs.randint(1, V, U).astype(np.int64)
    return dict(T=T, U=U, V=V, z=z, y=y, ref=viterbi(z, y, np.float64), f32=viterbi(z, y, np.float32))


def case(lattices, V):
    """The utterances of a grid case -> dict(lattices, V, utts, allow: the allowance of each float tensor of the call - all
    utterances together, as tests/test_rnnt_gpu.py takes it)."""
    utts = [utterance(t, u, V) for t, u in lattices]
    allow = {}
    for name in ("score", "token_logp", "blank_logp"):
        cat = lambda key: np.concatenate([np.ravel(x[key][name]).astype(np.float64) for x in utts])      # noqa: E731
        allow[name] = allowance(cat("f32"), cat("ref"))
    return dict(lattices=tuple(lattices), V=V, utts=utts, allow=allow)


def decisive(c):
    """At every node of every utterance's float64 best path that has two predecessors, the two candidates differ by more than
    twice the allowance of the case's scores: no float32 evaluation within the allowance can choose otherwise."""
    return all(x["ref"]["gap"] > 2.0 * c["allow"]["score"] for x in c["utts"])
