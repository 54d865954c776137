"""A dictionary-based numpy restatement of the CTC prefix beam search (csrc/ctc_beam.hip), parametrised by the
dtype of the logits it is given: float64 is the checker, float32 the yardstick of the device's rounding.  Blank = 0.
Prefixes are tuples of tokens; identity is identity of tuples.

  search(logits, K)        the search over the valid frames -> dict(hyps, scores, gap)
  enumerate_paths(logits)  every labelling's exact CTC log-likelihood by enumeration of all V^T frame paths
  grid() / grid_case()     the shapes, seeds and inputs of the GPU grid; judge() decides it against the restatements
"""
import itertools

import numpy as np

BLANK = 0


def log_probs(logits):
    """[T, V] raw logits of the valid frames -> x[t][v] = logits[t][v] - logsumexp_v logits[t], in the dtype of `logits`."""
    z = np.asarray(logits)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True, dtype=z.dtype)))).astype(z.dtype)


def collapse(tokens):
    out, prev = [], None
    for t in tokens:
        t = int(t)
        if t != BLANK and t != prev:
            out.append(t)
        prev = t
    return tuple(out)


def search(logits, K):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's), beam width K -> dict(hyps: the ranked prefixes
    (tuples), scores: their tot in the dtype, gap: the smallest difference, over all frames, between neighbouring ranks
    1 .. K + 1 of the select (+inf where the lower one is -inf or absent) - how far the search is from another outcome)."""
    z = np.asarray(logits)
    T, V = z.shape
    dt = z.dtype.type
    ninf = dt(-np.inf)
    x = log_probs(z) if T else z
    # the beam: parallel lists in rank order
    prefixes, pb, pnb = [()], [dt(0)], [ninf]
    gap = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            n = len(prefixes)
            pb_a, pnb_a = np.array(pb, dtype=dt), np.array(pnb, dtype=dt)
            tot_a = np.logaddexp(pb_a, pnb_a).astype(dt)
            last = np.array([p[-1] if p else -1 for p in prefixes])
            # stay
            spb = (tot_a + x[t, 0]).astype(dt)
            spnb = np.where(last >= 0, pnb_a + x[t, np.maximum(last, 0)], ninf).astype(dt)
            # extend: [n, V - 1]
            toks = np.arange(1, V)
            ext = (np.where(toks[None, :] == last[:, None], pb_a[:, None], tot_a[:, None]) + x[t, 1:][None, :]).astype(dt)
            # merge: p.c that is the prefix of entry k2 goes into k2's stay, entries k in ascending order
            where = {p: k for k, p in enumerate(prefixes)}
            for k in range(n):
                for k2 in range(n):
                    q = prefixes[k2]
                    if q and len(q) == len(prefixes[k]) + 1 and q[:-1] == prefixes[k]:
                        c = q[-1]
                        spnb[k2] = np.logaddexp(spnb[k2], ext[k, c - 1]).astype(dt)
                        ext[k, c - 1] = ninf
            assert len(where) == n
            stot = np.logaddexp(spb, spnb).astype(dt)
            cand = np.full(K + n * (V - 1), ninf, dtype=dt)
            cand[:n] = stot
            cand[K:] = ext.reshape(-1)
            cand = np.where(np.isnan(cand), ninf, cand)
            order = np.argsort(-cand.astype(np.float64), kind="stable")[:K + 1]      # ties to the lower flat index
            vals = cand[order].astype(np.float64)
            for r in range(min(K, len(vals) - 1)):
                if vals[r] > -np.inf:
                    d = vals[r] - vals[r + 1] if vals[r + 1] > -np.inf else np.inf
                    gap = min(gap, d)
            new_p, new_pb, new_pnb = [], [], []
            for idx in order[:K]:
                if not cand[idx] > -np.inf:
                    break
                if idx < K:
                    new_p.append(prefixes[idx]), new_pb.append(spb[idx]), new_pnb.append(spnb[idx])
                else:
                    k, c = divmod(int(idx) - K, V - 1)
                    new_p.append(prefixes[k] + (c + 1,)), new_pb.append(ninf), new_pnb.append(ext[k, c])
            prefixes, pb, pnb = new_p, new_pb, new_pnb
    scores = np.logaddexp(np.array(pb, dtype=dt), np.array(pnb, dtype=dt)).astype(dt)
    return dict(hyps=prefixes, scores=scores, gap=float(gap))


def enumerate_paths(logits):
    """Every labelling -> its exact CTC log-likelihood (float64), by enumeration of all V^T frame paths."""
    x = log_probs(np.asarray(logits, dtype=np.float64))
    T, V = x.shape
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        sc = float(sum(x[t, k] for t, k in enumerate(path)))
        key = collapse(path)
        mass[key] = np.logaddexp(mass.get(key, -np.inf), sc)
    return mass


# ---------------------------------------------------------------------------------------------------------------------
# The GPU grid (tests/test_ctc_beam_gpu.py) and its decision on the CPU (tests/test_ctc_beam_cpu.py asserts the cap).
GRID_V, GRID_K, GRID_T, GRID_SCALE = (2, 5, 34, 257), (1, 2, 4, 16), (1, 2, 7, 100), (50.0, 1.0)
# shapes on either side of the kernel's switches: K V = 1024 (one wave / four waves), four staged tokens per thread (256
# tokens of one wave, 1024 of four), T K = 4096 history entries (LDS / workspace)
EXTRA = ((64, 16, 7, 1.0), (65, 16, 7, 1.0), (256, 4, 7, 50.0), (260, 3, 7, 1.0), (1024, 2, 3, 50.0), (1030, 2, 3, 1.0),
         (5, 16, 256, 50.0), (5, 16, 257, 50.0))
UNDECIDED_CAP = 0.10


def grid():
    cases = [(V, K, T, s) for V in GRID_V for K in GRID_K for T in GRID_T for s in GRID_SCALE]
    return cases, list(EXTRA)


def case_seed(V, K, T, scale):
    return (V * 1000003 + K * 10007 + T * 101 + int(scale)) % (2 ** 31)


def grid_case(V, K, T, scale):
    """-> (logits float32 [3, T, V + 3] of which [:, :, :V] is the input (ld = V + 3), lens [3]): B = 3 ragged - the full
    length, about half, and no frames at all; NaN behind every utterance and in the padding columns."""
    rs = np.random.RandomState(case_seed(V, K, T, scale))
    z = (rs.normal(0, 1, size=(3, T, V + 3)) * scale).astype(np.float32)
    lens = np.array([T, (T + 1) // 2 if T > 1 else 1, 0], dtype=np.int32)
    z[:, :, V:] = np.nan
    for b in range(3):
        z[b, lens[b]:] = np.nan
    return z, lens


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


_JUDGED = {}


def judge(V, K, T, scale):
    """The restatements of one grid case, computed once per process -> a list over the utterances of dict(ref: the float64
    search, allowance, decisive).  allowance: 4 x the float32 restatement's error against float64 over the hypotheses both
    report (at least 8 ulps of the greatest score magnitude); decisive: both restatements report the same hypotheses in the
    same order and every select of the float64 search separates ranks 1 .. K + 1 by more than 2 x the allowance."""
    key = (V, K, T, scale)
    if key not in _JUDGED:
        z, lens = grid_case(V, K, T, scale)
        out = []
        for b in range(3):
            zb = z[b, :lens[b], :V]
            r64, r32 = search(zb.astype(np.float64), K), search(zb.astype(np.float32), K)
            s32 = dict(zip(r32["hyps"], r32["scores"]))
            errs = [abs(float(s32[h]) - float(s)) for h, s in zip(r64["hyps"], r64["scores"]) if h in s32]
            mag = max([abs(float(s)) for s in r64["scores"]] + [0.0])
            allowance = max(4 * max(errs + [0.0]), 8 * ulp32(mag))
            decisive = r32["hyps"] == r64["hyps"] and r64["gap"] > 2 * allowance
            out.append(dict(ref=r64, allowance=allowance, decisive=bool(decisive)))
        _JUDGED[key] = out
    return _JUDGED[key]
