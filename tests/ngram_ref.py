"""The n-gram LM restated for the tests (ngram.py, csrc/ngram.hip, csrc/ctc_beam.hip with an LM).

  backoff_logp(lm, context, c)   an independent float64 backoff evaluator (recursive: the backoffs add from the inside out)
  random_lm(V, order, seed)      a random backoff model over the ids 1 .. V - 1 (<s> = 1, </s> = 2), not normalised: the
                                 kernels do not care, and every path of the automaton is taken (tokens without a unigram,
                                 contexts that are no prefix of a listed n-gram, <s> inside a sequence)
  search_lm(logits, K, lm, alpha, beta, eos_term)
                                 ctc_beam_ref.search with the fused rank, parametrised by the dtype of the logits: float64
                                 is the checker, float32 the yardstick of the device's rounding
  grid() / grid_case() / judge() the shapes, inputs and verdicts of the GPU grid, in the style of ctc_beam_ref

The rank of a candidate is the kernel's, operation for operation: (tot + alpha lm) + beta len, every operation rounded on its
own in the dtype; lm is the sum in token order of the TABLE's float32 values (the device's inputs, as the logits are)."""
import numpy as np

import __graft_entry__ as entry
import ctc_beam_ref as R

entry._ensure_paths()
from ngram import NgramLM  # noqa: E402

BOS, EOS = 1, 2


def backoff_logp(lm, context, c):
    c = int(c)
    if (c,) not in lm.prob:
        return lm.oov_logp
    h = tuple(int(i) for i in context)
    h = h[max(0, len(h) - (lm.order - 1)):] if lm.order > 1 else ()

    def rec(h):
        p = lm.prob.get(h + (c,))
        if p is not None:
            return p
        return lm.backoff.get(h, 0.0) + rec(h[1:])
    return rec(h)


def random_lm(V, order, seed, oov_logp=-30.0):
    rs = np.random.RandomState(seed)
    prob, backoff = {}, {}
    toks = [w for w in range(1, V) if not (V > 5 and w == 3)]          # V > 5: token 3 has no unigram
    for w in toks:
        prob[(w,)] = float(rs.uniform(-6.0, -0.5))
    grams = [(w,) for w in toks]
    for n in range(2, order + 1):
        new = []
        for _ in range(min(4 * V, 200)):
            g = grams[rs.randint(len(grams))] + (toks[rs.randint(len(toks))],)
            if g not in prob:
                prob[g] = float(rs.uniform(-5.0, -0.1))
                backoff[g[:-1]] = float(rs.uniform(-2.0, 0.0))
                new.append(g)
        for _ in range(3):                                               # a history that no listed n-gram is a prefix of
            g = tuple(toks[rs.randint(len(toks))] for _ in range(n))
            if g not in prob:
                prob[g] = float(rs.uniform(-5.0, -0.1))
                new.append(g)
        grams = new or grams
    return NgramLM(order, V, BOS, EOS, prob, backoff, oov_logp=oov_logp)


def walk(table, ids, dt, eos_term=True):
    """The automaton walked on the host: -> (the sum in token order in dtype dt, the per-token values)."""
    state, total, per = table.start, dt(0), []
    for c in list(ids) + ([table.eos] if eos_term else []):
        v = dt(table.logp[state, c])
        total = dt(total + v)
        per.append(v)
        state = int(table.nxt[state, c])
    return total, per


def search_lm(logits, K, lm, alpha, beta, eos_term):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's) -> dict(hyps, score: the rank, ctc: tot, lm: the
    LM's sum (with the end term when eos_term), gap: as ctc_beam_ref.search defines it, over the ranks of every select and of
    the final ranking)."""
    table = lm.compile()
    z = np.asarray(logits)
    T, V = z.shape
    dt = z.dtype.type
    ninf = dt(-np.inf)
    a, bt = dt(np.float32(alpha)), dt(np.float32(beta))
    logp = table.logp.astype(z.dtype)
    x = R.log_probs(z) if T else z

    def rank(tot, lmv, n):
        return ((tot + (a * lmv).astype(z.dtype)).astype(z.dtype) + (bt * np.asarray(n).astype(z.dtype)).astype(z.dtype)).astype(z.dtype)

    prefixes, pb, pnb, lms, states = [()], [dt(0)], [ninf], [dt(0)], [table.start]
    gap = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            n = len(prefixes)
            pb_a, pnb_a = np.array(pb, dtype=dt), np.array(pnb, dtype=dt)
            lm_a, st_a = np.array(lms, dtype=dt), np.array(states)
            len_a = np.array([len(p) for p in prefixes])
            tot_a = np.logaddexp(pb_a, pnb_a).astype(dt)
            last = np.array([p[-1] if p else -1 for p in prefixes])
            spb = (tot_a + x[t, 0]).astype(dt)
            spnb = np.where(last >= 0, pnb_a + x[t, np.maximum(last, 0)], ninf).astype(dt)
            toks = np.arange(1, V)
            ext = (np.where(toks[None, :] == last[:, None], pb_a[:, None], tot_a[:, None]) + x[t, 1:][None, :]).astype(dt)
            for k in range(n):
                for k2 in range(n):
                    q = prefixes[k2]
                    if q and len(q) == len(prefixes[k]) + 1 and q[:-1] == prefixes[k]:
                        c = q[-1]
                        spnb[k2] = np.logaddexp(spnb[k2], ext[k, c - 1]).astype(dt)
                        ext[k, c - 1] = ninf
            stot = np.logaddexp(spb, spnb).astype(dt)
            ext_lm = (lm_a[:, None] + logp[st_a][:, 1:]).astype(dt)
            cand = np.full(K + n * (V - 1), ninf, dtype=dt)
            cand[:n] = rank(stot, lm_a, len_a)
            cand[K:] = rank(ext, ext_lm, (len_a + 1)[:, None]).reshape(-1)
            cand = np.where(np.isnan(cand), ninf, cand)
            order = np.argsort(-cand.astype(np.float64), kind="stable")[:K + 1]
            vals = cand[order].astype(np.float64)
            for r in range(min(K, len(vals) - 1)):
                if vals[r] > -np.inf:
                    gap = min(gap, vals[r] - vals[r + 1] if vals[r + 1] > -np.inf else np.inf)
            new = []
            for idx in order[:K]:
                if not cand[idx] > -np.inf:
                    break
                if idx < K:
                    new.append((prefixes[idx], spb[idx], spnb[idx], lms[idx], states[idx]))
                else:
                    k, c = divmod(int(idx) - K, V - 1)
                    new.append((prefixes[k] + (c + 1,), ninf, ext[k, c], ext_lm[k, c], int(table.nxt[states[k], c + 1])))
            prefixes, pb, pnb, lms, states = (list(col) for col in zip(*new))
    tot = np.logaddexp(np.array(pb, dtype=dt), np.array(pnb, dtype=dt)).astype(dt)
    lm_a = np.array(lms, dtype=dt)
    if eos_term:
        lm_a = (lm_a + logp[np.array(states), table.eos]).astype(dt)
    final = rank(tot, lm_a, np.array([len(p) for p in prefixes]))
    order = np.argsort(-final.astype(np.float64), kind="stable")
    vals = final[order].astype(np.float64)
    for r in range(len(vals) - 1):
        gap = min(gap, vals[r] - vals[r + 1])
    return dict(hyps=[prefixes[i] for i in order], score=final[order], ctc=tot[order], lm=lm_a[order], gap=float(gap))


# ---------------------------------------------------------------------------------------------------------------------
# The GPU grid (tests/test_ngram_gpu.py) and its decision on the CPU (tests/test_ngram_cpu.py asserts the cap).
GRID_V, GRID_K, GRID_T, GRID_SCALE = (3, 5, 34, 257), (1, 2, 4, 16), (1, 2, 7, 100), R.GRID_SCALE
ORDERS, WEIGHTS = (1, 2, 4), ((0.5, 0.0), (2.0, 1.5), (1.0, -1.0))
QUANTITIES = ("score", "ctc", "lm")


def grid():
    """-> (cases, extra): tuples (V, K, T, scale, order, alpha, beta); the order and the weights cycle over the cases."""
    shapes = [(V, K, T, s) for V in GRID_V for K in GRID_K for T in GRID_T for s in GRID_SCALE]
    extra = [c for c in R.EXTRA if c[0] >= 3]

    def full(i, c):
        return c + (ORDERS[i % 3],) + WEIGHTS[(i // 3) % 3]
    return [full(i, c) for i, c in enumerate(shapes)], [full(i + 1, c) for i, c in enumerate(extra)]


def grid_case(V, K, T, scale, order, alpha, beta):
    """-> (logits, lens: ctc_beam_ref.grid_case's - B = 3 ragged, ld = V + 3, NaN behind every utterance -, the LM)."""
    z, lens = R.grid_case(V, K, T, scale)
    return z, lens, random_lm(V, order, R.case_seed(V, K, T, scale) + order)


_JUDGED = {}


def judge(case, eos_term=True):
    """The restatements of one grid case, computed once per process -> a list over the utterances of dict(ref: the float64
    search, allowance: {quantity: 4 x the float32 restatement's error against float64 over the hypotheses both report, at
    least 8 ulps of the quantity's greatest magnitude}, decisive: both restatements report the same hypotheses in the same
    order and every select of the float64 search (the final ranking included) separates ranks 1 .. K + 1 by more than 2 x
    the allowance of the score)."""
    key = tuple(case) + (bool(eos_term),)
    if key not in _JUDGED:
        V, K, T, scale, order, alpha, beta = case
        z, lens, lm = grid_case(*case)
        out = []
        for b in range(3):
            zb = z[b, :lens[b], :V]
            r64 = search_lm(zb.astype(np.float64), K, lm, alpha, beta, eos_term)
            r32 = search_lm(zb.astype(np.float32), K, lm, alpha, beta, eos_term)
            at32 = {h: i for i, h in enumerate(r32["hyps"])}
            allowance = {}
            for q in QUANTITIES:
                errs = [abs(float(r32[q][at32[h]]) - float(v)) for h, v in zip(r64["hyps"], r64[q]) if h in at32]
                mag = max([abs(float(v)) for v in r64[q]] + [0.0])
                allowance[q] = max(4 * max(errs + [0.0]), 8 * R.ulp32(mag))
            decisive = r32["hyps"] == r64["hyps"] and r64["gap"] > 2 * allowance["score"]
            out.append(dict(ref=r64, allowance=allowance, decisive=bool(decisive)))
        _JUDGED[key] = out
    return _JUDGED[key]
