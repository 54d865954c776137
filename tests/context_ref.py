"""Contextual biasing restated for the tests (context.py, csrc/context.h, csrc/context.hip, csrc/ctc_beam.hip with a context;
DESIGN 4.32).

  brute_state(phrases, seq, space)   the state of the definition without an automaton: the longest suffix of seq that is a
                                     path of the trie (with word_start_only: that begins at a word start)
  brute_score(phrases, boosts, seq, space)   the bias of seq from that matcher, float64
  random_phrases(V, n, seed)         a phrase set with shared prefixes, a phrase that is a prefix of another, one that is a
                                     suffix of another's prefix, single tokens and repeated tokens
  dense(table)                       the whole goto function of a ContextTable, from its sparse form
  walk(table, root, ids, dt)         the scorer: the sum of the deltas in token order in dtype dt, then final
  search_ctx(logits, K, table, root, weight, lm, alpha, beta, eos_term)
                                     ctc_beam_ref.search / ngram_ref.search_lm with the context inside, parametrised by the
                                     dtype of the logits: float64 is the checker, float32 the yardstick of the device's rounding
  grid() / grid_case() / judge()     the shapes, inputs and verdicts of the GPU grid, in the style of ngram_ref

The operations are the kernel's: delta = credit[next] - pending[state] (one subtraction), bias + delta (one addition), the
rank of the search without a context, then + weight * bias (one product, one addition), each rounded on its own in the
dtype; credit and pending are the TABLE's float32 values (the device's inputs, as the logits are)."""
import numpy as np

import __graft_entry__ as entry
import ctc_beam_ref as R
import ngram_ref as N

entry._ensure_paths()
from context import ContextBatch, ContextGraph  # noqa: E402


# ------------------------------------------------------------------------------------------------- the definition, by force
def _paths(phrases):
    return {tuple(p[:i]) for p in phrases for i in range(len(p) + 1)}


def brute_state(phrases, seq, space=None):
    """-> the longest suffix of seq (a tuple) that is a path of the trie - with `space`, one that begins at the start of seq
    or right behind a <space>; None: no such suffix, not even the empty one (inside a word)."""
    paths = _paths(phrases)
    seq = tuple(int(c) for c in seq)
    for i in range(len(seq) + 1):
        if seq[i:] in paths and (space is None or i == 0 or seq[i - 1] == space):
            return seq[i:]
    return None


def _credit(phrases, boosts, path):
    """credit and pending of the trie node `path`, from the definition."""
    if not path:
        return 0.0, 0.0
    ends = {tuple(p) for p in phrases}
    arc = {}
    for p, b in zip(phrases, boosts):
        for i in range(1, len(p) + 1):
            arc[tuple(p[:i])] = max(arc.get(tuple(p[:i]), 0.0), float(b))
    start = max([i for i in range(1, len(path)) if path[:i] in ends] + [0])
    credit = 0.0
    for i in range(start + 1, len(path) + 1):
        credit += arc[path[:i]]
    return credit, (0.0 if path in ends else credit)


def brute_score(phrases, boosts, seq, space=None):
    phrases = [tuple(p) for p in phrases]
    total, prev = 0.0, ()
    for i in range(len(seq)):
        cur = brute_state(phrases, seq[:i + 1], space)
        total += _credit(phrases, boosts, cur or ())[0] - _credit(phrases, boosts, prev or ())[1]
        prev = cur
    return total - _credit(phrases, boosts, prev or ())[1]


def random_phrases(V, n, seed, space=None):
    """-> (phrases, boosts): n random phrases over 1 .. V-1 of 1 .. 4 tokens and, derived from them, a phrase that extends
    another, a proper prefix of one, the inner part of one (a suffix of its prefix), a single token and a repeated token."""
    rs = np.random.RandomState(seed)
    toks = [c for c in range(1, V)]
    out = [tuple(int(toks[rs.randint(len(toks))]) for _ in range(rs.randint(1, 5))) for _ in range(n)]
    long = max(out, key=len)
    if len(long) < 3:
        long = long + tuple(int(toks[rs.randint(len(toks))]) for _ in range(3 - len(long)))
        out.append(long)
    out += [long + (int(toks[rs.randint(len(toks))]),), long[:2], long[1:3], (long[0],), (long[-1], long[-1], long[-1])]
    if space is not None:
        out.append((long[0], space, long[1]))
    phrases = sorted(set(out))
    boosts = [float(rs.choice([0.5, 0.7, 1.5, 2.0, 3.25])) for _ in phrases]
    return [list(p) for p in phrases], boosts


# ------------------------------------------------------------------------------------------------- the table on the host
def dense(table):
    """next int64 [N, V] of a ContextTable from its sparse form (column 0 keeps the state)."""
    nxt = np.array(table.dflt[table.drow], dtype=np.int64)
    for s in range(table.N):
        lo, hi = int(table.arc_off[s]), int(table.arc_off[s + 1])
        nxt[s, table.arc_tok[lo:hi]] = table.arc_next[lo:hi]
    nxt[:, 0] = np.arange(table.N)
    return nxt


def walk(table, root, ids, dt, nxt=None):
    """The scorer on the host -> (the bias in dtype dt, the per-token deltas); root < 0: no biasing."""
    if root < 0:
        return dt(0), [dt(0)] * len(ids)
    cr, pe = table.credit.astype(dt), table.pending.astype(dt)
    s, total, per = int(root), dt(0), []
    for c in ids:
        n = table.next_state(s, int(c)) if nxt is None else int(nxt[s, int(c)])
        d = dt(cr[n] - pe[s])
        total = dt(total + d)
        per.append(d)
        s = n
    return dt(total - pe[s]), per


# ------------------------------------------------------------------------------------------------- the search
def search_ctx(logits, K, table, root, weight, lm=None, alpha=0.0, beta=0.0, eos_term=True, nxt=None):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's); table / root: the context and the root of this
    utterance's graph (< 0: none); lm: an NgramLM or None -> dict(hyps, score: the rank, ctc: tot, lm (with an LM), ctx: the
    bias with final, gap: as ctc_beam_ref.search defines it, over every select and the final ranking)."""
    z = np.asarray(logits)
    T, V = z.shape
    dt = z.dtype.type
    ninf = dt(-np.inf)
    wt = dt(np.float32(weight))
    on = root >= 0
    nxt = dense(table) if nxt is None else nxt
    cr, pe = table.credit.astype(z.dtype), table.pending.astype(z.dtype)
    tab = lm.compile() if lm is not None else None
    a, bt = dt(np.float32(alpha)), dt(np.float32(beta))
    logp = tab.logp.astype(z.dtype) if lm is not None else None
    x = R.log_probs(z) if T else z

    def rank(tot, lmv, n, bias):
        r = tot
        if lm is not None:
            r = ((tot + (a * lmv).astype(z.dtype)).astype(z.dtype) + (bt * np.asarray(n).astype(z.dtype)).astype(z.dtype)).astype(z.dtype)
        return (r + (wt * bias).astype(z.dtype)).astype(z.dtype)

    prefixes, pb, pnb, lms, states = [()], [dt(0)], [ninf], [dt(0)], [tab.start if lm is not None else 0]
    cst, bias = [int(root) if on else 0], [dt(0)]
    gap = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            n = len(prefixes)
            pb_a, pnb_a = np.array(pb, dtype=dt), np.array(pnb, dtype=dt)
            lm_a, st_a = np.array(lms, dtype=dt), np.array(states)
            cs_a, bi_a = np.array(cst), np.array(bias, dtype=dt)
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
            ext_lm = (lm_a[:, None] + logp[st_a][:, 1:]).astype(dt) if lm is not None else np.zeros((n, V - 1), dtype=dt)
            if on:
                ext_cs = nxt[cs_a][:, 1:]
                ext_bi = (bi_a[:, None] + (cr[ext_cs] - pe[cs_a][:, None]).astype(dt)).astype(dt)
            else:
                ext_cs = np.zeros((n, V - 1), dtype=np.int64)
                ext_bi = np.zeros((n, V - 1), dtype=dt)
            cand = np.full(K + n * (V - 1), ninf, dtype=dt)
            cand[:n] = rank(stot, lm_a, len_a, bi_a)
            cand[K:] = rank(ext, ext_lm, (len_a + 1)[:, None], ext_bi).reshape(-1)
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
                    new.append((prefixes[idx], spb[idx], spnb[idx], lms[idx], states[idx], cst[idx], bias[idx]))
                else:
                    k, c = divmod(int(idx) - K, V - 1)
                    new.append((prefixes[k] + (c + 1,), ninf, ext[k, c], ext_lm[k, c],
                                int(tab.nxt[states[k], c + 1]) if lm is not None else 0, int(ext_cs[k, c]), ext_bi[k, c]))
            prefixes, pb, pnb, lms, states, cst, bias = (list(col) for col in zip(*new))
    tot = np.logaddexp(np.array(pb, dtype=dt), np.array(pnb, dtype=dt)).astype(dt)
    lm_a = np.array(lms, dtype=dt)
    if lm is not None and eos_term:
        lm_a = (lm_a + logp[np.array(states), tab.eos]).astype(dt)
    bi_a = np.array(bias, dtype=dt)
    if on:
        bi_a = (bi_a - pe[np.array(cst)]).astype(dt)
    final = rank(tot, lm_a, np.array([len(p) for p in prefixes]), bi_a)
    order = np.argsort(-final.astype(np.float64), kind="stable")
    vals = final[order].astype(np.float64)
    for r in range(len(vals) - 1):
        gap = min(gap, vals[r] - vals[r + 1])
    out = dict(hyps=[prefixes[i] for i in order], score=final[order], ctc=tot[order], ctx=bi_a[order], gap=float(gap))
    if lm is not None:
        out["lm"] = lm_a[order]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The GPU grid (tests/test_context_gpu.py) and its decision on the CPU (tests/test_context_cpu.py asserts the cap).
GRID_V, GRID_K, GRID_T = (5, 34), (1, 4, 16), (1, 7, 40)
# either side of the kernel's switches: K V = 1024 (one wave / four waves) and T K = 4096 history entries (LDS / workspace)
# (the long utterances at a logit scale of 25: at 4 the sixteenth and seventeenth of a beam over four tokens lie closer, after
# 256 frames, than float32 can tell apart, and the restatements alone leave them undecided)
EXTRA = ((64, 16, 7, 4.0), (65, 16, 7, 4.0), (5, 16, 256, 25.0), (5, 16, 257, 25.0))
GRAPH_OF = ((0, 1, 0), (1, -1, 0), (-1, 0, 1))             # per utterance of a case: two graphs, and a row without one
WEIGHTS = (1.0, 0.6, 2.5)
UNDECIDED_CAP = 0.10


def _full(i, V, K, T, scale=None):
    """(V, K, T, scale, with_lm, ctx_weight, variant of GRAPH_OF): the modes, scales and weights cycle over the cases."""
    return (V, K, T, (1.0, 4.0)[(i // 2) % 2] if scale is None else scale, bool(i % 2), WEIGHTS[i % 3], i % 3)


def grid():
    """-> (cases, extra).  Every (V, K, T) of the grid runs with the context alone AND beside the n-gram LM."""
    cases, i = [], 0
    for V in GRID_V:
        for K in GRID_K:
            for T in GRID_T:
                for with_lm in (False, True):
                    c = _full(i, V, K, T)
                    cases.append(c[:4] + (with_lm,) + c[5:])
                    i += 1
    return cases, [_full(i, *c) for i, c in enumerate(EXTRA)]


def quantities(case):
    return ("score", "ctc", "ctx") + (("lm",) if case[4] else ())


_CASES = {}


def grid_case(case):
    """-> (logits, lens: ctc_beam_ref.grid_case's shapes - B = 3 ragged, ld = V + 3, NaN behind every utterance -, the
    ContextBatch of two graphs (the second with word_start_only where V allows a <space>), the n-gram LM or None)."""
    if case not in _CASES:
        V, K, T, scale, with_lm, weight, variant = case
        seed = R.case_seed(V, K, T, scale) + 7 * variant + int(with_lm)
        z, lens = R.grid_case(V, K, T, 1.0)
        z = (z * np.float32(scale)).astype(np.float32)
        space = V - 1 if V > 5 else None
        g0 = ContextGraph(*random_phrases(V, 4 if V <= 5 else 30, seed), V=V)
        p1, b1 = random_phrases(V, 3 if V <= 5 else 20, seed + 1, space)
        g1 = ContextGraph(p1, b1, V=V, word_start_only=space)
        lm = N.random_lm(V, 2 + variant % 2, seed + 2) if with_lm else None
        _CASES[case] = (z, lens, ContextBatch([g0, g1], GRAPH_OF[variant]), lm)
    return _CASES[case]


LM_WEIGHTS = (0.5, 0.25)                                    # alpha, beta of the cases with an LM


_JUDGED = {}


def judge(case):
    """The restatements of one grid case, computed once per process -> a list over the utterances of dict(ref: the float64
    search, allowance: {quantity: 4 x the float32 restatement's error against float64 over the hypotheses both report, at
    least 8 ulps of the quantity's greatest magnitude}, decisive: both restatements report the same hypotheses in the same
    order and every select of the float64 search (the final ranking included) separates ranks 1 .. K + 1 by more than 2 x
    the allowance of the score)."""
    if case not in _JUDGED:
        V, K, T, scale, with_lm, weight, variant = case
        z, lens, batch, lm = grid_case(case)
        table = batch.compile()
        nxt = dense(table)
        out = []
        for b in range(3):
            zb = z[b, :lens[b], :V]
            g = int(batch.graph_of[b])
            root = int(table.root[g]) if g >= 0 else -1
            kw = dict(lm=lm, alpha=LM_WEIGHTS[0], beta=LM_WEIGHTS[1], eos_term=True, nxt=nxt)
            r64 = search_ctx(zb.astype(np.float64), K, table, root, weight, **kw)
            r32 = search_ctx(zb.astype(np.float32), K, table, root, weight, **kw)
            at32 = {h: i for i, h in enumerate(r32["hyps"])}
            allowance = {}
            for q in quantities(case):
                errs = [abs(float(r32[q][at32[h]]) - float(v)) for h, v in zip(r64["hyps"], r64[q]) if h in at32]
                mag = max([abs(float(v)) for v in r64[q]] + [0.0])
                allowance[q] = max(4 * max(errs + [0.0]), 8 * R.ulp32(mag))
            decisive = r32["hyps"] == r64["hyps"] and r64["gap"] > 2 * allowance["score"]
            out.append(dict(ref=r64, allowance=allowance, decisive=bool(decisive)))
        _JUDGED[case] = out
    return _JUDGED[case]
