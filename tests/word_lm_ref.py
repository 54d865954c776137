"""The word-level LM and lexicon restated for the tests (word_lm.py, csrc/word_lm.h, csrc/word_lm.hip, csrc/ctc_beam.hip with
a word LM), in the style of tests/ngram_ref.py.

  backoff_logp(lm, context, w)   an independent float64 backoff evaluator over word ids (recursive)
  row_score(wlm, ids, eos_term)  the float64 score of a token row by that evaluator, and its number of words
  random_word_lm(V, order, seed, extra_words)
                                 a random lexicon over the letters 1 .. V - 2 (<space> = V - 1) and a random backoff model
                                 over its word ids, not normalised: words without a unigram, <unk> with and without one,
                                 contexts that are no prefix of a listed n-gram
  walk(table, ids, dt, eos_term) the kernels' walk of a token row over the TABLE's float32 values, in dtype dt
  search_wlm(logits, K, wlm, alpha, beta, eos_term, lexicon_only)
                                 ctc_beam_ref.search with the fused rank, parametrised by the dtype of the logits: float64
                                 is the checker, float32 the yardstick of the device's rounding
  grid() / grid_case() / judge() the shapes, inputs and verdicts of the GPU grid

The rank of a candidate is the kernel's, operation for operation: (tot + alpha lm) + beta n_words, every operation rounded
on its own in the dtype; lm is the sum in word order of the table's lookups (the device's inputs, as the logits are)."""
import numpy as np

import __graft_entry__ as entry
import ctc_beam_ref as R

entry._ensure_paths()
from ngram import NgramLM  # noqa: E402
from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_UNK, W_FIRST  # noqa: E402


def backoff_logp(lm, context, w):
    """ln p(w | context) of the NgramLM over word ids, by recursion: the backoffs add from the inside out."""
    w = int(w)
    if (w,) not in lm.prob:
        return lm.oov_logp
    h = tuple(int(i) for i in context)
    h = h[max(0, len(h) - (lm.order - 1)):] if lm.order > 1 else ()

    def rec(h):
        p = lm.prob.get(h + (w,))
        if p is not None:
            return p
        return lm.backoff.get(h, 0.0) + rec(h[1:])
    return rec(h)


def split(ids, space):
    """tests/wer_ref.py::words with an empty skip table, spelled out once more."""
    out, cur = [], []
    for t in ids:
        if int(t) == space:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(int(t))
    return out + ([tuple(cur)] if cur else [])


def row_score(wlm, ids, eos_term=True):
    """-> (the float64 score of a token row, its number of words); after a word without a unigram the context is empty."""
    lm = wlm.lm
    at = {sp: wlm.word_ids[i] for sp, i in wlm.lexicon.index.items()}
    ctx, total, words = (W_BOS,), 0.0, split(ids, wlm.space)
    for w in [at.get(sp, W_UNK) for sp in words] + ([W_EOS] if eos_term else []):
        total += backoff_logp(lm, ctx, w)
        ctx = ctx + (w,) if (w,) in lm.prob else ()
    return total, len(words)


def random_word_lm(V, order, seed, extra_words=(), oov_logp=-30.0):
    rs = np.random.RandomState(seed)
    letters = list(range(1, V - 1))
    spell = [tuple(w) for w in extra_words]
    for _ in range(12 if V <= 5 else 40):
        spell.append(tuple(int(letters[rs.randint(len(letters))]) for _ in range(rs.randint(1, 4))))
    lex = Lexicon(spell, None, V - 1, V=V)
    n = len(lex)
    W = W_FIRST + n
    ids = [W_EOS] + ([W_UNK] if seed % 2 else []) + [W_FIRST + i for i in range(n) if not (n > 3 and i == 1)]   # word 1: no unigram
    prob, backoff = {}, {}
    for w in ids:
        prob[(w,)] = float(rs.uniform(-6.0, -0.5))
    hist = [(W_BOS,)] + [(w,) for w in ids if w != W_EOS]
    for k in range(2, order + 1):
        new = []
        for _ in range(min(4 * W, 200)):
            g = hist[rs.randint(len(hist))] + (ids[rs.randint(len(ids))],)
            if g not in prob and W_EOS not in g[:-1]:
                prob[g] = float(rs.uniform(-5.0, -0.1))
                backoff[g[:-1]] = float(rs.uniform(-2.0, 0.0))
                if g[-1] != W_EOS:
                    new.append(g)
        for _ in range(3):                                               # a history that no listed n-gram is a prefix of
            g = tuple(ids[1 + rs.randint(len(ids) - 1)] for _ in range(k))
            if g not in prob:
                prob[g] = float(rs.uniform(-5.0, -0.1))
                new.append(g)
        hist = new or hist
    return WordLM(NgramLM(order, W, W_BOS, W_EOS, prob, backoff, oov_logp=oov_logp), lex)


def close(table, node, state, dt, lexicon_only=False):
    """The close pair of an entry whose pending word stands at trie node `node` (!= 0)."""
    w = -1 if node < 0 else int(table.trie_word[node])
    if w < 0:
        if lexicon_only:
            return dt(0), -1
        w = table.unk
    return table.lookup(state, w, dt)


def walk(table, ids, dt, eos_term=True):
    """-> (the sum in word order in dtype dt, the per-word terms, n_words)."""
    node, state, total, per = 0, table.start, dt(0), []
    for c in list(ids) + [table.space]:
        c = int(c)
        if c != table.space:
            node = -1 if node < 0 else int(table.trie_next[node, c])
        elif node != 0:
            lp, state = close(table, node, state, dt)
            total = dt(total + lp)
            per.append(lp)
            node = 0
    if eos_term:
        total = dt(total + table.lookup(state, table.eos, dt)[0])
    return total, per, len(per)


def search_wlm(logits, K, wlm, alpha, beta, eos_term=True, lexicon_only=False):
    """logits [T, V] of the VALID frames (their dtype is the arithmetic's) -> dict(hyps, score: the rank, ctc: tot, lm, nw,
    gap: as ctc_beam_ref.search defines it, over the ranks of every select and of the final ranking)."""
    table = wlm.compile()
    z = np.asarray(logits)
    T, V = z.shape
    dt = z.dtype.type
    ninf = dt(-np.inf)
    a, bt = dt(np.float32(alpha)), dt(np.float32(beta))
    space = table.space
    x = R.log_probs(z) if T else z

    def rank(tot, lmv, n):
        lmv, n = np.asarray(lmv, dtype=z.dtype), np.asarray(n).astype(z.dtype)
        return ((tot + (a * lmv).astype(z.dtype)).astype(z.dtype) + (bt * n).astype(z.dtype)).astype(z.dtype)

    def entry_of(node, state, lm, nw):
        clp, cnx = close(table, node, state, dt, lexicon_only) if node != 0 else (dt(0), state)
        return (node, state, lm, nw, clp, cnx)

    prefixes, pb, pnb, ent = [()], [dt(0)], [ninf], [entry_of(0, table.start, dt(0), 0)]
    gap = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            n = len(prefixes)
            pb_a, pnb_a = np.array(pb, dtype=dt), np.array(pnb, dtype=dt)
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
            lm_a = np.array([e[2] for e in ent], dtype=dt)
            nw_a = np.array([e[3] for e in ent])
            ext_lm = np.repeat(lm_a[:, None], V - 1, axis=1)
            ext_nw = np.repeat(nw_a[:, None], V - 1, axis=1)
            for k, e in enumerate(ent):
                if e[0] != 0:
                    ext_lm[k, space - 1] = dt(e[2] + e[4])
                    ext_nw[k, space - 1] = e[3] + 1
                if lexicon_only:
                    off = table.trie_next[e[0], 1:] < 0
                    off[space - 1] = e[0] != 0 and e[5] < 0
                    ext[k, off] = ninf
            cand = np.full(K + n * (V - 1), ninf, dtype=dt)
            cand[:n] = rank(stot, lm_a, nw_a)
            cand[K:] = rank(ext, ext_lm, ext_nw).reshape(-1)
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
                    new.append((prefixes[idx], spb[idx], spnb[idx], ent[idx]))
                else:
                    k, c = divmod(int(idx) - K, V - 1)
                    c += 1
                    node, state, lm, nw, clp, cnx = ent[k]
                    if c != space:
                        node = -1 if node < 0 else int(table.trie_next[node, c])
                    elif node != 0:
                        node, state, lm, nw = 0, cnx, dt(lm + clp), nw + 1
                    new.append((prefixes[k] + (c,), ninf, ext[k, c - 1], entry_of(node, state, lm, nw)))
            prefixes, pb, pnb, ent = (list(col) for col in zip(*new))
    tot = np.logaddexp(np.array(pb, dtype=dt), np.array(pnb, dtype=dt)).astype(dt)
    keep, lm_f, nw_f = [], [], []
    for i, (node, state, lm, nw, clp, cnx) in enumerate(ent):
        if node != 0:
            if cnx < 0:
                continue                                                 # lexicon_only: the pending node ends no word
            state, lm, nw = cnx, dt(lm + clp), nw + 1
        if eos_term:
            lm = dt(lm + table.lookup(state, table.eos, dt)[0])
        keep.append(i), lm_f.append(lm), nw_f.append(nw)
    tot = tot[keep]
    lm_f, nw_f = np.array(lm_f, dtype=dt), np.array(nw_f, dtype=np.int64)
    final = rank(tot, lm_f, nw_f) if keep else np.zeros(0, dtype=dt)
    order = np.argsort(-final.astype(np.float64), kind="stable")
    vals = final[order].astype(np.float64)
    for r in range(len(vals) - 1):
        gap = min(gap, vals[r] - vals[r + 1])
    return dict(hyps=[prefixes[keep[i]] for i in order], score=final[order], ctc=tot[order], lm=lm_f[order], nw=nw_f[order],
                gap=float(gap))


# ---------------------------------------------------------------------------------------------------------------------
# The GPU grid (tests/test_word_lm_gpu.py) and its decision on the CPU (tests/test_word_lm_cpu.py asserts the cap).
GRID_V, GRID_K, GRID_T, GRID_SCALE = (4, 5, 34, 257), (1, 2, 4, 16), (1, 2, 7, 100), R.GRID_SCALE
ORDERS, WEIGHTS = (1, 2, 3), ((0.5, 0.0), (2.0, 1.5), (1.0, -1.0))
QUANTITIES = ("score", "ctc", "lm")
UNDECIDED_CAP = 0.10


def grid():
    """-> (cases, extra): tuples (V, K, T, scale, order, alpha, beta, lexicon_only); the order, the weights and
    lexicon_only cycle over the cases.  extra: ctc_beam_ref.EXTRA, the shapes on either side of the kernel's switches (one
    wave / four, staged tokens / memory, history in LDS / the workspace)."""
    shapes = [(V, K, T, s) for V in GRID_V for K in GRID_K for T in GRID_T for s in GRID_SCALE]
    extra = [c for c in R.EXTRA if c[0] >= 4]

    def full(i, c):
        return c + (ORDERS[i % 3],) + WEIGHTS[(i // 3) % 3] + (bool((i // 2) % 2),)
    return [full(i, c) for i, c in enumerate(shapes)], [full(i + 1, c) for i, c in enumerate(extra)]


def grid_case(V, K, T, scale, order, alpha, beta, lexicon_only):
    """-> (logits, lens: ctc_beam_ref.grid_case's - B = 3 ragged, ld = V + 3, NaN behind every utterance -, the WordLM).  With
    <space> = V - 1 drawn as often as any letter the words are short; the lexicon holds the words of every utterance's
    best path (so that lexicon words are in reach) beside random ones."""
    z, lens = R.grid_case(V, K, T, scale)
    own = []
    for b in range(3):
        best = R.collapse(np.argmax(z[b, :lens[b], :V], axis=1)) if lens[b] else ()
        own += [w for w in split(best, V - 1) if len(w) <= 6][:8]
    return z, lens, random_word_lm(V, order, R.case_seed(V, K, T, scale) + order, extra_words=own)


_JUDGED = {}


def judge(case, eos_term=True):
    """The restatements of one grid case, computed once per process -> a list over the utterances of dict(ref: the float64
    search, allowance: {quantity: 4 x the float32 restatement's error against float64 over the hypotheses both report, at
    least 8 ulps of the quantity's greatest magnitude}, decisive: both restatements report the same hypotheses in the same
    order and every select of the float64 search (the final ranking included) separates ranks 1 .. K + 1 by more than 2 x
    the allowance of the score)."""
    key = tuple(case) + (bool(eos_term),)
    if key not in _JUDGED:
        V, K, T, scale, order, alpha, beta, lexicon_only = case
        z, lens, wlm = grid_case(*case)
        out = []
        for b in range(3):
            zb = z[b, :lens[b], :V]
            r64 = search_wlm(zb.astype(np.float64), K, wlm, alpha, beta, eos_term, lexicon_only)
            r32 = search_wlm(zb.astype(np.float32), K, wlm, alpha, beta, eos_term, lexicon_only)
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
