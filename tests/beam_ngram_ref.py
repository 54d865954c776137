"""CPU restatement of the attention beam search with an n-gram LM or a lexicon and word-level LM inside for the
tests, on top of beam_ref / beam_lm_ref / beam_ctc_ref (the search, the judge's and the CTC term) and ngram_ref / word_lm_ref
(the tables' walks).

  Pos / start / extend / finish   the LM position of a token sequence, its moves and its end term, over the compiled TABLE's
                                  float32 values: lm is an fp32 sum, every addition rounded on its own - the device's bits
  search(...)                     beam_ctc_ref.search (plain, judge, CTC) with the LM's term: float64 base, the rank
                                  (base' + weight lm') + bonus n'; with weight = bonus = 0 it is that search, decision for
                                  decision
  decode(...)                     the search over a decoder state dict: beam_ctc_ref.decode's step functions, this search
  select_f32(...)                 ONE step of one utterance in float32, operation for operation as the kernel orders them, on
                                  given row statistics: the yardstick of the exact select test
  grid() / grid_case() / judge()  the seeds and verdicts of the GPU grid

A candidate that lexicon_only forbids ranks -inf."""
import numpy as np
import torch

import beam_ctc_ref
import beam_ref
import ngram_ref as NR
import word_lm_ref as WR

F = np.float32
NGRAM, WORD = "ngram", "word"


def tlm(kind, table, weight=0.0, bonus=0.0, lexicon_only=False):
    """The LM of a search: kind NGRAM (table: NgramLM.compile()) or WORD (table: WordLM.compile())."""
    return dict(kind=kind, table=table, weight=float(weight), bonus=float(bonus), lexicon_only=bool(lexicon_only) and kind == WORD)


def start(lm):
    """The position of the empty sequence: n-gram (state, lm, len); word LM (node, word state, lm, nw)."""
    t = lm["table"]
    return (int(t.start), F(0), 0) if lm["kind"] == NGRAM else (0, int(t.start), F(0), 0)


def _close(lm, pos):
    """The close pair of a word position: (0, state) at the root."""
    node, state = pos[0], pos[1]
    if node == 0:
        return F(0), state
    lp, nxt = WR.close(lm["table"], node, state, F, lm["lexicon_only"])
    return F(lp), int(nxt)


def finish(lm, pos):
    """-> (lm, n) of the sequence as a complete hypothesis, the end-of-sentence term included - or None (lexicon_only and the
    pending node ends no word)."""
    t = lm["table"]
    if lm["kind"] == NGRAM:
        state, s, n = pos
        return F(s + F(t.logp[state, t.eos])), n
    node, state, s, nw = pos
    if node != 0:
        lp, nxt = _close(lm, pos)
        if nxt < 0:
            return None
        s, nw, state = F(s + lp), nw + 1, nxt
    return F(s + F(t.lookup(state, t.eos, F)[0])), nw


def extend(lm, pos, c):
    """-> the position after the non-<EOS> token c - or None (lexicon_only forbids it)."""
    t = lm["table"]
    if lm["kind"] == NGRAM:
        state, s, n = pos
        return int(t.nxt[state, c]), F(s + F(t.logp[state, c])), n + 1
    node, state, s, nw = pos
    if c != t.space:
        child = -1 if node < 0 else int(t.trie_next[node, c])
        if lm["lexicon_only"] and child < 0:
            return None
        return child, state, s, nw
    if node == 0:
        return pos
    lp, nxt = _close(lm, pos)
    if nxt < 0:
        return None
    return 0, nxt, F(s + lp), nw + 1


def lm_n(pos):
    return pos[-2], pos[-1]


def candidate_terms(lm, pos, V, eos):
    """lm' [V] float32 and n' [V] of every extension of `pos`; NaN / -1 where lexicon_only forbids it."""
    out_lm, out_n = np.full(V, np.nan, dtype=F), np.full(V, -1, dtype=np.int64)
    for v in range(V):
        r = finish(lm, pos) if v == eos else extend(lm, pos, v)
        if r is not None:
            out_lm[v], out_n[v] = r[0] if v == eos else r[-2], r[1] if v == eos else r[-1]
    return out_lm, out_n


def search(step, K, V, L, eos, lm, x=None, ctc_weight=0.0, lm_weight=None, length_penalty=0.0):
    """beam_ctc_ref.search with the LM's term.  -> its dict, hyps [(tokens, key, length)], and parts [(base, lm, n)] beside
    them in the same order (rank before the length penalty: rank)."""
    scores = np.full(K, -np.inf)
    scores[0] = 0.0
    paths = [[] for _ in range(K)]
    pos = [start(lm) for _ in range(K)]
    parents, toks = np.zeros(K, dtype=np.int64), None
    fin, margins = [], []            # (tokens, rank, length, base, lm, n)
    states = [beam_ctc_ref.prefix_init(x) for _ in range(K)] if ctc_weight else None
    w, beta = lm["weight"], lm["bonus"]
    t = 0
    for t in range(L):
        out = step(t, parents, toks)
        logits, lm_logits = out if lm_weight is not None else (out, None)
        fused = beam_ref.log_softmax(logits)
        if ctc_weight:
            psis = [beam_ctc_ref.prefix_scores(states[k], x, eos) if np.isfinite(scores[k]) else np.full(V, -np.inf)
                    for k in range(K)]
            term = np.stack([beam_ctc_ref.ctc_term(psis[k], states[k]["psi_prev"]) for k in range(K)])
            fused = (1.0 - ctc_weight) * fused + ctc_weight * term
        if lm_weight is not None:
            fused = fused + lm_weight * beam_ref.log_softmax(lm_logits)
        extra = np.zeros((K, V))
        for k in range(K):
            if np.isfinite(scores[k]):
                cl, cn = candidate_terms(lm, pos[k], V, eos)
                ok = cn >= 0
                extra[k] = np.where(ok, w * np.where(ok, cl, 0).astype(np.float64) + beta * cn, -np.inf)
        sel = beam_ref.select(scores, fused + extra, eos)
        margins.append(sel["margin"])
        for k, rk in sel["finished"]:
            l, n = finish(lm, pos[k])
            fin.append((paths[k] + [eos], float(rk), t + 1, float(scores[k] + fused[k, eos]), l, n))
        live = range(sel["nlive"])
        bp, tk = sel["bp"], sel["tok"]
        new_scores = np.full(K, -np.inf)
        for j in live:
            new_scores[j] = scores[bp[j]] + fused[bp[j], tk[j]]
        paths = [paths[bp[j]] + [int(tk[j])] if j < sel["nlive"] else [] for j in range(K)]
        pos = [extend(lm, pos[bp[j]], int(tk[j])) if j < sel["nlive"] else pos[j] for j in range(K)]
        if ctc_weight:
            states = [beam_ctc_ref.prefix_advance(states[bp[j]], x, int(tk[j]), psis[bp[j]]) if j < sel["nlive"] else states[j]
                      for j in range(K)]
        scores = new_scores
        if t == L - 1 and len(fin) < K:
            for j in live:                                   # they finish as they stand: the end term, no <EOS> token
                r = finish(lm, pos[j])
                if r is not None:
                    fin.append((paths[j], float(scores[j] + w * float(r[0]) + beta * r[1]), t + 1, float(scores[j]), r[0], r[1]))
        if len(fin) >= K or t == L - 1 or sel["nlive"] == 0:
            break
        parents, toks = bp, tk
    keys = [f[1] / (float(f[2]) ** length_penalty) if length_penalty else f[1] for f in fin]
    order = sorted(range(len(fin)), key=lambda i: (-keys[i], i))
    hyps = [(fin[i][0], keys[i], fin[i][2]) for i in order[:K]]
    parts = [fin[i][3:] for i in order[:K]]
    rank_margin = keys[order[0]] - keys[order[1]] if len(order) > 1 else np.inf
    return dict(hyps=hyps, parts=parts, margins=margins, rank_margin=rank_margin, steps=t + 1)


def decode(sd, enc_pad, enc_len, L, K, lm, ctc=None, ctc_weight=0.0, lm_sd=None, lm_weight=0.0, length_penalty=0.0):
    """The search over the decoder of state dict `sd` (and the judge lm_sd, and the CTC head ctc = (w [V, enc], b [V])): the
    step functions are beam_ctc_ref.decode's - its call of its own search is answered by this module's."""
    V = sd["decoder.output_layer.weight"].shape[0]
    enc_pad = torch.as_tensor(enc_pad)
    cw, cb = ctc if ctc is not None else (np.zeros((V, enc_pad.shape[2])), np.zeros(V))
    theirs = beam_ctc_ref.search
    beam_ctc_ref.search = lambda step, K_, V_, L_, eos, x, w, lw, lp: search(step, K_, V_, L_, eos, lm, x, w, lw, lp)
    try:
        return beam_ctc_ref.decode(sd, cw, cb, enc_pad, enc_len, L, K, ctc_weight if ctc is not None else 0.0, lm_sd, lm_weight,
                                   length_penalty)
    finally:
        beam_ctc_ref.search = theirs


def words_in_lexicon(table, ids):
    """Every word of the token row is spelled by the lexicon."""
    for word in WR.split(ids, table.space):
        node = 0
        for c in word:
            node = -1 if node < 0 else int(table.trie_next[node, c])
        if node < 0 or table.trie_word[node] < 0:
            return False
    return True


# ------------------------------------------------------------------ one step in float32, the kernel's operations
def fma32(a, b, c):
    """round_to_float32(a * b + c), rounded once, on float32 arrays: the product is exact in float64, the sum's float64 error
    (TwoSum) breaks the tie where the float64 sum lies exactly between two float32 values."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(F)
        tie = np.isfinite(s) & (r.astype(np.float64) != s) & (err != 0)
        up = np.nextafter(r, F(np.inf), dtype=F).astype(np.float64)
        down = np.nextafter(r, F(-np.inf), dtype=F).astype(np.float64)
        rr = r.astype(np.float64)
        other = np.where(s > rr, up, down)                     # the float32 neighbour on s's side of r
        half = np.abs(s - rr) == np.abs(other - s)             # s exactly between r and that neighbour
        flip = tie & half & (np.sign(err) == np.sign(other - rr))
    return np.where(flip, other, rr).astype(F)


def select_f32(scores, logits, stats, eos, lm, pos, t, L, nfin, lm_logits=None, lm_stats=None, lmw=0.0, psi=None, psi_prev=None,
               cw=0.0):
    """One utterance, step t.  scores [K] f32 (base), logits [K, V] f32, stats [K, 2] f32: the row maximum and log(sum exp(x -
    max)) AS THE DEVICE FORMS THEM (the sum's order is the kernel's own), pos: K positions; the judge's logits / stats / weight
    and the CTC psi [K, V] / psi_prev [K] / weight where the variant has them.  Every operation is rounded to float32 on its
    own, in the kernel's order; the ranking is a stable sort by rank, descending.
    -> dict(tok, bp, scores, pos (of the K slots; None: dead), fin [(step, slot, length, eos flag, rank, base, lm, n)], nlive, done)."""
    K, V = logits.shape
    w, beta = F(lm["weight"]), F(lm["bonus"])
    rank = np.full((K, V), -np.inf, dtype=F)
    base = np.full((K, V), -np.inf, dtype=F)
    cand_lm, cand_n = np.zeros((K, V), dtype=F), np.zeros((K, V), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            if scores[k] == -np.inf:
                continue
            sc = F(scores[k])
            lp = ((logits[k] - stats[k, 0]).astype(F) - stats[k, 1]).astype(F)
            # the existing select kernels as they are compiled: the judge's product is fused into its sum where it is the only
            # extra term, nothing is fused with the CTC terms alone, and with both only (1 - w) logp is fused into the score
            both = bool(cw) and lm_logits is not None
            c = (sc + lp).astype(F)
            if cw:
                omw = F(F(1) - F(cw))
                c = fma32(omw, lp, sc) if both else (sc + (omw * lp).astype(F)).astype(F)
                c = (c + (F(cw) * (psi[k] - psi_prev[k]).astype(F)).astype(F)).astype(F)
            if lm_logits is not None:
                llp = ((lm_logits[k] - lm_stats[k, 0]).astype(F) - lm_stats[k, 1]).astype(F)
                c = (c + (F(lmw) * llp).astype(F)).astype(F) if both else fma32(F(lmw), llp, c)
            base[k] = c
            cl, cn = candidate_terms(lm, pos[k], V, eos)
            ok = cn >= 0
            cand_lm[k], cand_n[k] = np.where(ok, cl, 0), cn
            r = ((c + (w * cand_lm[k]).astype(F)).astype(F) + (beta * cn.astype(F)).astype(F)).astype(F)
            rank[k] = np.where(ok, r, -np.inf)
    flat = rank.ravel()
    order = np.argsort(-flat, kind="stable")
    top = [int(i) for i in order[:2 * K] if flat[i] != -np.inf and not np.isnan(flat[i])]
    tok, bp = np.full(K, eos, dtype=np.int64), np.zeros(K, dtype=np.int64)
    new, new_pos = np.full(K, -np.inf, dtype=F), [None] * K
    fin, nlive, nf, live_idx = [], 0, int(nfin), []
    for r, idx in enumerate(top):
        k, v = divmod(idx, V)
        if v == eos:
            if r < K:
                fin.append((t, k, t + 1, 1, flat[idx], base[k, v], cand_lm[k, v], int(cand_n[k, v])))
        elif nlive < K:
            tok[nlive], bp[nlive], new[nlive] = v, k, base[k, v]
            new_pos[nlive] = extend(lm, pos[k], v)
            live_idx.append(idx)
            nlive += 1
    if t == L - 1 and nf + len(fin) < K:
        for j in range(nlive):
            r = finish(lm, new_pos[j])
            if r is not None:
                rk = F(F(new[j] + F(w * r[0])) + F(beta * F(r[1])))
                fin.append((t, j, t + 1, 0, rk, new[j], r[0], int(r[1])))
    nf += len(fin)
    return dict(tok=tok, bp=bp, scores=new, pos=new_pos, fin=fin, nlive=nlive, done=bool(nf >= K or t == L - 1 or nlive == 0))


# ------------------------------------------------------------------ the GPU grid of the end-to-end comparison
MARGIN = 1e-4                # tests/test_beam_lm_gpu.py's
LEFT_OUT_CAP = 0.25
EOS, BOS, SPACE = 2, 1, 33
V, D, ENC, LENS, L = 34, 320, 128, (12, 9), 10
VARIANTS = ("alone", "judge", "ctc")
KINDS = (NGRAM, WORD)
BEAMS = (1, 4)
# (kind, variant, K) -> the seed of the case: the first of 0, 1, .. for which the restatement alone has every utterance's
# decision margin above MARGIN where possible (find_seed below; tests/test_beam_ngram_cpu.py holds them to the cap)
SEEDS = {(kind, variant, K): 0 for kind in ("ngram", "word") for variant in ("alone", "judge", "ctc") for K in (1, 4)}


def grid():
    return [(kind, variant, K) for kind in KINDS for variant in VARIANTS for K in BEAMS]


def grid_lm(kind, seed):
    """The LM of a grid case over the V = 34 vocabulary (<PAD> 0, <BOS> 1, <EOS> 2, letters 3 .. 32, <space> 33)."""
    if kind == NGRAM:
        return NR.random_lm(V, 3, 900 + seed)
    return random_word_lm(910 + seed)


def random_word_lm(seed, n_words=40, order=2):
    """A random lexicon over the letters 3 .. SPACE - 1 with a random backoff model over it (word_lm_ref.random_word_lm's recipe
    on this vocabulary's ids: <BOS> and <EOS> are no letters)."""
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_UNK, W_FIRST
    rs = np.random.RandomState(seed)
    letters = list(range(3, SPACE))
    spell = {tuple(int(letters[rs.randint(len(letters))]) for _ in range(rs.randint(1, 4))) for _ in range(n_words)}
    lex = Lexicon(sorted(spell), None, SPACE, bos=BOS, eos=EOS, V=V)
    ids = [W_EOS, W_UNK] + [W_FIRST + i for i in range(len(lex)) if i != 1]               # word 1: no unigram
    prob = {(wd,): float(rs.uniform(-6.0, -0.5)) for wd in ids}
    backoff = {}
    hist = [(W_BOS,)] + [(wd,) for wd in ids if wd != W_EOS]
    for _ in range(150 if order > 1 else 0):
        g = hist[rs.randint(len(hist))] + (ids[rs.randint(len(ids))],)
        if g not in prob:
            prob[g] = float(rs.uniform(-5.0, -0.1))
            backoff[g[:-1]] = float(rs.uniform(-2.0, 0.0))
    return WordLM(NgramLM(order, W_FIRST + len(lex), W_BOS, W_EOS, prob, backoff), lex)


WEIGHTS = {NGRAM: (0.4, 0.3), WORD: (0.6, 0.5)}     # (weight, bonus) of the grid's searches
JUDGE_WEIGHT, CTC_WEIGHT = 0.3, 0.3
_CASES, _JUDGED = {}, {}


def grid_case(kind, variant, K):
    """-> dict(cfg, w: the E2E weights, lm_cfg / lm_w: the judge's, ctc: (w, b) of a CTC head, enc, lens, lm: the LM object) of
    a grid case, as arrays (no GPU); the decoder and the judge are test_beam_lm_gpu's smallest."""
    key = (kind, variant, K)
    if key not in _CASES:
        import test_beam_lm_gpu as tl
        seed = SEEDS[key]
        cfg, w = tl._e2e_weights(D, V, ENC, 300 + 10 * seed + K, 0.5 if K == 1 else 2.0)    # K > 1: searches that <EOS> ends
        lm_cfg, lm_w = tl._lm_weights("1x320", V, 400 + 10 * seed + K)
        rs = np.random.RandomState(500 + seed)
        ctc = ((rs.randn(V, ENC) * 0.3).astype(F), (rs.randn(V) * 0.1).astype(F))
        _CASES[key] = dict(cfg=cfg, w=w, lm_cfg=lm_cfg, lm_w=lm_w, ctc=ctc, enc=tl._enc_arrays(len(LENS), ENC, LENS, 600 + seed),
                           lens=list(LENS), lm=grid_lm(kind, seed))
    return _CASES[key]


def judge(key):
    """The restatement's verdict on a grid case, computed once: the list of search() results, one per utterance."""
    if key not in _JUDGED:
        kind, variant, K = key
        c = grid_case(*key)
        t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}      # noqa: E731
        lm = tlm(kind, c["lm"].compile(), *WEIGHTS[kind])
        _JUDGED[key] = decode(t(c["w"]), torch.from_numpy(c["enc"]), c["lens"], L, K, lm,
                              ctc=c["ctc"] if variant == "ctc" else None, ctc_weight=CTC_WEIGHT if variant == "ctc" else 0.0,
                              lm_sd=t(c["lm_w"]) if variant == "judge" else None, lm_weight=JUDGE_WEIGHT)
    return _JUDGED[key]


def decided(res):
    """A search() result whose every decision margin, the final ranking's included, is above MARGIN."""
    return min(min(res["margins"]), res["rank_margin"]) > MARGIN
