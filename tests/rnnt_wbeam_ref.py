"""A restatement of the transducer beam search with a lexicon and a word-level LM inside (csrc/rnnt_beam.hip's WLM kernels,
DESIGN 4.30) that needs no GPU.  The search is tests/rnnt_beam_ref.py's - its head (rnnt_ref), its merge (_lae), its selection
rule - and the word state is tests/word_lm_ref.py's (close, walk, the table's lookup); neither file is edited.  float64 is the
reference; float32 - the same recurrences in the same order - is the yardstick of the allowance.

    search(...)     one utterance -> dict(finals, steps, finalised), as rnnt_beam_ref.search; a final also has lm and nw
    judge(case)     the float64 and the float32 search of a case, the allowance and whether the case is decisive
    GRID / grid_case(..)   the seeded inputs the CPU and the GPU tests share

An entry carries (node, wstate, lm, nw) beside rnnt_beam_ref's fields: functions of its label sequence.  The blank keeps
them; a label k != space walks the trie (with lexicon_only a step off it is no candidate); `space` from the root changes
nothing, elsewhere it closes the pending word (lm += lp, nw += 1, wstate = s', node = root; with lexicon_only a node that
ends no word is no candidate).  rank = (tot + alpha lm) + beta nw, the weights fp32 values, every operation rounded on its
own.  A final closes its pending word the same way and then takes the end-of-sentence term."""
import numpy as np

import rnnt_beam_ref as BR
import rnnt_ref as R
import word_lm_ref as WR

ULP = BR.ULP


def _rank(tot, lm, nw, alpha, beta, dt):
    a, b = dt(np.float32(alpha)), dt(np.float32(beta))
    return dt(dt(dt(tot) + dt(a * dt(lm))) + dt(b * dt(nw)))


def _closed(table, e, dt, lexicon_only):
    """The entry's word state after its pending word has closed -> (lm, nw, wstate) or None (lexicon_only: no word ends)."""
    if e["node"] == 0:
        return e["lm"], e["nw"], e["wst"]
    lp, nx = WR.close(table, e["node"], e["wst"], dt, lexicon_only)
    if nx < 0:
        return None
    return dt(e["lm"] + lp), e["nw"] + 1, nx


def search(p, enc_h, bos, K, L, table, dt=np.float64, alpha=0.0, beta=0.0, eos_term=True, lexicon_only=False):
    """One utterance: p the head's parameters (numpy), enc_h [T, H], table a word_lm.WordTable on the host.  -> what
    rnnt_beam_ref.search returns; a final is dict(tokens, tot, lm, nw, rank, it, slot)."""
    p = {k: np.asarray(v).astype(dt) for k, v in p.items()}
    enc_h = np.asarray(enc_h)
    T = enc_h.shape[0]
    space = table.space

    def eos_lp(state):
        return dt(table.lookup(state, table.eos, dt)[0])
    if T == 0:
        lm0 = eos_lp(table.start) if eos_term else dt(0)
        return dict(finals=[dict(tokens=(), tot=dt(0), lm=lm0, nw=0, rank=_rank(dt(0), lm0, 0, alpha, beta, dt), it=-1, slot=0)],
                    steps=[], finalised=[()])
    pe = enc_h.astype(dt) @ p["lin_enc.weight"].T + p["lin_enc.bias"]
    V = p["lin_out.weight"].shape[0]
    zero = np.zeros(p["lstm.weight_hh_l0"].shape[1], dt)
    h, c = R._cell(p, bos, zero, zero, np)
    beam = [dict(seq=(), tot=dt(0), lm=dt(0), nw=0, node=0, wst=table.start, h=h, c=c, pp=p["lin_pred.weight"] @ h)]
    finals, steps, finalised = [], [], []
    for it in range(T + L):
        if not beam:
            break
        cands, rows = {}, []
        for e in beam:
            t = it - len(e["seq"])
            assert 0 <= t < T
            lg = p["lin_out.weight"] @ np.tanh(pe[t] + e["pp"], dtype=dt) + p["lin_out.bias"]
            mx = lg.max()
            rows.append((lg - dt(mx + np.log(np.exp(lg - mx, dtype=dt).sum(dtype=dt), dtype=dt))).astype(dt))
        for hi, e in enumerate(beam):                               # the blanks first: a merged candidate is its blank parent's
            tot = dt(e["tot"] + rows[hi][0])
            if it - len(e["seq"]) == T - 1:
                shut = _closed(table, e, dt, lexicon_only)
                if shut is None:
                    continue                                        # lexicon_only: the pending node ends no word - no final
                lm, nw, wst = shut
                if eos_term:
                    lm = dt(lm + eos_lp(wst))
                finals.append(dict(tokens=e["seq"], tot=tot, lm=lm, nw=nw, rank=_rank(tot, lm, nw, alpha, beta, dt), it=it, slot=hi))
                finalised.append(e["seq"])
            else:
                cands[e["seq"]] = dict(seq=e["seq"], tot=tot, lm=e["lm"], nw=e["nw"], node=e["node"], wst=e["wst"], flat=hi * V,
                                       parent=hi, tok=0)
        for hi, e in enumerate(beam):
            if len(e["seq"]) >= L:
                continue
            for k in range(1, V):
                seq = e["seq"] + (k,)
                lm, nw, node, wst = e["lm"], e["nw"], e["node"], e["wst"]
                allowed = True
                if k == space:
                    shut = _closed(table, e, dt, lexicon_only)
                    if shut is None:
                        allowed = False
                    else:
                        (lm, nw, wst), node = shut, 0
                else:
                    node = -1 if node < 0 else int(table.trie_next[node, k])
                    allowed = not (lexicon_only and node < 0)
                tot = dt(e["tot"] + rows[hi][k])
                if seq in cands:
                    assert cands[seq]["tok"] == 0 and allowed       # (what the lexicon admits is a function of the sequence)
                    cands[seq]["tot"] = BR._lae(cands[seq]["tot"], tot, dt)
                    continue
                if allowed:
                    cands[seq] = dict(seq=seq, tot=tot, lm=lm, nw=nw, node=node, wst=wst, flat=hi * V + k, parent=hi, tok=k)
        for cd in cands.values():
            cd["rank"] = _rank(cd["tot"], cd["lm"], cd["nw"], alpha, beta, dt)
        order = sorted((cd for cd in cands.values() if cd["rank"] > -np.inf), key=lambda cd: (-cd["rank"], cd["flat"]))
        kept = order[:K]
        gap = float(kept[-1]["rank"] - order[K]["rank"]) if len(order) > K else np.inf
        steps.append(dict(kept=[(cd["seq"], cd["tot"], cd["rank"]) for cd in kept], gap=gap))
        new = []
        for cd in kept:
            e = beam[cd["parent"]]
            if cd["tok"] == 0:
                h, c, pp = e["h"], e["c"], e["pp"]
            else:
                h, c = R._cell(p, cd["tok"], e["h"], e["c"], np)
                pp = p["lin_pred.weight"] @ h
            new.append(dict(seq=cd["seq"], tot=cd["tot"], lm=cd["lm"], nw=cd["nw"], node=cd["node"], wst=cd["wst"], h=h, c=c, pp=pp))
        beam = new
    assert not beam
    finals.sort(key=lambda f: (-f["rank"], f["it"], f["slot"]))
    return dict(finals=finals, steps=steps, finalised=finalised)


_JUDGED = {}


def judge(case):
    """case: dict(p, enc_h [T, H], bos, K, L, table and optionally alpha, beta, eos_term, lexicon_only, key: a hashable name
    under which the verdict is kept for the process).  rnnt_beam_ref.judge's rule -> dict(ref: the float64 search, f32: the
    float32 search, allowance: 4 x the float32 search's worst error against float64 on a kept candidate or a final - at least
    8 fp32 ulps of the largest score -, decisive: at every selection and in the final list the float64 rank gaps exceed
    twice the allowance accumulated so far, and the float32 search keeps the float64 search's candidates)."""
    if case.get("key") in _JUDGED:
        return _JUDGED[case["key"]]
    kw = dict(alpha=case.get("alpha", 0.0), beta=case.get("beta", 0.0), eos_term=case.get("eos_term", True),
              lexicon_only=case.get("lexicon_only", False))
    ref = search(case["p"], case["enc_h"], case["bos"], case["K"], case["L"], case["table"], np.float64, **kw)
    f32 = search(case["p"], case["enc_h"], case["bos"], case["K"], case["L"], case["table"], np.float32, **kw)
    K = case["K"]
    decisive, allow = len(ref["steps"]) == len(f32["steps"]), 0.0
    for a, b in zip(ref["steps"], f32["steps"]):
        if [s for s, _, _ in a["kept"]] != [s for s, _, _ in b["kept"]]:
            decisive = False
            break
        for (_, ta, ra), (_, tb, rb) in zip(a["kept"], b["kept"]):
            allow = max(allow, 4 * abs(float(tb) - float(ta)), 4 * abs(float(rb) - float(ra)),
                        8 * ULP * max(abs(float(ta)), abs(float(ra))))
        if not a["gap"] > 2 * allow:
            decisive = False
    fa, fb = ref["finals"], f32["finals"]
    if [f["tokens"] for f in fa[:K]] != [f["tokens"] for f in fb[:K]]:
        decisive = False
    else:
        for x, y in zip(fa[:K], fb[:K]):
            allow = max(allow, 4 * abs(float(y["tot"]) - float(x["tot"])), 4 * abs(float(y["rank"]) - float(x["rank"])),
                        8 * ULP * max(abs(float(x["tot"])), abs(float(x["rank"]))))
    for x, y in zip(fa[:K], fa[1:K + 1]):
        if not float(x["rank"] - y["rank"]) > 2 * allow:
            decisive = False
    out = dict(ref=ref, f32=f32, allowance=allow, decisive=decisive)
    if case.get("key") is not None:
        _JUDGED[case["key"]] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The GPU grid (tests/test_rnnt_wbeam_gpu.py) and its decision on the CPU (tests/test_rnnt_wbeam_cpu.py asserts the cap).
# (V, K, J, T', L, order, lexicon_only, eos_term, seed): every value of V in {5, 34}, K in {1, 4, 16}, J in {4, 32}, T' in
# {1, 7, 12}, L in {1, 6, 12}, the LM's order in 1 .. 3 and both settings of the two switches, every pair (K, T'), (K, L) and
# (T', L) at least once - the step kernel has one shape (256 threads, K-entry lists), so what its loops depend on is one entry
# / several / kKmax, V below a wave and V < K, every blank a final (T' = 1), the label cap binding at once (L = 1) or never.
GRID = (
    (5, 1, 4, 1, 1, 1, False, False, 1),
    (5, 4, 32, 7, 6, 2, True, True, 2),
    (5, 16, 4, 12, 12, 3, False, True, 3),
    (5, 16, 32, 1, 6, 2, True, False, 4),
    (5, 4, 4, 12, 1, 3, True, True, 5),
    (5, 1, 32, 7, 12, 1, False, True, 6),
    (34, 1, 32, 12, 6, 3, True, False, 7),
    (34, 4, 4, 1, 12, 1, False, True, 18),
    (34, 16, 32, 7, 1, 2, False, False, 9),
    (34, 16, 4, 7, 6, 3, True, True, 10),
    (34, 4, 32, 12, 12, 2, False, True, 11),
    (34, 1, 4, 1, 6, 1, True, True, 22),
    (34, 4, 32, 7, 6, 3, True, True, 13),
)
ALPHA, BETA = 0.8, 0.4
UNDECIDED_CAP = 0.10


def grid_id(g):
    return "V%d-K%d-J%d-T%d-L%d-o%d-lex%d-eos%d" % g[:8]


def grid_lens(T):
    """The ragged batch of five: one utterance without a frame."""
    return (T, 0, (T + 1) // 2, 1, max(T - 1, 1))


_CASES = {}


def grid_case(V, K, J, T, L, order, lexicon_only, eos_term, seed):
    """-> (p, [enc_h of the five utterances], the WordLM): the utterances share the head; <space> = V - 1 gets a bias, so
    that words close inside the search and not only at its end; the lexicon holds the words of every utterance's best plain
    hypothesis (so that lexicon words are in reach) beside random ones."""
    key = (V, K, J, T, L, order, lexicon_only, eos_term, seed)
    if key not in _CASES:
        p, _ = BR.grid_case(V, J, 1, 100 + seed, scale=0.7)
        p["lin_out.bias"][V - 1] += 2.0
        rs = np.random.RandomState(1100 + seed)
        utts = [rs.uniform(-1, 1, (t, 16)).astype(np.float32) for t in grid_lens(T)]
        own = []
        for u in utts:
            for f in BR.search(p, u, 1, K, L)["finals"][:2]:
                own += [w for w in WR.split(f["tokens"], V - 1) if len(w) <= 6][:4]
        _CASES[key] = (p, utts, WR.random_word_lm(V, order, 200 + seed, extra_words=own))
    return _CASES[key]


def grid_judge(g, b):
    """The verdict on utterance b of grid row g, computed once per process."""
    p, utts, wlm = grid_case(*g)
    return judge(dict(p=p, enc_h=utts[b], bos=1, K=g[1], L=g[4], table=wlm.compile(), alpha=ALPHA, beta=BETA, eos_term=g[7],
                      lexicon_only=g[6], key=("grid", g, b)))
