"""A restatement of the transducer beam search (csrc/rnnt_beam.hip) that needs no GPU: dictionaries keyed by
the label sequence, on rnnt_ref.py's head, in the dtype asked for.  float64 is the reference; float32 - the same recurrences
in the same order - is the yardstick of the allowance.

    search(...)    one utterance -> dict(finals, steps, finalised)
    judge(case)    the float64 and the float32 search of a case, the allowance and whether the case is decisive
    grid_case(..)  the seeded inputs the CPU and the GPU tests share

The search: at iteration i every entry has t + u = i.  Every entry proposes its blank (same sequence, (t + 1, u)) and, while
u < L, its V - 1 labels ((t, u + 1)); candidates of one sequence are ONE candidate with the logaddexp of their masses, which
keeps the flat index (parent V + token, blank = token 0) and the prediction state of its BLANK parent; the best K by rank
(greater first, the lower flat index on ties) are the next beam.  A blank taken at t = T - 1 is a final.  rank = tot, or
with an LM (tot + alpha lm) + beta u."""
import numpy as np

import rnnt_ref as R


def _lae(a, b, dt):
    m, n = (a, b) if a > b else (b, a)
    if n == -np.inf:
        return dt(m)
    return dt(m + np.log1p(np.exp(dt(n - m), dtype=dt), dtype=dt))


def _rank(tot, lm, u, alpha, beta, dt, fused):
    if not fused:
        return dt(tot)
    return dt(dt(dt(tot) + dt(dt(alpha) * dt(lm))) + dt(dt(beta) * dt(u)))


def search(p, enc_h, bos, K, L, dt=np.float64, table=None, alpha=0.0, beta=0.0, eos_term=True):
    """One utterance: p the head's parameters (numpy), enc_h [T, H]; table an ngram.NgramTable on the host or None.
    -> dict(finals: every final ever made, ranked, as dicts(tokens, tot, lm, rank, it, label_lp); steps: per iteration
    dict(kept: [(tokens, tot, rank)], gap: the rank gap between the last kept and the first rejected candidate, inf without
    one); finalised: the sequences in the order they finalised).  The caller takes finals[:K]."""
    p = {k: np.asarray(v).astype(dt) for k, v in p.items()}
    enc_h = np.asarray(enc_h)
    T = enc_h.shape[0]
    fused = table is not None
    logp = table.logp.astype(dt) if fused else None
    eos = table.eos if (fused and eos_term) else -1
    if T == 0:
        lm0 = dt(logp[table.start, eos]) if eos >= 0 else dt(0)
        return dict(finals=[dict(tokens=(), tot=dt(0), lm=lm0, rank=_rank(dt(0), lm0, 0, alpha, beta, dt, fused), it=-1,
                                 label_lp=dt(0))], steps=[], finalised=[()])
    pe = enc_h.astype(dt) @ p["lin_enc.weight"].T + p["lin_enc.bias"]
    V = p["lin_out.weight"].shape[0]
    zero = np.zeros(p["lstm.weight_hh_l0"].shape[1], dt)
    h, c = R._cell(p, bos, zero, zero, np)
    beam = [dict(seq=(), tot=dt(0), lm=dt(0), state=table.start if fused else 0, h=h, c=c, pp=p["lin_pred.weight"] @ h,
                 label_lp=dt(0))]
    finals, steps, finalised = [], [], []
    for it in range(T + L):
        if not beam:
            break
        cands = {}
        rows = []
        for hi, e in enumerate(beam):
            t = it - len(e["seq"])
            assert 0 <= t < T
            lg = p["lin_out.weight"] @ np.tanh(pe[t] + e["pp"], dtype=dt) + p["lin_out.bias"]
            mx = lg.max()
            rows.append((lg - dt(mx + np.log(np.exp(lg - mx, dtype=dt).sum(dtype=dt), dtype=dt))).astype(dt))
        for hi, e in enumerate(beam):                               # the blanks first: a merged candidate is its blank parent's
            u = len(e["seq"])
            tot = dt(e["tot"] + rows[hi][0])
            if it - u == T - 1:
                lm = dt(e["lm"] + logp[e["state"], eos]) if eos >= 0 else e["lm"]
                finals.append(dict(tokens=e["seq"], tot=tot, lm=lm, rank=_rank(tot, lm, u, alpha, beta, dt, fused), it=it,
                                   slot=hi, label_lp=e["label_lp"]))
                finalised.append(e["seq"])
            else:
                cands[e["seq"]] = dict(seq=e["seq"], tot=tot, lm=e["lm"], state=e["state"], flat=hi * V, parent=hi, tok=0,
                                       label_lp=e["label_lp"])
        for hi, e in enumerate(beam):
            if len(e["seq"]) >= L:
                continue
            for k in range(1, V):
                seq = e["seq"] + (k,)
                tot = dt(e["tot"] + rows[hi][k])
                if seq in cands:
                    assert cands[seq]["tok"] == 0                   # only a blank candidate can be met: one partner, two terms
                    cands[seq]["tot"] = _lae(cands[seq]["tot"], tot, dt)
                    continue
                cands[seq] = dict(seq=seq, tot=tot, lm=dt(e["lm"] + logp[e["state"], k]) if fused else dt(0),
                                  state=int(table.nxt[e["state"], k]) if fused else 0, flat=hi * V + k, parent=hi, tok=k,
                                  label_lp=dt(e["label_lp"] + rows[hi][k]))
        for cd in cands.values():
            cd["rank"] = _rank(cd["tot"], cd["lm"], len(cd["seq"]), alpha, beta, dt, fused)
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
            new.append(dict(seq=cd["seq"], tot=cd["tot"], lm=cd["lm"], state=cd["state"], h=h, c=c, pp=pp,
                            label_lp=cd["label_lp"]))
        beam = new
    assert not beam
    # ranked: greater first; the earlier final, then the lower slot, on ties
    finals.sort(key=lambda f: (-f["rank"], f["it"], f["slot"]))
    return dict(finals=finals, steps=steps, finalised=finalised)


ULP = 2.0 ** -23


def judge(case):
    """case: dict(p, enc_h [T, H], bos, K, L and optionally table, alpha, beta, eos_term).  -> dict(ref: the float64 search,
    f32: the float32 search, allowance: 4 x the float32 search's worst error against float64 on a kept candidate or a final -
    at least 8 fp32 ulps of the largest score -, decisive: at every selection and in the final list the float64 gap between
    the last kept and the first rejected rank exceeds twice the allowance accumulated so far, the same between neighbours
    of the final list, and the float32 search keeps the float64 search's candidates)."""
    kw = dict(table=case.get("table"), alpha=case.get("alpha", 0.0), beta=case.get("beta", 0.0),
              eos_term=case.get("eos_term", True))
    ref = search(case["p"], case["enc_h"], case["bos"], case["K"], case["L"], np.float64, **kw)
    f32 = search(case["p"], case["enc_h"], case["bos"], case["K"], case["L"], np.float32, **kw)
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
    return dict(ref=ref, f32=f32, allowance=allow, decisive=decisive)


def grid_case(V, J, T, seed, E=16, P=16, H=16, blank_bias=0.5, scale=1.5):
    """Seeded head parameters and one utterance of T frames -> (p, enc_h [T, H] float32)."""
    p = R.head_params(V, E, P, H, J, seed, blank_bias, scale)
    enc_h = np.random.RandomState(seed + 1000).uniform(-1, 1, (T, H)).astype(np.float32)
    return p, enc_h


def tie_params(V, J, seed, E=16, P=16, H=16):
    """A head whose lin_out is zero: every candidate of an entry ties."""
    p = R.head_params(V, E, P, H, J, seed)
    p["lin_out.weight"][:] = 0
    p["lin_out.bias"][:] = 0
    return p


# (V, K, J, T of the three utterances - one without a frame -, L, seed): the GPU grid, thinned to both sides of what the step
# kernel's work depends on - V below / past a wave's 64 lanes, J below / past one lane stride (64) and past 256, one entry /
# several / kKmax, fewer candidates than K (V = 3, L = 1), more (entry, token) pairs than waves, T' = 1 (every blank a final),
# L = 1 (the label cap binds at once) and L = 40 > T' (the cap never binds)
GRID = (
    (3, 1, 4, (1, 0, 2), 1, 1),
    (3, 16, 4, (2, 0, 1), 4, 2),
    (3, 4, 32, (7, 0, 2), 4, 3),
    (34, 1, 32, (7, 0, 1), 4, 4),
    (34, 2, 260, (2, 0, 7), 4, 5),
    (34, 4, 32, (33, 0, 7), 4, 6),
    (34, 16, 32, (7, 0, 2), 40, 7),
    (65, 2, 32, (7, 0, 1), 4, 8),
    (65, 4, 260, (2, 0, 7), 1, 9),
    (65, 16, 4, (7, 0, 2), 4, 10),
)


def grid_utterances(V, K, J, lens, L, seed):
    """-> (p, [enc_h of every utterance]) of one GRID row; the utterances share the head."""
    p, _ = grid_case(V, J, 1, seed)
    rs = np.random.RandomState(seed + 1000)
    return p, [rs.uniform(-1, 1, (t, 16)).astype(np.float32) for t in lens]
