"""The utterances of tests/test_batch_invariance_gpu.py (and of its CPU companion): every utterance is a dict that carries
everything that belongs to it - logits, length, labels or hypotheses, context graph, RIR and noise indices - and the builders
below lay a LIST of them out as one batch, in any order, on any time extent.  An utterance's outputs must not depend on the
rest of that list.

  arrangements(utts, extra)     the four runs of one case: base, every utterance alone, moved, padded
  frames_batch(...)             [B, T, V + cols] logits (NaN behind every length and in the padding columns), packed labels
  rnnt_batch / joint_batch      the transducer's lattices, U + 1 = the longest label count of the rows given
  mwer_batch, pairs_batch, waves_batch
  ctc_utts, align_utts, rnnt_utts, beam_utts, mwer_utts, edit_pairs, waves     the case tables

Shapes (the issue's): they are the smallest that still reach every switch of the kernels; tests/test_batch_invariance_cpu.py
pins them against the library's limits."""
import numpy as np

import context_ref as C
import ctc_beam_ref as R
import ngram_ref as N
import word_lm_ref as W

EXTRA_FRAMES, EXTRA_COLS = 5, 3                    # the padded run: T + 5 frames, ld = V + 3
EXTRA = -1                                         # the extra utterance's place in an order


# ------------------------------------------------------------------------------------------------- the transformations
def moved_order(n):
    """The moved run's rows as indices into the base batch: the extra utterance (EXTRA) in front, then the base reversed.
    With an even n the reversal alone would leave utterance n / 2 on its row: it changes places with the row behind it, so
    that no utterance keeps its row index."""
    order = [EXTRA] + list(range(n - 1, -1, -1))
    if n % 2 == 0 and n:
        order[n // 2], order[n // 2 + 1] = order[n // 2 + 1], order[n // 2]
    return order


def arrangements(utts, extra):
    """-> [(name, rows, owner, extra_frames, extra_cols)]: the list of utterances of each run, owner[r] = the base index of
    row r (EXTRA: nobody's).  `base` first; `alone` once per utterance."""
    n = len(utts)
    out = [("base", list(utts), list(range(n)), 0, 0)]
    out += [("alone", [utts[b]], [b], 0, 0) for b in range(n)]
    order = moved_order(n)
    out.append(("moved", [extra if i == EXTRA else utts[i] for i in order], order, 0, 0))
    out.append(("padded", list(utts), list(range(n)), EXTRA_FRAMES, EXTRA_COLS))
    return out


# ------------------------------------------------------------------------------------------------- the builders
def frames_batch(utts, extra_frames=0, extra_cols=0):
    """Utterances with z [T_b, V] (and labels y) -> dict(buf float32 [B, T, V + extra_cols] with T = max(T_b, 1) +
    extra_frames, NaN behind every length and in the extra columns; lens; labels packed int64; label_lens; offsets; V)."""
    V = utts[0]["z"].shape[1]
    T = max(max(u["z"].shape[0] for u in utts), 1) + extra_frames
    buf = np.full((len(utts), T, V + extra_cols), np.nan, dtype=np.float32)
    for i, u in enumerate(utts):
        buf[i, :u["z"].shape[0], :V] = u["z"]
    ys = [list(u.get("y", ())) for u in utts]
    lens = [u["z"].shape[0] for u in utts]
    return dict(buf=buf, lens=lens, V=V, T=T, labels=np.array([c for y in ys for c in y], dtype=np.int64),
                label_lens=[len(y) for y in ys], offsets=np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int64),
                g=np.array([u.get("g", 1.0) for u in utts], dtype=np.float32))


def rnnt_batch(utts, extra_frames=0, extra_cols=0):
    """Utterances with z [T_b, U_b + 1, V] -> buf float32 [B, T, U + 1, V + extra_cols], U = the longest label count of
    THESE rows; NaN on every padded node and column."""
    V = utts[0]["z"].shape[2]
    T = max(u["z"].shape[0] for u in utts) + extra_frames
    U = max(len(u["y"]) for u in utts)
    buf = np.full((len(utts), T, U + 1, V + extra_cols), np.nan, dtype=np.float32)
    for i, u in enumerate(utts):
        buf[i, :u["z"].shape[0], :len(u["y"]) + 1, :V] = u["z"]
    return dict(buf=buf, lens=[u["z"].shape[0] for u in utts], V=V, T=T, U=U,
                labels=np.array([c for u in utts for c in u["y"]], dtype=np.int64), label_lens=[len(u["y"]) for u in utts],
                g=np.array([u["g"] for u in utts], dtype=np.float32))


def joint_batch(utts, extra_frames=0):
    """Utterances with pe [T_b, J], pp [U_b + 1, J], dz [T_b, U_b + 1, J] -> the padded arrays, NaN on every padded node."""
    J = utts[0]["pe"].shape[1]
    T = max(u["pe"].shape[0] for u in utts) + extra_frames
    U = max(u["pp"].shape[0] for u in utts) - 1
    pe = np.full((len(utts), T, J), np.nan, dtype=np.float32)
    pp = np.full((len(utts), U + 1, J), np.nan, dtype=np.float32)
    dz = np.full((len(utts), T, U + 1, J), np.nan, dtype=np.float32)
    for i, u in enumerate(utts):
        t, u1 = u["pe"].shape[0], u["pp"].shape[0]
        pe[i, :t], pp[i, :u1], dz[i, :t, :u1] = u["pe"], u["pp"], u["dz"]
    return dict(pe=pe, pp=pp, dz=dz, lens=[u["pe"].shape[0] for u in utts], label_lens=[u["pp"].shape[0] - 1 for u in utts])


def mwer_batch(utts, extra_frames=0, extra_cols=0):
    """Utterances with logits [L_b, K, V], tokens [L_b, K], npos [K], err [K] -> time-major logits float32
    [L, B K, V + extra_cols] (rows r = b K + k; NaN at l >= npos_r and in the extra columns), tokens int64 [L, B K]
    (<EOS>-padded), npos, err int32 [B K]."""
    K, V = utts[0]["logits"].shape[1:]
    L = max(max(u["logits"].shape[0] for u in utts), 1) + extra_frames
    buf = np.full((L, len(utts) * K, V + extra_cols), np.nan, dtype=np.float32)
    tokens = np.full((L, len(utts) * K), MWER_EOS, dtype=np.int64)
    for i, u in enumerate(utts):
        for k in range(K):
            n = max(int(u["npos"][k]), 0)
            buf[:n, i * K + k, :V] = u["logits"][:n, k]
            tokens[:n, i * K + k] = u["tokens"][:n, k]
    return dict(buf=buf, tokens=tokens, npos=np.concatenate([u["npos"] for u in utts]).astype(np.int32),
                err=np.concatenate([u["err"] for u in utts]).astype(np.int32), B=len(utts), K=K, L=L, V=V)


def pairs_batch(pairs, extra_cols=0, ref_order=None):
    """(hypothesis, reference) pairs -> hyp int32 [N, cols], hyp_len, ref int32 [N, rcols], ref_len, ref_index (None: pair p
    scores against reference row p).  ref_order: the place of each pair's reference among the reference rows (a
    permutation); the columns behind a length hold ids no string uses."""
    n = len(pairs)
    cols = max(max(len(p["hyp"]) for p in pairs), 1) + extra_cols
    rcols = max(max(len(p["ref"]) for p in pairs), 1) + extra_cols
    hyp = np.full((n, cols), 10 ** 6, dtype=np.int32)
    ref = np.full((n, rcols), 10 ** 6 + 1, dtype=np.int32)
    place = list(range(n)) if ref_order is None else list(ref_order)
    assert sorted(place) == list(range(n))
    ref_len = np.zeros(n, dtype=np.int32)
    for i, p in enumerate(pairs):
        hyp[i, :len(p["hyp"])] = p["hyp"]
        ref[place[i], :len(p["ref"])] = p["ref"]
        ref_len[place[i]] = len(p["ref"])
    return dict(hyp=hyp, hyp_len=np.array([len(p["hyp"]) for p in pairs], dtype=np.int32), ref=ref, ref_len=ref_len,
                ref_index=None if ref_order is None else np.array(place, dtype=np.int32))


def waves_batch(waves, tail=0):
    """Waveforms (dicts with x float32 [n]) -> packed samples (NaN in `tail` samples behind the last offset), offsets."""
    offsets = np.concatenate([[0], np.cumsum([w["x"].size for w in waves])]).astype(np.int64)
    samples = np.concatenate([w["x"] for w in waves] + [np.full(tail, np.nan, dtype=np.float32)]).astype(np.float32)
    return dict(samples=samples, offsets=offsets, lens=[int(w["x"].size) for w in waves])


# ------------------------------------------------------------------------------------------------- 1, 3: CTC
CTC_V = 34
# (T', labels): 2L + 1 = 63 / 65 straddles the wave, 257 the workgroup - one row on each of the wave, block and strided paths
CTC_SHAPES = ((1, 0), (1, 1), (17, 0), (5, 4), (65, 31), (67, 32), (259, 128))
CTC_INFEASIBLE = 3                                 # (5, [a, a, a, b]): 4 labels + 2 repeats need 6 frames
CTC_EXTRA = (263, 40)
CTC_GRADS = (1.5, 0.0, -0.75, 1.0, -2.0, 0.5, -1.25, 0.875)      # upstream gradients of both signs and 0
_CACHE = {}


def _ctc_all():
    if "ctc" not in _CACHE:
        rs = np.random.RandomState(20240)
        a, b = 7, 19
        utts = []
        for i, (t, n) in enumerate(CTC_SHAPES + (CTC_EXTRA,)):
            y = [a] if n == 1 else [a, a, a, b] if (t, n) == (5, 4) else [int(c) for c in rs.randint(1, CTC_V, size=n)]
            utts.append(dict(z=(3.0 * rs.normal(0, 1, size=(t, CTC_V))).astype(np.float32), y=y, g=CTC_GRADS[i]))
        cannot = dict(z=(3.0 * rs.normal(0, 1, size=(2, CTC_V))).astype(np.float32), y=[a, b, a], g=1.0)
        _CACHE["ctc"] = (utts, cannot)
    return _CACHE["ctc"]


def ctc_utts():
    """-> (utterances, the extra one): item 1."""
    utts, _ = _ctc_all()
    return utts[:-1], utts[-1]


def align_utts():
    """-> (utterances, the extra one): item 1's without the infeasible one, and one with fewer frames than labels."""
    utts, cannot = _ctc_all()
    return [u for i, u in enumerate(utts[:-1]) if i != CTC_INFEASIBLE] + [cannot], utts[-1]


# ------------------------------------------------------------------------------------------------- 2: the transducer
RNNT_V, RNNT_J = 34, 32
RNNT_LATTICES = ((1, 0), (1, 1), (7, 0), (7, 3), (20, 9))
RNNT_EXTRA = (23, 11)


def rnnt_utts():
    if "rnnt" not in _CACHE:
        rs = np.random.RandomState(20241)
        utts = []
        for t, u in RNNT_LATTICES + (RNNT_EXTRA,):
            utts.append(dict(z=rs.uniform(-3, 3, (t, u + 1, RNNT_V)).astype(np.float32),
                             y=[int(c) for c in rs.randint(1, RNNT_V, size=u)],
                             g=np.float32(rs.uniform(0.5, 1.5) * rs.choice([-1.0, 1.0])),
                             pe=rs.uniform(-1.5, 1.5, (t, RNNT_J)).astype(np.float32),
                             pp=rs.uniform(-1.5, 1.5, (u + 1, RNNT_J)).astype(np.float32),
                             dz=rs.uniform(-1, 1, (t, u + 1, RNNT_J)).astype(np.float32)))
        _CACHE["rnnt"] = utts
    return _CACHE["rnnt"][:-1], _CACHE["rnnt"][-1]


# ------------------------------------------------------------------------------------------------- 4: the CTC beam search
# graph: the utterance's context graph (0, 1: the case's two graphs; -1: none).  (a) one wave, history in LDS; (b) row 0
# writes its history to the workspace, row 1 is at the LDS limit beside it; (c) K V above one wave's: four waves.
BEAM = dict(a=dict(V=34, K=4, lens=(0, 1, 7, 100), graph=(0, 1, -1, 1), extra=(120, 0)),
            b=dict(V=5, K=16, lens=(257, 256, 3, 0), graph=(0, 1, -1, 1), extra=(300, 0)),
            c=dict(V=260, K=4, lens=(7, 2), graph=(1, -1), extra=(9, 0)))
MODES = ("plain", "ngram", "word_lm", "word_lm_lexicon", "context", "context_ngram")
MODE_OUTPUTS = dict(plain=("hyp", "hyp_len", "score"), ngram=("hyp", "hyp_len", "score", "ctc_score", "lm_score"),
                    word_lm=("hyp", "hyp_len", "score", "ctc_score", "lm_score", "n_words"),
                    word_lm_lexicon=("hyp", "hyp_len", "score", "ctc_score", "lm_score", "n_words"),
                    context=("hyp", "hyp_len", "score", "ctc_score", "ctx_score"),
                    context_ngram=("hyp", "hyp_len", "score", "ctc_score", "lm_score", "ctx_score"))
NGRAM_WEIGHTS = C.LM_WEIGHTS                       # alpha, beta: the context grid's
WORD_LM_WEIGHTS = W.WEIGHTS[1]                     # alpha, beta: the word LM grid's second pair
CTX_WEIGHT = C.WEIGHTS[2]


def beam_utts(name):
    """-> (utterances, the extra one, fixtures): fixtures = dict(graphs: the case's two ContextGraphs - the second with
    word_start_only where V allows a <space> -, ngram, word_lm), from the builders of the modes' own GPU modules."""
    key = "beam_" + name
    if key not in _CACHE:
        spec = BEAM[name]
        V = spec["V"]
        rs = np.random.RandomState(20242 + V)
        utts = [dict(z=rs.normal(0, 1, size=(t, V)).astype(np.float32), graph=g)
                for t, g in zip(spec["lens"] + spec["extra"][:1], spec["graph"] + spec["extra"][1:])]
        seed = R.case_seed(V, spec["K"], max(spec["lens"]), 1.0)
        space = V - 1 if V > 5 else None
        g0 = C.ContextGraph(*C.random_phrases(V, 4 if V <= 5 else 30, seed), V=V)
        p1, b1 = C.random_phrases(V, 3 if V <= 5 else 20, seed + 1, space)
        g1 = C.ContextGraph(p1, b1, V=V, word_start_only=space)
        own = []
        for u in utts:                                           # (word_lm_ref.grid_case: lexicon words in reach)
            best = R.collapse(np.argmax(u["z"], axis=1)) if u["z"].shape[0] else ()
            own += [w for w in W.split(best, V - 1) if len(w) <= 6][:8]
        fixtures = dict(graphs=[g0, g1], ngram=N.random_lm(V, 2, seed + 2), word_lm=W.random_word_lm(V, 2, seed + 3, extra_words=own))
        _CACHE[key] = (utts[:-1], utts[-1], fixtures)
    return _CACHE[key]


def graph_index(utts, name):
    """-> (the order of the case's graphs in this run's ContextBatch, graph_of): base and padded keep the graphs' order;
    moved swaps them, so that no row's graph index is its row index; alone holds the utterance's own graph only."""
    ids = [u["graph"] for u in utts]
    if name == "alone":
        return ([ids[0]], [0]) if ids[0] >= 0 else ([0], [-1])
    if name == "moved":
        return [1, 0], [1 - i if i >= 0 else -1 for i in ids]
    return [0, 1], ids


def beam_kwargs(mode, fixtures, utts, name):
    """The keyword arguments of ops.ctc_beam for `mode` on this run's rows."""
    from context import ContextBatch
    kw = {}
    if mode in ("ngram", "context_ngram"):
        kw.update(ngram=fixtures["ngram"], ngram_weight=NGRAM_WEIGHTS[0], ngram_bonus=NGRAM_WEIGHTS[1])
    if mode.startswith("word_lm"):
        kw.update(word_lm=fixtures["word_lm"], word_lm_weight=WORD_LM_WEIGHTS[0], word_bonus=WORD_LM_WEIGHTS[1],
                  lexicon_only=mode == "word_lm_lexicon")
    if mode.startswith("context"):
        order, graph_of = graph_index(utts, name)
        kw.update(context=ContextBatch([fixtures["graphs"][i] for i in order], graph_of), ctx_weight=CTX_WEIGHT)
    return kw


# ------------------------------------------------------------------------------------------------- 5: MWER
MWER_V, MWER_K, MWER_L, MWER_EOS = 34, 4, 6, 2
MWER_SCALE, MWER_G = 0.25, -1.5                    # arguments of the call, the same in every run
# positions per hypothesis (its length + 1 for <EOS>; 0: an unused slot): the empty hypothesis, L positions, an unused slot
MWER_NPOS = ((1, 6, 3, 4), (6, 0, 2, 5), (3, 3, 1, 4))
MWER_EXTRA_NPOS = (9, 7, 2, 8)


def mwer_utts():
    if "mwer" not in _CACHE:
        rs = np.random.RandomState(20243)
        utts = []
        for npos in MWER_NPOS + (MWER_EXTRA_NPOS,):
            L = max(npos)
            tokens = rs.randint(3, MWER_V, size=(L, MWER_K)).astype(np.int64)
            for k, n in enumerate(npos):
                tokens[max(n - 1, 0):, k] = MWER_EOS
            utts.append(dict(logits=(2.0 * rs.normal(0, 1, size=(L, MWER_K, MWER_V))).astype(np.float32), tokens=tokens,
                             npos=np.array(npos, dtype=np.int32), err=rs.randint(0, 6, size=MWER_K).astype(np.int32)))
        _CACHE["mwer"] = utts
    return _CACHE["mwer"][:-1], _CACHE["mwer"][-1]


# ------------------------------------------------------------------------------------------------- 6: edit distances
ED_SPACE = 4                                       # letters from 5 up
ED_LENGTHS = ((0, 0), (0, 2), (5, 0), (9, 9), (12, 15), (70, 64), (130, 129), (None, 37))      # None: ED_MAX_COLS


def edit_pairs(ed_max):
    """Eight (hypothesis, reference) pairs: empty on either side and on both, equal strings, and a hypothesis of `ed_max`
    tokens -> (pairs, the extra one).  No row may be longer than ed_max, so the extra pair cannot be strictly longer than
    that hypothesis: it is at the limit on BOTH sides, which makes the reference extent of the moved run the longest."""
    key = "ed_%d" % ed_max
    if key not in _CACHE:
        rs = np.random.RandomState(20244)

        def draw(n):
            return [int(c) for c in rs.choice([ED_SPACE, 5, 6, 7, 8, 9], size=n, p=[0.25, 0.15, 0.15, 0.15, 0.15, 0.15])]
        pairs = []
        for nh, nr in ED_LENGTHS + ((None, None),):
            hyp, ref = draw(ed_max if nh is None else nh), draw(ed_max if nr is None else nr)
            if (nh, nr) == (9, 9):
                ref = list(hyp)
            pairs.append(dict(hyp=hyp, ref=ref))
        _CACHE[key] = pairs
    return _CACHE[key][:-1], _CACHE[key][-1]


def moved_ref_order(n):
    """The place of each moved pair's reference: the references stay in the BASE order with the extra one last, while the
    hypotheses are reversed behind the extra one - ref_index is no identity."""
    return [n if i == EXTRA else i for i in moved_order(n)]


# ------------------------------------------------------------------------------------------------- 7: the front end
WAVE_SAMPLES, WAVE_EXTRA = (1, 400, 1101), 1500    # in-batch offsets 0, 1, 401, 1502: odd; alone every row starts at 0
SPEEDS = (0.9, 1.0, 1.1)
FE_CFG = dict(n_mels=8, delta_order=2, cmvn="utterance")


def waves():
    """-> (waveforms, the extra one, banks): every waveform carries its factor, RIR and clip indices, start and scale;
    banks = dict(rirs, clips)."""
    if "waves" not in _CACHE:
        rs = np.random.RandomState(20245)
        rows = []
        for n, f, rir, clip, start, scale in zip(WAVE_SAMPLES + (WAVE_EXTRA,), (0, 2, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 0),
                                                 (3, 0, 50, 7), (0.5, 0.3, 0.1, 0.2)):
            rows.append(dict(x=(0.3 * rs.normal(0, 1, size=n)).astype(np.float32), factor=f, rir=rir, clip=clip, start=start,
                             scale=np.float32(scale)))
        rirs = [(rs.normal(0, 1, size=n) * np.exp(-np.arange(n) / 40.0)).astype(np.float32) for n in (300, 64)]
        clips = [(0.1 * rs.normal(0, 1, size=n)).astype(np.float32) for n in (777, 130)]
        _CACHE["waves"] = (rows[:-1], rows[-1], dict(rirs=rirs, clips=clips))
    return _CACHE["waves"]
