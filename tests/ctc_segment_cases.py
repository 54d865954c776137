"""The random cases of the CTC segmentation tests (tests/test_ctc_segment_gpu.py runs them on the device,
tests/test_ctc_segment_cpu.py caps their exemptions over the restatement alone), with their float64 / float32 restatements
(tests/ctc_segment_ref.py), computed once per process and left unchanged.

A case is (V, group, scale, free_ends): a ragged batch of recordings, each (frames, [utterance label lists]).  The groups put
S = 2 L + 1 on both sides of every edge of csrc/ctc_segment.hip's layout, at T' = 2 L + 3:
  small    L in 0, 1, 2, 7, 8 (thread edges of K = 4: S = 5 / 15 / 17), 31, 32 (S = 63 / 65: the 32-state words of the
           backtrace), plus T' = 1, repeats, a tight row, the infeasible kinds and recordings with much more audio than text
  wave4    L in 127, 128 (S = 255 / 257: the first wave of K = 4), 200
  switch   L in 511, 512 (S = 1 023 / 1 025: K = 4 on 256 threads / K = 16 on 128 threads)
  k16      L in 1023, 1024 (S = 2 047 / 2 049: the wave edge of K = 16, and ctc_align's own limit)
  wide     L in 2047, 2048 (S = 4 095 / 4 097: four / five waves of K = 16)
The window of a case is one of 1, 30 and 10**6 (larger than any utterance), by the case's position in GRID."""
import numpy as np

import ctc_segment_ref as SR

VOCABS = (2, 5, 34, 257)
GROUPS = dict(small=(2, 7, 8, 31, 32), wave4=(127, 128, 200), switch=(511, 512), k16=(1023, 1024), wide=(2047, 2048))
WINDOWS = (1, 30, 10 ** 6)
# case -> seed offset, where the default draw misses the cap: at scale 50 a frame's best token has x = -1e-7, which a free end's
# 0 beats by less than any allowance - the default draw has such a frame next to the text of a 17-frame recording
SEED = {(34, "small", 50.0, 1): 1}
N_INFEASIBLE = 4

GRID = ([(V, g, 1.0, f) for V in VOCABS for g in ("small", "wave4") for f in (0, 1)]
        + [(34, g, 50.0, f) for g in ("small", "wave4") for f in (0, 1)]
        + [(V, g, 1.0, f) for V, g in ((34, "switch"), (5, "k16"), (257, "wide"), (2, "wide")) for f in (0, 1)])


def case_id(c):
    return "V%d-%s-x%g-free%d" % c


def labels(rs, V, n, equal=False):
    if equal or V == 2:
        return [int(rs.randint(1, V))] * n
    return [int(v) for v in rs.randint(1, V, size=n)]


def split(rs, ys):
    """A label list -> utterances: a one-label utterance, an empty one, then two to four random pieces (from 3 labels on)."""
    if len(ys) < 3:
        return [list(ys)]
    cuts = sorted(int(c) for c in rs.randint(1, len(ys), size=int(rs.randint(1, 4))))
    edges = [0, 1, 1] + [c for c in cuts if c > 1] + [len(ys)]
    return [list(ys[a:b]) for a, b in zip(edges[:-1], edges[1:])]


def recordings(V, group, seed):
    rs = np.random.RandomState(seed)
    a = int(rs.randint(1, V))
    b = a % (V - 1) + 1 if V > 2 else a
    recs = []
    if group == "small":
        recs += [(1, [[]]), (1, [[a]]), (17, []), (9, [[], []]), (3, [[a], [a]]), (2, [[a, b] if b != a else [a]]),
                 (29, split(rs, labels(rs, V, 13, equal=True))),
                 (40, split(rs, labels(rs, V, 5))), (64, [[a], [], [b]]), (57, [labels(rs, V, 4), labels(rs, V, 1), labels(rs, V, 6)]),
                 # infeasible: 4 labels + 2 repeats (3 where b == a) need > 5 frames; labels outside [1, V); no frames
                 (5, [[a, a], [a, b]]), (7, [[a], [V]]), (6, [[0, a]]), (0, [[a]])]
    for L in GROUPS[group]:
        recs.append((2 * L + 3, split(rs, labels(rs, V, L))))
    L0 = GROUPS[group][0]
    recs.append((2 * L0 - 1, split(rs, labels(rs, V, L0, equal=True))))    # tight: one strict path
    return recs


def allow(f32, ref):
    f32, ref = np.asarray(f32, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err32 = float(np.abs(f32 - ref).max()) if ref.size else 0.0
    floor = 8.0 * float(np.spacing(np.float32(np.abs(ref).max()))) if ref.size else 0.0
    return max(4.0 * err32, floor)


def restated(z, recs, free_ends, window, with_gap=True):
    """The CPU side of a case: per recording the float64 and the float32 restatement, the allowances (max(4 x the float32
    restatement's error, 8 ulp) per tensor: scores, token sums, utterance sums, utterance confidences) and the census."""
    r64 = [SR.segment(z[i, :t].astype(np.float64), u, free_ends, window, with_gap) for i, (t, u) in enumerate(recs)]
    r32 = [SR.segment(z[i, :t], u, free_ends, window, False) for i, (t, u) in enumerate(recs)]
    feas = [i for i, r in enumerate(r64) if r["feasible"]]
    assert [i for i, r in enumerate(r32) if r["feasible"]] == feas

    def cat(rs, name):
        return np.concatenate([np.atleast_1d(np.asarray(rs[i][name], dtype=np.float64)) for i in feas] + [np.zeros(0)])
    allows = {name: allow(cat(r32, name), cat(r64, name)) for name in ("score", "token_logp", "utt_logp", "utt_conf")}
    decisive = {i: r64[i]["gap"] > 2.0 * allows["score"] for i in feas}
    return dict(r64=r64, r32=r32, feasible=feas, allows=allows, decisive=decisive)


_CASES = {}


def case(c):
    if c in _CASES:
        return _CASES[c]
    V, group, scale, free_ends = c
    recs = recordings(V, group, 100 + V)
    rs = np.random.RandomState(7 * V + len(group) + SEED.get(c, 0))
    B, T = len(recs), max(t for t, _ in recs)
    z = (scale * rs.normal(0, 1, size=(B, T, V))).astype(np.float32)
    window = WINDOWS[GRID.index(c) % len(WINDOWS)]
    out = dict(z=z, recs=recs, V=V, free_ends=free_ends, window=window, **restated(z, recs, free_ends, window))
    assert len(out["feasible"]) == B - (N_INFEASIBLE if group == "small" else 0), (c, out["feasible"])
    _CASES[c] = out
    return out
