"""CTC segmentation without a GPU: the numpy restatement (tests/ctc_segment_ref.py) against tests/ctc_align_ref.py - equal to
it without free ends, the best strict alignment over all windows of frames with them -, the utterance fields against direct
loops, the header's declarations, hb.ctc_segment_ws_bytes on plain integers, and the exemption census of the GPU grid."""
import os
import re

import numpy as np
import pytest

import ctc_align_ref as R
import ctc_segment_cases as C
import ctc_segment_ref as SR

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_without_free_ends_it_is_the_alignment(dt):
    """tests/test_ctc_align_gpu.py's kind of random cases (ragged, repeats, infeasible rows, up to 200 labels): every field
    the two restatements share is equal, the gap included."""
    rs = np.random.RandomState(3)
    n = 0
    for V in (2, 5, 34):
        a = int(rs.randint(1, V))
        utts = [(1, []), (1, [a]), (17, []), (3, [a, a]), (5, [a, a, a, a]), (29, C.labels(rs, V, 13, equal=True)), (7, [a, V]),
                (6, [0, a]), (0, [a]), (65, C.labels(rs, V, 31)), (67, C.labels(rs, V, 32)), (403, C.labels(rs, V, 200))]
        for T, y in utts:
            z = rs.normal(0, 1, size=(T, V)).astype(dt)
            want, got = R.align(z, y), SR.segment(z, C.split(rs, y), free_ends=False, window=7)
            assert got["feasible"] == want["feasible"]
            for name in ("score", "path", "first", "last", "token_logp", "gap"):
                assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), (V, T, name)
            if want["feasible"]:
                assert np.array_equal(got["states"], want["states"]) and got["score"].dtype == dt
                n += 1
            else:
                assert (got["utt_begin"] == -1).all() and (got["utt_end"] == -1).all()
                assert np.isneginf(got["utt_logp"]).all() and np.isneginf(got["utt_conf"]).all()
    assert n >= 20


@pytest.mark.parametrize("T,V,y", [(1, 3, [1]), (5, 3, [2]), (7, 3, [1, 1]), (9, 4, [1, 2, 2]), (12, 4, [3, 1, 2, 1]), (12, 3, [2, 2, 2, 1]),
                                   (3, 3, [1, 2])])
def test_free_ends_are_the_best_window(T, V, y):
    """float64: a free path is a strict path on its own window of frames, so the free score is the maximum over all windows
    [t0, t1] of the strict alignment of z[t0 : t1 + 1]; and the frames of the free path that are inside the text are such a
    window, whose strict score is the free score."""
    for seed in range(4):
        z = np.random.RandomState(100 * T + seed).normal(0, 2, size=(T, V))
        free = SR.segment(z, [y], free_ends=True, window=3)
        best = -np.inf
        for t0 in range(T):
            for t1 in range(t0, T):
                best = max(best, _strict(z, t0, t1, y))
        assert free["feasible"] == (best > -np.inf)
        if not free["feasible"]:
            continue
        assert abs(float(free["score"]) - best) <= 1e-12
        inside = np.nonzero(free["path"] != SR.OUTSIDE)[0]
        t0, t1 = int(inside[0]), int(inside[-1])
        assert inside.tolist() == list(range(t0, t1 + 1))
        assert abs(_strict(z, t0, t1, y) - best) <= 1e-12
        assert R.collapse(free["path"][t0:t1 + 1]) == y and free["gap"] >= -1e-12
        assert free["utt_begin"][0] == free["first"][0] and free["utt_end"][0] == free["last"][-1]
        # the text's own frames start and end with a label: free blanks are never cheaper inside than outside
        assert free["first"][0] == t0 and free["last"][-1] == t1


def _strict(z, t0, t1, y):
    """The strict alignment's score on the frames t0 .. t1 alone."""
    return float(R.align(z[t0:t1 + 1], y, with_gap=False)["score"])


def test_l0_and_the_outside_frames():
    z = np.random.RandomState(1).normal(0, 1, size=(6, 4))
    for utts in ([], [[]], [[], []]):
        free = SR.segment(z, utts, free_ends=True)
        assert free["feasible"] and free["score"] == 0 and (free["path"] == SR.OUTSIDE).all()
        assert free["utt_begin"].tolist() == [-1] * len(utts) and free["utt_logp"].tolist() == [0.0] * len(utts)
        strict = SR.segment(z, utts, free_ends=False)
        assert (strict["path"] == 0).all() and strict["score"] == R.align(z, [])["score"]


def test_utterance_fields_against_direct_loops():
    """utt_begin / utt_end from the spans, utt_logp and utt_conf recomputed with python floats; an empty utterance between two
    others takes no frames and leaves its neighbours' fields alone."""
    rs = np.random.RandomState(8)
    z = rs.normal(0, 2, size=(60, 6))
    utts = [[1, 2, 3, 1], [], [4], [5, 5, 2]]
    flat = [k for u in utts for k in u]
    for window in (1, 4, 30, 1000):
        for free in (False, True):
            r = SR.segment(z, utts, free_ends=free, window=window)
            x = R.log_probs(z)
            tok = np.where(r["path"] == SR.OUTSIDE, 0, r["path"])
            assert np.array_equal(r["fx"], x[np.arange(60), tok])
            o = 0
            for u, labels in enumerate(utts):
                if not labels:
                    assert (r["utt_begin"][u], r["utt_end"][u], r["utt_logp"][u], r["utt_conf"][u]) == (-1, -1, 0.0, 0.0)
                    continue
                bg, en = int(r["first"][o]), int(r["last"][o + len(labels) - 1])
                o += len(labels)
                assert (r["utt_begin"][u], r["utt_end"][u]) == (bg, en)
                vals = [float(x[t, tok[t]]) for t in range(bg, en + 1)]
                total = 0.0
                for v in vals:
                    total += v
                assert r["utt_logp"][u] == total
                means = []
                for i in range(0, len(vals), window):
                    s = 0.0
                    for v in vals[i:i + window]:
                        s += v
                    means.append(s / len(vals[i:i + window]))
                assert r["utt_conf"][u] == min(means)
                if window >= len(vals):
                    assert r["utt_conf"][u] == total / len(vals)
                if window == 1:
                    assert r["utt_conf"][u] == min(vals)
            same = SR.segment(z, [u for u in utts if u], free_ends=free, window=window)
            keep = [i for i, u in enumerate(utts) if u]
            assert np.array_equal(same["path"], r["path"]) and np.array_equal(same["utt_conf"], r["utt_conf"][keep])
            assert r["token_logp"].shape == (len(flat),)


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert re.search(r"^#define ASR_CTC_SEG_MAX_LABELS 8191$", header, flags=re.M)
    assert re.search(r"^int asr_ctc_segment_ws_bytes\(int B, int T, int V, int max_label_len, int64_t\* ws_bytes\);", header, flags=re.M)
    decl = re.search(r"^int asr_ctc_segment_f32\(([^;]*)\);", header, flags=re.M).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"\s+", " ", decl).split(",")]
    assert names == ["B", "T", "V", "logits", "ld", "frame_lens", "labels", "label_offsets", "max_label_len", "free_ends", "N",
                     "utt_offsets", "rec_utts", "window", "path", "score", "first", "last", "token_logp", "utt_begin", "utt_end",
                     "utt_logp", "utt_conf", "ws", "ws_bytes", "stream"]
    assert re.search(r"^#define ASR_ABI_VERSION 8$", header, flags=re.M)
    entry.build()
    import hip_backend as hb
    assert hb.ABI_VERSION == 8 and hb.load().asr_abi_version() == 8
    assert {"asr_ctc_segment_ws_bytes", "asr_ctc_segment_f32"} <= set(hb.EXPORTS)
    assert hb.CTC_SEG_MAX_LABELS == 8191


def test_ws_bytes_on_plain_integers():
    """hb.ctc_segment_ws_bytes needs no GPU; it is the header's formula: 8 B T W + 12 R with W = ceil((2 L + 1) / 32) and
    R = B T rounded up to 64; V < 2 and 8 192 labels are refused."""
    entry.build()
    import hip_backend as hb

    def formula(B, T, L):
        return 8 * B * T * ((2 * L + 1 + 31) // 32) + 12 * ((B * T + 63) // 64 * 64)
    for B, T, V, L in ((32, 100, 34, 100), (1, 1, 2, 0), (3, 7, 5, 2), (1, 65, 5, 15), (1, 65, 5, 16), (2, 4099, 257, 2048),
                       (8, 7500, 34, 8000), (1, 8200, 5, hb.CTC_SEG_MAX_LABELS), (64, 20000, 34, hb.CTC_SEG_MAX_LABELS)):
        assert hb.ctc_segment_ws_bytes(B, T, V, L) == formula(B, T, L), (B, T, V, L)
    assert hb.ctc_segment_ws_bytes(64, 20000, 34, 8191) > 2 ** 32                # 64-bit arithmetic
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_segment_ws_bytes(2, 10, 1, 3)
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_segment_ws_bytes(2, 10, 5, hb.CTC_SEG_MAX_LABELS + 1)
    with pytest.raises(RuntimeError):
        hb.ctc_segment_ws_bytes(0, 10, 5, 3)


def test_ops_refuses_before_any_launch():
    """Counts that do not sum to the packed labels and window < 1 are ValueErrors, 8 192 labels in one recording and V = 1 are
    UnsupportedShape - all on the host, before any launch (CPU tensors never reach a kernel)."""
    import torch
    entry.build()
    import hip_backend as hb
    import ops
    before = dict(hb.LAUNCHES)
    z, lens, ys = torch.zeros(1, 4, 5), torch.tensor([4], dtype=torch.int32), torch.ones(3, dtype=torch.long)
    with pytest.raises(ValueError, match="sum to"):
        ops.ctc_segment(z, lens, ys, [[1, 1]])
    with pytest.raises(ValueError, match="window"):
        ops.ctc_segment(z, lens, ys, [[1, 2]], window=0)
    with pytest.raises(ValueError, match="recordings"):
        ops.ctc_segment(z, lens, ys, [[1, 2], []])
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_segment(z, lens, torch.ones(8192, dtype=torch.long), [[8000, 192]])
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_segment(torch.zeros(1, 4, 1), lens, torch.zeros(0, dtype=torch.long), [[]])
    assert dict(hb.LAUNCHES) == before


def test_exemption_cap():
    """Over the restatement alone: at most 1 in 8 of the feasible recordings of the GPU grid non-decisive (gap <= 2 x
    allowance), none of those with T' <= 64."""
    total = loose = 0
    for c in C.GRID:
        k = C.case(c)
        for i in k["feasible"]:
            total += 1
            if not k["decisive"][i]:
                loose += 1
                assert k["recs"][i][0] > 64, (c, i, k["r64"][i]["gap"], k["allows"]["score"])
    print("ctc_segment_parity census: %d feasible recordings, %d non-decisive" % (total, loose))
    assert total >= 8 * len(C.GRID) // 2 and 8 * loose <= total
