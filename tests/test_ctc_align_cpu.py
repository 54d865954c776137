"""CTC forced alignment and best-path decoding without a GPU: the numpy restatement (tests/ctc_align_ref.py) against the
enumeration of every frame path, the tie rule on all-equal logits, and hb.ctc_align_ws_bytes on plain integers."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_align_ref as R

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T,V", [(1, 3), (2, 3), (4, 3), (6, 3), (5, 4)])
def test_restatement_against_enumeration(T, V):
    """All V^T frame paths in float64: per label sequence (every one up to length T) the best score over the paths that
    collapse to it is the restatement's score, attained by the restatement's path; no such path <=> infeasible; the best
    path's probability is at most the sum over all of them (F.ctc_loss); the best-path decode is the collapse of the frame
    argmax, which is the best of ALL paths."""
    rs = np.random.RandomState(10 * T + V)
    z = rs.normal(0, 2, size=(T, V))
    x = R.log_probs(z)
    best = {}
    for path in itertools.product(range(V), repeat=T):
        key = tuple(R.collapse(path))
        sc = float(sum(x[t, k] for t, k in enumerate(path)))
        if key not in best or sc > best[key]:
            best[key] = sc
    # accumulated rounding of T additions in another order: a few float64 ulps of the score
    eps = 64 * np.finfo(np.float64).eps
    n_feasible = 0
    for L in range(T + 1):
        for labels in itertools.product(range(1, V), repeat=L):
            res = R.align(z, list(labels))
            assert res["feasible"] == (labels in best), labels
            if not res["feasible"]:
                assert res["score"] == -np.inf and (res["path"] == -1).all() and (res["first"] == -1).all()
                assert np.isneginf(res["token_logp"]).all()
                continue
            n_feasible += 1
            assert abs(res["score"] - best[labels]) <= eps * max(1.0, abs(best[labels])), labels
            assert R.collapse(res["path"]) == list(labels)
            assert abs(float(R.path_score(x, res["path"])) - best[labels]) <= eps * max(1.0, abs(best[labels]))
            assert res["gap"] >= -eps * max(1.0, abs(best[labels]))
            for i, k in enumerate(labels):
                span = res["path"][res["first"][i]:res["last"][i] + 1]
                assert (span == k).all() and res["last"][i] >= res["first"][i]
            total = res["token_logp"].sum() + x[res["path"] == 0, 0].sum()
            assert abs(total - res["score"]) <= eps * max(1.0, abs(res["score"]))
            if L > 0:
                nll = F.ctc_loss(torch.from_numpy(x).unsqueeze(1), torch.tensor([labels]), torch.tensor([T]), torch.tensor([L]),
                                 blank=0, reduction="none", zero_infinity=False)
                assert res["score"] <= -float(nll) + eps * max(1.0, abs(float(nll))), labels
    assert n_feasible == len(best)
    frame_tok, ids = R.best_path(z)
    assert frame_tok.tolist() == z.argmax(-1).tolist() and ids == R.collapse(z.argmax(-1))
    top = max(best.items(), key=lambda kv: kv[1])
    assert tuple(ids) == top[0]


def test_tie_rule_on_all_equal_logits():
    """Every path ties (each frame gives -log V whatever the token).  Forward, `stay` wins wherever the state was reachable a
    frame earlier, so a state's stored choice is a move only at the EARLIEST frame the state can be reached; the end takes
    S - 1, the trailing blank.  Going back the path therefore stays in every state down to that earliest frame: the labels
    take the earliest frames and the trailing blank takes the rest."""
    for dt in (np.float64, np.float32):
        z = np.zeros((9, 4), dtype=dt)
        res = R.align(z, [2, 2, 3])
        # earliest frames of the states 0 .. 6 of (0 2 0 2 0 3 0): 0 0 1 2 3 3 4 - the repeat 2 2 needs its blank, 2 -> 3 skips it
        assert res["feasible"] and abs(res["gap"]) <= 64 * np.finfo(dt).eps * 9 * np.log(4)      # (v + g: other roundings)
        assert res["states"].tolist() == [1, 2, 3, 5, 6, 6, 6, 6, 6]
        assert res["path"].tolist() == [2, 0, 2, 3, 0, 0, 0, 0, 0]
        assert res["first"].tolist() == [0, 2, 3] and res["last"].tolist() == [0, 2, 3]
        assert abs(float(res["score"]) + 9 * np.log(4)) <= 16 * np.finfo(dt).eps * 9 * np.log(4)
        # a tight row: exactly one path
        tight = R.align(np.zeros((4, 4), dtype=dt), [2, 2, 3])
        assert tight["path"].tolist() == [2, 0, 2, 3] and tight["gap"] == np.inf
        assert not R.align(np.zeros((3, 4), dtype=dt), [2, 2, 3])["feasible"]
        empty = R.align(np.zeros((3, 4), dtype=dt), [])
        assert empty["feasible"] and empty["path"].tolist() == [0, 0, 0]
        assert not R.align(np.zeros((3, 4), dtype=dt), [4])["feasible"] and not R.align(np.zeros((0, 4), dtype=dt), [])["feasible"]


def test_best_path_rules():
    nan, inf = np.nan, np.inf
    z = np.array([[0, 1, 1, nan], [nan, nan, nan, nan], [-inf, -inf, -inf, -inf], [0, 0, 3, 3], [0, 0, 3, 3], [5, 0, 0, 0],
                  [0, 0, 3, 3], [nan, 2, inf, 1]], dtype=np.float32)
    frame_tok, ids = R.best_path(z)
    assert frame_tok.tolist() == [1, 0, 0, 2, 2, 0, 2, 2] and ids == [1, 2, 2]


def test_ws_bytes_on_plain_integers():
    """hb.ctc_align_ws_bytes needs no GPU; it is the header's formula: 8 R with R = B T rounded up to 64, plus 16 B T W with
    W = ceil((2 L + 1) / 64) when T W 16 exceeds the LDS budget; V < 2 and 1 024 labels are refused."""
    entry.build()
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    budget = int(re.search(r"#define ASR_CTC_ALIGN_LDS_BYTES (\d+)", header).group(1))
    assert budget == hb.CTC_ALIGN_LDS_BYTES and budget % 16 == 0
    source = open(os.path.join(ROOT, "semi-supervised-asr_amd", "csrc", "ctc_align.hip")).read()
    assert "constexpr int kBpLdsBytes = ASR_CTC_ALIGN_LDS_BYTES;" in source

    def formula(B, T, L):
        R_ = (B * T + 63) // 64 * 64
        W = (2 * L + 1 + 63) // 64
        return 8 * R_ + (16 * B * T * W if T * W * 16 > budget else 0)
    for B, T, V, L in ((32, 100, 34, 100), (8, 200, 34, 100), (1, 1, 2, 0), (3, 7, 5, 2), (1, budget // 16, 5, 31),
                       (1, budget // 16 + 1, 5, 31), (2, budget // (16 * 7) + 1, 5, 200), (2, budget // (16 * 7), 5, 200),
                       (1, 4000, 300, hb.CTC_MAX_LABELS)):
        assert hb.ctc_align_ws_bytes(B, T, V, L) == formula(B, T, L), (B, T, V, L)
    assert hb.ctc_align_ws_bytes(32, 100, 34, 100) == 8 * 3200           # the workload's shapes backtrace out of LDS
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_align_ws_bytes(2, 10, 1, 3)
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_align_ws_bytes(2, 10, 5, hb.CTC_MAX_LABELS + 1)
    assert hb.CTC_MAX_LABELS + 1 == 1024
    with pytest.raises(RuntimeError):
        hb.ctc_align_ws_bytes(0, 10, 5, 3)
