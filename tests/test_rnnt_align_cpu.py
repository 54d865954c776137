"""Transducer forced alignment without a GPU: the float64 restatement tests/rnnt_align_ref.py against an
enumeration of every path and against the loss restatement, the tie rule, the structural identities the GPU test holds the
kernel to, the decisiveness of every case of the GPU grid, and the C ABI's two entries."""
import os
import re

import numpy as np
import pytest

import rnnt_align_ref as A
import rnnt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random(T, U, V, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-3, 3, (T, U + 1, V)), rs.randint(1, V, U)


def test_float64_viterbi_is_the_best_of_all_paths():
    """Every T <= 4, U <= 3, V <= 4: the score is the maximum over the enumeration, and the path is the enumeration's where
    only one path attains it."""
    unique = 0
    for T in range(1, 5):
        for U in range(0, 4):
            for V in range(2, 5):
                z, y = _random(T, U, V, 100 * T + 10 * U + V)
                r = A.viterbi(z, y)
                best, emit, n_best = A.brute_force(z, y)
                assert abs(float(r["score"]) - best) <= 1e-12, (T, U, V)
                if n_best == 1:
                    unique += 1
                    assert r["emit_frame"].tolist() == emit, (T, U, V)
    assert unique >= 40


@pytest.mark.parametrize("T,U", [(1, 0), (1, 4), (6, 0), (3, 2), (5, 5), (2, 7)])
def test_score_is_bounded_by_the_likelihood(T, U):
    """One path's probability is at most the sum over all: score <= -nll; with one path only (U = 0 or T = 1) they are equal."""
    z, y = _random(T, U, 6, 7 * T + U)
    score, nll = float(A.viterbi(z, y)["score"]), float(R.loss_and_grad(z, y)[0])
    assert score <= -nll + 1e-12
    if U == 0 or T == 1:
        assert abs(score + nll) <= 1e-12
    else:
        assert score < -nll - 1e-6


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("T,U", [(5, 3), (65, 64), (1, 2), (4, 0)])
def test_tie_rule_on_the_all_equal_lattice(T, U, dt):
    """Equal logits everywhere: every path ties exactly and the blank predecessor wins - every label is emitted at frame 0."""
    r = A.viterbi(np.zeros((T, U + 1, 5), np.float32), np.ones(U, np.int64), dt)
    assert r["emit_frame"].tolist() == [0] * U and r["frame_labels"].tolist() == [U] * T
    assert r["gap"] == (0.0 if T > 1 and U > 0 else np.inf)


def check_structure(emit_frame, frame_labels, T, U):
    """The identities of an alignment's integer outputs (the GPU test holds the kernel's outputs to the same function)."""
    emit_frame, frame_labels = np.asarray(emit_frame), np.asarray(frame_labels)
    assert emit_frame.shape == (U,) and frame_labels.shape == (T,)
    assert ((emit_frame >= 0) & (emit_frame < T)).all() and (np.diff(emit_frame) >= 0).all()
    assert (np.diff(frame_labels) >= 0).all() and frame_labels[-1] == U and frame_labels[0] >= 0
    steps = np.diff(np.concatenate([[0], frame_labels]))
    assert steps.tolist() == np.bincount(emit_frame, minlength=T).tolist()


@pytest.mark.parametrize("lattices,V", A.GRID, ids=lambda v: str(v).replace(" ", ""))
def test_grid_cases_are_decisive_and_well_formed(lattices, V):
    """Every case of the GPU grid: the structural identities on the float64 and the float32 restatement, the same path in
    both, score = the sum of its parts, and the case is DECISIVE - the GPU test leaves out no case as undecided."""
    c = A.case(lattices, V)
    assert A.decisive(c), [(x["T"], x["U"], x["ref"]["gap"]) for x in c["utts"]] + [c["allow"]["score"]]
    for x in c["utts"]:
        for r in (x["ref"], x["f32"]):
            check_structure(r["emit_frame"], r["frame_labels"], x["T"], x["U"])
        assert x["ref"]["emit_frame"].tolist() == x["f32"]["emit_frame"].tolist()
        parts = float(x["ref"]["token_logp"].sum() + x["ref"]["blank_logp"].sum())
        assert abs(parts - float(x["ref"]["score"])) <= 1e-9 * max(1.0, abs(parts))
        assert float(x["ref"]["score"]) <= -float(R.loss_and_grad(x["z"], x["y"])[0]) + 1e-9


NEW_EXPORTS = ("asr_transducer_align_ws_bytes", "asr_transducer_align_f32")


def test_exports_are_declared():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_transducer_align_\w+)\s*\(", header, flags=re.M))
    assert declared == set(NEW_EXPORTS) and declared <= set(hb.EXPORTS)
    assert "BLANK predecessor (t-1,u) wins" in header
    assert hb.ABI_VERSION == 8 and "#define ASR_ABI_VERSION 8" in header
    lib = hb.load()
    assert lib.asr_abi_version() == 8
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name


def test_workspace_bytes_and_refused_shapes():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    r64 = lambda n: (n + 63) // 64 * 64                                         # noqa: E731
    for B, T, U, V in ((1, 1, 0, 2), (5, 7, 6, 34), (32, 100, 100, 34), (2, 3, 257, 3), (1, 4, hb.RNNT_MAX_LABELS, 5)):
        want = 8 * r64(B * T * (U + 1)) + 8 * B * (T + U) * ((U + 1 + 63) // 64)
        assert hb.rnnt_align_ws_bytes(B, T, U, V) == want, (B, T, U, V)
    for B, T, U, V in ((2, 5, 3, 1),                                            # V < 2
                       (2, 5, hb.RNNT_MAX_LABELS + 1, 5),
                       (1 << 15, 1 << 15, 1000, 34),                            # 2^40 nodes: beyond the launch grids
                       (1 << 12, 1 << 12, 1000, 1 << 20)):                      # 2^24 nodes of 2^20 logits: beyond 2^40 elements
        with pytest.raises(hb.UnsupportedShape):
            hb.rnnt_align_ws_bytes(B, T, U, V)
        with pytest.raises(hb.UnsupportedShape):                                # ... where the loss refuses them too
            hb.rnnt_ws_bytes(B, T, U, 4, V)
    with pytest.raises(RuntimeError):
        hb.rnnt_align_ws_bytes(0, 5, 3, 5)
