"""CTC prefix beam search and two-pass decoding without a GPU: the dictionary-based restatement (tests/ctc_beam_ref.py)
against the enumeration of every frame path where the beam cannot prune, the tie rule, the merge case, the share of the GPU
grid the restatement leaves undecided, the header's declarations, hb.ctc_beam_ws_bytes on plain integers and the
`two_pass_decode` config key."""
import os
import re

import numpy as np
import pytest

import ctc_beam_ref as R

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("V,T", [(3, 1), (3, 2), (3, 3), (2, 1), (2, 2), (2, 3), (2, 4)])
def test_restatement_against_enumeration(V, T):
    """At K = 16 no labelling of these shapes is ever pruned (at most 15 of them exist), so the search IS the CTC forward
    of every labelling at once: each reported score is the labelling's exact log-likelihood, every labelling is reported,
    and the order is descending."""
    rs = np.random.RandomState(100 * V + T)
    z = rs.normal(0, 2, size=(T, V))
    mass = R.enumerate_paths(z)
    assert len(mass) <= 16
    res = R.search(z, 16)
    assert sorted(res["hyps"]) == sorted(mass) and len(set(res["hyps"])) == len(res["hyps"])
    eps = 64 * np.finfo(np.float64).eps
    for h, s in zip(res["hyps"], res["scores"]):
        assert abs(s - mass[h]) <= eps * max(1.0, abs(mass[h])), (h, s, mass[h])
    assert all(a >= b for a, b in zip(res["scores"], res["scores"][1:]))
    assert abs(np.logaddexp.reduce(res["scores"])) <= eps * len(mass)             # the masses of all labellings sum to 1
    # float32: the yardstick follows within its own rounding
    r32 = R.search(z.astype(np.float32), 16)
    for h, s in zip(r32["hyps"], r32["scores"]):
        assert abs(float(s) - mass[h]) <= 64 * np.finfo(np.float32).eps * max(1.0, abs(mass[h]))


@pytest.mark.parametrize("K", [1, 2, 4, 16])
def test_tie_rule_on_all_equal_logits(K):
    """T' = 1, all logits equal: the stay of the empty prefix and every extension score -log V exactly, so the lower flat
    index decides: the empty prefix (index 0), then the tokens 1 .. K - 1."""
    for dt in (np.float64, np.float32):
        res = R.search(np.zeros((1, 20), dtype=dt), K)
        assert res["hyps"] == [()] + [(c,) for c in range(1, K)]
        assert all(s == res["scores"][0] for s in res["scores"]) and res["gap"] == 0.0
        assert abs(float(res["scores"][0]) + np.log(20)) <= 4 * np.finfo(dt).eps * np.log(20)


def test_merge_case():
    """Frame 0 leaves the beam {(), (1)}.  In frame 1 the extension () . 1 IS the entry (1): its mass joins the stay of (1)
    and is no candidate of its own - p(1) = 0.4 * 0.3 + 0.4 * 0.7 + 0.6 * 0.7, p() = 0.6 * 0.3; (1) . 1 has no path in two
    frames, so two entries are live at K = 4."""
    z = np.log(np.array([[0.6, 0.4], [0.3, 0.7]]))
    res = R.search(z, 4)
    assert res["hyps"] == [(1,), ()]
    assert np.allclose(np.exp(res["scores"]), [0.82, 0.18], rtol=1e-14, atol=0)
    # a longer one: (1 2) is reached from (1) . 2 in frame 2 while (1 2) is in the beam since frame 1
    z = np.log(np.array([[0.5, 0.4, 0.1], [0.2, 0.1, 0.7], [0.3, 0.1, 0.6]]))
    res = R.search(z, 16)
    mass = R.enumerate_paths(z)
    assert np.isclose(res["scores"][res["hyps"].index((1, 2))], mass[(1, 2)], rtol=1e-14)
    assert len(res["hyps"]) == len(set(res["hyps"])) == len(mass)


def test_empty_utterance_and_width_one():
    res = R.search(np.zeros((0, 5)), 4)
    assert res["hyps"] == [()] and res["scores"].tolist() == [0.0]
    z = np.random.RandomState(3).normal(0, 3, size=(12, 6))
    assert len(R.search(z, 1)["hyps"]) == 1


def test_grid_stays_within_the_cap_on_undecided_cases():
    """The GPU grid's seeds, judged by the restatements alone: the utterances where float64 cannot tell the device's choice
    (a select separated by no more than 2 x the allowance, or a float32 restatement that already chooses otherwise) are at
    most 10 % of the grid; the GPU test skips check 3 for exactly these."""
    cases, extra = R.grid()
    assert len(cases) == 128
    verdicts = [u["decisive"] for c in cases + extra for u in R.judge(*c)]
    undecided = verdicts.count(False)
    print("undecided: %d of %d utterances" % (undecided, len(verdicts)))
    assert undecided <= R.UNDECIDED_CAP * len(verdicts), (undecided, len(verdicts))
    # the cap is not met by the empty utterances alone: most utterances with frames are decided too
    with_frames = [u["decisive"] for c in cases + extra for u in R.judge(*c)[:2]]
    assert with_frames.count(False) <= 0.15 * len(with_frames)


def test_new_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert re.search(r"^int asr_ctc_beam_ws_bytes\(int B, int T, int V, int K, int64_t\* ws_bytes\);", header, flags=re.M)
    assert re.search(r"^int asr_ctc_beam_f32\(int B, int T, int V, int K, const float\* logits, int64_t ld, "
                     r"const int32_t\* frame_lens, int32_t\* hyp,\s+int32_t\* hyp_len, float\* score, void\* ws, "
                     r"asr_stream_t stream\);", header, flags=re.M)
    assert re.search(r"#define ASR_ABI_VERSION 8\b", header)
    entry.build()
    import hip_backend as hb
    assert "asr_ctc_beam_f32" in hb.EXPORTS and "asr_ctc_beam_ws_bytes" in hb.EXPORTS and hb.ABI_VERSION == 8
    assert int(re.search(r"#define ASR_CTC_BEAM_ONE_WAVE_KV (\d+)", header).group(1)) == hb.CTC_BEAM_ONE_WAVE_KV
    assert int(re.search(r"#define ASR_CTC_BEAM_LDS_ENTRIES (\d+)", header).group(1)) == hb.CTC_BEAM_LDS_ENTRIES
    # the grid's extra shapes sit on either side of these switches
    _, extra = R.grid()
    kv = {V * K for V, K, _, _ in extra}
    assert hb.CTC_BEAM_ONE_WAVE_KV in kv and any(hb.CTC_BEAM_ONE_WAVE_KV < n <= hb.CTC_BEAM_ONE_WAVE_KV + 64 for n in kv)
    tk = {T * K for _, K, T, _ in extra}
    assert hb.CTC_BEAM_LDS_ENTRIES in tk and hb.CTC_BEAM_LDS_ENTRIES + 16 in tk


def test_ws_bytes_on_plain_integers():
    """hb.ctc_beam_ws_bytes needs no GPU; it is the header's formula; V < 2 and a width outside 1 .. 16 are refused."""
    entry.build()
    import hip_backend as hb

    def formula(B, T, K):
        return 4 * ((B * T + 63) // 64 * 64) + (8 * B * T * K if T * K > hb.CTC_BEAM_LDS_ENTRIES else 0)
    for B, T, V, K in ((32, 100, 50, 4), (32, 100, 50, 8), (1, 1, 2, 1), (3, 7, 5, 2), (2, 256, 5, 16), (2, 257, 5, 16),
                       (1, 4097, 34, 1), (1, 4096, 34, 1)):
        assert hb.ctc_beam_ws_bytes(B, T, V, K) == formula(B, T, K), (B, T, V, K)
    for bad in ((2, 10, 1, 3), (2, 10, 5, 0), (2, 10, 5, hb.BEAM_KMAX + 1)):
        with pytest.raises(hb.UnsupportedShape):
            hb.ctc_beam_ws_bytes(*bad)
    with pytest.raises(RuntimeError):
        hb.ctc_beam_ws_bytes(0, 10, 5, 3)


def test_two_pass_decode_config_validation():
    entry.build()
    from solver import Solver
    assert Solver.two_pass_config({}, False) is False and Solver.two_pass_config({}, True) is False
    assert Solver.two_pass_config(dict(two_pass_decode=False, ctc_greedy_decode=True), False) is False
    assert Solver.two_pass_config(dict(two_pass_decode=True, beam_size=4, lm_weight=0.3, ctc_decode_weight=0.5), True) is True
    with pytest.raises(ValueError, match="ctc_greedy_decode"):
        Solver.two_pass_config(dict(two_pass_decode=True, ctc_greedy_decode=True), True)
    with pytest.raises(ValueError, match="CTC head"):
        Solver.two_pass_config(dict(two_pass_decode=True), False)
