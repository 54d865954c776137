"""The case table of tests/test_lstm_shapes_gpu.py without a GPU: the fp32 restatement of every case meets the case's own
limits against the float64 one (so the reference, the seeds and the limits are consistent with each other before any
kernel is judged by them), the exemption cap holds on the reference alone, the saturated cases saturate, and the backward
path every case names is the one libasr_hip.so's own dispatch (asr_lstm_bwd_persist_fuses_dw, which needs no device)
gives for its width and arithmetic.  No case is skipped: the longest float64 recurrence (T = 300) takes about a second."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import test_lstm_shapes_gpu as G  # noqa: E402


@pytest.mark.parametrize("case", G.CASES)
def test_fp32_restatement_meets_the_limits_of_the_case(case):
    inp = G._inputs_of(case["name"])
    ref, ref32 = G._references_of(case["name"])
    lens = inp["lens"]
    assert (lens[0] == case["T"] or case["lens"] is not None) and all(1 <= n <= case["T"] for n in lens)
    assert case["B"] < 3 or min(lens) == 1, "a case of three or more utterances has one of length 1"
    for b, n in enumerate(lens):
        assert float(inp["x"][b, n:].abs().sum()) == 0.0
        assert n == case["T"] or float(inp["dy"][b, n:].abs().max()) > 0.0, "the upstream gradient has noise on padding frames"
    if case["sat"]:
        ok, seen = G._saturation_ok(case, inp, ref)
        assert ok, "%s: share beyond +-30, count beyond +-90, of: %s" % (case["name"], seen)
    G._check(case, inp, ref32, ref, "fp32 on the CPU")


def test_backward_paths_of_the_table_are_the_library_s():
    entry.build()
    import hip_backend as hb
    lib = hb.load()
    bad = []
    for prm in G.CASES:
        case = prm.values[0]
        got = lib.asr_lstm_bwd_persist_fuses_dw(case["H"], hb._arith_code(case["arith"]))
        want = G.BWD_KINDS[case["kind"]]
        if got != want or (case["bwd"] == "persist") != (got >= 0):
            bad.append((case["name"], case["kind"], case["bwd"], got))
        # a width without an instantiation runs per step both ways; a persistent backward is never behind a per-step forward
        if case["H"] not in G.PERSIST_WIDTHS and (case["fwd"], case["bwd"]) != ("step", "step"):
            bad.append((case["name"], "no instantiation at this width", case["fwd"], case["bwd"]))
        if case["fwd"] == "step" and case["bwd"] == "persist":
            bad.append((case["name"], "persistent backward behind a per-step forward"))
    assert not bad, bad


def test_the_table_holds_every_case_the_dispatch_has():
    """The boundaries of rows_per_group / fwd_rows16 (csrc/lstm_persist.hip) on both sides, in numbers: 4-row groups hold
    4 * 8 / ndir utterances, a launch of 8-row groups 8 * 8 / ndir, a 16-row forward block 16 * 8 / ndir."""
    seen = {(c["H"], c["ndir"], c["B"], c["layout"]) for c in (p.values[0] for p in G.CASES) if c["arith"] == "bf16x6"}
    for ndir in (1, 2):
        g = 8 // ndir
        sizes = {4 * g, 4 * g + 1, 8 * g, 8 * g + 1, 16 * g - 1, 16 * g} | ({16 * g + 1} if ndir == 2 else set())
        for B in sizes:
            for layout in (("tm", "packed") if ndir == 2 else ("tm",)):
                assert (512, ndir, B, layout) in seen, (ndir, B, layout)
    names = [p.values[0]["name"] for p in G.CASES]
    assert len(set(names)) == len(names)
