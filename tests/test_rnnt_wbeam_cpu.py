"""The restatement of the transducer beam search with a word LM inside (tests/rnnt_wbeam_ref.py) against the plain search's
restatement, the word LM's float64 evaluator and the head's own loss, and the conditions the GPU tests lean on: no GPU needed."""
import os
import re

import numpy as np
import pytest

import rnnt_beam_ref as BR
import rnnt_wbeam_ref as WB
import word_lm_ref as WR
from test_rnnt_beam_cpu import seq_logp


def _key(f):
    return f["tokens"], float(f["tot"]), float(f["rank"])


@pytest.mark.parametrize("gi", (2, 9, 10))
def test_zero_weights_are_the_plain_search(gi):
    """alpha = beta = 0, no end term, lexicon_only off: the finals, their masses and their order are rnnt_beam_ref.search's."""
    g = WB.GRID[gi]
    p, utts, wlm = WB.grid_case(*g)
    for dt in (np.float64, np.float32):
        for u in utts:
            plain = BR.search(p, u, 1, g[1], g[4], dt)
            zero = WB.search(p, u, 1, g[1], g[4], wlm.compile(), dt, eos_term=False)
            assert [_key(f) for f in plain["finals"]] == [_key(f) for f in zero["finals"]]
            assert [s["kept"] for s in plain["steps"]] == [s["kept"] for s in zero["steps"]]


@pytest.mark.parametrize("g", WB.GRID, ids=[WB.grid_id(g) for g in WB.GRID])
def test_lm_is_the_row_score_and_the_lexicon_binds(g):
    """lm of every final is the word LM's float64 score of its tokens (the table's values are the float64 ones rounded to
    float32 once: 1e-5 relative), nw its number of words, the rank the fused form; with lexicon_only every final splits into
    lexicon words, and the lexicon is in reach (some final has a word)."""
    V, K, J, T, L, order, lexicon_only, eos_term, seed = g
    p, utts, wlm = WB.grid_case(*g)
    a, b = float(np.float32(WB.ALPHA)), float(np.float32(WB.BETA))
    words = 0
    for i in range(len(utts)):
        finals = WB.grid_judge(g, i)["ref"]["finals"]
        assert len(finals) >= 1 and (utts[i].shape[0] > 0 or [f["tokens"] for f in finals] == [()])
        for f in finals:
            want, n = WR.row_score(wlm, f["tokens"], eos_term)
            assert abs(float(f["lm"]) - want) <= 1e-5 * max(1.0, abs(want)) and f["nw"] == n, (i, f["tokens"])
            assert abs(float(f["rank"]) - ((float(f["tot"]) + a * float(f["lm"])) + b * n)) <= 1e-12
            assert float(f["lm"]) == float(WR.walk(wlm.compile(), f["tokens"], np.float64, eos_term)[0])
            if lexicon_only:
                assert all(w in wlm.lexicon.index for w in WR.split(f["tokens"], wlm.space)), (i, f["tokens"])
            words += n
    assert words > 0


def test_the_weights_change_the_search():
    g = WB.GRID[10]
    p, utts, wlm = WB.grid_case(*g)
    plain = [f["tokens"] for f in BR.search(p, utts[0], 1, g[1], g[4])["finals"][:g[1]]]
    assert plain != [f["tokens"] for f in WB.grid_judge(g, 0)["ref"]["finals"][:g[1]]]


@pytest.mark.parametrize("T", (1, 2, 4))
@pytest.mark.parametrize("lexicon_only", (False, True))
def test_exhaustive_finals_are_below_the_sequence_probability(T, lexicon_only):
    """V = 3 (blank, one letter, <space>), L = 3, K = 16: every sequence the lexicon admits stays in the beam; every final's
    tot is the beam's share of log P(y | x) - without lexicon_only all of it."""
    p, enc_h = BR.grid_case(3, 8, T, 31)
    wlm = WR.random_word_lm(3, 2, 7)
    out = WB.search(p, enc_h, 1, 16, 3, wlm.compile(), alpha=0.7, beta=0.3, lexicon_only=lexicon_only)
    assert len(set(f["tokens"] for f in out["finals"])) == len(out["finals"]) and (lexicon_only or len(out["finals"]) == 15)
    for f in out["finals"]:
        lp = seq_logp(p, enc_h, 1, f["tokens"])
        assert float(f["tot"]) <= lp + 1e-12 and abs(float(f["tot"]) - lp) <= 1e-12, f["tokens"]
    case = dict(p=p, enc_h=enc_h, bos=1, K=16, L=3, table=wlm.compile(), alpha=0.7, beta=0.3, lexicon_only=lexicon_only)
    assert WB.judge(case)["decisive"]


def test_the_grid_is_decisive():
    """Every utterance of the GPU grid is decided between the float64 and the float32 restatement (the cap on undecided
    ones is 10 %; the seeds are chosen so that none is), and the grid covers what it says it covers."""
    total = undecided = 0
    for g in WB.GRID:
        for b in range(5):
            total += 1
            undecided += not WB.grid_judge(g, b)["decisive"]
    print("rnnt-wbeam grid: %d of %d utterances undecided" % (undecided, total))
    assert undecided <= WB.UNDECIDED_CAP * total
    assert undecided == 0
    cols = list(zip(*WB.GRID))
    assert [set(c) for c in cols[:8]] == [{5, 34}, {1, 4, 16}, {4, 32}, {1, 7, 12}, {1, 6, 12}, {1, 2, 3}, {False, True}, {False, True}]
    for i, j in ((1, 3), (1, 4), (3, 4)):
        assert len(set(zip(cols[i], cols[j]))) == 9
    assert all(0 in [u.shape[0] for u in WB.grid_case(*g)[1]] and len(WB.grid_case(*g)[1]) == 5 for g in WB.GRID)


def test_workspace_size_refusals_and_names_need_no_gpu():
    """asr_transducer_wbeam_ws_bytes runs on plain integers: its documented formula, the K range of the plain search; the four
    entries are declared in the header and exported, and belong to neither older group."""
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    r64 = lambda n: (n + 63) // 64 * 64                                  # noqa: E731
    for B, K in ((1, 1), (3, 16), (5, 4), (32, 8), (700, 16)):
        assert hb.rnnt_wbeam_ws_bytes(B, K) == 4 * 7 * r64(B * K)
    for K in (0, 17, -1):
        with pytest.raises(hb.UnsupportedShape):
            hb.rnnt_wbeam_ws_bytes(3, K)
    with pytest.raises(RuntimeError):
        hb.rnnt_wbeam_ws_bytes(0, 4)                                     # (an argument error, not a shape)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_transducer_wbeam_\w+)\s*\(", header, flags=re.M))
    assert declared == {"asr_transducer_wbeam_ws_bytes", "asr_transducer_wbeam_init_f32", "asr_transducer_wbeam_step_f32",
                        "asr_transducer_wbeam_backtrace_f32"}
    assert declared <= set(hb.EXPORTS) and all(hasattr(hb.load(), n) for n in declared)
    assert not any(n.startswith(("asr_transducer_beam_", "asr_rnnt_")) for n in declared)
    assert len(set(re.findall(r"^int\s+(asr_transducer_beam_\w+)\s*\(", header, flags=re.M))) == 5
    assert "#define ASR_ABI_VERSION 8" in header


def test_solver_keys():
    """rnnt_word_lm goes with rnnt_beam_decode alone and not beside ngram_lm; word_lm beside rnnt_beam_decode is still
    refused in the old words."""
    import __graft_entry__ as entry
    entry._ensure_paths()
    from solver import Solver
    assert Solver.rnnt_beam_config(dict(rnnt_beam_decode=True, rnnt_word_lm=dict(arpa="w.arpa", weight=0.5, bonus=0.1,
                                                                                 lexicon="l.txt", lexicon_only=True)), True)
    assert Solver.rnnt_beam_config(dict(), True) is False
    with pytest.raises(ValueError, match="set rnnt_beam_decode"):
        Solver.rnnt_beam_config(dict(rnnt_word_lm=dict(arpa="w.arpa")), True)
    with pytest.raises(ValueError, match="two LMs for one search"):
        Solver.rnnt_beam_config(dict(rnnt_beam_decode=True, rnnt_word_lm=dict(arpa="w.arpa"), ngram_lm="c.arpa"), True)
    with pytest.raises(ValueError, match="does not combine with word_lm"):
        Solver.rnnt_beam_config(dict(rnnt_beam_decode=True, word_lm="w.arpa"), True)
    for bad in (dict(weight=0.5), dict(arpa="w.arpa", alpha=1.0), "w.arpa"):
        with pytest.raises(ValueError, match="rnnt_word_lm is a dictionary"):
            Solver.rnnt_beam_config(dict(rnnt_beam_decode=True, rnnt_word_lm=bad), True)
    with pytest.raises(ValueError, match="needs the transducer head"):
        Solver.rnnt_beam_config(dict(rnnt_beam_decode=True, rnnt_word_lm=dict(arpa="w.arpa")), False)
