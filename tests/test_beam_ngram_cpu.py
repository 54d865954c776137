"""The attention beam search with an n-gram or word-level LM inside, without a GPU: the restatement
(tests/beam_ngram_ref.py) against the searches it builds on and against the scorers' restatements, the configuration keys of
Solver.test, the declared entries, and the seeds of the GPU grid held to their cap on left-out cases."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import beam_ctc_ref
import beam_lm_ref
import beam_ngram_ref as R
import beam_ref
import ngram_ref as NR
import word_lm_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, V, L, EOS = 3, R.V, 9, R.EOS


def _steps(seed, judge=False, eos_bias=1.0):
    """A step function over fixed random logits that depend on the step and the beams' last tokens."""
    def step(t, parents, toks):
        last = np.zeros(K, dtype=np.int64) if toks is None else np.asarray(toks)
        out = []
        for which in range(2 if judge else 1):
            rows = [np.random.RandomState(seed + 1000 * which + 37 * t + int(c)).randn(V) * 2.0 for c in last]
            a = np.stack(rows)
            a[:, EOS] += eos_bias
            out.append(a)
        return tuple(out) if judge else out[0]
    return step


def _lms():
    return [R.tlm(R.NGRAM, R.grid_lm(R.NGRAM, 3).compile()), R.tlm(R.WORD, R.grid_lm(R.WORD, 3).compile())]


@pytest.mark.parametrize("lp", [0.0, 0.7])
def test_zero_weights_are_the_searches_without_the_lm(lp):
    x = beam_ctc_ref.log_probs(np.random.RandomState(5).randn(11, V))
    for lm in _lms():
        got = R.search(_steps(1), K, V, L, EOS, lm, length_penalty=lp)
        want = beam_ref.search(_steps(1), K, V, L, EOS, lp)
        assert got["hyps"] == want["hyps"] and got["margins"] == want["margins"] and got["steps"] == want["steps"]
        got = R.search(_steps(2, True), K, V, L, EOS, lm, lm_weight=0.4, length_penalty=lp)
        want = beam_lm_ref.search(_steps(2, True), K, V, L, EOS, 0.4, lp)
        assert got["hyps"] == want["hyps"] and got["margins"] == want["margins"]
        got = R.search(_steps(3), K, V, L, EOS, lm, x=x, ctc_weight=0.3, length_penalty=lp)
        want = beam_ctc_ref.search(_steps(3), K, V, L, EOS, x, 0.3, None, lp)
        assert got["hyps"] == want["hyps"] and got["margins"] == want["margins"]
        assert all(p[0] == h[1] * (float(h[2]) ** lp if lp else 1.0) or abs(p[0] - h[1] * float(h[2]) ** lp) < 1e-12
                   for p, h in zip(got["parts"], got["hyps"]))


@pytest.mark.parametrize("eos_bias", [8.0, -30.0])      # searches that <EOS> ends, and searches that run into L
def test_parts_are_the_scorers(eos_bias):
    for lm, (w, beta) in zip(_lms(), ((0.5, 0.3), (0.7, 0.6))):
        lm = dict(lm, weight=w, bonus=beta)
        res = R.search(_steps(7, eos_bias=eos_bias), K, V, L, EOS, lm)
        assert res["hyps"] and any(h[0][-1] == EOS for h in res["hyps"]) == (eos_bias > 0)
        for (toks, key, n), (base, s, cnt) in zip(res["hyps"], res["parts"]):
            ids = toks[:-1] if toks[-1] == EOS else toks
            assert n == len(toks)
            if lm["kind"] == R.NGRAM:
                want, _ = NR.walk(lm["table"], ids, np.float32, eos_term=True)
                assert cnt == len(ids)
            else:
                want, _, nw = WR.walk(lm["table"], ids, np.float32, eos_term=True)
                assert cnt == nw == len(WR.split(ids, lm["table"].space))
            assert np.float32(s).tobytes() == np.float32(want).tobytes()
            assert abs(key - (base + w * float(s) + beta * cnt)) <= 1e-9 * max(1.0, abs(key))


def test_the_lm_steers_the_search():
    lm = _lms()[0]
    plain = beam_ref.search(_steps(7), K, V, L, EOS)
    fused = R.search(_steps(7), K, V, L, EOS, dict(lm, weight=1.5))
    assert [h[0] for h in fused["hyps"]] != [h[0] for h in plain["hyps"]]


def test_lexicon_only_keeps_lexicon_words():
    wlm = R.grid_lm(R.WORD, 3)
    table = wlm.compile()
    kept = 0
    for seed in range(6):
        res = R.search(_steps(20 + seed, eos_bias=0.0), K, V, 6, EOS, R.tlm(R.WORD, table, 0.5, 0.5, lexicon_only=True))
        for toks, _, _ in res["hyps"]:
            ids = toks[:-1] if toks and toks[-1] == EOS else toks
            assert R.words_in_lexicon(table, ids), ids
            kept += 1
        free = R.search(_steps(20 + seed, eos_bias=0.0), K, V, 6, EOS, R.tlm(R.WORD, table, 0.5, 0.5))
        assert any(not R.words_in_lexicon(table, [c for c in h[0] if c != EOS]) for h in free["hyps"])
    assert kept > 0
    # a lexicon no sequence can satisfy: letters that start no word, nothing else possible
    only = np.full((K, V), -np.inf)
    starts = {int(c) for c in np.nonzero(table.trie_next[0] >= 0)[0]}
    bad = [c for c in range(3, R.SPACE) if c not in starts]
    assert bad
    only[:, bad[0]] = 0.0
    res = R.search(lambda t, p, k: only, K, V, 4, EOS, R.tlm(R.WORD, table, 0.5, 0.5, lexicon_only=True))
    assert res["hyps"] == []


def test_grid_stays_within_the_cap_on_left_out_cases():
    """The GPU grid's seeds judged by the restatement alone: at most LEFT_OUT_CAP of the grid's utterances have a decision
    margin at or below MARGIN (tests/test_beam_ngram_gpu.py leaves those out of the token comparison only), and no variant is
    left out as a whole."""
    grid = R.grid()
    assert len(grid) == 12 and set(R.SEEDS) == set(grid)
    assert {g[0] for g in grid} == set(R.KINDS) and {g[1] for g in grid} == set(R.VARIANTS) and {g[2] for g in grid} == {1, 4}
    verdicts = {g: [R.decided(r) for r in R.judge(g)] for g in grid}
    flat = [v for g in grid for v in verdicts[g]]
    print("left out: %d of %d utterances" % (flat.count(False), len(flat)))
    assert flat.count(False) <= R.LEFT_OUT_CAP * len(flat)
    for kind in R.KINDS:
        for variant in R.VARIANTS:
            assert any(v for g in grid if g[:2] == (kind, variant) for v in verdicts[g]), (kind, variant)
    steps = [r["steps"] for g in grid for r in R.judge(g)]
    assert min(steps) < R.L and max(steps) == R.L            # searches that <EOS> ends and searches that finish as they stand


def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_beam_tlm_ws_bytes", "asr_beam_tlm_init_f32", "asr_beam_select_tlm_f32", "asr_beam_backtrack_tlm"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert re.search(r"^#define ASR_ABI_VERSION 8$", header, flags=re.M)
    entry.build()
    import hip_backend as hb
    for name in ("asr_beam_tlm_ws_bytes", "asr_beam_tlm_init_f32", "asr_beam_select_tlm_f32", "asr_beam_backtrack_tlm"):
        assert name in hb.EXPORTS and hasattr(hb.load(), name)
    assert hb.beam_tlm_ws_bytes(2, 4) == 4 * (4 * 64 + 3 * 128)          # plain integers: no GPU
    assert hb.beam_tlm_ws_bytes(32, 8) == 4 * (4 * 256 + 3 * 1536)
    with pytest.raises(hb.UnsupportedShape):
        hb.beam_tlm_ws_bytes(2, 17)


def test_config_keys():
    entry.build()
    from solver import Solver
    cfg = Solver.att_lm_config
    assert cfg({}) == (None, None) and cfg(dict(beam_size=4, lm_weight=0.3)) == (None, None)
    ng = dict(arpa="lm.arpa", weight=0.5, bonus=0.2)
    wd = dict(arpa="w.arpa", lexicon="l.txt", weight=0.5, bonus=1, lexicon_only=True)
    assert cfg(dict(beam_size=4, att_ngram_lm=ng)) == ("ngram", ng)
    assert cfg(dict(beam_size=2, att_word_lm=wd, lm_weight=0.3, ctc_decode_weight=0.3)) == ("word", wd)
    assert cfg(dict(beam_size=2, att_word_lm=dict(arpa="w.arpa"))) == ("word", dict(arpa="w.arpa"))
    with pytest.raises(ValueError, match="two LMs for one search"):
        cfg(dict(beam_size=4, att_ngram_lm=ng, att_word_lm=wd))
    for name, sub in (("att_ngram_lm", ng), ("att_word_lm", wd)):
        with pytest.raises(ValueError, match="beam_size > 1"):
            cfg({name: sub})
        with pytest.raises(ValueError, match="beam_size > 1"):
            cfg({name: sub, "beam_size": 1})
        for other in ("rnnt_beam_decode", "rnnt_greedy_decode", "two_pass_decode", "ctc_beam_decode", "ctc_greedy_decode"):
            with pytest.raises(ValueError, match="does not combine with %s" % other):
                cfg({name: sub, "beam_size": 4, other: True})
        with pytest.raises(ValueError, match="a dictionary with `arpa`"):
            cfg({name: "lm.arpa", "beam_size": 4})
        with pytest.raises(ValueError, match="a dictionary with `arpa`"):
            cfg({name: {k: v for k, v in sub.items() if k != "arpa"}, "beam_size": 4})
        with pytest.raises(ValueError, match="got alpha"):
            cfg({name: dict(sub, alpha=1.0), "beam_size": 4})
    with pytest.raises(ValueError, match="got lexicon"):
        cfg(dict(beam_size=4, att_ngram_lm=dict(ng, lexicon="l.txt")))
    # the top-level keys keep their meaning: an ngram_lm beside the attention beam search is still refused
    with pytest.raises(ValueError):
        Solver.ngram_config(dict(ngram_lm="x.arpa", beam_size=4), False, False)
    config = open(os.path.join(ROOT, "semi-supervised-asr_amd", "config.yaml")).read()
    for key in ("att_ngram_lm", "att_word_lm"):
        assert re.search(r"^# %s: \{arpa: " % key, config, flags=re.M) and not re.search(r"^%s:" % key, config, flags=re.M)
