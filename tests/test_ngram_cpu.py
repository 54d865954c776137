"""The n-gram LM without a GPU (ngram.py, tests/ngram_ref.py): ARPA in and out, the automaton against explicit
backoff, the Witten-Bell estimate's rows, the fused search's restatement against the plain one and against the enumeration
of every labelling, the share of the GPU grid the restatements leave undecided, and the config keys."""
import os
import re

import numpy as np
import pytest

import ctc_beam_ref as R
import ngram_ref as N
from ngram import NgramLM

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN10 = np.log(10.0)

THREE_GRAM = """
\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.7\ta\t-0.3
-0.9\tb\t-0.2
-1.2\tc

\\2-grams:
-0.4\t<s> a\t-0.1
-0.6\ta b\t-0.25
-0.8\tb </s>
-0.5\tb a

\\3-grams:
-0.2\t<s> a b
-0.3\ta b </s>

\\end\\
"""
WORDS = {"a": 3, "b": 4, "c": 5}


def _text(V, seed, n=20, longest=8):
    rs = np.random.RandomState(seed)
    labels = list(range(3, V))
    return [[int(rs.choice(labels)) for _ in range(rs.randint(0, longest))] if labels else [] for _ in range(n)]


def test_hand_written_three_gram_parses_to_known_values():
    lm = NgramLM.from_arpa(THREE_GRAM, WORDS, 1, 2)
    assert lm.order == 3 and lm.V == 6 and (1,) not in lm.prob
    # <s> a b </s>: the trigrams are listed
    assert np.isclose(lm.score([3, 4]), (-0.4 - 0.2 - 0.3) * LN10, rtol=1e-15)
    # <s> b: no bigram -> backoff(<s>) + p(b);  then b a listed;  then (b a) </s>: no trigram, (b a) carries no backoff,
    # (a </s>) is no bigram: backoff(a) + p(</s>)
    assert np.isclose(lm.score([4, 3]), (-0.5 - 0.9 - 0.5 - 0.3 - 1.0) * LN10, rtol=1e-15)
    # c after (a b): backoff(a b) + backoff(b) + p(c);  a token without a unigram scores oov_logp
    assert np.isclose(lm.token_logp((1, 3, 4), 5), (-0.25 - 0.2 - 1.2) * LN10, rtol=1e-15)
    assert lm.token_logp((3,), 1) == -30.0 == lm.oov_logp
    table = lm.compile()
    assert table.logp.dtype == np.float32 and table.nxt.dtype == np.int32 and table.logp.shape == table.nxt.shape == (table.S, 6)
    assert lm.states()[:2] == [(1,), ()] and table.start == 0 and (table.logp[:, 0] == 0).all()
    assert set(lm.states()) == {(1,), (), (3,), (4,), (5,), (2,), (1, 3), (3, 4), (4, 2), (4, 3)}


def test_unknown_word_is_refused_by_name():
    with pytest.raises(ValueError, match="'c'"):
        NgramLM.from_arpa(THREE_GRAM, {"a": 3, "b": 4}, 1, 2)
    with pytest.raises(ValueError):
        NgramLM(2, 5, 1, 2, {(3,): -1.0}, {}, oov_logp=-np.inf)
    with pytest.raises(ValueError):
        NgramLM(2, 5, 1, 1, {(3,): -1.0}, {})


@pytest.mark.parametrize("V,order", [(3, 2), (5, 3), (34, 4)])
def test_arpa_round_trip(V, order, tmp_path):
    lm = NgramLM.estimate(_text(V, 7 * V + order), order, V, N.BOS, N.EOS)
    words = {"w%d" % i: i for i in range(3, V)}
    text = lm.to_arpa({i: w for w, i in words.items()})
    back = NgramLM.from_arpa(text, words, N.BOS, N.EOS, V=V)
    a, b = lm.compile(), back.compile()
    assert lm.states() == back.states() and np.array_equal(a.nxt, b.nxt) and a.start == b.start
    assert np.abs(a.logp64 - b.logp64).max() <= 1e-13 * max(1.0, np.abs(a.logp64).max())
    path = tmp_path / "lm.arpa"
    path.write_text(text)
    assert np.array_equal(NgramLM.from_arpa(str(path), words, N.BOS, N.EOS, V=V).compile().logp, b.logp)


@pytest.mark.parametrize("V", [3, 5, 34])
@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_automaton_against_explicit_backoff(V, order):
    """Every (state, token): the table's float64 value is the explicit evaluator's to float64 rounding (NgramLM.token_logp
    and the independent tests/ngram_ref.backoff_logp), the float32 table is that value rounded once, every successor is a
    state - and it is the longest suffix of state . c that is one; random sequences walk to the same sums."""
    for lm in (N.random_lm(V, order, 1000 * V + order), NgramLM.estimate(_text(V, V + order), order, V, N.BOS, N.EOS)):
        table, states = lm.compile(), lm.states()
        index = {s: i for i, s in enumerate(states)}
        assert len(index) == len(states) == table.S
        assert table.nxt.min() >= 0 and table.nxt.max() < table.S
        for i, s in enumerate(states):
            for c in range(1, V):
                want = N.backoff_logp(lm, s, c)
                assert abs(table.logp64[i, c] - want) <= 1e-13 * max(1.0, abs(want)), (s, c)
                assert abs(lm.token_logp(s, c) - want) <= 1e-13 * max(1.0, abs(want)), (s, c)
                full = (s + (c,))[max(0, len(s) + 1 - (order - 1)):] if order > 1 else ()
                while full not in index:
                    full = full[1:]
                assert table.nxt[i, c] == index[full], (s, c)
        assert np.array_equal(table.logp, table.logp64.astype(np.float32))
        rs = np.random.RandomState(V * order)
        for _ in range(30):
            ids = [int(rs.randint(1, V)) for _ in range(rs.randint(0, 12))]
            total, _ = N.walk(table, ids, np.float64)
            exact = sum(N.backoff_logp(lm, (N.BOS,) + tuple(ids[:i]), c) for i, c in enumerate(ids + [N.EOS]))
            assert abs(float(total) - exact) <= 1e-5 * max(1.0, abs(exact))             # (the table is float32)
            assert abs(lm.score(ids) - exact) <= 1e-12 * max(1.0, abs(exact))


@pytest.mark.parametrize("V,order", [(3, 1), (5, 2), (5, 5), (34, 3), (34, 5)])
def test_estimate_is_proper(V, order):
    """Every context's distribution over {labels with a unigram} + {</s>} sums to 1 within 1e-12 - at every state of the
    automaton, and after histories the text never held."""
    lm = NgramLM.estimate(_text(V, 31 * V + order, n=40), order, V, N.BOS, N.EOS)
    events = [c for c in range(1, V) if (c,) in lm.prob]
    assert N.EOS in events and N.BOS not in events and events == [c for c in range(2, V)]
    rs = np.random.RandomState(order)
    contexts = lm.states() + [tuple(int(c) for c in rs.randint(2, V, size=rs.randint(0, 6))) for _ in range(20)]
    for h in contexts:
        total = sum(np.exp(N.backoff_logp(lm, h, c)) for c in events)
        assert abs(total - 1.0) <= 1e-12, (h, total)


def test_compile_refuses_a_table_beyond_int32():
    lm = N.random_lm(5, 2, 1)
    lm.V = 2 ** 30
    with pytest.raises(ValueError, match="2\\*\\*31"):
        lm.compile()


@pytest.mark.parametrize("V,K,T,scale", [(3, 16, 3, 1.0), (5, 4, 7, 1.0), (34, 2, 20, 50.0), (34, 16, 12, 1.0)])
def test_without_weights_the_search_is_the_plain_one(V, K, T, scale):
    z = np.random.RandomState(V * K + T).normal(0, scale, size=(T, V))
    lm = N.random_lm(V, 3, 5)
    for dt in (np.float64, np.float32):
        plain, fused = R.search(z.astype(dt), K), N.search_lm(z.astype(dt), K, lm, 0.0, 0.0, False)
        assert fused["hyps"] == plain["hyps"]
        assert np.array_equal(fused["score"], plain["scores"]) and np.array_equal(fused["ctc"], plain["scores"])
        for h, v in zip(fused["hyps"], fused["lm"]):
            assert v == N.walk(lm.compile(), h, dt, eos_term=False)[0]


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("alpha,beta,eos_term", [(0.5, 0.0, True), (2.0, 1.5, False), (1.0, -1.0, True)])
def test_exhaustive_definition(T, order, alpha, beta, eos_term):
    """V = 3, K = 16: at most 15 labellings exist, the beam holds them all, so the ranked list IS every labelling of
    ctc_beam_ref.enumerate_paths ranked by mass + alpha lm + beta len (+ alpha x the end term), scores to 1e-12.  This is
    the definition the kernel is held to."""
    z = np.random.RandomState(10 * T + order).normal(0, 2, size=(T, 3))
    lm = N.random_lm(3, order, 77 + order)
    table = lm.compile()
    mass = R.enumerate_paths(z)
    res = N.search_lm(z, 16, lm, alpha, beta, eos_term)
    want = []
    for h, m in mass.items():
        l, _ = N.walk(table, h, np.float64, eos_term=eos_term)
        want.append((m + alpha * float(l) + beta * len(h), h, m, float(l)))
    want.sort(key=lambda r: -r[0])
    assert res["hyps"] == [r[1] for r in want]
    for got, col in ((res["score"], 0), (res["ctc"], 2), (res["lm"], 3)):
        assert np.abs(np.array(got, dtype=np.float64) - np.array([r[col] for r in want])).max() <= 1e-12 * 64
    # the table's float32 values are the LM: they are the host evaluation's within float32 rounding
    for h in mass:
        assert abs(float(N.walk(table, h, np.float64, eos_term=eos_term)[0]) - lm.score(h, eos_term)) <= 1e-5 * (len(h) + 1) * 8


def test_grid_stays_within_the_cap_on_undecided_cases():
    """The GPU grid's seeds judged by the restatements alone: at most ctc_beam_ref.UNDECIDED_CAP of its utterances are
    undecided; tests/test_ngram_gpu.py compares only scores there."""
    cases, extra = N.grid()
    assert len(cases) == 128 and len(extra) == len(R.EXTRA) and any(c[0] == 1030 for c in extra)
    assert {c[4] for c in cases} == set(N.ORDERS) and {c[5:] for c in cases} == set(N.WEIGHTS)
    assert len({c[4:] for c in cases}) == 9
    verdicts = [u["decisive"] for c in cases + extra for u in N.judge(c)]
    undecided = verdicts.count(False)
    print("undecided: %d of %d utterances" % (undecided, len(verdicts)))
    assert undecided <= R.UNDECIDED_CAP * len(verdicts), (undecided, len(verdicts))


def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert re.search(r"^int asr_ngram_score_f32\(int N, int L, int S, int V, const float\* lm_logp, const int32_t\* lm_next, "
                     r"int lm_start, int eos,", header, flags=re.M)
    assert re.search(r"^int asr_ctc_beam_lm_f32\(int B, int T, int V, int K, const float\* logits, int64_t ld, "
                     r"const int32_t\* frame_lens, int S,", header, flags=re.M)
    entry.build()
    import hip_backend as hb
    assert "asr_ngram_score_f32" in hb.EXPORTS and "asr_ctc_beam_lm_f32" in hb.EXPORTS
    assert hasattr(hb.load(), "asr_ngram_score_f32") and hasattr(hb.load(), "asr_ctc_beam_lm_f32")


def test_config_keys():
    entry.build()
    from solver import Solver
    assert Solver.ngram_config({}, False, True) == (False, None, 0.0, 0.0)
    assert Solver.ngram_config(dict(ctc_beam_decode=True, beam_size=4), False, True) == (True, None, 0.0, 0.0)
    assert Solver.ngram_config(dict(ctc_beam_decode=True, ngram_lm="x.arpa", ngram_weight=0.5, ngram_bonus=1), False, True) == \
        (True, "x.arpa", 0.5, 1.0)
    assert Solver.ngram_config(dict(two_pass_decode=True, ngram_lm="x.arpa"), True, True) == (False, "x.arpa", 0.0, 0.0)
    with pytest.raises(ValueError, match="ctc_beam_decode or two_pass_decode"):
        Solver.ngram_config(dict(ngram_lm="x.arpa", beam_size=4), False, True)
    with pytest.raises(ValueError, match="ctc_beam_decode or two_pass_decode"):
        Solver.ngram_config(dict(ngram_lm="x.arpa", ctc_greedy_decode=True), False, True)
    with pytest.raises(ValueError, match="without ngram_lm"):
        Solver.ngram_config(dict(ngram_weight=0.5, two_pass_decode=True), True, True)
    with pytest.raises(ValueError, match="three decoders"):
        Solver.ngram_config(dict(ctc_beam_decode=True, two_pass_decode=True), True, True)
    with pytest.raises(ValueError, match="CTC head"):
        Solver.ngram_config(dict(ctc_beam_decode=True), False, False)
    with pytest.raises(ValueError, match="lm_weight"):
        Solver.ngram_config(dict(ctc_beam_decode=True, lm_weight=0.3), False, True)
    config = open(os.path.join(ROOT, "semi-supervised-asr_amd", "config.yaml")).read()
    for key in ("ctc_beam_decode", "ngram_lm", "ngram_weight", "ngram_bonus"):
        assert re.search(r"^# %s:" % key, config, flags=re.M) and not re.search(r"^%s:" % key, config, flags=re.M)
