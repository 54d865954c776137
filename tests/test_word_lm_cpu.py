"""The word-level LM and lexicon without a GPU (word_lm.py, tests/word_lm_ref.py): ARPA in and out, the trie
against a dictionary, the sparse lookup against the recursive evaluator and NgramLM's dense table, the estimate's rows, word
counting against tests/wer_ref.py, the fused search's restatement against the plain one and against the enumeration of every
labelling, the share of the GPU grid the restatements leave undecided, the entries and the config keys."""
import os
import re

import numpy as np
import pytest

import ctc_beam_ref as R
import wer_ref
import word_lm_ref as WR
from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_UNK, W_FIRST

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "<space>": 3, "a": 4, "b": 5, "c": 6, "d": 7}


def _rows(V, space, seed, n=30, longest=14):
    rs = np.random.RandomState(seed)
    pool = [t for t in range(1, V) if t != space] + [space] * max(1, (V - 2) // 3)
    return [[int(pool[rs.randint(len(pool))]) for _ in range(rs.randint(0, longest))] for _ in range(n)]


def test_lexicon_refuses_by_name_and_spells_by_characters():
    lex = Lexicon(["ab", "abc", "d", "ab"], VOCAB, VOCAB["<space>"], 1, 2)
    assert lex.spellings == [(4, 5), (4, 5, 6), (7,)] and lex.V == 8
    with pytest.raises(ValueError, match="'axb'"):
        Lexicon(["ab", "axb"], VOCAB, 3, 1, 2)
    for bad in ((0,), (3,), (1,), (2,), (8,), ()):
        with pytest.raises(ValueError):
            Lexicon([bad], VOCAB, 3, 1, 2)


@pytest.mark.parametrize("V,n", [(4, 6), (8, 40), (34, 300)])
def test_trie_against_a_dictionary(V, n):
    rs = np.random.RandomState(V + n)
    letters = list(range(1, V - 1))
    words = [tuple(int(letters[rs.randint(len(letters))]) for _ in range(rs.randint(1, 6))) for _ in range(n)]
    lex = Lexicon(words, None, V - 1, V=V)
    ids = [100 + i for i in range(len(lex))]
    nxt, word = lex.compile(ids)
    table = {w: 100 + i for w, i in lex.index.items()}
    assert nxt.dtype == word.dtype == np.int32 and nxt.shape == (len(word), V) and (nxt[:, [0, V - 1]] == -1).all()
    assert sorted(int(w) for w in word if w >= 0) == sorted(table.values())
    probes = words + [tuple(int(letters[rs.randint(len(letters))]) for _ in range(rs.randint(1, 7))) for _ in range(400)]
    for w in probes:
        node = 0
        for c in w:
            node = -1 if node < 0 else int(nxt[node, c])
        assert (word[node] if node >= 0 else -1) == table.get(w, -1), w


@pytest.mark.parametrize("order", [1, 2, 3])
def test_arpa_round_trip(order, tmp_path):
    rows = _rows(8, 3, 5 * order)
    rows = [[t for t in r if t not in (1, 2)] for r in rows]
    lm = WordLM.estimate(rows, 3, order, V=8, bos=1, eos=2)
    sym = {i: s for s, i in VOCAB.items()}
    names = {wid: "".join(sym[c] for c in sp) for sp, wid in zip(lm.lexicon.spellings, lm.word_ids)}
    names[W_UNK] = "<unk>"
    text = lm.lm.to_arpa(names)
    path = tmp_path / "words.arpa"
    path.write_text(text)
    chars = {s: i for s, i in VOCAB.items() if len(s) == 1}
    for back in (WordLM.from_arpa(text, chars, 3, bos=1, eos=2, V=8), WordLM.from_arpa(str(path), chars, 3, bos=1, eos=2, V=8)):
        assert (back.V, back.space, back.bos, back.eos, back.order) == (8, 3, 1, 2, order)
        assert sorted(back.lexicon.spellings) == sorted(lm.lexicon.spellings)
        for r in rows[:12] + [[4, 4, 4, 4, 3, 7]]:                   # (the last row holds a word outside the lexicon)
            assert abs(back.score(r) - lm.score(r)) <= 1e-12 * max(1.0, abs(lm.score(r)))
        assert back.compile().A == lm.compile().A and back.compile().S == lm.compile().S
    # a given lexicon: only its words can be spelled, the others are <unk>
    short = WordLM.from_arpa(text, chars, 3, lexicon=list(names.values())[:2] + ["d" * 15], bos=1, eos=2, V=8)
    assert len(short.lexicon) == 3 and short.W == lm.W + 1
    t = short.compile()
    assert sorted(int(w) for w in t.trie_word if w >= 0) == [W_FIRST, W_FIRST + 1, W_FIRST + 2] and t.uni_next[W_FIRST + 2] == -1


@pytest.mark.parametrize("V", [4, 5, 34])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_sparse_lookup_against_the_evaluator_and_the_dense_table(V, order):
    """Every (state, word): the sparse lookup over the float64 values is the recursive evaluator's and the dense table's of
    NgramLM.compile() over the same word ids to 1e-12, and the successor is the dense table's - a word without a unigram
    scores oov_logp and goes to the empty context.  The float32 tables are those values rounded once."""
    for seed in (2 * V + order, 2 * V + order + 1):                  # (an odd seed: <unk> has a unigram)
        wlm = WR.random_word_lm(V, order, seed)
        lm, t = wlm.lm, wlm.compile()
        dense, states = lm.compile(), lm.states()
        assert t.S == dense.S == len(states) and t.start == dense.start and states[t.empty] == ()
        assert ((W_UNK,) in lm.prob) == bool(seed % 2) and any((w,) not in lm.prob for w in wlm.word_ids)
        assert (np.diff(t.arc_off) >= 0).all() and t.arc_off[-1] == t.A
        for s in range(t.S):
            arcs = t.arc_word[t.arc_off[s]:t.arc_off[s + 1]]
            assert (np.diff(arcs) > 0).all()
            for w in range(1, t.W):
                lp, nx = t.lookup(s, w, np.float64, exact=True)
                want = WR.backoff_logp(lm, states[s], w)
                assert abs(lp - want) <= 1e-12 * max(1.0, abs(want)), (states[s], w)
                assert abs(lp - dense.logp64[s, w]) <= 1e-12 * max(1.0, abs(want)), (states[s], w)
                if (w,) in lm.prob:
                    assert nx == dense.nxt[s, w], (states[s], w)
                else:
                    assert lp == lm.oov_logp and nx == t.empty
        exact = t.exact
        assert np.array_equal(t.arc_logp, exact[0].astype(np.float32)) and np.array_equal(t.bo_logp, exact[1].astype(np.float32))
        assert np.array_equal(t.uni_logp, exact[2].astype(np.float32))
        # rows: the table's walk is the evaluator's score within float32 rounding of the table; n_words is the split's
        for row in _rows(V, V - 1, seed):
            row = [c for c in row if c != 0]
            for eos_term in (True, False):
                want, n = WR.row_score(wlm, row, eos_term)
                got, per, nw = WR.walk(t, row, np.float64, eos_term)
                assert nw == n == len(per) == wlm.n_words(row)
                assert abs(float(got) - want) <= 1e-5 * max(1.0, abs(want))
                assert abs(wlm.score(row, eos_term) - want) <= 1e-12 * max(1.0, abs(want))


def test_compile_refuses_what_the_kernels_cannot_trust():
    wlm = WR.random_word_lm(5, 2, 3)
    t = wlm.compile()
    for field, at, value in (("arc_next", 0, t.S), ("trie_next", (0, 1), t.N), ("trie_word", 1, t.W), ("bo_state", 2, -1),
                             ("uni_logp", 4, np.inf), ("arc_off", 1, t.A + 1)):
        arrays = {k: np.array(v) for k, v in t.arrays().items() if k != "n_arcs"}
        arrays[field][at] = value
        arrays["n_arcs"] = t.A
        from word_lm import WordTable
        with pytest.raises(ValueError):
            WordLM.check_table(WordTable(arrays, t.V, t.space, t.start, t.empty, t.eos, t.unk, t.order))
    wlm = WR.random_word_lm(5, 2, 3)
    wlm.lexicon.V = 2 ** 30
    with pytest.raises(ValueError, match="2\\*\\*31"):
        wlm.compile()


@pytest.mark.parametrize("V,order", [(5, 1), (8, 2), (8, 3), (34, 3)])
def test_estimate_is_proper(V, order):
    """Every context's distribution over {words, <unk>, </s>} sums to 1 within 1e-12, at every state and after histories
    the text never held; the lexicon is the words seen."""
    rows = _rows(V, V - 1, 7 * V + order, n=40)
    wlm = WordLM.estimate(rows, V - 1, order, V=V)
    seen = sorted({w for r in rows for w in wer_ref.words(r, V - 1)})
    assert wlm.lexicon.spellings == seen and wlm.W == W_FIRST + len(seen)
    events = [w for w in range(1, wlm.W) if (w,) in wlm.lm.prob]
    assert events == [w for w in range(2, wlm.W)]
    rs = np.random.RandomState(order)
    contexts = wlm.lm.states() + [tuple(int(c) for c in rs.randint(3, wlm.W, size=rs.randint(0, 5))) for _ in range(20)]
    for h in contexts:
        total = sum(np.exp(WR.backoff_logp(wlm.lm, h, w)) for w in events)
        assert abs(total - 1.0) <= 1e-12, (h, total)


@pytest.mark.parametrize("V", [4, 8, 34])
def test_words_are_wer_refs_words(V):
    space = V - 1
    wlm = WR.random_word_lm(V, 2, V)
    t = wlm.compile()
    rows = _rows(V, space, V, n=200) + [[space], [space, space, 1, space, space, 2, space], [1] * 100, []]
    for row in rows:
        want = wer_ref.words(row, space)
        assert WR.split(row, space) == want and wlm.n_words(row) == len(want)
        assert WR.walk(t, [c for c in row], np.float32, True)[2] == len(want)


@pytest.mark.parametrize("V,K,T,scale", [(4, 16, 3, 1.0), (5, 4, 7, 1.0), (34, 2, 20, 50.0), (34, 16, 12, 1.0)])
def test_without_weights_the_search_is_the_plain_one(V, K, T, scale):
    z = np.random.RandomState(V * K + T).normal(0, scale, size=(T, V))
    wlm = WR.random_word_lm(V, 3, 5)
    for dt in (np.float64, np.float32):
        plain, fused = R.search(z.astype(dt), K), WR.search_wlm(z.astype(dt), K, wlm, 0.0, 0.0, False, False)
        assert fused["hyps"] == plain["hyps"]
        assert np.array_equal(fused["score"], plain["scores"]) and np.array_equal(fused["ctc"], plain["scores"])
        for h, v, n in zip(fused["hyps"], fused["lm"], fused["nw"]):
            total, _, nw = WR.walk(wlm.compile(), h, dt, eos_term=False)
            assert v == total and n == nw == len(wer_ref.words(h, V - 1))


def _in_lexicon(wlm, h):
    return all(w in wlm.lexicon.index for w in wer_ref.words(h, wlm.space))


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("alpha,beta,eos_term,lexicon_only", [(0.5, 0.0, True, False), (2.0, 1.5, False, False), (1.0, -1.0, True, True),
                                                              (0.75, 0.5, False, True)])
def test_exhaustive_definition(T, order, alpha, beta, eos_term, lexicon_only):
    """V = 4 (blank, a, b, <space>), K = 16: at most 3 + 9 + 27 + 1 labellings exist for T <= 3 and the beam of a frame
    never drops one that matters - with T <= 2 it holds them all, so the ranked list IS every labelling of
    ctc_beam_ref.enumerate_paths ranked by mass + alpha lm + beta n_words (+ alpha x the end term), scores to 1e-12; with
    lexicon_only only the labellings that are sequences of lexicon words.  T = 3 has 40 labellings: the list is then the
    top 16 of them as long as no labelling was cut early, which the test asserts through the definition itself."""
    z = np.random.RandomState(10 * T + order).normal(0, 2, size=(T, 4))
    wlm = WR.random_word_lm(4, order, 77 + order, extra_words=[(1,), (2, 1)])
    table = wlm.compile()
    mass = R.enumerate_paths(z)
    res = WR.search_wlm(z, 16, wlm, alpha, beta, eos_term, lexicon_only)
    want = []
    for h, m in mass.items():
        if lexicon_only and not _in_lexicon(wlm, h):
            continue
        l, _, n = WR.walk(table, h, np.float64, eos_term=eos_term)
        assert n == len(wer_ref.words(h, 3))
        want.append((m + alpha * float(l) + beta * n, h, m, float(l), n))
    want.sort(key=lambda r: -r[0])
    if T <= 2:
        assert len(want) <= 16 and res["hyps"] == [r[1] for r in want]
    else:                                                            # the beam may have cut a prefix: what it reports is ranked right
        at = {r[1]: r for r in want}
        assert all(h in at for h in res["hyps"]) and res["hyps"][0] == want[0][1]
        want = [at[h] for h in res["hyps"]]
        assert all(a[0] >= b[0] for a, b in zip(want, want[1:]))
    for got, col in ((res["score"], 0), (res["ctc"], 2), (res["lm"], 3), (res["nw"], 4)):
        assert np.abs(np.array(got, dtype=np.float64) - np.array([r[col] for r in want])).max() <= 1e-12 * 64
    for h in mass:                                                   # the table's float32 values are the LM within rounding
        assert abs(float(WR.walk(table, h, np.float64, eos_term)[0]) - wlm.score(h, eos_term)) <= 1e-5 * (len(h) + 1) * 8
    if lexicon_only:
        assert all(_in_lexicon(wlm, h) for h in res["hyps"])


def test_grid_stays_within_the_cap_on_undecided_cases():
    """The GPU grid's seeds judged by the restatements alone: at most UNDECIDED_CAP of its utterances are undecided;
    tests/test_word_lm_gpu.py compares only scores there."""
    cases, extra = WR.grid()
    assert len(cases) == 128 and len(extra) == len(R.EXTRA) and any(c[0] == 1030 for c in extra)
    assert {c[4] for c in cases} == set(WR.ORDERS) and {c[5:7] for c in cases} == set(WR.WEIGHTS) and {c[7] for c in cases} == {False, True}
    assert len({c[4:] for c in cases}) == 18
    verdicts = [u["decisive"] for c in cases + extra for u in WR.judge(c)]
    undecided = verdicts.count(False)
    print("undecided: %d of %d utterances" % (undecided, len(verdicts)))
    assert undecided <= WR.UNDECIDED_CAP * len(verdicts), (undecided, len(verdicts))
    kept = [len(u["ref"]["hyps"]) for c in cases + extra if c[7] for u in WR.judge(c)]
    assert sum(1 for n in kept if n >= 1) >= len(kept) // 2, "lexicon_only leaves most utterances without a hypothesis"


def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert re.search(r"^int asr_word_lm_score_f32\(int N, int L, const asr_word_lm_t\* lm, int eos_term,", header, flags=re.M)
    assert re.search(r"^int asr_ctc_beam_wlm_f32\(int B, int T, int V, int K, const float\* logits, int64_t ld, "
                     r"const int32_t\* frame_lens,\n\s+const asr_word_lm_t\* lm,", header, flags=re.M)
    assert re.search(r"^#define ASR_ABI_VERSION 8$", header, flags=re.M)
    entry.build()
    import hip_backend as hb
    assert "asr_word_lm_score_f32" in hb.EXPORTS and "asr_ctc_beam_wlm_f32" in hb.EXPORTS
    assert hasattr(hb.load(), "asr_word_lm_score_f32") and hasattr(hb.load(), "asr_ctc_beam_wlm_f32")


def test_config_keys():
    entry.build()
    from solver import Solver
    assert Solver.word_lm_config({}, False, False) == (None, None, 0.0, 0.0, False)
    assert Solver.word_lm_config(dict(word_lm="w.arpa", word_lm_weight=0.5, word_bonus=1, lexicon="l.txt", lexicon_only=True),
                                 False, True) == ("w.arpa", "l.txt", 0.5, 1.0, True)
    assert Solver.word_lm_config(dict(word_lm="w.arpa"), True, False) == ("w.arpa", None, 0.0, 0.0, False)
    with pytest.raises(ValueError, match="ctc_beam_decode or two_pass_decode"):
        Solver.word_lm_config(dict(word_lm="w.arpa", beam_size=4), False, False)
    with pytest.raises(ValueError, match="ngram_lm"):
        Solver.word_lm_config(dict(word_lm="w.arpa", ngram_lm="x.arpa"), False, True)
    for key in ("lexicon", "word_lm_weight", "word_bonus", "lexicon_only"):
        with pytest.raises(ValueError, match="without word_lm"):
            Solver.word_lm_config({key: 1}, True, False)
    config = open(os.path.join(ROOT, "semi-supervised-asr_amd", "config.yaml")).read()
    for key in ("word_lm", "lexicon", "word_lm_weight", "word_bonus", "lexicon_only"):
        assert re.search(r"^# %s:" % key, config, flags=re.M) and not re.search(r"^%s:" % key, config, flags=re.M)
