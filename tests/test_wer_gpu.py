"""The word edit-distance kernel (asr_word_edit_distance_i32, csrc/edit_distance.hip) against its plain-Python
restatement (tests/wer_ref.py): exact integer equality of the distances, the word counts and the totals; utils.calculate_wer_ids
on the GPU against the strings of tests/golden/text.json; Solver.test with `wer_on_gpu` off and on; E2E.mwer_forward with
unit="word"."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import synth
import utils
import wer_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SKIP = 4                     # ids 0..3 are dropped before scoring (2 is <EOS>)
EOS = 2
SPACE = 4                      # letters from 5 up
A, B, C = 5, 6, 7
COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 257)      # words a side: across every C of the strip (64, 128, 256, 512 columns)


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _table(alphabet):
    t = torch.zeros(N_SKIP + 1 + alphabet, dtype=torch.uint8)
    t[:N_SKIP] = 1
    return t


def _pad(rows, fill):
    width = max(1, max(len(r) for r in rows))
    return [list(r) + [fill] * (width - len(r)) for r in rows]


def _launch(hb, hyps, refs, table, *, dtype=torch.int32, eos=EOS, ref_index=None, totals=None, hyp_len=None, space=SPACE):
    hyp = torch.tensor(_pad(hyps, EOS), dtype=dtype, device=DEV)
    ref = torch.tensor(_pad(refs, 0), dtype=torch.int32, device=DEV)
    lens = [len(h) for h in hyps] if hyp_len is None else hyp_len
    kw = dict(eos=eos, skip=None if table is None else table.to(DEV), totals=totals,
              hyp_len=torch.tensor(lens, dtype=torch.int32, device=DEV))
    if ref_index is not None:
        kw["ref_index"] = torch.tensor(ref_index, dtype=torch.int32, device=DEV)
    dist, hyp_n, ref_n = hb.word_edit_distance(hyp, ref, torch.tensor([len(r) for r in refs], dtype=torch.int32, device=DEV),
                                               space, **kw)
    assert dist.dtype == hyp_n.dtype == ref_n.dtype == torch.int32 and dist.is_cuda
    return dist.tolist(), hyp_n.tolist(), ref_n.tolist()


def _expect(hyps, refs, table, eos=EOS, ref_index=None, space=SPACE):
    return wer_ref.word_edit_distance(hyps, refs, space, () if table is None else table.tolist(), eos, ref_index)


def _render(rs, words, fillers):
    """Words -> a raw row: one to three spaces between them, now and then some in front and behind, a token of `fillers`
    (dropped before scoring) after about one token in twelve."""
    row = [SPACE] * int(rs.randint(0, 3))
    for i, w in enumerate(words):
        if i:
            row += [SPACE] * int(rs.choice([1, 1, 1, 2, 3]))
        row += list(w)
    row += [SPACE] * int(rs.randint(0, 3))
    out = []
    for t in row:
        out.append(int(t))
        if rs.uniform() < 1.0 / 12:
            out.append(int(rs.choice(fillers)))
    return out


def _draw_words(rs, n, alphabet):
    return [tuple(rs.randint(N_SKIP + 1, N_SKIP + 1 + alphabet, size=int(rs.randint(1, 6))).tolist()) for _ in range(n)]


_GRID = {}


def _grid(alphabet):
    """Every (hypothesis, reference) combination of COUNTS, words of 1 .. 5 letters; every other pair a hypothesis mutated from
    its reference (about 15 % of the words redrawn), the rest independent draws.  Raw rows, the expected values: made once."""
    if alphabet not in _GRID:
        rs = np.random.RandomState(alphabet)
        hyps, refs, counts = [], [], []
        for (i, a), (j, b) in itertools.product(enumerate(COUNTS), enumerate(COUNTS)):
            rw = _draw_words(rs, b, alphabet)
            if (i * 13 + j) % 2 and a and b:
                hw = [rw[k % b] for k in range(a)]
                fresh = _draw_words(rs, a, alphabet)
                hw = [fresh[k] if rs.uniform() < 0.15 else hw[k] for k in range(a)]
            else:
                hw = _draw_words(rs, a, alphabet)
            tail = rs.randint(0, N_SKIP + 1 + alphabet, size=int(rs.randint(0, 9))).tolist()
            hyps.append(_render(rs, hw, [0, 1, 3]) + [EOS] + tail)
            refs.append(_render(rs, rw, [0, 1, 2, 3]))               # (an <EOS> inside a reference is dropped, not a cut)
            counts.append((a, b))
        table = _table(alphabet)
        want = _expect(hyps, refs, table)
        assert want[1] == [a for a, _ in counts] and want[2] == [b for _, b in counts]
        _GRID[alphabet] = hyps, refs, table, want
    return _GRID[alphabet]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("alphabet", [2, 30])
def test_kernel_over_the_grid_of_word_counts(hb, alphabet, dtype):
    hyps, refs, table, want = _grid(alphabet)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = _launch(hb, hyps, refs, table, dtype=dtype, totals=totals)
    bad = [(want[1][p], want[2][p], got[0][p], want[0][p]) for p in range(len(hyps)) if got[0][p] != want[0][p]]
    print("alphabet %d: %d pairs, %d wrong distances %s" % (alphabet, len(hyps), len(bad), bad[:8]))
    assert got[1] == want[1] and got[2] == want[2] and got[0] == want[0]
    assert totals.tolist() == [sum(want[0]), sum(want[2])]


def test_more_than_1024_reference_words_take_the_strip_path(hb):
    rs = np.random.RandomState(3)
    table = _table(2)
    ref = [A if rs.uniform() < 0.5 else B for _ in range(1025)]
    hyp = [t for t in ref[:200] if rs.uniform() > 0.1] + [C] + ref[900:]
    spaced = lambda ws: [t for w in ws for t in (w, SPACE)][:-1]
    hyps, refs = [spaced(hyp) + [EOS], spaced(ref[:30])], [spaced(ref), spaced(ref)]
    assert len(refs[0]) == 2049
    want = _expect(hyps, refs, table)
    assert want[2] == [1025, 1025] and want[1][0] > 300
    assert _launch(hb, hyps, refs, table) == want


SEGMENTATION = [
    ([SPACE, SPACE, A, B, SPACE, SPACE, SPACE, C, SPACE], [A, B, SPACE, C]),        # leading, trailing and repeated spaces
    ([SPACE, SPACE, SPACE], [A, SPACE, B]), ([A, SPACE, B], [SPACE]),               # a side of spaces only
    ([], []), ([EOS, A], []), ([], [A, B]), ([SPACE], [SPACE, SPACE]),               # empty sides
    ([A, SPACE, 0, SPACE, B], [A, SPACE, B]),                                        # a dropped token between spaces
    ([A, 0, B], [A, B]), ([A, 3, B, SPACE, 1], [A, SPACE, B]),                       # ... inside a word: it joins the letters
    ([0, 1, 3, 0], [A]), ([A], [0, 2, 1]),                                           # a side of dropped tokens only
    ([A, B, EOS, C, SPACE, A], [A, B, C]),                                           # <EOS> cuts a word
    ([A, SPACE, EOS, B], [A, SPACE, B]), ([A, SPACE, B, SPACE, EOS], [A, SPACE, B]), # ... directly behind a space
    ([A] * 100 + [SPACE, B], [A] * 100 + [SPACE, C]),                                # a word longer than 64 tokens
    ([A] * 99 + [B, SPACE, B], [A] * 100 + [SPACE, B]),                              # ... that differs in its last token
    ([A] * 300, [A] * 299), ([A, SPACE] * 29 + [SPACE, SPACE] + [B] * 10, [A, SPACE] * 29 + [B] * 10),   # a word over column 64
    ([A, SPACE] * 31 + [B, B, C], [A, SPACE] * 31 + [B, SPACE, C]),                  # columns 62 .. 64: one word or two
    ([A, SPACE] * 32 + [B], [A, SPACE] * 32 + [C]), ([A, SPACE] * 32, [SPACE, A] * 32),   # a word that starts at column 64
]


def test_segmentation(hb):
    table = _table(3)
    hyps, refs = [c[0] for c in SEGMENTATION], [c[1] for c in SEGMENTATION]
    want = _expect(hyps, refs, table)
    assert want[0] == [0, 2, 2, 0, 0, 1, 0, 0, 0, 2, 1, 1, 1, 1, 0, 1, 1, 1, 0, 2, 1, 0]       # (worked out by hand)
    assert want[1][7:10] == [2, 1, 1] and want[1][12:15] == [1, 1, 2] and want[1][18:] == [30, 32, 33, 32]
    assert _launch(hb, hyps, refs, table) == want
    assert _launch(hb, hyps, refs, table, dtype=torch.int64) == want
    # hyp_len shorter than the row, no <EOS> before it: what lies behind is not read - a word cut short, a space kept off
    hyps = [[A, B, SPACE, C, C, SPACE, A], [A, SPACE, B, SPACE, C]]
    refs = [[A, B, SPACE, C], [A, SPACE, B]]
    lens = [4, 3]
    want = _expect([h[:n] for h, n in zip(hyps, lens)], refs, table)
    assert want == ([0, 0], [2, 2], [2, 2])
    assert _launch(hb, hyps, refs, table, hyp_len=lens) == want
    # no skip table and no cut: every id is a token, <EOS> included
    hyps, refs = [[0, SPACE, EOS, 1]], [[0, SPACE, EOS]]
    assert _launch(hb, hyps, refs, None, eos=-1) == _expect(hyps, refs, None, eos=-1) == ([1], [2], [2])


def test_words_are_equal_only_when_their_tokens_are(hb):
    table = _table(2)
    cases = [([A, B], [A, B, B]), ([A, B], [B, A]), ([A, A, B], [A, B, A]), ([A, B], [A, B])]
    # every word over {A, B} of 1 .. 7 letters, the hypothesis a permutation of them: a hash that sums, or that looks at a
    # prefix only, calls different words equal here
    every = [w for n in range(1, 8) for w in itertools.product((A, B), repeat=n)]
    assert len(every) == 254
    order = np.random.RandomState(8).permutation(len(every))
    join = lambda ws: [t for w in ws for t in list(w) + [SPACE]][:-1]
    cases.append((join([every[i] for i in order]), join(every)))
    assert len(cases[-1][1]) < 2000
    hyps, refs = [c[0] for c in cases], [c[1] for c in cases]
    want = _expect(hyps, refs, table)
    assert want[0][:4] == [1, 1, 1, 0] and want[1][4] == want[2][4] == 254 and want[0][4] > 200
    assert _launch(hb, hyps, refs, table) == want


def test_k_hypotheses_per_reference_and_totals_over_two_launches(hb):
    K = 4
    rs = np.random.RandomState(K)
    table = _table(30)
    ref_words = [_draw_words(rs, n, 30) for n in (20, 3, 0, 70, 9)]
    refs = [_render(rs, w, [0, 1, 2, 3]) for w in ref_words]
    index = [b for b in range(len(refs)) for _ in range(K)]
    hyps = []
    for b in index:
        kept = [w for w in ref_words[b] if rs.uniform() > 0.2] + _draw_words(rs, int(rs.randint(0, 3)), 30)
        hyps.append(_render(rs, kept, [0, 1, 3]) + [EOS] * int(rs.randint(0, 4)))
    hyps[-1] = [EOS] * 12                                                # a rank the search left empty
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    want = _expect(hyps, refs, table, ref_index=index)
    assert len(set(want[0])) > 3
    assert _launch(hb, hyps, refs, table, ref_index=index, totals=totals) == want
    assert totals.tolist() == [sum(want[0]), sum(want[2])]
    order = list(reversed(index))
    want2 = _expect(hyps, refs, table, ref_index=order)
    assert _launch(hb, hyps, refs, table, ref_index=order, totals=totals) == want2
    assert totals.tolist() == [sum(want[0]) + sum(want2[0]), sum(want[2]) + sum(want2[2])]


def test_declines(hb):
    lib = hb.load()
    n, cols = 2, hb.ED_MAX_COLS + 1
    hyp = torch.full((n, cols), A, dtype=torch.int32, device=DEV)
    ref = torch.full((n, cols), A, dtype=torch.int32, device=DEV)
    lens = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    out = torch.full((3, n), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_pairs=n, hyp_p=p(hyp), hyp_cols=8, ldh=cols, ldr=8, ref_len=p(lens), dist=p(out), elem=4, space=SPACE):
        return lib.asr_word_edit_distance_i32(n_pairs, hyp_p, elem, ldh, hyp_cols, None, p(ref), ldr, ref_len, None, EOS, None,
                                              0, space, dist, None, None, None, hb.stream())
    assert call(hyp_cols=cols) == hb.ASR_E_SHAPE and call(ldr=cols) == hb.ASR_E_SHAPE
    assert call() == 0
    assert call(space=-1) == -1                                          # ASR_E_ARG
    for bad in (dict(n_pairs=0), dict(hyp_p=None), dict(ref_len=None), dict(dist=None), dict(elem=2), dict(ldh=4)):
        assert call(**bad) == -1, bad
    with pytest.raises(hb.UnsupportedShape):
        hb.word_edit_distance(hyp, ref, lens, SPACE)
    with pytest.raises(RuntimeError):
        hb.word_edit_distance(hyp[:, :8], ref[:, :8], lens, -1)
    # the whole width at the limit, 80 KiB of LDS: 4 096 raw columns a side, 2 048 one-letter words
    row = [A, SPACE] * (hb.ED_MAX_COLS // 2)
    other = [B if i % 7 == 0 else A for i in range(300)]
    hyps, refs = [[t for w in other for t in (w, SPACE)] + [SPACE] * (hb.ED_MAX_COLS - 600)], [row]
    assert len(row) == len(hyps[0]) == hb.ED_MAX_COLS
    want = _expect(hyps, refs, None)
    assert want[2] == [2048] and want[1] == [300]
    assert _launch(hb, hyps, refs, None) == want
    # calculate_wer_ids: one over-long hypothesis sends the call to the host loop, same three values
    rs = np.random.RandomState(11)
    vocab, nls = synth.wsj_vocab(), list(synth.NON_LANG_SYMS)
    letters = [i for s, i in vocab.items() if s not in nls]
    long_hyps = [rs.choice(letters, size=k).tolist() + [vocab["<EOS>"]] for k in (hb.ED_MAX_COLS + 4, 40)]
    short_refs = [rs.choice(letters, size=k).tolist() for k in (60, 50)]
    got = utils.calculate_wer_ids(long_hyps, short_refs, vocab, nls, vocab["<EOS>"], torch.device(DEV))
    hs = utils.to_sents(utils.remove_pad_eos(long_hyps, eos=vocab["<EOS>"]), vocab, nls)
    rf = utils.to_sents(short_refs, vocab, nls)
    assert got == (utils.calculate_wer(hs, rf), [utils.edit_distance(h.split(), r.split()) for h, r in zip(hs, rf)],
                   [len(r.split()) for r in rf])
    assert sum(got[2]) > 2


def test_text_json_on_the_gpu(hb, golden_dir, monkeypatch):
    with open(os.path.join(golden_dir, "text.json")) as f:
        t = json.load(f)
    launches = []
    real = hb.word_edit_distance
    monkeypatch.setattr(hb, "word_edit_distance", lambda *a, **k: launches.append(1) or real(*a, **k))
    wer, dist, ref_n = utils.calculate_wer_ids(t["preds"], t["refs"], t["vocab"], t["non_lang_syms"], t["vocab"]["<EOS>"],
                                               torch.device(DEV))
    assert len(launches) == 1, "one launch, on the device"
    assert wer == utils.calculate_wer(t["hyp"], t["ref"])
    assert dist == [utils.edit_distance(h.split(), r.split()) for h, r in zip(t["hyp"], t["ref"])]
    assert ref_n == [len(r.split()) for r in t["ref"]]


# ------------------------------------------------------------------------------------------------------------------ Solver
@pytest.mark.parametrize("beam_size", [1, 4])
def test_test_reports_wer_with_wer_on_gpu_and_is_unchanged_without(hb, tmp_path, monkeypatch, capsys, beam_size):
    import test_cer_gpu as tc
    s = tc._solver(str(tmp_path), monkeypatch, beam_size=beam_size)
    replay = tc._Replay(s.model, monkeypatch)
    launches = dict(token=[], word=[])
    real_token, real_word = hb.edit_distance, hb.word_edit_distance
    monkeypatch.setattr(hb, "edit_distance", lambda *a, **k: launches["token"].append(a[0].shape[0]) or real_token(*a, **k))
    monkeypatch.setattr(hb, "word_edit_distance", lambda *a, **k: launches["word"].append(a[0].shape[0]) or real_word(*a, **k))
    state = {k: v.clone() for k, v in s.model.state_dict().items()}

    def run():
        replay.rewind()
        capsys.readouterr()
        cer = s.test(state_dict=state)
        line = capsys.readouterr().out.splitlines()[-1]
        with open("eval.txt") as f:
            text = f.read().splitlines()
        return cer, line, text, dict(s.last_test)

    # without the key: the parent's record, line and launches
    cer_off, line_off, text_off, last_off = run()
    assert launches == dict(token=[], word=[])
    assert last_off == dict(cer=cer_off, best_of_k_cer=None, dist=None, ref_n=None)
    assert line_off == "eval: 6 utterances, CER=%.4f" % cer_off
    # with it: one word launch over all K hypotheses of all utterances; the CER side as before
    s.config["wer_on_gpu"] = True
    cer_on, line_on, text_on, last = run()
    assert launches == dict(token=[], word=[6 * beam_size]) and cer_on == cer_off and text_on == text_off
    refs = utils.to_sents([list(tokens) for _, tokens in s._dataset("eval", None, sort=False)], s.vocab, s.non_lang_syms)
    assert last["wer"] == utils.calculate_wer(text_on, refs) and type(last["wer"]) is float
    assert [d[0] for d in last["word_dist"]] == [utils.edit_distance(h.split(), r.split()) for h, r in zip(text_on, refs)]
    assert last["word_ref_n"] == [len(r.split()) for r in refs] and sum(last["word_ref_n"]) > 6
    assert {k: last[k] for k in last_off} == last_off, "the CER side does not change"
    want_line = line_off + ", WER=%.4f" % last["wer"]
    if beam_size == 1:
        assert "best_of_k_wer" not in last and all(len(d) == 1 for d in last["word_dist"])
        assert line_on == want_line
        return
    eos = s.vocab["<EOS>"]
    best = 0
    for b, ref in enumerate(refs):
        tokens = replay.memo["beams", b][0]
        hyps = utils.to_sents(utils.remove_pad_eos(tokens[0].cpu().tolist(), eos=eos), s.vocab, s.non_lang_syms)
        dist = [utils.edit_distance(h.split(), ref.split()) for h in hyps]
        assert last["word_dist"][b] == dist
        best += min(dist)
    assert last["best_of_k_wer"] == float(best) / float(sum(last["word_ref_n"])) <= last["wer"]
    assert line_on == want_line + ", best of 4: WER=%.4f" % last["best_of_k_wer"]
    # both keys: one launch each
    s.config["cer_on_gpu"] = True
    launches["word"].clear()
    cer_both, line_both, _, last_both = run()
    assert launches == dict(token=[24], word=[24]) and cer_both == cer_off
    assert last_both["best_of_k_cer"] is not None and last_both["wer"] == last["wer"]
    assert last_both["best_of_k_wer"] == last["best_of_k_wer"]
    assert line_both == "eval: 6 utterances, CER=%.4f, best of 4 hypotheses: CER=%.4f, WER=%.4f, best of 4: WER=%.4f" % (
        cer_off, last_both["best_of_k_cer"], last["wer"], last["best_of_k_wer"])


# ------------------------------------------------------------------------------------------------------------------ MWER
MWER_SPACE = 3                 # the tiny model's vocabulary: 0 .. 8, <EOS> = 2; 3 plays <space>, 4 .. 8 the letters
MWER_REFS = [[4, 5, 3, 6, 7], [4, 3, 5, 3, 6]]                            # "ab cd", "a b c"
MWER_HYPS = [[[4, 5, 3, 6, 7],             # the reference: 0 token errors, 0 word errors
              [4, 5, 6, 7],                # the space lost: 1 token error, 2 word errors
              [8, 8, 3, 6, 7]],            # two letters of one word wrong: 2 token errors, 1 word error
             [[4, 3, 5, 3, 6],
              [4, 3, 3, 5, 6, 3],          # "a  bc ": 3 token errors, 2 word errors
              None]]                       # an unused slot


def _mwer_case():
    import test_beam_ctc_gpu as tbc
    net, _, xs, ilens, _ = tbc._modules((0, 0.0, 14))
    B, K, T = 2, 3, 7
    tokens = torch.full((B, K, T), EOS, dtype=torch.int64)
    lens = torch.full((B, K), -1, dtype=torch.int32)
    for b, k in itertools.product(range(B), range(K)):
        if MWER_HYPS[b][k] is not None:
            tokens[b, k, :len(MWER_HYPS[b][k])] = torch.tensor(MWER_HYPS[b][k])
            lens[b, k] = len(MWER_HYPS[b][k])
    ys = [torch.tensor(r, dtype=torch.int64, device=DEV) for r in MWER_REFS]
    return net, xs[:B], ilens[:B], ys, (tokens.to(DEV), lens.to(DEV))


def test_mwer_forward_on_word_errors(hb):
    import ops
    net, xs, ilens, ys, hyps = _mwer_case()
    B, K = 2, 3
    flat = [h if h is not None else [] for row in MWER_HYPS for h in row]
    index = [b for b in range(B) for _ in range(K)]
    word_err = wer_ref.word_edit_distance(flat, MWER_REFS, MWER_SPACE, (), EOS, index)[0]
    token_err = [utils.edit_distance(h, MWER_REFS[b]) for h, b in zip(flat, index)]
    assert word_err == [0, 2, 1, 0, 2, 3] and token_err == [0, 1, 2, 0, 3, 5]
    with pytest.raises(ValueError, match="space_id"):
        net.mwer_forward(xs, ilens, ys, K, ce_weight=0.0, hyps=hyps, unit="word")
    net.space_id = MWER_SPACE
    with hb.deterministic():
        word = net.mwer_forward(xs, ilens, ys, K, ce_weight=0.0, hyps=hyps, unit="word").detach().clone()
        assert net.last_mwer["err"].tolist() == word_err
        token = net.mwer_forward(xs, ilens, ys, K, ce_weight=0.0, hyps=hyps, unit="token").detach().clone()
        assert net.last_mwer["err"].tolist() == token_err
        default = net.mwer_forward(xs, ilens, ys, K, ce_weight=0.0, hyps=hyps).detach().clone()
        # the step's own composition, fed the restatement's errors
        want = {}
        for name, err in (("word", word_err), ("token", token_err)):
            enc_h, enc_lens = net.encoder(xs, ilens)
            _, logits, tok_lb, npos = net.decoder.score_hypotheses_grad(enc_h, enc_lens, hyps[0], hyps[1], scores=False)
            loss, _ = ops.mwer_loss(logits, tok_lb, npos, torch.tensor(err, dtype=torch.int32, device=DEV), 1.0 / B, n_utts=B)
            want[name] = loss.detach().clone()
    bits = lambda t: int(t.view(torch.int32))
    print("mwer loss on word errors %.7f, on token errors %.7f" % (float(word), float(token)))
    assert bits(word) == bits(want["word"]) and bits(token) == bits(want["token"]) == bits(default)
    assert bits(word) != bits(token) and float(word) != 0.0
