"""The transducer beam search with a lexicon and a word-level LM inside, on the GPU (csrc/rnnt_beam.hip's WLM kernels, the
asr_transducer_wbeam_* entries) against tests/rnnt_wbeam_ref.py.

Every batch of the grid is ragged, holds five utterances - one without a frame - and carries NaN in the encoder output (so
in PE) behind every utterance.  Hypotheses, their order and n_words are compared exactly where rnnt_wbeam_ref.judge is
decisive (tests/test_rnnt_wbeam_cpu.py holds that every utterance of the grid is), scores within its allowance; the bound
rnnt_score <= log P(hyp | x) + allowance and lm_score == ops.word_lm_score(hyp), bit for bit, hold everywhere."""
import os

import numpy as np
import pytest
import torch

import poison as P
import rnnt_beam_ref as BR
import rnnt_wbeam_ref as WB
import word_lm_ref as WR
import test_rnnt_beam_gpu as TB

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture(autouse=True)
def _clean_pools():
    yield
    P.empty_pool()


def _wkw(wlm, alpha=WB.ALPHA, beta=WB.BETA, eos_term=True, lexicon_only=False):
    return dict(word_lm=wlm, word_lm_weight=alpha, word_bonus=beta, eos_term=eos_term, lexicon_only=lexicon_only)


def _rows(out):
    """-> per utterance [(tokens, score, tot, lm, nw)] of the used slots; checks the layout on the way."""
    hyp, hyp_len, score, tot, lm, nw = out
    res = []
    for b in range(hyp.shape[0]):
        used = int((hyp_len[b] >= 0).sum())
        assert (hyp_len[b, :used] >= 0).all() and (hyp_len[b, used:] == -1).all() and (nw[b, used:] == -1).all()
        assert np.isfinite(score[b, :used]).all() and np.isfinite(tot[b, :used]).all() and np.isfinite(lm[b, :used]).all()
        assert np.isneginf(score[b, used:]).all() and np.isneginf(tot[b, used:]).all() and np.isneginf(lm[b, used:]).all()
        assert (np.diff(score[b, :used]) <= 0).all() and (hyp[b, used:] == -1).all() and (nw[b, :used] >= 0).all()
        rows = []
        for k in range(used):
            n = int(hyp_len[b, k])
            assert (hyp[b, k, n:] == -1).all()
            rows.append((tuple(int(v) for v in hyp[b, k, :n]), float(score[b, k]), float(tot[b, k]), float(lm[b, k]), int(nw[b, k])))
        assert len(set(r[0] for r in rows)) == len(rows)
        res.append(rows)
    return res


def _lm_bits(wlm, out, eos_term):
    """lm_score and n_words of every used slot are ops.word_lm_score's of the returned row, bit for bit."""
    import ops
    hyp, hyp_len, _, _, lm, nw = out
    L = hyp.shape[2]
    want, words = ops.word_lm_score(wlm, torch.from_numpy(hyp.reshape(-1, L)).to(DEV), torch.from_numpy(hyp_len.reshape(-1)).to(DEV),
                                    eos_term=eos_term)
    want, words = want.cpu().numpy().reshape(lm.shape), words.cpu().numpy().reshape(nw.shape)
    used = hyp_len >= 0
    assert lm[used].tobytes() == want[used].tobytes() and np.array_equal(nw[used], words[used])


def _rank_bits(out, alpha, beta):
    _, hyp_len, score, tot, lm, nw = out
    used = hyp_len >= 0
    f32 = np.float32
    assert np.array_equal(score[used], (tot[used] + f32(alpha) * lm[used]) + f32(beta) * nw[used].astype(f32))


def _compare(what, p, utts, K, L, out, wlm, judged, head=None, alpha=WB.ALPHA, beta=WB.BETA, eos_term=True, lexicon_only=False):
    """judged(b) -> rnnt_wbeam_ref.judge's verdict on utterance b.  Exact hypotheses, order and n_words and scores within the
    allowance where it is decisive; with `head` the bound rnnt_score <= -ops.rnnt_loss(hyp) + allowance everywhere."""
    rows = _rows(out)
    V = p["lin_out.weight"].shape[0]
    bound = TB._loss_bound(head, utts, [[(r[0], r[1]) for r in rr] for rr in rows]) if head is not None else {}
    _lm_bits(wlm, out, eos_term)
    _rank_bits(out, alpha, beta)
    worst, undecided = 0.0, 0
    for b in range(len(utts)):
        assert all(1 <= v < V for r in rows[b] for v in r[0]) and all(len(r[0]) <= L for r in rows[b])
        if lexicon_only:
            assert all(w in wlm.lexicon.index for r in rows[b] for w in WR.split(r[0], wlm.space)), (what, b)
        j = judged(b)
        want = j["ref"]["finals"][:K]
        over = [(r[2] - bound[(b, r[0])]) / j["allowance"] for r in rows[b] if (b, r[0]) in bound]
        if over:
            assert max(over) <= 1.0, (what, b, max(over))
        if not j["decisive"]:
            undecided += 1
            continue
        assert [r[0] for r in rows[b]] == [f["tokens"] for f in want], (what, b, rows[b], [f["tokens"] for f in want])
        assert [r[4] for r in rows[b]] == [f["nw"] for f in want], (what, b)
        allow = max(j["allowance"], 8 * ULP)
        errs = [abs(r[1] - float(f["rank"])) for r, f in zip(rows[b], want)] + [abs(r[2] - float(f["tot"])) for r, f in zip(rows[b], want)]
        worst = max([worst] + [e / allow for e in errs])
    print("rnnt-wbeam-parity %s: worst error / allowance %.3f over %d utterances, %d undecided" % (what, worst, len(utts), undecided))
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("g", WB.GRID, ids=[WB.grid_id(g) for g in WB.GRID])
def test_grid(hb, g):
    V, K, J, T, L, order, lexicon_only, eos_term, seed = g
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    out = TB._run(head, utts, K, L, **_wkw(wlm, eos_term=eos_term, lexicon_only=lexicon_only))
    assert len(out) == 6
    _compare("grid " + WB.grid_id(g), p, utts, K, L, out, wlm, lambda b: WB.grid_judge(g, b), head=head, eos_term=eos_term,
             lexicon_only=lexicon_only)
    empty = _rows(out)[1]                                            # the utterance without a frame: the empty hypothesis alone
    assert [r[0] for r in empty] == [()] and empty[0][2] == 0.0 and empty[0][4] == 0 and (eos_term or empty[0][3] == 0.0)


@pytest.mark.parametrize("gi", (2, 10))
def test_zero_weights_are_the_plain_search(hb, gi):
    """alpha = beta = 0, no end term, lexicon_only off: hyp, hyp_len and rnnt_score are the plain search's bits."""
    g = WB.GRID[gi]
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    plain = TB._run(head, utts, g[1], g[4])
    zero = TB._run(head, utts, g[1], g[4], **_wkw(wlm, 0.0, 0.0, eos_term=False))
    assert TB._bits(plain) == TB._bits([zero[0], zero[1], zero[3]])
    assert zero[2].tobytes() == zero[3].tobytes()
    _lm_bits(wlm, zero, False)


def test_lexicon_only(hb):
    """Every returned row consists of lexicon words; a lexicon that admits nothing the beam reaches leaves unused slots."""
    g = WB.GRID[9]
    p, utts, wlm = WB.grid_case(*g)
    out = TB._run(TB._head(p), utts, g[1], g[4], **_wkw(wlm, lexicon_only=True))
    rows = _rows(out)
    assert sum(len(r) for r in rows) > len(rows)
    assert all(w in wlm.lexicon.index for rr in rows for r in rr for w in WR.split(r[0], wlm.space))
    # K = 1, L = 1, a head that prefers label 1 to everything and the one word (1, 2): the beam is the sequence (1) from
    # the first iteration on; its node ends no word - it is no final, and nothing else is left
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_FIRST
    V = 5
    p = BR.tie_params(V, 4, 3)
    p["lin_out.bias"][1] = 6.0
    one = WordLM(NgramLM(1, W_FIRST + 1, W_BOS, W_EOS, {(W_EOS,): -1.0, (W_FIRST,): -1.0}, {}), Lexicon([(1, 2)], None, V - 1, V=V))
    utts = [np.ones((2, 16), np.float32), np.zeros((0, 16), np.float32), -np.ones((3, 16), np.float32)]
    for b, u in enumerate(utts):                                     # (two frames or more: with one, the empty sequence is a final)
        ref = WB.search(p, u, 1, 1, 1, one.compile(), lexicon_only=True)["finals"]
        assert [f["tokens"] for f in ref] == ([()] if b == 1 else [])
    hyp, hyp_len, score, tot, lm, nw = TB._run(TB._head(p), utts, 1, 1, **_wkw(one, lexicon_only=True))
    for b in (0, 2):
        assert hyp_len[b, 0] == -1 and nw[b, 0] == -1 and (hyp[b] == -1).all()
        assert np.isneginf(score[b, 0]) and np.isneginf(tot[b, 0]) and np.isneginf(lm[b, 0])
    assert hyp_len[1, 0] == 0 and nw[1, 0] == 0 and tot[1, 0] == 0.0


@pytest.mark.parametrize("K", (1, 2, 4, 16))
def test_tie_rule(hb, K):
    """lin_out zero: every candidate of one length ties; at zero weights the slot order is the plain search's."""
    V = 5
    p = BR.tie_params(V, 4, 3)
    wlm = WR.random_word_lm(V, 2, 5)
    utts = [np.ones((1, 16), np.float32), np.zeros((0, 16), np.float32), -np.ones((2, 16), np.float32)]
    rows = _rows(TB._run(TB._head(p), utts, K, 3, **_wkw(wlm, 0.0, 0.0, eos_term=False)))
    for b, enc_h in enumerate(utts):
        want = BR.search(p, enc_h, 1, K, 3)["finals"][:K]
        assert [r[0] for r in rows[b]] == [f["tokens"] for f in want], (K, b, rows[b])


def test_reproducible_and_independent(hb):
    g = WB.GRID[12]
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    kw = _wkw(wlm, eos_term=g[7], lexicon_only=g[6])
    first = TB._run(head, utts, g[1], g[4], **kw)
    assert TB._bits(first) == TB._bits(TB._run(head, utts, g[1], g[4], **kw))
    with hb.deterministic():
        assert TB._bits(first) == TB._bits(TB._run(head, utts, g[1], g[4], **kw))
    for b, u in enumerate(utts):                                     # a row alone: the bits it has inside the batch
        alone = TB._run(head, [u], g[1], g[4], **kw)
        for a, f in zip(alone, first):
            assert a[0].tobytes() == f[b].tobytes(), b


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_buffers(hb, pattern):
    """From an empty pool and from the poisoned leftover of a larger call in the same capacity class: the clean bits.  The
    extra workspace (node, word state, words) is part of the same lease: the init kernel or the step kernel writes every
    word of it that a kernel of the call reads, and what indexes the LM's tables is clamped."""
    import ops
    g = WB.GRID[12]
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    K, L = g[1], g[4]
    kw = _wkw(wlm, eos_term=g[7], lexicon_only=g[6])
    P.empty_pool()
    clean = TB._bits(TB._run(head, utts, K, L, **kw))
    for variant in ("empty pool", "leftover"):
        P.empty_pool()
        st = P.Stats()
        if variant == "leftover":
            TB._run(head, utts, K, L + 2, **kw)
            keys = [k for k in ops._POOL.free if k[0] == "rnnt_beam"]
            assert len(keys) == 1 and P.poison_pool(pattern, st) >= 1
        with P.poisoned(pattern, st):
            got = TB._bits(TB._run(head, utts, K, L, **kw))
        if variant == "leftover":
            assert [k for k in ops._POOL.free if k[0] == "rnnt_beam"] == keys      # (the same capacity class: the leftover was used)
        assert st.total > 0 and got == clean, (pattern, variant)
        print("rnnt-wbeam-poison %-5s %-10s %s; bit-identical" % (pattern, variant, st.line()))


def test_launches_per_iteration(hb):
    """The plain search's count, under keys of its own: 4 (T' + L) + 2 launches, T' + L of them the step kernel."""
    import ops
    g = WB.GRID[1]
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    K, L = g[1], g[4]
    x, ld = TB._batch(utts)
    with torch.no_grad():
        pe = head.project_enc(x)
        before = dict(hb.LAUNCHES)
        w_ih, w_hh, b_ih, b_hh = head.lstm.direction_params(0)
        out = ops.rnnt_beam(pe, ld, torch.cat([w_ih, w_hh], 1).contiguous(), (b_ih + b_hh).contiguous(), head.lin_pred.weight,
                            head.lin_out.weight, head.lin_out.bias, head.embedding.weight, 1, K, L, word_lm=wlm, word_lm_weight=0.5)
    assert len(out) == 6 and out[5].dtype == torch.int32
    T = x.shape[1]
    assert hb.LAUNCHES["rnnt_wbeam_launch"] - before.get("rnnt_wbeam_launch", 0) == 4 * (T + L) + 2
    assert hb.LAUNCHES["rnnt_wbeam_step"] - before.get("rnnt_wbeam_step", 0) == T + L
    assert hb.LAUNCHES["rnnt_beam_launch"] == before.get("rnnt_beam_launch", 0)


def test_refusals(hb):
    import ngram
    g = WB.GRID[1]
    p, utts, wlm = WB.grid_case(*g)
    head = TB._head(p)
    with pytest.raises(hb.UnsupportedShape):
        TB._run(head, utts, 2, 4, **_wkw(WR.random_word_lm(34, 2, 3)))       # a lexicon spelled in another vocabulary
    for K in (0, 17):
        with pytest.raises(hb.UnsupportedShape):
            TB._run(head, utts, K, 4, **_wkw(wlm))
    with pytest.raises(ValueError, match="two LMs"):
        TB._run(head, utts, 2, 4, ngram=ngram.NgramLM.estimate([[3, 4]], 2, 5, 1, 2), **_wkw(wlm))
    for weights in ((float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(RuntimeError):
            TB._run(head, utts, 2, 4, **_wkw(wlm, *weights))
    # through ctypes: the n-gram table and the word LM in one call
    x, lens = TB._batch(utts)
    B, K, L, V, J, E, Pd = len(utts), 2, 4, 5, g[2], 16, 16
    with torch.no_grad():
        pe = head.project_enc(x).contiguous()
    T = pe.shape[1]
    f = lambda *s: torch.zeros(*s, device=DEV)                       # noqa: E731
    h, c, xh, pp = f(B * K, Pd), f(B * K, Pd), f(B * K, E + Pd), f(B * K, J)
    ws, wws = f(hb.rnnt_beam_ws_bytes(B, T, J, V, K, L, E, Pd) // 4 + 1), f(hb.rnnt_wbeam_ws_bytes(B, K) // 4)
    run = hb.RnntWordBeam(pe, head.lin_out.weight.detach(), head.lin_out.bias.detach(), head.embedding.weight.detach(), lens, K, L,
                          h, c, xh, pp, ws, wlm.to(DEV), wws, 0.5, 0.0)
    run.args.lm_logp, run.args.lm_next, run.args.lm_states = hb.ptr(ws), hb.ptr(ws), 1
    with pytest.raises(RuntimeError):
        run.init(1)
    with pytest.raises(RuntimeError, match="extra workspace"):
        hb.RnntWordBeam(pe, head.lin_out.weight.detach(), head.lin_out.bias.detach(), head.embedding.weight.detach(), lens, K, L,
                        h, c, xh, pp, ws, wlm.to(DEV), wws[:8], 0.5, 0.0)


# ------------------------------------------------------------------------------------------------ model and solver
def test_recognize_rnnt_beams(hb):
    """E2E.recognize_rnnt_beams(word_lm=...) against the float64 search of the head's weights on the model's own encoder
    output; last_rnnt_beams carries the parts and n_words."""
    import synth
    net, xs, ilens = TB._tiny(rnnt_weight=0.3, rnnt_joint_dim=32)
    V, K, L = synth.TINY["output_dim"], 4, 6
    wlm = WR.random_word_lm(V, 2, 9)
    ids = net.recognize_rnnt_beams(xs, ilens, K, max_dec_timesteps=L, word_lm=wlm, word_lm_weight=0.6, word_bonus=0.3)
    last = net.last_rnnt_beams
    assert tuple(last["tokens"].shape) == (len(ilens), K, L) and set(last["parts"]) == {"rnnt", "lm"}
    assert tuple(last["n_words"].shape) == (len(ilens), K) and last["n_words"].dtype == torch.int32
    with torch.no_grad():
        enc_h, _ = net.encoder(xs, ilens)
    frames = net.encoder.enc2.last_lens_dev.cpu().tolist()
    p = {k: v.detach().cpu().numpy() for k, v in net.rnnt.state_dict().items()}
    utts = [enc_h[b, :frames[b]].cpu().numpy() for b in range(len(ilens))]
    out = [last[k].cpu().numpy() for k in ("tokens", "lengths", "scores")] + [last["parts"][k].cpu().numpy() for k in ("rnnt", "lm")] + \
        [last["n_words"].cpu().numpy()]
    table = wlm.compile()
    _compare("model", p, utts, K, L, out, wlm,
             lambda b: WB.judge(dict(p=p, enc_h=utts[b], bos=1, K=K, L=L, table=table, alpha=0.6, beta=0.3)), alpha=0.6, beta=0.3)
    assert ids == [list(r[0][0]) for r in _rows(out)]
    net.recognize_rnnt_beams(xs, ilens, 2, max_dec_timesteps=L)
    assert net.last_rnnt_beams["parts"] == {} and "n_words" not in net.last_rnnt_beams


def test_solver(hb, tmp_path, monkeypatch, capsys):
    """Solver.test with rnnt_beam_decode + rnnt_word_lm: the ARPA file's word LM sits inside the transducer search; without
    the key the launches are the plain search's."""
    import test_ctc_gpu as TC
    from dataloader import get_data_loader
    from word_lm import WordLM, W_UNK
    root = str(tmp_path / "s")
    solver, dev = TC._solver(root, monkeypatch, rnnt_weight=0.3, rnnt_joint_dim=32)
    state = {k: v.clone() for k, v in solver.model.state_dict().items()}
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    plain = sorted(i for s, i in solver.vocab.items() if not s.startswith("<"))
    solver.vocab = {(letters[plain.index(i)] if i in plain else s): i for s, i in solver.vocab.items()}     # one-character symbols
    vocab = solver.vocab
    special = {vocab["<PAD>"], vocab["<BOS>"], vocab["<EOS>"], vocab["<NOISE>"]}
    sym = {i: s for s, i in vocab.items()}
    loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    text = [[int(c) for c in y if int(c) not in special] for batch in solver._feed(loader, sharded=False) for y in batch.ys_host]
    lm = WordLM.estimate(text, vocab["<space>"], 3, V=len(vocab), bos=vocab["<BOS>"], eos=vocab["<EOS>"])
    names = {wid: "".join(sym[c] for c in sp) for sp, wid in zip(lm.lexicon.spellings, lm.word_ids)}
    names[W_UNK] = "<unk>"
    arpa = os.path.join(root, "words.arpa")
    with open(arpa, "w") as f:
        f.write(lm.lm.to_arpa(names))
    cfg = dict(solver.config, rnnt_beam_decode=True, beam_size=4, cer_on_gpu=True, max_dec_timesteps=12)

    def run(**extra):
        solver.config = dict(cfg, **extra)
        before = dict(hb.LAUNCHES)
        cer = solver.test(state_dict=state)
        return cer, {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
    cer, n_plain = run()
    assert not any(k.startswith(("rnnt_wbeam", "word_lm")) for k in n_plain)
    calls = n_plain["rnnt_beam_launch"] - 4 * n_plain["rnnt_beam_step"]
    assert calls % 2 == 0 and calls >= 2                            # 4 (T' + L) + 2 per utterance: what the search launched before
    plain_scores = solver.model.last_rnnt_beams["scores"].clone()
    assert solver.model.last_rnnt_beams["parts"] == {}
    capsys.readouterr()
    cer, n = run(rnnt_word_lm=dict(arpa=arpa, weight=0.8, bonus=0.5))
    text_out = capsys.readouterr().out
    last = solver.model.last_rnnt_beams
    assert np.isfinite(cer) and "best of 4 hypotheses: CER=" in text_out and solver.last_test["best_of_k_cer"] <= cer
    assert set(last["parts"]) == {"rnnt", "lm"} and not torch.equal(last["scores"], plain_scores)
    assert n["rnnt_wbeam_launch"] == n_plain["rnnt_beam_launch"] and n["rnnt_wbeam_step"] == n_plain["rnnt_beam_step"]
    assert "rnnt_beam_launch" not in n
    used = last["lengths"] >= 0
    want = (last["parts"]["rnnt"][used] + last["parts"]["lm"][used] * 0.8) + last["n_words"][used].float() * 0.5
    assert torch.equal(last["scores"][used], want)
    lex = os.path.join(root, "lexicon.txt")
    with open(lex, "w") as f:
        f.write("\n".join(sorted(names[w] for w in lm.word_ids)[:3]) + "\n")
    cer, _ = run(rnnt_word_lm=dict(arpa=arpa, lexicon=lex, weight=0.8, lexicon_only=True))
    assert np.isfinite(cer)
    for extra, msg in ((dict(rnnt_beam_decode=False, rnnt_greedy_decode=True, beam_size=1, rnnt_word_lm=dict(arpa=arpa)), "set rnnt_beam_decode"),
                       (dict(rnnt_word_lm=dict(arpa=arpa), ngram_lm=arpa), "two LMs for one search"),
                       (dict(rnnt_word_lm=dict(arpa=arpa, wieght=1.0)), "rnnt_word_lm is a dictionary"),
                       (dict(word_lm=arpa), "does not combine with word_lm")):
        with pytest.raises(ValueError, match=msg):
            run(**extra)
    solver.vocab = {("<blank>" if s == "<space>" else s): i for s, i in vocab.items()}
    with pytest.raises(ValueError, match="needs <space> in the vocabulary"):
        run(rnnt_word_lm=dict(arpa=arpa))
