"""The attention beam search with an n-gram or word-level LM inside, on the GPU (csrc/beam.hip's select kernel with its KIND and
the asr_beam_*_tlm entries): the select alone against a stable sort in float32, bit for bit; the search against
the float64 restatement (tests/beam_ngram_ref.py); zero weights against the search without the LM; the parts against the
scorers; lexicon_only; launches and memory; the untouched plain entries; poisoned buffers; refusals, the model and the solver.
Every case prints one `beam-ngram-parity` line."""
import os

import numpy as np
import pytest
import torch

import beam_ngram_ref as R
import ngram_ref as NR
import poison as P
import test_beam_gpu as tb
import test_beam_lm_gpu as tl
import word_lm_ref as WR

pytestmark = pytest.mark.gpu
F = np.float32
EOS = R.EOS
FCAP = 48


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32).tolist()


# ------------------------------------------------------------------ 1. the select alone, exact
def _round64(n):
    return (n + 63) // 64 * 64


class _Ws:
    """The extra workspace as the entries lay it out: a | b | n | lm over round64(B K) words each, then fin_base | fin_lm |
    fin_n over round64(B FCAP)."""

    def __init__(self, hb, B, K):
        self.t = torch.full((hb.beam_tlm_ws_bytes(B, K) // 4,), 0x7fc00000, dtype=torch.int32, device="cuda")     # NaN / junk
        r, f = _round64(B * K), _round64(B * FCAP)
        cut = lambda i, n, shape: self.t[i:i + n].view(*shape)                                    # noqa: E731
        self.a, self.b, self.n = (cut(i * r, B * K, (B, K)) for i in range(3))
        self.lm = cut(3 * r, B * K, (B, K)).view(torch.float32)
        self.fin_base, self.fin_lm = (cut(4 * r + i * f, B * FCAP, (B, FCAP)).view(torch.float32) for i in range(2))
        self.fin_n = cut(4 * r + 2 * f, B * FCAP, (B, FCAP))


def _select_tables(V, seed):
    """A 7-state n-gram automaton over V tokens, and a 6-word lexicon (one word a prefix of another) with a bigram word LM."""
    from ngram import NgramLM, NgramTable
    from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_UNK, W_FIRST
    rs = np.random.RandomState(seed)
    logp = (-rs.rand(7, V) * 5).astype(F)
    logp[:, 0] = 0
    ngram = NgramTable(logp, rs.randint(0, 7, size=(7, V)).astype(np.int32), 3, 1, EOS, 3)
    space = V - 1
    letters = list(range(3, space))
    a, b = letters[0], letters[-1]
    words = [(a,), (a, a), (a, b, a), (b,), (b, b, a, a), (b, a)] if len(letters) > 1 else [(a,) * n for n in range(1, 7)]
    lex = Lexicon(words, None, space, bos=1, eos=EOS, V=V)
    ids = [W_EOS, W_UNK] + [W_FIRST + i for i in range(6) if i != 1]                      # word 1 has no unigram
    prob = {(w,): float(rs.uniform(-6, -0.5)) for w in ids}
    backoff = {}
    for h in [W_BOS] + ids[1:]:
        for w in rs.choice(ids, 3, replace=False):
            prob[(h, int(w))] = float(rs.uniform(-5, -0.1))
        backoff[(h,)] = float(rs.uniform(-2, 0))
    wlm = WordLM(NgramLM(2, W_FIRST + 6, W_BOS, W_EOS, prob, backoff), lex)
    return ngram, wlm.compile()


def _row_stats(hb, rows):
    """(max, log(sum exp(x - max))) of every row AS THE DEVICE FORMS THEM: the plain select over one-beam utterances at score
    0 ranks (x - max) - lsum, whose greatest value is -lsum exactly."""
    n, V = rows.shape
    s = hb.BeamSearch(n, 1, V, 2, EOS, "cuda")
    s.select(_cuda(rows), 0)
    torch.cuda.synchronize()
    top = torch.where(s.nfin > 0, s.fin_score[:, 0], s.scores[:, 0]).cpu().numpy()
    return np.stack([rows.max(axis=1), -top], axis=1).astype(F)


def _select_inputs(K, V, kind, table, seed):
    rs = np.random.RandomState(seed)
    B = 3
    logits = (rs.randn(B, K, V) * 3).astype(F)
    lm_logits = (rs.randn(B, K, V) * 2).astype(F)
    psi = (-rs.rand(B, K, V) * 6).astype(F)
    psi[:, :, 0] = -np.inf                                                   # the blank is no candidate
    psi_prev = (-rs.rand(B, K) * 6).astype(F)
    scores = (-rs.rand(B, K) * 4).astype(F)
    logits[0, 0, EOS] = logits[0, 0].max() + 6.0                             # an <EOS> at rank < K ...
    if K > 1:
        logits[0, K - 1, EOS] = logits[0, K - 1].max() + 0.25                # ... and one further down
        logits[2, 1] = logits[2, 0]                                          # two equal beams: ties by the flat index
        lm_logits[2, 1], psi[2, 1], psi_prev[2, 1], scores[2, 1] = lm_logits[2, 0], psi[2, 0], psi_prev[2, 0], scores[2, 0]
        scores[0, K // 2] = -np.inf                                          # a row at -inf
    if K > 2:
        scores[2, 2:] = -np.inf                                              # fewer than 2K finite candidates at V = 5
    if V > 4:
        logits[:, :, 4] = logits[:, :, 3]
    pos = []
    for b in range(B):
        row = []
        for k in range(K):
            lm = F(-rs.rand() * 9)
            if kind == R.NGRAM:
                row.append((int(rs.randint(7)), lm, int(rs.randint(0, 9))))
            else:
                node = [0, -1, 1, int(rs.randint(table.N)), int(rs.randint(table.N))][(b + k) % 5]       # the root, off the trie, nodes
                row.append((node, int(rs.randint(table.S)), lm, int(rs.randint(0, 5))))
        pos.append(row)
    if K > 1:
        pos[2][1] = pos[2][0]
    return logits, lm_logits, psi, psi_prev, scores, pos


SELECT_GRID = [(K, V, kind, lex) for K in (1, 3, 16) for V in (5, 34, 300)
               for kind, lex in ((R.NGRAM, False), (R.WORD, False), (R.WORD, True))]


@pytest.mark.parametrize("K,V,kind,lexicon_only", SELECT_GRID,
                         ids=["K%d-V%d-%s%s" % (k, v, kind, "-lex" if lex else "") for k, v, kind, lex in SELECT_GRID])
def test_select_against_a_stable_sort_bit_for_bit(hb, K, V, kind, lexicon_only):
    ngram, wtable = _select_tables(V, 11 * K + V)
    table = ngram if kind == R.NGRAM else wtable
    weight, bonus = 0.37, 0.21
    lm = R.tlm(kind, table, weight, bonus, lexicon_only)
    logits, lm_logits, psi, psi_prev, scores, pos = _select_inputs(K, V, kind, table, 100 * K + V)
    B, L, lmw, cw = 3, 6, 0.45, 0.3
    stats = _row_stats(hb, logits.reshape(B * K, V)).reshape(B, K, 2)
    lm_stats = _row_stats(hb, lm_logits.reshape(B * K, V)).reshape(B, K, 2)
    dev_table = table.to("cuda")
    checked = 0
    for variant in ("plain", "LM", "CTC", "both"):
        for last in (False, True):
            t = L - 1 if last else 2
            s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
            s.scores.copy_(_cuda(scores))
            s.done[1] = 1                                                    # one utterance is done already
            s.ndone[0] = 1
            s.nfin[0] = 1                                                    # and one holds a finished hypothesis
            ws = _Ws(hb, B, K)
            for b in range(B):
                for k in range(K):
                    p = pos[b][k]
                    ws.a[b, k], ws.n[b, k], ws.lm[b, k] = p[0], p[-1], float(p[-2])
                    if kind == R.WORD:
                        ws.b[b, k] = p[1]
            x = hb.BeamTableLm(s, ws.t, ngram=dev_table if kind == R.NGRAM else None,
                               word_lm=dev_table if kind == R.WORD else None, weight=weight, bonus=bonus, lexicon_only=lexicon_only)
            before = [v.clone() for v in (s.scores, s.tok_hist, s.bp_hist, s.fin, s.fin_score, ws.t)]
            use_lm, use_ctc = variant in ("LM", "both"), variant in ("CTC", "both")

            class Ctc:
                pass
            ctc = Ctc()
            ctc.psi, ctc.psi_prev = _cuda(psi.reshape(B * K, V)), _cuda(psi_prev.reshape(B * K))
            x.select(_cuda(logits.reshape(B * K, V)), t, _cuda(lm_logits.reshape(B * K, V)) if use_lm else None, lmw,
                     ctc if use_ctc else None, cw)
            torch.cuda.synchronize()
            ndone = 1
            for b in (0, 2):
                ref = R.select_f32(scores[b], logits[b], stats[b], EOS, lm, pos[b], t, L, 1 if b == 0 else 0,
                                   lm_logits[b] if use_lm else None, lm_stats[b], lmw, psi[b] if use_ctc else None,
                                   psi_prev[b], cw if use_ctc else 0.0)
                what = (K, V, kind, lexicon_only, variant, last, b)
                n = ref["nlive"]
                assert s.tok_hist[t, b].tolist() == ref["tok"].tolist(), what
                assert s.bp_hist[t, b].tolist() == ref["bp"].tolist(), what
                assert _bits(s.scores[b].cpu().numpy()) == _bits(ref["scores"]), what
                for j in range(n):
                    p = ref["pos"][j]
                    assert int(ws.a[b, j]) == p[0] and int(ws.n[b, j]) == p[-1], what
                    assert _bits(ws.lm[b, j].item()) == _bits(p[-2]), what
                    if kind == R.WORD:
                        assert int(ws.b[b, j]) == p[1], what
                first = 1 if b == 0 else 0
                nf = int(s.nfin[b])
                assert nf == first + len(ref["fin"]), (what, nf, ref["fin"])
                for i, f in enumerate(ref["fin"]):
                    at = first + i
                    assert tuple(s.fin[b, at].tolist()) == f[:4], what
                    assert _bits(s.fin_score[b, at].item()) == _bits(f[4]), what
                    assert _bits(ws.fin_base[b, at].item()) == _bits(f[5]) and _bits(ws.fin_lm[b, at].item()) == _bits(f[6]), what
                    assert int(ws.fin_n[b, at]) == f[7], what
                assert int(s.done[b]) == int(ref["done"]), what
                ndone += int(ref["done"])
                checked += 1
            assert int(s.ndone[0]) == ndone
            for was, now in zip(before, (s.scores, s.tok_hist, s.bp_hist, s.fin, s.fin_score)):     # the done utterance: untouched
                was, now = (v.view(torch.int32) for v in (was, now))                                # (bits: the buffers start undefined)
                assert torch.equal(was[1] if was.dim() < 3 or was.shape[0] == B else was[:, 1],
                                   now[1] if now.dim() < 3 or now.shape[0] == B else now[:, 1])
    print("beam-ngram-parity select K%d V%d %s%s: %d utterance-steps, worst error 0 ulp / allowance 0; left out 0"
          % (K, V, kind, " lexicon_only" if lexicon_only else "", checked))


# ------------------------------------------------------------------ the search on a decoder
_NETS = {}


def _case(key):
    """The modules and inputs of a grid case on the GPU (built once per case)."""
    if key not in _NETS:
        c = R.grid_case(*key)
        net, judge = tl._e2e_module(c["cfg"], c["w"]), tl._lm_module(c["lm_cfg"], c["lm_w"])
        enc = _cuda(c["enc"])
        cw, cb = (_cuda(a) for a in c["ctc"])
        ctc_logits = (enc.reshape(-1, enc.shape[2]) @ cw.t() + cb).view(enc.shape[0], enc.shape[1], -1).contiguous()
        _NETS[key] = (net, judge, enc, c["lens"], ctc_logits, torch.tensor(c["lens"], dtype=torch.int32).cuda(), c["lm"])
    return _NETS[key]


def _lm_kw(kind, lm, weight, bonus, lexicon_only=False):
    if kind == R.NGRAM:
        return dict(ngram=lm, ngram_weight=weight, ngram_bonus=bonus)
    return dict(word_lm=lm, word_lm_weight=weight, word_bonus=bonus, lexicon_only=lexicon_only)


def _variant_kw(key, judge, ctc_logits, ctc_lens):
    if key[1] == "judge":
        return dict(lm=judge, lm_weight=R.JUDGE_WEIGHT)
    if key[1] == "ctc":
        return dict(ctc_logits=ctc_logits, ctc_lens=ctc_lens, ctc_decode_weight=R.CTC_WEIGHT)
    return {}


def _run(key, weight=None, bonus=None, with_lm=True, lexicon_only=False, L=R.L):
    net, judge, enc, lens, ctc_logits, ctc_lens, lm = _case(key)
    w, b = R.WEIGHTS[key[0]]
    kw = _variant_kw(key, judge, ctc_logits, ctc_lens)
    if with_lm:
        kw.update(_lm_kw(key[0], lm, w if weight is None else weight, b if bonus is None else bonus, lexicon_only))
    toks, scores = net.decoder.recognize_beams(enc, lens, L, key[2], nbest=True, **kw)
    return toks, scores, net.decoder.last_beams


def _record_bits(toks, scores, last):
    out = [toks.cpu().numpy().tobytes(), scores.cpu().numpy().tobytes()]
    if last is not None:
        out += [last[k].cpu().numpy().tobytes() for k in ("lengths", "n_words")]
        out += [last["parts"][k].cpu().numpy().tobytes() for k in ("att", "lm")]
    return out


GRID_IDS = ["%s-%s-K%d" % g for g in R.grid()]


def _check_search(hb, key):
    toks, scores, last = _run(key)
    ref = R.judge(key)
    w, beta = R.WEIGHTS[key[0]]
    worst, left_out = 0.0, 0
    for b, r in enumerate(ref):
        if not R.decided(r):
            left_out += 1
            continue
        n = len(r["hyps"])
        got = [tb._cut(toks[b, k].tolist()) for k in range(n)]
        assert got == [tb._cut(h[0]) for h in r["hyps"]], (key, b, got, r["hyps"])
        assert last["lengths"][b, :n].tolist() == [h[2] for h in r["hyps"]]
        assert np.isneginf(scores[b, n:].cpu().numpy()).all()
        for name, got_v, want in (("score", scores[b, :n], [h[1] for h in r["hyps"]]),
                                  ("att", last["parts"]["att"][b, :n], [p[0] for p in r["parts"]]),
                                  ("lm", last["parts"]["lm"][b, :n], [float(p[1]) for p in r["parts"]])):
            got_v, want = got_v.cpu().numpy().astype(np.float64), np.array(want)
            worst = max(worst, float(np.max(np.abs(got_v - want) / np.abs(want))))
            np.testing.assert_allclose(got_v, want, rtol=1e-4, err_msg="%s %s" % (key, name))      # tests/test_beam_lm_gpu.py's gate
        assert last["n_words"][b, :n].tolist() == [p[2] for p in r["parts"]]
    return worst, left_out


@pytest.mark.parametrize("key", R.grid(), ids=GRID_IDS)
def test_search_against_the_float64_restatement(hb, key):
    worst, left_out = _check_search(hb, key)
    print("beam-ngram-parity search %s-%s-K%d: worst relative error %.2e / allowance 1e-4; left out %d of %d utterances"
          % (key + (worst, left_out, len(R.LENS))))


@pytest.mark.parametrize("key", R.grid(), ids=GRID_IDS)
def test_zero_weights_are_the_search_without_the_lm(hb, key):
    toks, scores, last = _run(key, 0.0, 0.0)
    toks0, scores0, none = _run(key, with_lm=False)
    assert none is None and last is not None
    assert torch.equal(toks, toks0) and _bits(scores.cpu().numpy()) == _bits(scores0.cpu().numpy())
    assert torch.equal(last["parts"]["att"], scores0)                       # rank == base at zero weights
    net, judge, enc, lens, ctc_logits, ctc_lens, lm = _case(key)
    best, best_score = net.decoder.recognize_beams(enc, lens, R.L, key[2], **_variant_kw(key, judge, ctc_logits, ctc_lens))
    assert torch.equal(best, toks[:, 0]) and torch.equal(best_score, scores[:, 0])
    print("beam-ngram-parity zero %s-%s-K%d: tokens, scores, lengths bit-identical; left out 0" % key)


def _check_parts(key, toks, scores, last, weight, bonus):
    net, _, _, _, _, _, lm = _case(key)

    class Shim:                                                              # E2E's scorers read .decoder and parameters()
        decoder = net.decoder
        parameters = net.parameters
    import model as M
    used = last["lengths"] > 0
    if key[0] == R.NGRAM:
        want = M.E2E.ngram_score(Shim, lm, toks)
        is_eos = toks == EOS
        count = torch.where(is_eos.any(-1), is_eos.int().argmax(-1), torch.full_like(toks[..., 0], toks.shape[-1])).int()
    else:
        want, count = M.E2E.word_lm_score(Shim, lm, toks)
    assert used.any()
    assert torch.equal(last["parts"]["lm"][used].view(torch.int32), want[used].view(torch.int32)), key
    assert torch.equal(last["n_words"][used], count[used].int()), key
    rank = (last["parts"]["att"] + torch.tensor(weight, dtype=torch.float32) * last["parts"]["lm"]) + \
        torch.tensor(bonus, dtype=torch.float32) * last["n_words"].float()
    assert torch.equal(scores[used].view(torch.int32), rank[used].view(torch.int32)), key
    assert (last["n_words"][~used] == -1).all() and torch.isneginf(scores[~used]).all()
    return int(used.sum())


@pytest.mark.parametrize("key", R.grid(), ids=GRID_IDS)
def test_parts_are_the_scorers_bit_for_bit(hb, key):
    toks, scores, last = _run(key)
    n = _check_parts(key, toks, scores, last, *R.WEIGHTS[key[0]])
    print("beam-ngram-parity parts %s-%s-K%d: %d hypotheses, lm_score / n_words / rank 0 ulp / allowance 0; left out 0" % (key + (n,)))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_lexicon_only(hb, variant):
    key = (R.WORD, variant, 4)
    toks, scores, last = _run(key, lexicon_only=True)
    table = _case(key)[6].compile()
    used = (last["lengths"] > 0).cpu().numpy()
    assert used.any()
    for b in range(toks.shape[0]):
        for k in range(toks.shape[1]):
            if used[b, k]:
                assert R.words_in_lexicon(table, [c for c in tb._cut(toks[b, k].tolist()) if c != EOS]), (b, k, toks[b, k])
    _check_parts(key, toks, scores, last, *R.WEIGHTS[R.WORD])
    # a lexicon the audio cannot satisfy: its only word is one letter, and the decoder never gives that letter, a <space> (at
    # the root it would be no word either) or the empty sentence - every candidate of step 0 ranks -inf
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM, W_BOS, W_EOS, W_UNK, W_FIRST
    net, judge, enc, lens, ctc_logits, ctc_lens, _ = _case(key)
    one = WordLM(NgramLM(1, W_FIRST + 1, W_BOS, W_EOS, {(W_EOS,): -1.0, (W_UNK,): -2.0, (W_FIRST,): -1.0}, {}),
                 Lexicon([(3,)], None, R.SPACE, bos=R.BOS, eos=EOS, V=R.V))
    bias = net.decoder.output_layer.bias.data
    keep = bias.clone()
    bias[[3, EOS, R.SPACE]] = float("-inf")
    try:
        toks, scores = net.decoder.recognize_beams(enc, lens, R.L, 4, nbest=True, word_lm=one, word_lm_weight=0.5,
                                                   lexicon_only=True, **_variant_kw(key, judge, ctc_logits, ctc_lens))
        last = net.decoder.last_beams
    finally:
        bias.copy_(keep)
    torch.cuda.synchronize()
    finite = np.isfinite(scores.cpu().numpy())
    assert not finite.any() and (last["lengths"] == 0).all() and (toks == EOS).all() and (last["n_words"] == -1).all()
    assert torch.isneginf(last["parts"]["att"]).all() and torch.isneginf(last["parts"]["lm"]).all()
    print("beam-ngram-parity lexicon_only %s: lexicon words only; unsatisfiable lexicon: %d of %d ranks empty at -inf, no fault; left out 0"
          % (variant, int((~finite).sum()), finite.size))


def test_launches_and_memory(hb):
    key = (R.NGRAM, "alone", 4)
    net, judge, enc, lens, _, _, lm = _case(key)
    counts = []
    for kw in ({}, _lm_kw(R.NGRAM, lm, 0.4, 0.3), _lm_kw(R.WORD, _case((R.WORD, "alone", 4))[6], 0.4, 0.3)):
        hb.LAUNCHES.clear()
        net.decoder.recognize_beams(enc, lens, R.L, 4, **kw)
        counts.append((hb.LAUNCHES["beam_launch"], hb.LAUNCHES["beam_step"]))
        assert counts[-1][1] > 0 and counts[-1][0] <= 7 * counts[-1][1]
    assert all(c[0] == 7 * c[1] - 1 or c[0] == 7 * c[1] for c in counts)                 # 7 per step, none behind the last select
    hb.LAUNCHES.clear()
    net.decoder.recognize_beams(enc, lens, R.L, 4, lm=judge, lm_weight=0.3, **_lm_kw(R.NGRAM, lm, 0.4, 0.3))
    with_lm = (hb.LAUNCHES["beam_lm_launch"], hb.LAUNCHES["beam_lm_step"])
    hb.LAUNCHES.clear()
    net.decoder.recognize_beams(enc, lens, R.L, 4, lm=judge, lm_weight=0.3)
    plain = (hb.LAUNCHES["beam_lm_launch"], hb.LAUNCHES["beam_lm_step"])
    assert with_lm[1] > 0 and with_lm[0] * plain[1] == plain[0] * with_lm[1] or with_lm[0] - 9 * with_lm[1] == plain[0] - 9 * plain[1]
    # memory does not depend on max_dec_timesteps, the history apart
    net2 = tb._decoder_net(320, 34, 128, 41, eos_bias=-30.0)                 # no <EOS>: every step runs
    enc2, lens2 = tb._enc(2, 20, 128, (20, 14), 9)
    peaks = []
    for L in (20, 200):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pred, _ = net2.decoder.recognize_beams(enc2, lens2, L, 4, **_lm_kw(R.NGRAM, lm, 0.4, 0.3))
        torch.cuda.synchronize()
        history = 2 * 4 * L * 2 * 4 + 2 * 4 * L * 12                          # tok_hist, bp_hist; the returned tokens (int32, int64)
        peaks.append(torch.cuda.max_memory_allocated() - base - history)
        del pred
    assert abs(peaks[1] - peaks[0]) < 2 ** 20, peaks
    print("beam-ngram-parity launches: %s launches / steps plain, n-gram, word LM; peak apart from the history %s bytes at L = 20, 200; "
          "left out 0" % (counts, peaks))


def test_plain_entries_are_untouched(hb, golden_dir):
    """The existing select / backtrack entries on one fixed case: the outputs recorded from the parent build."""
    g = np.load(os.path.join(golden_dir, "beam_plain_select.npz"))
    B, K, V, L = 3, 4, 34, 6
    logits, scores = tb._select_case(K, V, EOS, 77)
    assert np.array_equal(g["logits"], logits) and _bits(g["scores_in"]) == _bits(scores)
    for name, t in (("mid", 3), ("last", L - 1)):
        s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
        s.scores.copy_(_cuda(scores))
        s.tok_hist.zero_()
        s.bp_hist.zero_()
        for step in range(t):                                                # a history for the backtrack to follow
            s.tok_hist[step] = 3 + step
        s.select(_cuda(logits.reshape(B * K, V)), t)
        toks, sc, lens = s.backtrack(0.5)
        torch.cuda.synchronize()
        nf = s.nfin.cpu().numpy()
        assert np.array_equal(g[name + "_tok"], s.tok_hist[t].cpu().numpy()) and np.array_equal(g[name + "_bp"], s.bp_hist[t].cpu().numpy())
        assert _bits(g[name + "_scores"]) == _bits(s.scores.cpu().numpy()) and np.array_equal(g[name + "_nfin"], nf)
        for b in range(B):
            assert np.array_equal(g[name + "_fin"][b, :nf[b]], s.fin[b, :nf[b]].cpu().numpy())
            assert _bits(g[name + "_fin_score"][b, :nf[b]]) == _bits(s.fin_score[b, :nf[b]].cpu().numpy())
        assert np.array_equal(g[name + "_out_tok"], toks.cpu().numpy()) and _bits(g[name + "_out_score"]) == _bits(sc.cpu().numpy())
        assert np.array_equal(g[name + "_out_len"], lens.cpu().numpy())
    print("beam-ngram-parity plain entries: select and backtrack outputs equal the parent build's record, 0 ulp; left out 0")


def test_select_variants_keep_their_bits(hb, golden_dir):
    """The candidate expressions that beam_plain_select.npz does not cover - the judge, the CTC prefix score, both, and the
    plain select at the longest list (K = 4 and 16: M = 8 and 32), at t = 3 and t = L - 1 - against the outputs recorded from
    the build before the select kernels were folded into one (tests/golden/make_beam_select_golden.py), 0 ulp.  The inputs'
    checksums are part of the record: a generator that drifts fails here and not as a difference of the outputs."""
    import make_beam_select_golden as G
    g = np.load(os.path.join(golden_dir, "beam_select_variants.npz"))
    rec = G.record(hb)
    assert sorted(rec) == sorted(g.files)
    inputs = [k for k in rec if k.startswith("in_")]
    assert len(inputs) == 10 and all(int(rec[k]) == int(g[k]) for k in inputs), "the inputs are not the recorded ones"
    bad = [k for k in rec if k not in inputs and not (rec[k].dtype == g[k].dtype and rec[k].shape == g[k].shape
                                                       and np.array_equal(G.bits(rec[k]), G.bits(g[k])))]
    assert not bad, bad
    assert len(rec) - len(inputs) == 9 * 2 * len(G.CASES) and all(int(g[k].max()) > 0 for k in g.files if k.endswith("_nfin"))
    print("beam-ngram-parity select variants: %d cases x 2 steps, %d arrays equal the record of the build before the fold, 0 ulp; "
          "left out 0" % (len(G.CASES), len(rec) - len(inputs)))


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_buffers(hb, pattern):
    """The searches of cases 2 to 4 with every torch.empty of the call poisoned - the beam state, the extra workspace (the
    positions, the finished parts), the outputs: the clean bits."""
    n = 0
    for key in [(R.NGRAM, "alone", 4), (R.NGRAM, "judge", 1), (R.WORD, "ctc", 4), (R.WORD, "alone", 1)]:
        for weights in ((None, None), (0.0, 0.0)):
            P.empty_pool()
            clean = _record_bits(*_run(key, *weights))
            P.empty_pool()
            st = P.Stats()
            with P.poisoned(pattern, st):
                toks, scores, last = _run(key, *weights)
                got = _record_bits(toks, scores, last)
            assert st.total > 0 and got == clean, (pattern, key, weights)
            if weights[0] is None:
                _check_parts(key, toks, scores, last, *R.WEIGHTS[key[0]])
            n += 1
    print("beam-ngram-parity poison %-5s: %d searches bit-identical to the clean run; left out 0" % (pattern, n))


# ------------------------------------------------------------------ 9. refusals, the model, the solver
def test_refusals(hb):
    import ngram
    key = (R.NGRAM, "alone", 4)
    net, judge, enc, lens, _, _, lm = _case(key)
    wlm = _case((R.WORD, "alone", 4))[6]
    with pytest.raises(ValueError, match="two LMs"):
        net.decoder.recognize_beams(enc, lens, R.L, 4, ngram=lm, word_lm=wlm)
    with pytest.raises(ValueError, match="predicts 5 tokens"):
        net.decoder.recognize_beams(enc, lens, R.L, 4, ngram=ngram.NgramLM.estimate([[3, 4]], 2, 5, 1, 2))
    with pytest.raises(ValueError, match="spells in"):
        net.decoder.recognize_beams(enc, lens, R.L, 4, word_lm=WR.random_word_lm(20, 2, 3))
    B, K, V, L = 2, 4, R.V, 6
    s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
    ws = torch.zeros(hb.beam_tlm_ws_bytes(B, K) // 4, dtype=torch.int32, device="cuda")
    table, wtable = lm.to("cuda"), wlm.to("cuda")
    logits = torch.zeros(B * K, V, device="cuda")
    with pytest.raises(RuntimeError, match="extra workspace"):
        hb.BeamTableLm(s, ws[:16], ngram=table)
    with pytest.raises(ValueError):
        hb.BeamTableLm(s, ws, ngram=table, word_lm=wtable)
    with pytest.raises(hb.UnsupportedShape):
        hb.BeamTableLm(hb.BeamSearch(B, K, 20, L, EOS, "cuda"), ws, word_lm=wtable)
    for weights in ((float("nan"), 0.0), (0.0, float("inf"))):               # ASR_E_ARG before any launch
        x = hb.BeamTableLm(s, ws, ngram=table, weight=weights[0], bonus=weights[1])
        for call in (x.init, lambda: x.select(logits, 0), x.backtrack):
            with pytest.raises(RuntimeError, match="code -1"):
                call()
    x = hb.BeamTableLm(s, ws, ngram=table, weight=0.5)
    x.init()
    for t in (-1, L):
        with pytest.raises(RuntimeError, match="code -1"):
            x.select(logits, t)
    x.struct.kind = 3
    with pytest.raises(RuntimeError, match="code -1"):
        x.init()
    x.struct.kind = hb.BEAM_TLM_NGRAM
    x.struct.lm_start = x.struct.lm_states                                   # ASR_E_SHAPE
    with pytest.raises(hb.UnsupportedShape):
        x.select(logits, 0)
    x.struct.lm_start = 0
    x.struct.ws_bytes = 64
    with pytest.raises(RuntimeError, match="code -1"):
        x.select(logits, 0)
    y = hb.BeamTableLm(s, ws, word_lm=wtable)
    y._word.V = V + 1                                                        # a word LM over another vocabulary: ASR_E_SHAPE
    with pytest.raises(hb.UnsupportedShape):
        y.init()
    y._word.V = V
    y._word.trie_next = None
    with pytest.raises(RuntimeError, match="code -1"):
        y.init()
    torch.cuda.synchronize()
    assert int(s.ndone[0]) == 0 and int(s.nfin.sum()) == 0                   # nothing was launched on the refused calls


def test_e2e_keeps_the_record(hb):
    import synth
    import model as M
    cfg = dict(synth.TINY)
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
    net.eval()
    xs, ilens, _ = synth.batch(cfg["input_dim"], cfg["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    V, K, L = cfg["output_dim"], 3, 6
    lm = NR.random_lm(V, 2, 5)
    assert (lm.bos, lm.eos) == (net.decoder.bos, net.decoder.eos)
    toks, scores = net.recognize_beams(torch.from_numpy(xs).cuda(), ilens, L, K, nbest=True, ngram=lm, ngram_weight=0.5, ngram_bonus=0.2)
    last = net.last_beams
    assert set(last) == {"tokens", "lengths", "scores", "parts", "n_words"} and set(last["parts"]) == {"att", "lm"}
    assert torch.equal(last["tokens"].long(), toks) and torch.equal(last["scores"], scores)
    used = last["lengths"] > 0
    assert torch.equal(net.ngram_score(lm, toks)[used].view(torch.int32), last["parts"]["lm"][used].view(torch.int32))
    net.recognize_beams(torch.from_numpy(xs).cuda(), ilens, L, K)
    assert net.last_beams is None


def test_solver(hb, tmp_path, monkeypatch, capsys):
    """Solver.test with att_ngram_lm and with att_word_lm on the synthetic corpus: CER reported, the hypotheses those of
    E2E.recognize_beams called directly."""
    import test_ctc_gpu as TC
    from dataloader import get_data_loader
    from ngram import NgramLM
    from word_lm import WordLM, W_UNK
    root = str(tmp_path / "s")
    solver, dev = TC._solver(root, monkeypatch)
    state = {k: v.clone() for k, v in solver.model.state_dict().items()}
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    plain = sorted(i for s, i in solver.vocab.items() if not s.startswith("<"))
    solver.vocab = {(letters[plain.index(i)] if i in plain else s): i for s, i in solver.vocab.items()}     # one-character symbols
    vocab = solver.vocab
    special = {vocab["<PAD>"], vocab["<BOS>"], vocab["<EOS>"], vocab["<NOISE>"]}
    sym = {i: s for s, i in vocab.items()}
    loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    text = [[int(c) for c in y if int(c) not in special] for batch in solver._feed(loader, sharded=False) for y in batch.ys_host]
    V, bos, eos = len(vocab), vocab["<BOS>"], vocab["<EOS>"]
    wlm = WordLM.estimate(text, vocab["<space>"], 2, V=V, bos=bos, eos=eos)
    names = {wid: "".join(sym[c] for c in sp) for sp, wid in zip(wlm.lexicon.spellings, wlm.word_ids)}
    names[W_UNK] = "<unk>"
    warpa, narpa = os.path.join(root, "words.arpa"), os.path.join(root, "chars.arpa")
    with open(warpa, "w") as f:
        f.write(wlm.lm.to_arpa(names))
    nlm = NgramLM.estimate(text, 2, V, bos, eos)
    with open(narpa, "w") as f:
        f.write(nlm.to_arpa({i: s for i, s in sym.items() if i not in (bos, eos)}))
    cfg = dict(solver.config, beam_size=3, max_dec_timesteps=12)
    test_loader = get_data_loader(solver._dataset(cfg["test_set"], None, sort=False), batch_size=1, shuffle=False, drop_last=False)

    def run(**extra):
        solver.config = dict(cfg, **extra)
        capsys.readouterr()
        cer = solver.test(state_dict=state)
        with open(os.path.join(root, "%s.txt" % cfg["test_set"])) as f:
            return cer, f.read().splitlines(), capsys.readouterr().out

    def direct(**kw):
        solver.model.eval()
        preds, refs = [], []
        for batch in solver._feed(test_loader, sharded=False):
            xs, ilens, _ = batch
            p, _ = solver.model.recognize_beams(xs, ilens, 12, 3, **kw)
            preds += p.cpu().numpy().tolist()
            refs += batch.ys_host
        solver.model.train()
        return solver.ind2sent(preds, refs)[1]

    monkeypatch.chdir(root)
    _, plain_lines, _ = run()
    loaded_n = NgramLM.from_arpa(narpa, {s: i for s, i in vocab.items() if s not in ("<s>", "</s>")}, bos, eos, V=V)
    cer, lines, out = run(att_ngram_lm=dict(arpa=narpa, weight=0.8, bonus=0.3))
    assert np.isfinite(cer) and "CER=" in out
    assert set(solver.model.last_beams["parts"]) == {"att", "lm"}
    assert lines == direct(ngram=loaded_n, ngram_weight=0.8, ngram_bonus=0.3)
    cer, lines, out = run(att_word_lm=dict(arpa=warpa, weight=0.8, bonus=0.5))
    assert np.isfinite(cer) and "CER=" in out
    assert lines == direct(word_lm=solver.load_word_lm(warpa), word_lm_weight=0.8, word_bonus=0.5)
    cer, zero_lines, _ = run(att_word_lm=dict(arpa=warpa))
    assert zero_lines == plain_lines                                         # weight 0: the search without it
    for extra, msg in ((dict(att_ngram_lm=dict(arpa=narpa), att_word_lm=dict(arpa=warpa)), "two LMs for one search"),
                       (dict(att_ngram_lm=dict(arpa=narpa), beam_size=1), "beam_size > 1"),
                       (dict(att_word_lm=dict(arpa=warpa, wieght=1.0)), "att_word_lm is a dictionary"),
                       (dict(att_ngram_lm=dict(weight=1.0)), "att_ngram_lm is a dictionary"),
                       (dict(att_word_lm=dict(arpa=warpa), ctc_greedy_decode=True, beam_size=3), "ctc_greedy_decode")):
        with pytest.raises(ValueError, match=msg):
            run(**extra)
    print("beam-ngram-parity solver: att_ngram_lm and att_word_lm hypotheses equal E2E.recognize_beams; left out 0")
