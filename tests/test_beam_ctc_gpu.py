"""Joint CTC-attention beam search on the GPU (csrc/ctc_prefix.hip, the CTC select of csrc/beam.hip, ops.beam_search with
ctc, E2E.recognize_beams(ctc_decode_weight=...), Solver.test with ctc_decode_weight): the prefix score and advance kernels
against the float64 restatement (tests/beam_ctc_ref.py), the CTC select against a stable sort, the search against the
restatement, the paths without CTC untouched, launches, memory and the solver switch.

Tolerance of the kernel cases: none is written down here.  Every case also runs the restatement in float32 numpy on the same
inputs; the kernel's worst absolute error against float64 may be at most 4 x that float32 error, with a floor of 8 fp32 ulps
of the tensor's largest magnitude; -inf must match exactly and nothing may be NaN.  Each case prints its worst ratios
(kernel error / allowance; profiles/ctc_prefix_parity.txt keeps them)."""
import os
import types

import numpy as np
import pytest
import torch

import beam_ctc_ref as R
import beam_lm_ref
import beam_ref
import synth
import test_beam_gpu as tb
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
EOS = 2
MARGIN = 1e-4


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ the score and advance kernels
def _compare(got, ref64, ref32, worst, name):
    """-inf exactly where float64 has it, no NaN, and the finite entries within the allowance of the module docstring."""
    got, ref64, ref32 = np.asarray(got), np.asarray(ref64), np.asarray(ref32)
    assert not np.isnan(got).any(), name
    ninf = np.isneginf(ref64)
    assert np.array_equal(np.isneginf(got), ninf), "%s: -inf where float64 is finite, or the reverse" % name
    assert np.isfinite(got[~ninf]).all(), name
    if (~ninf).any():
        err = float(np.abs(got[~ninf].astype(np.float64) - ref64[~ninf]).max())
        err32 = float(np.abs(ref32[~ninf].astype(np.float64) - ref64[~ninf]).max())
        allow = max(4.0 * err32, 8.0 * float(np.spacing(np.float32(np.abs(ref64[~ninf]).max()))))
        worst[name] = max(worst.get(name, 0.0), err / allow)
        assert err <= allow, "%s: error %.3g above %.3g (float32 restatement %.3g)" % (name, err, allow, err32)


def _kernel_case(hb, V, Tp, K, scale):
    """Four chained steps from the empty prefix over 4 utterances of Tp, 2 Tp / 3, 1 and Tp - 1 valid frames (at least 1); the
    last one is done from the start and the last beam of utterance 0 is dead (K > 1).  Backpointers and tokens are synthetic:
    any live predecessor, any label - odd rows repeat their predecessor's last label once it has one.  With T_b = 1 (and
    with T' <= 2 everywhere) the prefixes outgrow the frames: -inf throughout, no NaN.  The logits sit in a [B, T', V + 3]
    buffer whose pad columns and frames behind T_b are NaN."""
    rs = np.random.RandomState(1000 * V + 10 * Tp + K)
    lens = [Tp, max(1, (2 * Tp) // 3), 1, max(1, Tp - 1)]
    B, L, R_ = len(lens), 5, len(lens) * K
    z = (rs.randn(B, Tp, V) * scale).astype(np.float32)
    buf = np.full((B, Tp, V + 3), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        buf[b, :n, :V] = z[b, :n]
    s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
    sc = np.zeros((B, K), dtype=np.float32)
    if K > 1:
        sc[0, K - 1] = -np.inf
    s.scores.copy_(torch.from_numpy(sc))
    s.done[B - 1] = 1
    live = [[k for k in range(K) if np.isfinite(sc[b, k])] if b != B - 1 else [] for b in range(B)]
    lens_dev = hb.to_device_i32(lens, "cuda")
    cps = hb.CtcPrefixState(s, _cuda(buf)[:, :, :V], lens_dev, 0, lens)
    torch.cuda.synchronize()
    x = {np.float64: [R.log_probs(z[b, :lens[b]].astype(np.float64)) for b in range(B)],
         np.float32: [R.log_probs(z[b, :lens[b]]) for b in range(B)]}
    st = {dt: [[R.prefix_init(x[dt][b]) for _ in range(K)] for b in range(B)] for dt in x}
    worst = {}

    def state_of(slot):
        return cps.state[slot].cpu().numpy().reshape(B, K, Tp, 2)

    def check_state(slot, name):
        got = state_of(slot)
        for dt_i, part in enumerate(("r_n", "r_b")):
            pick = lambda dt: np.concatenate([st[dt][b][k][part] for b in range(B) for k in live[b]])      # noqa: E731
            g = np.concatenate([got[b, k, :lens[b], dt_i] for b in range(B) for k in live[b]])
            _compare(g, pick(np.float64), pick(np.float32), worst, name + " " + part)

    got = state_of(0)                                                      # the init: the empty prefix in all B K rows
    for b in range(B):
        assert np.isneginf(got[b, :, :lens[b], 0]).all() and (got[b, :, :lens[b], 1] == got[b, :1, :lens[b], 1]).all()
    check_state(0, "init")
    assert (cps.last[0] == -1).all() and (cps.psi_prev == 0).all()
    np.testing.assert_allclose(cps.lse.cpu().numpy()[0, :lens[0]],
                               np.log(np.exp(z[0, :lens[0]].astype(np.float64)).sum(-1)), rtol=1e-5)
    for t in range(4):
        cps.psi.fill_(7.0)
        cps.score()
        torch.cuda.synchronize()
        psi = cps.psi.cpu().numpy().reshape(B, K, V)
        ref = {dt: [[R.prefix_scores(st[dt][b][k], x[dt][b], EOS) for k in range(K)] for b in range(B)] for dt in x}
        for b in range(B):
            for k in range(K):
                if k not in live[b]:
                    assert (psi[b, k] == 7.0).all(), "a dead row or a done utterance was scored"
        pick = lambda dt: np.stack([ref[dt][b][k] for b in range(B) for k in live[b]])                      # noqa: E731
        _compare(np.stack([psi[b, k] for b in range(B) for k in live[b]]), pick(np.float64), pick(np.float32), worst,
                 "psi step %d" % t)
        bp, tok = np.zeros((B, K), dtype=np.int32), np.full((B, K), EOS, dtype=np.int32)
        for b in range(B):
            for k in live[b]:
                bp[b, k] = live[b][rs.randint(len(live[b]))]
                labels = [v for v in range(1, V) if v != EOS]
                tok[b, k] = labels[rs.randint(len(labels))]
                prev = st[np.float64][b][bp[b, k]]["last"]
                if k % 2 == 1 and prev >= 1:
                    tok[b, k] = prev
        s.bp_hist[t], s.tok_hist[t] = _cuda(bp), _cuda(tok)
        src, dst = cps.cur, 1 - cps.cur
        cps.state[dst].fill_(7.0)
        cps.last[dst].fill_(-7)
        prev_before = cps.psi_prev.clone()
        cps.advance(t)
        torch.cuda.synchronize()
        assert cps.cur == dst
        got_last, got_prev = cps.last[dst].cpu().numpy().reshape(B, K), cps.psi_prev.cpu().numpy().reshape(B, K)
        got_state = state_of(dst)
        for dt in x:
            st[dt] = [[R.prefix_advance(st[dt][b][bp[b, k]], x[dt][b], tok[b, k], ref[dt][b][bp[b, k]]) if k in live[b]
                       else st[dt][b][k] for k in range(K)] for b in range(B)]
        for b in range(B):
            for k in range(K):
                if k in live[b]:                                          # an exact gather of psi_prev, last token, flag
                    assert got_last[b, k] == tok[b, k]
                    assert got_prev[b, k].tobytes() == psi[b, bp[b, k], tok[b, k]].tobytes()
                    assert (got_state[b, k, lens[b]:] == 7.0).all()        # frames behind T_b are not written
                else:                                                     # dead rows and done utterances: untouched
                    assert got_last[b, k] == -7 and (got_state[b, k] == 7.0).all()
                    assert got_prev[b, k] == prev_before.cpu().numpy().reshape(B, K)[b, k]
        check_state(dst, "advance step %d" % t)
        if t >= 1:                                                        # longer than one frame allows
            assert all(np.isneginf(st[np.float64][2][k]["r_n"]).all() for k in live[2])
    return worst


def _report(what, worst):
    top = max(worst.items(), key=lambda kv: kv[1])
    print("ctc_prefix_parity %s: worst error / allowance %.3f (%s); psi %.3f, state %.3f"
          % (what, top[1], top[0], max(v for k, v in worst.items() if k.startswith("psi")),
             max(v for k, v in worst.items() if not k.startswith("psi"))))


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("Tp", [1, 2, 64, 65, 100])
@pytest.mark.parametrize("V", [3, 34, 65, 257])
def test_prefix_kernels_against_float64(hb, V, Tp, K):
    """V = 65 crosses a wave of token lanes, T' = 65 a round of the advance chain; T_b = 1; repeated last labels; prefixes
    longer than T_b; NaN behind T_b; dead rows and done utterances left untouched."""
    _report("V=%d T'=%d K=%d" % (V, Tp, K), _kernel_case(hb, V, Tp, K, 3.0))


@pytest.mark.parametrize("Tp", [1, 2, 64, 65, 100])
def test_prefix_kernels_logits_scaled_by_50(hb, Tp):
    """Probabilities underflow in linear space (logits ~ 150 N(0, 1)): same allowance, nothing NaN."""
    _report("V=34 T'=%d K=4 x50" % Tp, _kernel_case(hb, 34, Tp, 4, 150.0))


def test_advance_refuses_aliasing_and_the_init_refuses_shapes(hb):
    import ctypes
    B, K, V, Tp = 2, 4, 9, 6
    z = torch.randn(B, Tp, V, device="cuda")
    lens = hb.to_device_i32([6, 4], "cuda")
    s = hb.BeamSearch(B, K, V, 5, EOS, "cuda")
    cps = hb.CtcPrefixState(s, z, lens)
    s.bp_hist[0].zero_(), s.tok_hist[0].fill_(3)
    lib = hb.load()
    for src, dst in ((0, 0), (1, 1), (0, 2)):                              # in place (or no slot at all): ASR_E_ARG
        assert lib.asr_ctc_prefix_advance_f32(ctypes.byref(cps.struct), ctypes.byref(s.struct), 0, src, dst, hb.stream()) == -1
    cps.struct.state[1] = cps.struct.state[0]
    with pytest.raises(RuntimeError, match="code -1"):
        cps.advance(0)
    with pytest.raises(hb.UnsupportedShape):                               # V < 3
        hb.CtcPrefixState(hb.BeamSearch(B, K, 2, 5, 1, "cuda"), z[:, :, :2].contiguous(), lens)
    with pytest.raises(hb.UnsupportedShape):                               # <EOS> == blank
        hb.CtcPrefixState(hb.BeamSearch(B, K, V, 5, 0, "cuda"), z, lens)
    for bad in ([6, 0], [7, 4]):                                           # frame_lens < 1 or > T'
        with pytest.raises(hb.UnsupportedShape):
            hb.CtcPrefixState(s, z, hb.to_device_i32(bad, "cuda"), 0, bad)
    with pytest.raises(RuntimeError, match="code -1"):                     # a weight outside [0, 1]
        s.select_ctc(torch.zeros(B * K, V, device="cuda"), cps, 1.5, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the select kernel with CTC
def _ref_select_ctc(logits, scores, psi, psi_prev, lam, lm_logits, lmw, eos):
    """beam_ref.select on fp32 candidates formed in the contract's order, every operation rounded to fp32 on its own:
    c = score + (1 - lam) * logp; c = c + lam * (psi - psi_prev); with an LM c = c + lmw * logp_lm.  NaN (-inf - -inf) never
    enters: it is -inf here."""
    f = np.float32

    def lsm(x):
        x = x.astype(f)
        m = x.max(axis=-1, keepdims=True)
        return ((x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=f)).astype(f)).astype(f)
    sc = scores.astype(f)
    with np.errstate(invalid="ignore"):
        c = (sc[:, None] + ((f(1) - f(lam)) * lsm(logits)).astype(f)).astype(f)
        c = (c + (f(lam) * (psi.astype(f) - psi_prev.astype(f)[:, None]).astype(f)).astype(f)).astype(f)
        if lm_logits is not None:
            c = (c + (f(lmw) * lsm(lm_logits)).astype(f)).astype(f)
    c = np.where(np.isnan(c), f(-np.inf), c).astype(f)
    return beam_ref.select(np.where(np.isfinite(sc), f(0), f(-np.inf)).astype(f), c, eos)


def _psi_case(logits, K, V, seed):
    rs = np.random.RandomState(seed)
    B = logits.shape[0]
    psi = (-rs.rand(B, K, V) * 30).astype(np.float32)
    psi_prev = (-rs.rand(B, K) * 20).astype(np.float32)
    psi[:, :, 0] = -np.inf                                                 # the blank
    psi[1, 0] = -np.inf                                                    # a live row without any extension
    if V > 8:
        psi[:, :, 7] = -np.inf
    if K > 1:
        psi[0, 1], psi_prev[0, 1] = psi[0, 0], psi_prev[0, 0]              # the planted tie between beams 0 and 1 survives
    if V > 4:
        psi[:, :, 4] = psi[:, :, 3]                                        # and the ties inside a row
    return psi, psi_prev


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("lam", [0.3, 1.0])
@pytest.mark.parametrize("V", [3, 34, 257])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_select_ctc_kernel_against_a_stable_sort(hb, K, V, lam, with_lm):
    logits, scores = tb._select_case(K, V, EOS, 100 * K + V)
    psi, psi_prev = _psi_case(logits, K, V, 3 * K + V)
    rs = np.random.RandomState(7 * K + V)
    lm_logits = (rs.randn(*logits.shape) * 2).astype(np.float32) if with_lm else None
    if with_lm and K > 1:
        lm_logits[0, 1] = lm_logits[0, 0]
    if with_lm and V > 4:
        lm_logits[:, :, 4] = lm_logits[:, :, 3]
    B, L, t = logits.shape[0], 6, 3
    s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
    s.scores.copy_(torch.from_numpy(scores))
    ctc = types.SimpleNamespace(psi=_cuda(psi.reshape(B * K, V)), psi_prev=_cuda(psi_prev.reshape(B * K)))
    s.select_ctc(_cuda(logits.reshape(B * K, V)), ctc, lam, t, _cuda(lm_logits.reshape(B * K, V)) if with_lm else None, 0.6)
    torch.cuda.synchronize()
    ndone = 0
    for b in range(B):
        ref = _ref_select_ctc(logits[b], scores[b], psi[b], psi_prev[b], lam, lm_logits[b] if with_lm else None, 0.6, EOS)
        nlive = ref["nlive"]
        assert s.tok_hist[t, b].tolist() == ref["tok"].tolist(), (b, s.tok_hist[t, b], ref["tok"])
        assert s.bp_hist[t, b].tolist() == ref["bp"].tolist(), b
        assert 0 not in s.tok_hist[t, b, :nlive].tolist()                  # a blank is never emitted
        got_sc = s.scores[b].cpu().numpy()
        np.testing.assert_allclose(got_sc[:nlive], ref["scores"][:nlive], rtol=1e-6, atol=1e-5)
        assert np.isneginf(got_sc[nlive:]).all()
        fin = [(t, k, t + 1, 1) for k, _ in ref["finished"]]
        nf = int(s.nfin[b])
        assert nf == len(fin) and [tuple(r) for r in s.fin[b, :nf].tolist()] == fin
        np.testing.assert_allclose(s.fin_score[b, :nf].cpu().numpy(), np.array([sc for _, sc in ref["finished"]], dtype=np.float32),
                                   rtol=1e-6, atol=1e-5)
        done = len(fin) >= K or nlive == 0
        assert int(s.done[b]) == int(done)
        ndone += int(done)
    assert int(s.ndone[0]) == ndone


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("V", [3, 34, 257])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_select_ctc_with_weight_zero_is_the_select_without_it_bit_for_bit(hb, K, V, with_lm):
    logits, scores = tb._select_case(K, V, EOS, 100 * K + V)
    psi, psi_prev = _psi_case(logits, K, V, 3 * K + V)
    lm_logits = (np.random.RandomState(V + K).randn(*logits.shape) * 2).astype(np.float32)
    B, L, t = logits.shape[0], 6, 5                                        # the last step: live beams finish as they stand
    out = []
    for joint in (False, True):
        s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
        s.scores.copy_(torch.from_numpy(scores))
        s.tok_hist.zero_(), s.bp_hist.zero_(), s.fin.zero_(), s.fin_score.zero_()
        lg, lm = _cuda(logits.reshape(B * K, V)), _cuda(lm_logits.reshape(B * K, V))
        if joint:
            ctc = types.SimpleNamespace(psi=_cuda(psi.reshape(B * K, V)), psi_prev=_cuda(psi_prev.reshape(B * K)))
            s.select_ctc(lg, ctc, 0.0, t, lm if with_lm else None, 0.6)
        elif with_lm:
            s.select_lm(lg, lm, 0.6, t)
        else:
            s.select(lg, t)
        torch.cuda.synchronize()
        out.append([x.clone() for x in (s.scores.view(torch.int32), s.tok_hist, s.bp_hist, s.fin, s.fin_score.view(torch.int32),
                                        s._counters)])
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the search on the tiny model with a CTC head
TINY_ILENS = (47, 38, 29)            # -> 12, 10 and 8 encoder frames


def _tiny_arrays(cand):
    """cand (seed offset, <EOS> bias, L) -> (decoder weights, ctc_lo weight / bias, LM weights, features, L): the tiny_e2e
    model (synth.e2e_weights(TINY, 11)) with its output layer scaled by 4 (wider gaps) and an <EOS> bias, a CTC head from a
    seeded generator, the tiny_lm judge (synth.lm_weights(TINY_LM, 31)) scaled likewise, and ragged features."""
    off, eos_bias, L = cand
    t = synth.TINY
    w = synth.e2e_weights(t, 11)
    w["decoder.output_layer.weight"] = w["decoder.output_layer.weight"] * 4.0
    w["decoder.output_layer.bias"] = w["decoder.output_layer.bias"] * 4.0
    w["decoder.output_layer.bias"][EOS] += eos_bias
    rs = np.random.RandomState(500 + off)
    head_w = (rs.randn(t["output_dim"], t["enc_hidden_dim"]) * 1.5).astype(np.float32)
    head_b = (rs.randn(t["output_dim"]) * 0.5).astype(np.float32)
    lm_w = synth.lm_weights(dict(synth.TINY_LM, output_dim=t["output_dim"]), 31)
    lm_w["output_layer.weight"] = lm_w["output_layer.weight"] * 4.0
    lm_w["output_layer.bias"] = lm_w["output_layer.bias"] * 4.0
    xs = np.zeros((len(TINY_ILENS), max(TINY_ILENS), t["input_dim"]), dtype=np.float32)
    for b, n in enumerate(TINY_ILENS):
        xs[b, :n] = rs.randn(n, t["input_dim"])
    return w, head_w, head_b, lm_w, xs, L


def _tensors(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _restate(case, cand):
    """The float64 restatement of one case, the encoder included (the oracle's), on the CPU.  case (K, lam, with LM)."""
    K, lam, with_lm = case
    w, head_w, head_b, lm_w, xs, L = _tiny_arrays(cand)
    sd = {k: v.double() for k, v in _tensors(w).items()}
    enc, lens = O.encoder_forward(sd, torch.from_numpy(xs).double(), list(TINY_ILENS), synth.TINY["enc_n_layers"],
                                  synth.TINY["subsample"], 0.0, training=False)
    if lam == 0.0 and not with_lm:
        return beam_ref.decode(sd, enc, lens, L, K)
    return R.decode(sd, head_w, head_b, enc, lens, L, K, lam, _tensors(lm_w) if with_lm else None, 0.5)


def _modules(cand):
    import model as M
    w, head_w, head_b, lm_w, xs, L = _tiny_arrays(cand)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), ctc_weight=0.3, **synth.TINY).cuda()
    net.load_state_dict(dict(_tensors(w), **{"ctc_lo.weight": torch.from_numpy(head_w), "ctc_lo.bias": torch.from_numpy(head_b)}))
    net.eval()
    lm = M.LM(bos=1, eos=EOS, pad=0, labeldist=None, **dict(synth.TINY_LM, output_dim=synth.TINY["output_dim"], ls_weight=0.0)).cuda()
    lm.load_state_dict(_tensors(lm_w))
    lm.eval()
    return net, lm, _cuda(xs), list(TINY_ILENS), L


SEARCH_GRID = [(K, lam, with_lm) for K in (1, 4) for lam in (0.3, 0.7) for with_lm in (False, True)]
# Every case has its own candidate (seed offset, <EOS> bias, L): the first of SEARCH_TRIES for which the RESTATEMENT alone has
# (4 B + 4) // 5 = 3 of the 3 utterances with a smallest decision margin above MARGIN, one of them running >= 6 steps -
# beam_lm_ref.find_seeds(_restate, SEARCH_GRID, SEARCH_TRIES, MARGIN, 6), no GPU involved.  Recorded per case: the candidate,
# the restatement's smallest margin and its step count per utterance.
SEARCH_TRIES = [(off, bias, L) for L in (14, 9) for bias in (0.0, 1.0, -1.0, 2.0) for off in range(8)]
SEARCH_CASES = {
    (1, 0.3, False): ((2, 0.0, 14), [4.039877e-02, 6.288395e-02, 5.737292e-02], [8, 6, 6]),
    (1, 0.3, True): ((0, 0.0, 14), [1.303701e-02, 9.078954e-03, 1.957566e-02], [10, 9, 7]),
    (1, 0.7, False): ((0, 0.0, 14), [5.650806e-02, 4.469854e-02, 2.708713e-02], [8, 7, 6]),
    (1, 0.7, True): ((0, 0.0, 14), [1.310779e-02, 4.569599e-03, 4.307205e-02], [9, 7, 6]),
    (4, 0.3, False): ((0, 0.0, 14), [8.441275e-03, 1.709696e-02, 3.210156e-03], [8, 6, 5]),
    (4, 0.3, True): ((0, 0.0, 14), [4.369632e-04, 2.591896e-03, 4.010293e-03], [10, 8, 7]),
    (4, 0.7, False): ((0, 0.0, 14), [1.247100e-02, 8.629137e-04, 8.708369e-03], [9, 8, 6]),
    (4, 0.7, True): ((0, 0.0, 14), [8.851573e-04, 4.113010e-03, 1.642816e-04], [9, 8, 6]),
}
# "CTC matters": the first candidate of SEARCH_TRIES for which the restatement's best hypothesis of every utterance differs
# between ctc_decode_weight 0 and 0.7 at K = 4, all margins (ranking included) above MARGIN.
MATTERS = (0, 0.0, 14)


@pytest.mark.parametrize("case", SEARCH_GRID, ids=lambda c: "K%d-w%s-%s" % (c[0], c[1], "lm" if c[2] else "nolm"))
def test_joint_beams_against_the_float64_restatement(hb, case):
    K, lam, with_lm = case
    cand, margins, steps = SEARCH_CASES[case]
    net, lm, xs, ilens, L = _modules(cand)
    kw = dict(lm=lm, lm_weight=0.5) if with_lm else {}
    hb.LAUNCHES.clear()
    toks, scores = net.recognize_beams(xs, ilens, L, K, nbest=True, ctc_decode_weight=lam, **kw)
    assert hb.LAUNCHES["beam_ctc_step"] > 0 and hb.LAUNCHES["beam_step"] == 0 and hb.LAUNCHES["beam_lm_step"] == 0
    best, best_score = net.recognize_beams(xs, ilens, L, K, ctc_decode_weight=lam, **kw)
    assert torch.equal(best, toks[:, 0]) and torch.equal(best_score, scores[:, 0])
    ref = _restate(case, cand)
    np.testing.assert_allclose([min(r["margins"]) for r in ref], margins, rtol=1e-6)          # the recorded restatement
    assert [r["steps"] for r in ref] == steps
    B = len(ref)
    qualified, long_enough = 0, False
    for b in range(B):
        r = ref[b]
        if min(r["margins"]) <= MARGIN:
            continue
        qualified += 1
        long_enough = long_enough or r["steps"] >= 6
        got = [tb._cut(toks[b, k].tolist()) for k in range(len(r["hyps"]))]
        assert got == [h[0] for h in r["hyps"]], (b, got, r["hyps"])
        np.testing.assert_allclose(scores[b, :len(r["hyps"])].cpu().numpy(), [h[1] for h in r["hyps"]], rtol=1e-4)
    assert qualified >= (4 * B + 4) // 5, margins
    assert long_enough, steps


def test_ctc_matters(hb):
    """The best hypothesis of a fixed model changes with the CTC weight the way the restatement says (a joint path that
    ignored psi would return the plain hypothesis)."""
    net, lm, xs, ilens, L = _modules(MATTERS)
    plain, _ = net.recognize_beams(xs, ilens, L, 4)
    joint, _ = net.recognize_beams(xs, ilens, L, 4, ctc_decode_weight=0.7)
    ref_plain, ref = _restate((4, 0.0, False), MATTERS), _restate((4, 0.7, False), MATTERS)
    differ = 0
    for b in range(len(ilens)):
        assert min(ref[b]["margins"] + [ref[b]["rank_margin"]]) > MARGIN
        assert min(ref_plain[b]["margins"] + [ref_plain[b]["rank_margin"]]) > MARGIN
        assert tb._cut(joint[b].tolist()) == ref[b]["hyps"][0][0]
        assert tb._cut(plain[b].tolist()) == ref_plain[b]["hyps"][0][0]
        differ += tb._cut(joint[b].tolist()) != tb._cut(plain[b].tolist())
        assert len(tb._cut(joint[b].tolist())) <= net.encoder.enc2.last_lens_dev[b].item() + 1      # labels <= frames
    assert differ == len(ilens)


def test_weight_zero_takes_the_path_without_ctc(hb):
    net, lm, xs, ilens, L = _modules(MATTERS)
    for kw, kind in ((dict(), "beam"), (dict(lm=lm, lm_weight=0.5), "beam_lm")):
        hb.LAUNCHES.clear()
        want = net.recognize_beams(xs, ilens, L, 4, nbest=True, **kw)
        counts = dict(hb.LAUNCHES)
        assert counts[kind + "_step"] > 0
        hb.LAUNCHES.clear()
        got = net.recognize_beams(xs, ilens, L, 4, nbest=True, ctc_decode_weight=0.0, **kw)
        beams = lambda c: {k: v for k, v in c.items() if k.startswith("beam")}                 # noqa: E731
        assert beams(hb.LAUNCHES) == beams(counts) and hb.LAUNCHES["beam_ctc_step"] == 0
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the decoder alone: logits without a weight change nothing either
    with torch.no_grad():
        enc_h, enc_lens = net.encoder(xs, ilens)
        z = torch.randn(enc_h.shape[0], enc_h.shape[1], synth.TINY["output_dim"], device="cuda")
        a = net.decoder.recognize_beams(enc_h, enc_lens, L, 4, ctc_logits=z, ctc_lens=net.encoder.enc2.last_lens_dev)
        b = net.decoder.recognize_beams(enc_h, enc_lens, L, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_joint_launches_per_step(hb):
    """the prefix score and the advance on top of the plain step's 7 launches (9) or the LM step's 8 + n_layers
    (10 + n_layers); the last step has neither reorder nor advance; the init runs once and is not a step's."""
    net, lm, xs, ilens, L = _modules(MATTERS)
    for kw, per_step in ((dict(), 9), (dict(lm=lm, lm_weight=0.5), 10 + lm.n_layers)):
        hb.LAUNCHES.clear()
        net.recognize_beams(xs, ilens, L, 4, ctc_decode_weight=0.3, **kw)
        steps = hb.LAUNCHES["beam_ctc_step"]
        assert steps > 1 and hb.LAUNCHES["beam_step"] == 0 and hb.LAUNCHES["beam_lm_step"] == 0
        assert hb.LAUNCHES["beam_ctc_launch"] in (per_step * steps, per_step * steps - 2)


def test_joint_memory_does_not_grow_with_max_dec_timesteps(hb):
    import test_beam_lm_gpu as tl
    import model as M
    cfg, w = tl._e2e_weights(512, 34, 512, 41, -30.0, out_scale=1.0)      # no <EOS>: a search ends when its prefixes outgrow the frames
    net = M.E2E(labeldist=synth.labeldist(34, 12), ctc_weight=0.3, **cfg).cuda()
    torch.manual_seed(3)
    net.load_state_dict(_tensors(w), strict=False)
    net.eval()
    lens = [60, 50, 40, 30]
    enc = _cuda(tl._enc_arrays(4, 512, lens, 9))
    with torch.no_grad():
        z = torch.nn.functional.linear(enc, net.ctc_lo.weight * 0.05, net.ctc_lo.bias)          # flat: no prefix dies
    lens_dev = hb.to_device_i32(lens, "cuda")
    peaks = []
    for L in (50, 400):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pred, _ = net.decoder.recognize_beams(enc, lens, L, 4, ctc_logits=z, ctc_lens=lens_dev, ctc_decode_weight=0.1)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert pred.shape == (4, L)
        del pred
    assert abs(peaks[1] - peaks[0]) < 16 * 2 ** 20, peaks


def test_solver_test_with_ctc_decode_weight(hb, tmp_path, monkeypatch):
    import test_ctc_gpu as tc
    from dataloader import get_data_loader
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    jsd = {k: v.clone() for k, v in solver.judge.state_dict().items()}

    def run(**extra):
        solver.config = dict(cfg, **extra)
        solver.test(state_dict=sd, judge_state_dict=jsd if extra.get("lm_weight") else None)
        with open(os.path.join(root, "dev.txt")) as f:
            return f.read().splitlines()

    def direct(K, **kw):
        loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
        solver.model.eval(), solver.judge.eval()
        preds, refs = [], []
        for batch in solver._feed(loader, sharded=False):
            xs, ilens, _ = batch
            p, _ = solver.model.recognize_beams(xs, ilens, cfg["max_dec_timesteps"], K, **kw)
            preds += p.cpu().numpy().tolist()
            refs += batch.ys_host
        solver.model.train(), solver.judge.train()
        return solver.ind2sent(preds, refs)[1]

    plain_lines = run()
    hb.LAUNCHES.clear()
    assert run(ctc_decode_weight=0) == plain_lines and hb.LAUNCHES["beam_ctc_step"] == 0      # the key at 0: the lines without it
    hb.LAUNCHES.clear()
    greedy_joint = run(ctc_decode_weight=0.4)                                    # beam_size 1: the joint search all the same
    assert hb.LAUNCHES["beam_ctc_step"] > 0
    assert greedy_joint == direct(1, ctc_decode_weight=0.4)
    hb.LAUNCHES.clear()
    lines = run(beam_size=4, beam_length_penalty=0.5, ctc_decode_weight=0.4, lm_weight=0.6)
    assert hb.LAUNCHES["beam_ctc_step"] > 0 and hb.LAUNCHES["beam_lm_step"] == 0
    assert lines == direct(4, length_penalty=0.5, lm=solver.judge, lm_weight=0.6, ctc_decode_weight=0.4)
    assert solver.judge.training and solver.model.training
    solver.config = dict(cfg, ctc_decode_weight=1.5)
    with pytest.raises(ValueError):
        solver.test(state_dict=sd)
    solver.model.train()
