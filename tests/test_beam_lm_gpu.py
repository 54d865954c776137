"""Shallow-fusion beam search on the GPU (csrc/lm_step.hip, the LM entries of csrc/beam.hip, ops.beam_search with lm,
Decoder.recognize_beams(lm=...), Solver.test with lm_weight): the LM step kernel against a float64 step (bounded by the
error of LM.forward_step), the fused select against a stable sort, the LM reorder as a permutation, the search against
the float64 restatement (tests/beam_lm_ref.py), the plain path untouched, launches, memory and the solver switch."""
import os

import numpy as np
import pytest
import torch

import beam_lm_ref
import beam_ref
import synth
import test_beam_gpu as tb

pytestmark = pytest.mark.gpu
EOS = 2
MARGIN = 1e-4
LMS = {"1x320": dict(n_layers=1, hidden_dim=320, embedding_dim=48), "2x640": dict(n_layers=2, hidden_dim=640, embedding_dim=256)}


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ the LM step kernel
def _step_case(layers, H, In, R, seed):
    cfg = dict(output_dim=20, embedding_dim=In, hidden_dim=H, n_layers=layers)
    w = synth.lm_weights(cfg, seed)
    for k in w:                                   # synth's 1/sqrt(H) weights leave the gates near 0: widen them
        if k.startswith("LSTM.weight"):
            w[k] = w[k] * 3.0
    rs = np.random.RandomState(seed + 1)
    xs = rs.randn(4, R, In).astype(np.float32)
    h0 = (rs.rand(layers, R, H).astype(np.float32) * 2 - 1) * 0.8
    c0 = rs.randn(layers, R, H).astype(np.float32)
    return w, xs, h0, c0


@pytest.mark.parametrize("R", [1, 4, 37, 128, 512])
@pytest.mark.parametrize("In", ["H", 256, 48])
@pytest.mark.parametrize("H", [320, 640])
@pytest.mark.parametrize("layers", [1, 2])
def test_lm_step_against_float64(hb, layers, H, In, R):
    """Four chained steps from a random non-zero state.  The bar is not a number fixed here: the worst error of h and c
    against float64 may be at most twice the worst error of LM.forward_step (the asr_gemm_f32 path + torch pointwise) on
    the same inputs.  Both errors are printed (DESIGN 4.9 quotes them)."""
    import model as M
    In = H if In == "H" else In
    w, xs, h0, c0 = _step_case(layers, H, In, R, 1000 * layers + H + In + R)
    sd64 = {k: torch.from_numpy(v).double() for k, v in w.items()}
    lm = M.LM(output_dim=20, embedding_dim=In, hidden_dim=H, dropout_rate=0.0, n_layers=layers, bos=1, eos=EOS, pad=0,
              ls_weight=0.0, labeldist=None).cuda()
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    lm.eval()
    st = hb.LmStepState(R, lm.embedding.weight, [lm.LSTM.direction_params(l) for l in range(layers)])
    for l in range(layers):
        st.xin[l][0][:, st.in_dim[l]:] = _cuda(h0[l])
        st.cell[l][0].copy_(_cuda(c0[l]))
    h64, c64 = torch.from_numpy(h0).double(), torch.from_numpy(c0).double()
    hz, cz = _cuda(h0), _cuda(c0)
    err_new = err_old = 0.0
    for t in range(xs.shape[0]):
        x = _cuda(xs[t])
        st.xin[0][0][:, :In] = x
        st.step()
        for l in range(layers):                      # identity reorder: slot 1 -> slot 0
            st.xin[l][0][:, st.in_dim[l]:] = st.xin[l][1][:, st.in_dim[l]:]
            st.cell[l][0].copy_(st.cell[l][1])
        _, hz, cz = lm.forward_step(x.unsqueeze(1), hz, cz)
        _, h64, c64 = beam_lm_ref.lm_step(sd64, torch.from_numpy(xs[t]).double(), h64, c64)
        got_h = torch.stack([st.xin[l][1][:, st.in_dim[l]:] for l in range(layers)]).double().cpu()
        got_c = torch.stack([st.cell[l][1] for l in range(layers)]).double().cpu()
        if layers > 1:                               # the x part of the next layer's input row is this layer's h
            assert torch.equal(st.xin[1][0][:, :H], st.xin[0][1][:, st.in_dim[0]:])
        err_new = max(err_new, float((got_h - h64).abs().max()), float((got_c - c64).abs().max()))
        err_old = max(err_old, float((hz.double().cpu() - h64).abs().max()), float((cz.double().cpu() - c64).abs().max()))
    print("lm_step layers=%d H=%d In=%d R=%d: worst |err| vs float64 %.3e (forward_step %.3e)" % (layers, H, In, R, err_new, err_old))
    assert err_old > 0 and err_new <= 2.0 * err_old, (err_new, err_old)


def test_lm_step_refuses_unsupported_shapes(hb):
    f = lambda *s: torch.zeros(*s, device="cuda")                      # noqa: E731
    with pytest.raises(RuntimeError, match="code -2"):                 # H not a multiple of 16
        hb.lm_step(4, 24, 16, f(4, 40), f(96, 40), f(96), f(4, 24), f(4, 24), f(4, 24))
    with pytest.raises(RuntimeError, match="code -2"):                 # more rows than the kernel serves
        hb.lm_step(513, 32, 16, f(513, 48), f(128, 48), f(128), f(513, 32), f(513, 32), f(513, 32))
    c = f(4, 32)
    with pytest.raises(RuntimeError, match="code -1"):                 # the cell state in place
        hb.lm_step(4, 32, 16, f(4, 48), f(128, 48), f(128), c, c, f(4, 32))
    with pytest.raises(ValueError):
        hb.LmStepState(600, f(9, 16), [(f(128, 16), f(128, 32), f(128), f(128))])


# ------------------------------------------------------------------ the fused select kernel
def _ref_select_lm(logits, lm_logits, lam, scores, eos):
    """beam_ref.select on fp32 candidates formed like the kernel's: (score + logp) + lam * logp_lm, every operation
    rounded to fp32 on its own; logp = (x - max) - log(sum exp)."""
    def lsm(x):
        x = x.astype(np.float32)
        m = x.max(axis=-1, keepdims=True)
        return ((x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    lp, lq = lsm(logits), lsm(lm_logits)
    sc = scores.astype(np.float32)
    fused = (sc[:, None] + lp).astype(np.float32) + (np.float32(lam) * lq).astype(np.float32)
    # select() adds scores itself: hand it the fused candidates as "logp" of zero-score beams, dead beams kept dead
    return beam_ref.select(np.where(np.isfinite(sc), np.float32(0), np.float32(-np.inf)).astype(np.float32),
                           fused.astype(np.float32), eos)


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("V", [2, 33, 140, 8192])
@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_select_lm_kernel_against_a_stable_sort(hb, K, V, lam):
    eos = EOS if V > EOS else V - 1
    logits, scores = tb._select_case(K, V, eos, 100 * K + V)
    rs = np.random.RandomState(7 * K + V)
    lm_logits = (rs.randn(*logits.shape) * 2).astype(np.float32)
    if K > 1:
        lm_logits[0, 1] = lm_logits[0, 0]                              # the planted tie between beams 0 and 1 survives
    if V > 4:
        lm_logits[:, :, 4] = lm_logits[:, :, 3]                        # and the ties inside a row
    B, L, t = logits.shape[0], 6, 3
    s = hb.BeamSearch(B, K, V, L, eos, "cuda")
    s.scores.copy_(torch.from_numpy(scores))
    s.select_lm(_cuda(logits.reshape(B * K, V)), _cuda(lm_logits.reshape(B * K, V)), lam, t)
    torch.cuda.synchronize()
    ndone = 0
    for b in range(B):
        ref = _ref_select_lm(logits[b], lm_logits[b], lam, scores[b], eos)
        nlive = ref["nlive"]
        assert s.tok_hist[t, b].tolist() == ref["tok"].tolist(), (b, s.tok_hist[t, b], ref["tok"])
        assert s.bp_hist[t, b].tolist() == ref["bp"].tolist(), b
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


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("V", [2, 33, 140, 8192])
def test_select_lm_with_weight_zero_is_the_plain_select_bit_for_bit(hb, K, V):
    eos = EOS if V > EOS else V - 1
    logits, scores = tb._select_case(K, V, eos, 100 * K + V)
    lm_logits = (np.random.RandomState(V + K).randn(*logits.shape) * 2).astype(np.float32)
    B, L, t = logits.shape[0], 6, 5                                    # the last step: live beams finish as they stand
    out = []
    for fused in (False, True):
        s = hb.BeamSearch(B, K, V, L, eos, "cuda")
        s.scores.copy_(torch.from_numpy(scores))
        s.tok_hist.zero_(), s.bp_hist.zero_(), s.fin.zero_(), s.fin_score.zero_()
        lg = _cuda(logits.reshape(B * K, V))
        if fused:
            s.select_lm(lg, _cuda(lm_logits.reshape(B * K, V)), 0.0, t)
        else:
            s.select(lg, t)
        torch.cuda.synchronize()
        out.append([x.clone() for x in (s.scores.view(torch.int32), s.tok_hist, s.bp_hist, s.fin, s.fin_score.view(torch.int32),
                                        s._counters)])
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the LM reorder
def test_reorder_lm_is_an_exact_permutation(hb):
    B, K, V, L, H, E, t = 3, 4, 11, 5, 32, 16, 2
    rs = np.random.RandomState(3)
    s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
    bp = rs.randint(0, K, size=(B, K)).astype(np.int32)
    tok = rs.randint(0, V, size=(B, K)).astype(np.int32)
    s.bp_hist[t], s.tok_hist[t] = _cuda(bp), _cuda(tok)
    s.done[1] = 1                                                       # a done utterance: its rows stay as they are
    f = lambda *shape: _cuda(rs.randn(*shape).astype(np.float32))       # noqa: E731
    R = B * K
    layers = [(f(4 * H, E), f(4 * H, H), f(4 * H), f(4 * H)), (f(4 * H, H), f(4 * H, H), f(4 * H), f(4 * H))]
    st = hb.LmStepState(R, f(V, E), layers)
    for l in range(2):
        st.xin[l].copy_(f(*st.xin[l].shape))
        st.cell[l].copy_(f(*st.cell[l].shape))
    before = [(x.clone(), c.clone()) for x, c in zip(st.xin, st.cell)]
    # with the decoder's gather in the same launch
    D, O, Ed, Tp = 48, 32, 16, 37
    x_src, c_src, w_src, emb = f(R, D + O + Ed), f(R, D), f(R, Tp), f(V, Ed)
    x_dst, c_dst, w_dst = (torch.full_like(a, 7.0) for a in (x_src, c_src, w_src))
    s.reorder_lm(t, st, (x_src, x_dst, c_src, c_dst, w_src, w_dst, emb, D, O))
    torch.cuda.synchronize()
    src = (torch.arange(B).repeat_interleave(K) * K + torch.from_numpy(bp).reshape(-1).long()).cuda()
    live = torch.tensor([b != 1 for b in range(B) for _ in range(K)]).cuda()
    tk = torch.from_numpy(tok).reshape(-1).long().cuda()
    for l in range(2):
        In = st.in_dim[l]
        x0, c0 = before[l]
        assert torch.equal(st.xin[l][1], x0[1]) and torch.equal(st.cell[l][1], c0[1])          # the source slot is only read
        assert torch.equal(st.xin[l][0][live][:, In:], x0[1].index_select(0, src)[live][:, In:])
        assert torch.equal(st.cell[l][0][live], c0[1].index_select(0, src)[live])
        assert torch.equal(st.xin[l][0][~live], x0[0][~live]) and torch.equal(st.cell[l][0][~live], c0[0][~live])
        if l == 0:
            assert torch.equal(st.xin[0][0][live][:, :In], st.emb.index_select(0, tk)[live])
        else:
            assert torch.equal(st.xin[l][0][:, :In], x0[0][:, :In])                            # x parts above layer 0: untouched
    assert torch.equal(x_dst[live][:, :D + O], x_src.index_select(0, src)[live][:, :D + O])
    assert torch.equal(x_dst[live][:, D + O:], emb.index_select(0, tk)[live])
    assert torch.equal(c_dst[live], c_src.index_select(0, src)[live]) and torch.equal(w_dst[live], w_src.index_select(0, src)[live])
    assert (x_dst[~live] == 7.0).all() and (c_dst[~live] == 7.0).all() and (w_dst[~live] == 7.0).all()
    # the LM state alone
    x_dst.fill_(7.0)
    s.reorder_lm(t, st)
    torch.cuda.synchronize()
    assert (x_dst == 7.0).all()
    # in place is refused: ASR_E_ARG
    alias = st.reorder_struct()
    alias.x_dst[0] = alias.x_src[0]
    with pytest.raises(RuntimeError, match="code -1"):
        s.reorder_lm(t, st)
    st._reorder = None
    alias = st.reorder_struct()
    alias.c_dst[1] = alias.c_src[1]
    with pytest.raises(RuntimeError, match="code -1"):
        s.reorder_lm(t, st)


# ------------------------------------------------------------------ the search on decoders with an LM
def _e2e_weights(D, V, enc_dim, seed, eos_bias, out_scale=4.0):
    """The weights of test_beam_gpu._decoder_net, as arrays (the seed search below runs without a GPU)."""
    cfg = dict(synth.CFG1, enc_hidden_dim=enc_dim, dec_hidden_dim=D, att_dim=D, att_odim=D, output_dim=V)
    w = synth.e2e_weights(cfg, seed)
    w["decoder.output_layer.weight"] = w["decoder.output_layer.weight"] * out_scale
    w["decoder.output_layer.bias"] = w["decoder.output_layer.bias"] * out_scale
    w["decoder.output_layer.bias"][EOS] += eos_bias
    return cfg, w


def _lm_weights(name, V, seed, out_scale=4.0, bias=None):
    cfg = dict(LMS[name], output_dim=V)
    w = synth.lm_weights(cfg, seed)
    w["output_layer.weight"] = w["output_layer.weight"] * out_scale
    w["output_layer.bias"] = w["output_layer.bias"] * out_scale
    if bias is not None:
        w["output_layer.bias"][bias[0]] += bias[1]
    return cfg, w


def _enc_arrays(B, enc_dim, lens, seed):
    rs = np.random.RandomState(seed)
    enc = rs.randn(B, max(lens), enc_dim).astype(np.float32)
    for b, n in enumerate(lens):
        enc[b, n:] = 0.1
    return enc


def _lm_module(cfg, w):
    import model as M
    lm = M.LM(dropout_rate=0.0, bos=1, eos=EOS, pad=0, ls_weight=0.0, labeldist=None, **cfg).cuda()
    lm.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    lm.eval()
    return lm


def _e2e_module(cfg, w):
    import model as M
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    return net


def _search_case(case, cand):
    """case (K, D, lm name, B, lm_weight), cand (seed offset, <EOS> bias, L) -> (cfg, w, lm_cfg, lm_w, enc, lens, L)."""
    K, D, name, B, lam = case
    off, eos_bias, L = cand
    enc_dim, V = (128, 30) if D == 320 else (512, 140)
    lens = (36, 30, 22, 15, 8)[:B]
    cfg, w = _e2e_weights(D, V, enc_dim, 31 + K + 100 * off, eos_bias)
    lm_cfg, lm_w = _lm_weights(name, V, 61 + K + 100 * off)
    return cfg, w, lm_cfg, lm_w, _enc_arrays(B, enc_dim, lens, 7 + K + 100 * off), list(lens), L


def _restate(case, cand):
    _, w, _, lm_w, enc, lens, L = _search_case(case, cand)
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}      # noqa: E731
    return beam_lm_ref.decode(t(w), t(lm_w), torch.from_numpy(enc), lens, L, case[0], case[4])


SEARCH_GRID = [(K, D, name, B, lam) for K in (1, 2, 4, 8) for D in (320, 512) for name in ("1x320", "2x640")
               for B in (1, 5) for lam in (0.3, 0.7)]
# The naive grid (one seed rule, <EOS> bias 2.5 or 0) does not meet both conditions of the test below in the float64
# restatement alone (searches of 1 - 2 steps, or margins under 1e-4 over 14 steps), so every case has its own candidate
# (seed offset, <EOS> bias, L): the first of SEARCH_TRIES for which the RESTATEMENT has >= (4B + 4) // 5 utterances with a
# smallest margin above MARGIN, one of them running >= 6 steps - beam_lm_ref.find_seeds(_restate, SEARCH_GRID, SEARCH_TRIES,
# MARGIN, 6), no GPU involved.  Recorded per case: candidate, the restatement's smallest margin and step count per utterance.
SEARCH_TRIES = [(off, bias, L) for L in (14, 8) for bias in (1.0, 0.5, 1.5, 0.0) for off in range(6)]
SEARCH_CASES = {
    (1, 320, '1x320', 1, 0.3): ((5, 1.0, 14), [3.165273e-04], [14]),
    (1, 320, '1x320', 1, 0.7): ((1, 0.5, 14), [3.662265e-03], [14]),
    (1, 320, '1x320', 5, 0.3): ((2, 1.0, 14), [1.041692e-01, 4.750460e-03, 1.904672e-01, 4.544665e-02, 6.028614e-02], [1, 14, 1, 1, 1]),
    (1, 320, '1x320', 5, 0.7): ((0, 0.5, 14), [5.645417e-02, 8.159260e-03, 3.708255e-03, 2.718477e-04, 6.173907e-03], [2, 14, 1, 10, 14]),
    (1, 320, '2x640', 1, 0.3): ((5, 1.0, 14), [5.059627e-04], [14]),
    (1, 320, '2x640', 1, 0.7): ((5, 1.0, 14), [1.240112e-03], [14]),
    (1, 320, '2x640', 5, 0.3): ((2, 1.0, 14), [1.488933e-01, 5.583675e-02, 2.502028e-01, 1.878243e-01, 1.633056e-01], [1, 14, 1, 1, 1]),
    (1, 320, '2x640', 5, 0.7): ((5, 1.0, 14), [1.240112e-03, 2.786595e-02, 1.577298e-02, 2.744336e-02, 1.804312e-02], [14, 2, 2, 2, 1]),
    (1, 512, '1x320', 1, 0.3): ((0, 0.5, 14), [8.216617e-04], [14]),
    (1, 512, '1x320', 1, 0.7): ((0, 0.5, 14), [3.101029e-04], [14]),
    (1, 512, '1x320', 5, 0.3): ((0, 0.5, 14), [8.216617e-04, 9.745696e-04, 9.084596e-02, 1.223264e-01, 1.409278e-03], [14, 14, 1, 1, 14]),
    (1, 512, '1x320', 5, 0.7): ((3, 1.0, 14), [1.488782e-02, 4.454281e-02, 1.058349e-02, 3.793500e-03, 1.722539e-01], [1, 1, 1, 14, 1]),
    (1, 512, '2x640', 1, 0.3): ((0, 0.5, 14), [1.738994e-03], [14]),
    (1, 512, '2x640', 1, 0.7): ((0, 0.5, 14), [1.433501e-03], [14]),
    (1, 512, '2x640', 5, 0.3): ((0, 0.5, 14), [1.738994e-03, 3.759095e-03, 5.462828e-02, 5.719537e-02, 4.639748e-04], [14, 14, 1, 1, 14]),
    (1, 512, '2x640', 5, 0.7): ((0, 0.5, 14), [1.433501e-03, 2.561516e-04, 3.933592e-03, 9.218956e-02, 6.331972e-04], [14, 14, 1, 1, 14]),
    (2, 320, '1x320', 1, 0.3): ((0, 0.5, 14), [1.248824e-03], [14]),
    (2, 320, '1x320', 1, 0.7): ((0, 0.5, 14), [1.759883e-03], [14]),
    (2, 320, '1x320', 5, 0.3): ((0, 0.5, 14), [1.248824e-03, 2.482019e-03, 9.728437e-05, 2.386196e-03, 1.474061e-03], [14, 2, 14, 14, 14]),
    (2, 320, '1x320', 5, 0.7): ((0, 1.0, 14), [2.342230e-02, 5.127570e-03, 2.060566e-02, 3.438247e-03, 1.371530e-04], [2, 2, 2, 14, 8]),
    (2, 320, '2x640', 1, 0.3): ((0, 0.5, 14), [7.128354e-03], [14]),
    (2, 320, '2x640', 1, 0.7): ((0, 0.5, 14), [4.579467e-03], [14]),
    (2, 320, '2x640', 5, 0.3): ((0, 0.5, 14), [7.128354e-03, 1.443137e-03, 3.113366e-03, 2.338526e-03, 1.562899e-03], [14, 2, 4, 14, 8]),
    (2, 320, '2x640', 5, 0.7): ((0, 0.5, 14), [4.579467e-03, 5.106141e-04, 2.898669e-03, 4.706932e-03, 1.788981e-03], [14, 2, 3, 14, 12]),
    (2, 512, '1x320', 1, 0.3): ((1, 0.5, 14), [5.367912e-04], [14]),
    (2, 512, '1x320', 1, 0.7): ((0, 0.5, 14), [8.521939e-04], [14]),
    (2, 512, '1x320', 5, 0.3): ((0, 0.5, 14), [8.998436e-03, 1.274228e-03, 1.874721e-04, 2.896834e-04, 6.444925e-04], [2, 14, 14, 14, 4]),
    (2, 512, '1x320', 5, 0.7): ((0, 0.5, 14), [8.521939e-04, 3.311113e-03, 6.785264e-05, 1.534127e-03, 1.089698e-03], [14, 14, 14, 14, 14]),
    (2, 512, '2x640', 1, 0.3): ((1, 0.5, 14), [2.052306e-03], [14]),
    (2, 512, '2x640', 1, 0.7): ((1, 0.5, 14), [2.176587e-04], [14]),
    (2, 512, '2x640', 5, 0.3): ((0, 0.5, 14), [1.615757e-03, 2.138492e-03, 1.970986e-04, 6.800980e-03, 2.672468e-03], [3, 14, 14, 2, 8]),
    (2, 512, '2x640', 5, 0.7): ((0, 0.5, 14), [9.465850e-03, 4.909224e-04, 1.219298e-03, 1.323762e-03, 1.507963e-03], [3, 14, 2, 14, 9]),
    (4, 320, '1x320', 1, 0.3): ((0, 0.5, 14), [3.060115e-04], [14]),
    (4, 320, '1x320', 1, 0.7): ((0, 0.5, 14), [6.910997e-04], [14]),
    (4, 320, '1x320', 5, 0.3): ((0, 0.5, 14), [3.060115e-04, 1.005938e-02, 2.304468e-03, 4.918415e-04, 5.828377e-03], [14, 2, 3, 14, 3]),
    (4, 320, '1x320', 5, 0.7): ((0, 0.5, 14), [6.910997e-04, 1.460954e-02, 2.044086e-04, 1.611285e-03, 1.632701e-03], [14, 3, 4, 4, 14]),
    (4, 320, '2x640', 1, 0.3): ((0, 0.5, 14), [2.753864e-03], [14]),
    (4, 320, '2x640', 1, 0.7): ((0, 0.5, 14), [6.229791e-04], [14]),
    (4, 320, '2x640', 5, 0.3): ((0, 0.5, 14), [2.753864e-03, 7.590397e-03, 1.059901e-03, 8.254004e-04, 4.078243e-04], [14, 2, 14, 14, 3]),
    (4, 320, '2x640', 5, 0.7): ((0, 0.5, 14), [6.229791e-04, 1.956313e-03, 1.737680e-03, 3.905701e-04, 2.434576e-03], [14, 3, 14, 14, 4]),
    (4, 512, '1x320', 1, 0.3): ((2, 1.0, 14), [1.656411e-03], [14]),
    (4, 512, '1x320', 1, 0.7): ((2, 0.5, 14), [1.979116e-04], [14]),
    (4, 512, '1x320', 5, 0.3): ((2, 1.0, 14), [1.656411e-03, 6.703267e-04, 1.957776e-03, 7.265611e-03, 2.517336e-03], [14, 2, 2, 2, 2]),
    (4, 512, '1x320', 5, 0.7): ((0, 0.5, 14), [3.387597e-03, 7.687169e-04, 6.585025e-04, 3.308709e-04, 4.306147e-04], [3, 2, 14, 5, 14]),
    (4, 512, '2x640', 1, 0.3): ((2, 1.0, 14), [1.829526e-03], [14]),
    (4, 512, '2x640', 1, 0.7): ((2, 1.0, 14), [9.979701e-04], [14]),
    (4, 512, '2x640', 5, 0.3): ((2, 1.0, 14), [1.829526e-03, 8.740873e-04, 3.746154e-03, 1.283202e-02, 2.862042e-03], [14, 2, 2, 2, 2]),
    (4, 512, '2x640', 5, 0.7): ((2, 1.0, 14), [9.979701e-04, 2.453667e-03, 5.945005e-03, 2.804358e-03, 5.695774e-03], [14, 2, 2, 2, 2]),
    (8, 320, '1x320', 1, 0.3): ((3, 0.5, 14), [2.085154e-03], [6]),
    (8, 320, '1x320', 1, 0.7): ((3, 0.5, 14), [2.995305e-04], [7]),
    (8, 320, '1x320', 5, 0.3): ((0, 0.5, 14), [7.272611e-03, 6.639907e-04, 2.027658e-03, 4.513992e-04, 1.380760e-03], [2, 14, 3, 3, 8]),
    (8, 320, '1x320', 5, 0.7): ((1, 0.5, 14), [6.833800e-03, 9.969093e-05, 1.721767e-04, 1.008112e-03, 3.985387e-03], [3, 14, 3, 6, 3]),
    (8, 320, '2x640', 1, 0.3): ((2, 0.5, 14), [4.976570e-04], [14]),
    (8, 320, '2x640', 1, 0.7): ((2, 0.5, 14), [2.810743e-04], [14]),
    (8, 320, '2x640', 5, 0.3): ((0, 0.5, 14), [1.345773e-03, 1.725633e-04, 1.977658e-03, 2.846555e-03, 5.388357e-05], [3, 14, 3, 3, 7]),
    (8, 320, '2x640', 5, 0.7): ((2, 1.0, 14), [2.860546e-03, 1.029140e-03, 1.327448e-02, 7.343068e-04, 2.524357e-03], [3, 2, 2, 14, 3]),
    (8, 512, '1x320', 1, 0.3): ((0, 0.5, 14), [1.535480e-04], [6]),
    (8, 512, '1x320', 1, 0.7): ((1, 0.5, 14), [2.000565e-04], [14]),
    (8, 512, '1x320', 5, 0.3): ((1, 0.5, 14), [9.978205e-06, 3.868810e-04, 3.402419e-03, 1.041363e-03, 6.784655e-04], [14, 4, 14, 4, 3]),
    (8, 512, '1x320', 5, 0.7): ((0, 1.0, 14), [8.969951e-03, 3.534711e-03, 1.112782e-04, 2.556819e-03, 6.125123e-04], [2, 2, 14, 2, 2]),
    (8, 512, '2x640', 1, 0.3): ((1, 0.5, 14), [1.560805e-03], [14]),
    (8, 512, '2x640', 1, 0.7): ((0, 0.5, 14), [1.135799e-03], [14]),
    (8, 512, '2x640', 5, 0.3): ((0, 1.0, 14), [7.302837e-04, 6.324301e-04, 2.249456e-04, 1.186106e-03, 2.750492e-03], [2, 3, 9, 2, 2]),
    (8, 512, '2x640', 5, 0.7): ((0, 1.0, 14), [3.229610e-03, 1.612019e-04, 1.238776e-04, 5.863703e-04, 3.411304e-04], [3, 7, 10, 3, 3]),
}


@pytest.mark.parametrize("case", SEARCH_GRID, ids=lambda c: "K%d-D%d-%s-B%d-w%s" % c)
def test_fused_beams_against_the_float64_restatement(hb, case):
    K, D, name, B, lam = case
    cand, margins, steps = SEARCH_CASES[case]
    cfg, w, lm_cfg, lm_w, enc, lens, L = _search_case(case, cand)
    net, lm = _e2e_module(cfg, w), _lm_module(lm_cfg, lm_w)
    enc_d = _cuda(enc)
    hb.LAUNCHES.clear()
    toks, scores = net.decoder.recognize_beams(enc_d, lens, L, K, nbest=True, lm=lm, lm_weight=lam)
    assert hb.LAUNCHES["beam_lm_step"] > 0 and hb.LAUNCHES["beam_step"] == 0
    best, best_score = net.decoder.recognize_beams(enc_d, lens, L, K, lm=lm, lm_weight=lam)
    assert torch.equal(best, toks[:, 0]) and torch.equal(best_score, scores[:, 0])
    ref = _restate(case, cand)
    np.testing.assert_allclose([min(r["margins"]) for r in ref], margins, rtol=1e-6)          # the recorded restatement
    assert [r["steps"] for r in ref] == steps
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


def _plain_case():
    cfg, w = _e2e_weights(320, 34, 128, 43, 0.5)
    lm_cfg, lm_w = _lm_weights("1x320", 34, 44)
    enc = _enc_arrays(3, 128, (20, 14, 9), 3)
    return _e2e_module(cfg, w), _lm_module(lm_cfg, lm_w), _cuda(enc), [20, 14, 9]


def test_no_lm_and_weight_zero_take_the_plain_path(hb):
    net, lm, enc, lens = _plain_case()
    hb.LAUNCHES.clear()
    want = net.decoder.recognize_beams(enc, lens, 10, 4, nbest=True)
    per_step = hb.LAUNCHES["beam_launch"] / hb.LAUNCHES["beam_step"]
    for kw in (dict(lm=None, lm_weight=0.7), dict(lm=lm, lm_weight=0.0), dict(lm=None)):
        hb.LAUNCHES.clear()
        got = net.decoder.recognize_beams(enc, lens, 10, 4, nbest=True, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert hb.LAUNCHES["beam_lm_step"] == 0 and hb.LAUNCHES["beam_launch"] / hb.LAUNCHES["beam_step"] == per_step
        assert hb.LAUNCHES["beam_launch"] <= 7 * hb.LAUNCHES["beam_step"]
    e2e = net.recognize_beams                                            # the keywords reach E2E.recognize_beams too
    xs = torch.randn(2, 40, 80, device="cuda")
    a = e2e(xs, [40, 31], 6, 2, lm=lm, lm_weight=0.0)
    b = e2e(xs, [40, 31], 6, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_mismatched_lm_is_refused_before_any_launch(hb):
    net, lm, enc, lens = _plain_case()
    other = _lm_module(*_lm_weights("1x320", 35, 44))
    hb.LAUNCHES.clear()
    with pytest.raises(ValueError):
        net.decoder.recognize_beams(enc, lens, 10, 4, lm=other, lm_weight=0.5)
    lm.eos = 3
    with pytest.raises(ValueError):
        net.decoder.recognize_beams(enc, lens, 10, 4, lm=lm, lm_weight=0.5)
    assert sum(hb.LAUNCHES.values()) == 0


def test_the_lm_matters(hb):
    """An LM whose output bias favours one token strongly: the best hypothesis of a fixed net changes the way the
    restatement says (a fused path that ignored lm_logits would return the plain hypothesis)."""
    K, L, V, fav = 4, 8, 34, 9
    cfg, w = _e2e_weights(320, V, 128, 43, 0.0)
    lm_cfg, lm_w = _lm_weights("1x320", V, 44, bias=(fav, 12.0))
    net, lm = _e2e_module(cfg, w), _lm_module(lm_cfg, lm_w)
    lens = [20, 14]
    enc = _enc_arrays(2, 128, lens, 3)
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}      # noqa: E731
    plain, _ = net.decoder.recognize_beams(_cuda(enc), lens, L, K)
    fused, _ = net.decoder.recognize_beams(_cuda(enc), lens, L, K, lm=lm, lm_weight=1.0)
    ref = beam_lm_ref.decode(t(w), t(lm_w), torch.from_numpy(enc), lens, L, K, 1.0)
    ref_plain = beam_ref.decode(t(w), torch.from_numpy(enc), lens, L, K)
    for b in range(2):
        assert min(ref[b]["margins"]) > MARGIN and min(ref_plain[b]["margins"]) > MARGIN
        assert tb._cut(fused[b].tolist()) == ref[b]["hyps"][0][0]
        assert tb._cut(plain[b].tolist()) == ref_plain[b]["hyps"][0][0]
        assert tb._cut(fused[b].tolist()) != tb._cut(plain[b].tolist())
        assert tb._cut(fused[b].tolist()).count(fav) > tb._cut(plain[b].tolist()).count(fav)


def test_fused_launches_per_step(hb):
    for name in ("1x320", "2x640"):
        cfg, w = _e2e_weights(320, 34, 128, 43, 0.0)
        net, lm = _e2e_module(cfg, w), _lm_module(*_lm_weights(name, 34, 44))
        enc = _cuda(_enc_arrays(2, 128, (20, 14), 3))
        hb.LAUNCHES.clear()
        net.decoder.recognize_beams(enc, [20, 14], 10, 4, lm=lm, lm_weight=0.5)
        assert hb.LAUNCHES["beam_lm_step"] > 0 and hb.LAUNCHES["beam_step"] == 0 and hb.LAUNCHES["beam_launch"] == 0
        assert hb.LAUNCHES["beam_lm_launch"] <= (8 + lm.n_layers) * hb.LAUNCHES["beam_lm_step"]


def test_fused_memory_does_not_grow_with_max_dec_timesteps(hb):
    cfg, w = _e2e_weights(512, 34, 512, 41, -30.0, out_scale=1.0)      # no <EOS>: every step runs
    net, lm = _e2e_module(cfg, w), _lm_module(*_lm_weights("2x640", 34, 42, out_scale=1.0))
    lens = [60, 50, 40, 30]
    enc = _cuda(_enc_arrays(4, 512, lens, 9))
    peaks = []
    for L in (50, 400):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pred, _ = net.decoder.recognize_beams(enc, lens, L, 4, lm=lm, lm_weight=0.5)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert pred.shape == (4, L)
        del pred
    assert abs(peaks[1] - peaks[0]) < 16 * 2 ** 20, peaks


def test_solver_test_with_lm_weight(hb, tmp_path, monkeypatch):
    import test_solver_gpu as ts
    from dataloader import get_data_loader
    from solver import Solver
    root = str(tmp_path)
    vocab = ts._vocab()
    ts._write_data(root, vocab)
    monkeypatch.chdir(root)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = ts._config(root)
    solver = Solver(cfg)
    sd, jsd = solver.model.state_dict(), {k: v.clone() for k, v in solver.judge.state_dict().items()}

    def run(**extra):
        solver.config = dict(cfg, **extra)
        solver.test(state_dict=sd, judge_state_dict=jsd if "lm_weight" in extra else None)
        with open(os.path.join(root, "eval.txt")) as f:
            return f.read().splitlines()

    def direct(K, **kw):
        loader = get_data_loader(solver._dataset("eval", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
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
    assert run(lm_weight=0) == plain_lines                                      # the key at 0: the lines without it
    hb.LAUNCHES.clear()
    lines = run(beam_size=4, beam_length_penalty=0.5, lm_weight=0.6)
    assert hb.LAUNCHES["beam_lm_step"] > 0
    assert lines == direct(4, length_penalty=0.5, lm=solver.judge, lm_weight=0.6)
    assert solver.judge.training and solver.model.training
    hb.LAUNCHES.clear()
    greedy_fused = run(lm_weight=0.6)                                            # beam_size 1: LM-fused greedy
    assert hb.LAUNCHES["beam_lm_step"] > 0
    assert greedy_fused == direct(1, lm=solver.judge, lm_weight=0.6)
    # the judge is read from the checkpoint beside the recogniser's when no state dict is passed
    solver.save_judge(cfg["load_judge_path"])
    solver.config = dict(cfg, beam_size=4, beam_length_penalty=0.5, lm_weight=0.6)
    solver.test(state_dict=sd)
    with open(os.path.join(root, "eval.txt")) as f:
        assert f.read().splitlines() == lines
