"""Beam search on the GPU (csrc/beam.hip, ops.beam_search, Decoder.recognize_beams, Solver.test with beam_size): the
select kernel against a stable-sort reference, the reorder kernel as a permutation, K = 1 against greedy decoding, K > 1
against the float64 restatement (tests/beam_ref.py), memory independent of max_dec_timesteps, and the solver switch."""
import os

import numpy as np
import pytest
import torch

import beam_ref
import synth

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


# ------------------------------------------------------------------ select kernel alone
def _select_case(K, V, eos, seed):
    """3 utterances: 0 with a planted tie (beams 0 and 1 identical) and duplicate logits inside rows, 1 with its last
    beam dead, 2 with only beam 0 live (the start of a search)."""
    rs = np.random.RandomState(seed)
    B = 3
    logits = (rs.randn(B, K, V) * 3).astype(np.float32)
    scores = (-rs.rand(B, K) * 4).astype(np.float32)
    logits[:, 0, eos] = logits[:, 0].max(axis=1) + 0.5            # an <EOS> at the top of some rows
    if K > 1:
        logits[0, 1] = logits[0, 0]
        scores[0, 1] = scores[0, 0]
        scores[1, K - 1] = -np.inf
    scores[2, 1:] = -np.inf
    scores[2, 0] = 0.0
    if V > 4:
        logits[:, :, 4] = logits[:, :, 3]                          # ties inside a row
    return logits, scores


def _ref_select(logits, scores, eos):
    """The walk of beam_ref.select on fp32 log-probabilities formed like the kernel's: (x - max) - log(sum exp)."""
    x = logits.astype(np.float32)
    m = x.max(axis=-1, keepdims=True)
    lp = (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    return beam_ref.select(scores.astype(np.float32), lp.astype(np.float32), eos)


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("V", [2, 33, 140, 8192])
@pytest.mark.parametrize("last", [False, True])
def test_select_kernel_against_a_stable_sort(hb, K, V, last):
    eos = EOS if V > EOS else V - 1
    logits, scores = _select_case(K, V, eos, 100 * K + V)
    B, L = logits.shape[0], 6
    t = L - 1 if last else 3
    s = hb.BeamSearch(B, K, V, L, eos, "cuda")
    s.scores.copy_(torch.from_numpy(scores))
    s.nfin[1] = 1                                       # one hypothesis already finished before
    s.fin[1, 0] = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    s.fin_score[1, 0] = -0.25
    s.select(torch.from_numpy(logits.reshape(B * K, V)).cuda(), t)
    torch.cuda.synchronize()
    ndone = 0
    for b in range(B):
        ref = _ref_select(logits[b], scores[b], eos)
        nlive = ref["nlive"]
        assert s.tok_hist[t, b].tolist() == ref["tok"].tolist(), (b, s.tok_hist[t, b], ref["tok"])
        assert s.bp_hist[t, b].tolist() == ref["bp"].tolist(), b
        got_sc = s.scores[b].cpu().numpy()
        np.testing.assert_allclose(got_sc[:nlive], ref["scores"][:nlive], rtol=1e-6, atol=1e-5)
        assert np.isneginf(got_sc[nlive:]).all()
        fin = [(0, 0, 1, 1)] if b == 1 else []
        fsc = [-0.25] if b == 1 else []
        for k, sc in ref["finished"]:
            fin.append((t, k, t + 1, 1))
            fsc.append(sc)
        if last and len(fin) < K:
            for j in range(nlive):
                fin.append((t, j, t + 1, 0))
                fsc.append(ref["scores"][j])
        nf = int(s.nfin[b])
        assert nf == len(fin), (b, nf, fin)
        assert [tuple(r) for r in s.fin[b, :nf].tolist()] == fin
        np.testing.assert_allclose(s.fin_score[b, :nf].cpu().numpy(), np.array(fsc, dtype=np.float32), rtol=1e-6, atol=1e-5)
        done = len(fin) >= K or last or nlive == 0
        assert int(s.done[b]) == int(done)
        ndone += int(done)
    assert int(s.ndone[0]) == ndone
    # a done utterance is left untouched by the next step
    before = [x.clone() for x in (s.scores, s.nfin, s.fin, s.tok_hist)]
    s.done.fill_(1)
    s.select(torch.from_numpy(logits.reshape(B * K, V)).cuda(), min(t + 1, L - 1) if not last else t)
    for a, b_ in zip(before, (s.scores, s.nfin, s.fin, s.tok_hist)):
        assert torch.equal(a, b_)


def test_select_rejects_a_beam_wider_than_16(hb):
    s = hb.BeamSearch(1, 16, 8, 4, EOS, "cuda")
    s.struct.K = 17
    with pytest.raises(RuntimeError, match="code -2"):
        s.select(torch.zeros(16, 8, device="cuda"), 0)


# ------------------------------------------------------------------ reorder kernel
def test_reorder_is_an_exact_permutation(hb):
    B, K, V, L, D, O, E, Tp = 3, 4, 11, 5, 48, 32, 16, 37
    t = 2
    rs = np.random.RandomState(3)
    s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
    bp = rs.randint(0, K, size=(B, K)).astype(np.int32)
    tok = rs.randint(0, V, size=(B, K)).astype(np.int32)
    s.bp_hist[t] = torch.from_numpy(bp).cuda()
    s.tok_hist[t] = torch.from_numpy(tok).cuda()
    s.done[1] = 1                                                   # a done utterance: its rows stay as they are
    KX = D + O + E + 16                                             # a padded row stride
    cuda = lambda a: torch.from_numpy(a).cuda()                     # noqa: E731
    x_src = cuda(rs.randn(B * K, KX).astype(np.float32))
    c_src = cuda(rs.randn(B * K, D).astype(np.float32))
    w_src = cuda(rs.rand(B * K, Tp).astype(np.float32))
    emb = cuda(rs.randn(V, E).astype(np.float32))
    x_dst, c_dst, w_dst = (torch.full_like(a, 7.0) for a in (x_src, c_src, w_src))
    s.reorder(t, x_src, x_dst, c_src, c_dst, w_src, w_dst, emb, D, O)
    torch.cuda.synchronize()
    for b in range(B):
        for j in range(K):
            r, src = b * K + j, b * K + int(bp[b, j])
            if b == 1:
                assert (x_dst[r] == 7.0).all() and (c_dst[r] == 7.0).all() and (w_dst[r] == 7.0).all()
                continue
            assert torch.equal(x_dst[r, :D + O], x_src[src, :D + O])
            assert torch.equal(x_dst[r, D + O:D + O + E], emb[int(tok[b, j])])
            assert (x_dst[r, D + O + E:] == 7.0).all()
            assert torch.equal(c_dst[r], c_src[src]) and torch.equal(w_dst[r], w_src[src])
    with pytest.raises(RuntimeError):                               # in place is refused
        s.reorder(t, x_src, x_src, c_src, c_dst, w_src, w_dst, emb, D, O)


# ------------------------------------------------------------------ the search on decoders
def _decoder_net(D, V, enc_dim, seed, eos_bias=0.0, out_scale=1.0):
    """E2E at decoder width D (attention, context = D, embedding 128, 10 channels of kernel 2*100+1), output_dim V, with
    the output layer scaled (wider logit gaps) and an <EOS> bias (utterances that finish early)."""
    import model as M
    cfg = dict(synth.CFG1, enc_hidden_dim=enc_dim, dec_hidden_dim=D, att_dim=D, att_odim=D, output_dim=V)
    w = synth.e2e_weights(cfg, seed)
    w["decoder.output_layer.weight"] = w["decoder.output_layer.weight"] * out_scale
    w["decoder.output_layer.bias"] = w["decoder.output_layer.bias"] * out_scale
    w["decoder.output_layer.bias"][EOS] += eos_bias
    net = M.E2E(labeldist=synth.labeldist(V, 12), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    return net


def _enc(B, Tp, enc_dim, lens, seed):
    rs = np.random.RandomState(seed)
    enc = rs.randn(B, Tp, enc_dim).astype(np.float32)
    for b, n in enumerate(lens):
        enc[b, n:] = 0.1
    return torch.from_numpy(enc).cuda(), list(lens)


def _cut(row):
    row = list(row)
    return row[:row.index(EOS) + 1] if EOS in row else row


def test_k1_is_greedy_on_the_tiny_model(hb, golden_dir):
    import model as M
    g = dict(np.load(os.path.join(golden_dir, "tiny_e2e.npz")))
    net = M.E2E(labeldist=g["labeldist"], **synth.TINY).cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()})
    net.eval()
    enc, lens = torch.from_numpy(g["enc_h"]).cuda(), g["enc_lens"].tolist()
    pred, scores = net.decoder.recognize_beams(enc, lens, 5, 1)
    assert pred.shape == (3, 5) and pred.dtype == torch.int64 and scores.shape == (3,)
    with torch.no_grad():
        _, _, greedy, _ = net.decoder(enc, lens, ys=None, max_dec_timesteps=5)
    for b in range(3):
        assert _cut(pred[b].tolist()) == _cut(g["gr_pred"][b].tolist()) == _cut(greedy[b].tolist())
        n = len(_cut(pred[b].tolist()))
        assert (pred[b, n:] == EOS).all()
    # E2E.recognize_beams = encoder + decoder
    xs, ilens, _ = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    p2, _ = net.recognize_beams(torch.from_numpy(xs).cuda(), ilens, 5, 1)
    assert [_cut(r) for r in p2.tolist()] == [_cut(r) for r in g["gr_pred"].tolist()]


@pytest.mark.parametrize("D,enc_dim,B,lens", [(320, 128, 4, (40, 33, 27, 12)), (320, 128, 1, (25,)),
                                              (512, 512, 5, (48, 40, 31, 20, 9)), (512, 512, 1, (30,))])
def test_k1_is_greedy(hb, D, enc_dim, B, lens):
    V, L = 34, 24
    net = _decoder_net(D, V, enc_dim, 21, eos_bias=1.0, out_scale=4.0)
    enc, lens = _enc(B, max(lens), enc_dim, lens, 5)
    pred, _ = net.decoder.recognize_beams(enc, lens, L, 1)
    with torch.no_grad():
        logits, _, greedy, _ = net.decoder(enc, lens, ys=None, max_dec_timesteps=L)
    top2 = logits.topk(2, dim=-1).values
    gap = (top2[..., 0] - top2[..., 1]).cpu().numpy()
    checked = 0
    for b in range(B):
        want = _cut(greedy[b].tolist())
        if D == 512 and gap[b, :len(want)].min() <= MARGIN:      # the persistent greedy kernel's logits differ in the last bits
            continue
        assert _cut(pred[b].tolist()) == want, b
        checked += 1
    assert checked >= max(1, (4 * B) // 5)


@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("D,enc_dim,V", [(320, 128, 30), (512, 512, 140)])
@pytest.mark.parametrize("B", [1, 5])
def test_beams_against_the_float64_restatement(hb, K, D, enc_dim, V, B):
    L = 14
    lens = (36, 30, 22, 15, 8)[:B]
    net = _decoder_net(D, V, enc_dim, 31 + K, eos_bias=2.5, out_scale=4.0)
    enc, lens = _enc(B, max(lens), enc_dim, lens, 7 + K)
    toks, scores = net.decoder.recognize_beams(enc, lens, L, K, nbest=True)
    best, best_score = net.decoder.recognize_beams(enc, lens, L, K)
    assert torch.equal(best, toks[:, 0]) and torch.equal(best_score, scores[:, 0])
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    ref = beam_ref.decode(sd, enc.cpu(), lens, L, K)
    qualified = 0
    for b in range(B):
        r = ref[b]
        if min(r["margins"]) <= MARGIN:
            continue
        qualified += 1
        got = [_cut(toks[b, k].tolist()) for k in range(len(r["hyps"]))]
        assert got == [h[0] for h in r["hyps"]], (b, got, r["hyps"])
        np.testing.assert_allclose(scores[b, :len(r["hyps"])].cpu().numpy(), [h[1] for h in r["hyps"]], rtol=1e-4)
    assert qualified >= max(1, (4 * B + 4) // 5), [min(r["margins"]) for r in ref]


def test_memory_does_not_grow_with_max_dec_timesteps(hb):
    net = _decoder_net(512, 34, 512, 41, eos_bias=-30.0)            # no <EOS>: every step runs
    enc, lens = _enc(4, 60, 512, (60, 50, 40, 30), 9)
    peaks = []
    for L in (50, 400):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pred, _ = net.decoder.recognize_beams(enc, lens, L, 4)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert pred.shape == (4, L)
        del pred
    assert abs(peaks[1] - peaks[0]) < 16 * 2 ** 20, peaks


def test_launches_per_step(hb):
    net = _decoder_net(320, 34, 128, 43)
    enc, lens = _enc(2, 20, 128, (20, 14), 3)
    hb.LAUNCHES.clear()
    net.decoder.recognize_beams(enc, lens, 10, 4)
    assert hb.LAUNCHES["beam_step"] > 0
    assert hb.LAUNCHES["beam_launch"] <= 7 * hb.LAUNCHES["beam_step"]


def test_solver_test_with_beam_size(hb, tmp_path, monkeypatch):
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
    sd = solver.model.state_dict()

    def run(**extra):
        solver.config = dict(cfg, **extra)
        solver.test(state_dict=sd)
        with open(os.path.join(root, "eval.txt")) as f:
            return f.read().splitlines()

    greedy_lines = run()
    assert run(beam_size=1) == greedy_lines
    # today's greedy output, formed directly
    loader = get_data_loader(solver._dataset("eval", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
    solver.model.eval()
    preds, beam_preds, refs = [], [], []
    for batch in solver._feed(loader, sharded=False):
        xs, ilens, _ = batch
        with torch.no_grad():
            _, _, p, _ = solver.model(xs, ilens, ys=None, max_dec_timesteps=cfg["max_dec_timesteps"])
        preds += p.cpu().numpy().tolist()
        bp, _ = solver.model.recognize_beams(xs, ilens, cfg["max_dec_timesteps"], 4, length_penalty=0.5)
        beam_preds += bp.cpu().numpy().tolist()
        refs += batch.ys_host
    solver.model.train()
    assert solver.ind2sent(preds, refs)[1] == greedy_lines
    beam_lines = run(beam_size=4, beam_length_penalty=0.5)
    assert beam_lines == solver.ind2sent(beam_preds, refs)[1]
