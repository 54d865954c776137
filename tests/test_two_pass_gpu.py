"""Two-pass decoding on the GPU (E2E.recognize_two_pass, E2E.recognize_ctc_beams, Solver.test with `two_pass_decode`;
DESIGN 4.18) on the tiny model of tiny_e2e.npz with a CTC head (the modules of tests/test_beam_ctc_gpu.py): the rescoring
pass against E2E.forward and LM.forward on the same hypotheses, the combination and ranking against a host restatement from
the parts, w = 1 and K = 1, and the solver switch."""
import os

import numpy as np
import pytest
import torch

import test_beam_ctc_gpu as tb
from test_hip_parity import _close

pytestmark = pytest.mark.gpu
EOS = 2
CAND = (0, 0.0, 14)


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture(scope="module")
def tiny(hb):
    net, lm, xs, ilens, _ = tb._modules(CAND)
    return net, lm, xs, ilens


def _parts(net):
    p = net.last_two_pass
    return {k: (None if v is None else v.cpu().numpy()) for k, v in p.items()}


def _hyps(p, b, k):
    n = int(p["hyp_len"][b, k])
    return None if n < 0 else [int(c) for c in p["hyp"][b, k, :n]]


def test_rescoring_pass_against_the_teacher_forced_forwards(hb, tiny):
    """att[b][k] is what E2E.forward gives hypothesis k of utterance b (the sum of its len + 1 token log-probabilities) in a
    batch of the same padded T', lm[b][k] what LM.forward gives it: within the allowance of the teacher-forced parity tests
    (tests/test_hip_parity.py::_close, rtol 1e-3 of the largest magnitude + 1e-5)."""
    net, lm, xs, ilens = tiny
    K = 4
    hb.LAUNCHES.clear()
    tokens, scores = net.recognize_two_pass(xs, ilens, K, ctc_weight=0.4, nbest=True, lm=lm, lm_weight=0.5)
    assert hb.LAUNCHES["ctc_beam"] == 1 and hb.LAUNCHES["ctc_beam_launch"] == 2
    p = _parts(net)
    B, _, T = p["hyp"].shape
    assert tokens.shape == (B, K, T + 1) and scores.shape == (B, K) and tokens.dtype == torch.long and tokens.is_cuda
    assert (p["hyp_len"][:, 0] >= 0).all() and (p["hyp_len"] > 0).any()
    att_ref, lm_ref = np.zeros((B, K)), np.zeros((B, K))
    head_weight, net.ctc_weight = net.ctc_weight, 0.0            # (the forward without its CTC loss term: hypotheses may be empty)
    try:
        with torch.no_grad():
            lps = []
            for k in range(K):
                ys = [torch.tensor(_hyps(p, b, k) or [], dtype=torch.long, device="cuda") for b in range(B)]
                lps.append(net(xs, ilens, ys, tf_rate=1.0, olength=T + 1)[1])
    finally:
        net.ctc_weight = head_weight
    with torch.no_grad():
        for k in range(K):
            hyps = [_hyps(p, b, k) or [] for b in range(B)]
            ys = [torch.tensor(h, dtype=torch.long, device="cuda") for h in hyps]
            lp = lps[k]
            lp_lm, _, _ = lm(ys)
            for b, h in enumerate(hyps):
                att_ref[b, k] = float(lp[b, :len(h) + 1].double().sum())
                lm_ref[b, k] = float(lp_lm[b, :len(h) + 1].double().sum())
    live = p["hyp_len"] >= 0
    _close(p["att"][live], att_ref[live], what="att")
    _close(p["lm"][live], lm_ref[live], what="lm")
    print("att: max abs err %.3g at scale %.3g; lm: %.3g at %.3g" % (
        np.abs(p["att"][live] - att_ref[live]).max(), np.abs(att_ref[live]).max(),
        np.abs(p["lm"][live] - lm_ref[live]).max(), np.abs(lm_ref[live]).max()))


@pytest.mark.parametrize("w,lmw,alpha", [(0.4, 0.0, 0.0), (0.4, 0.5, 0.0), (0.0, 0.7, 0.0), (0.3, 0.5, 0.5)])
def test_ranking_is_the_combination_of_the_parts(hb, tiny, w, lmw, alpha):
    """(1 - w) att + w ctc + lm_weight lm in fp32, every operation rounded on its own, over (len + 1)**alpha; ranked with ties
    to the lower k; unused slots at -inf behind the rest."""
    net, lm, xs, ilens = tiny
    K = 4
    tokens, scores = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, length_penalty=alpha, nbest=True,
                                            lm=lm if lmw else None, lm_weight=lmw)
    p = _parts(net)
    f = np.float32
    total = (p["att"].astype(f) * f(f(1.0) - f(w))).astype(f) + (p["ctc"].astype(f) * f(w)).astype(f)
    if lmw:
        total = (total + (p["lm"].astype(f) * f(lmw)).astype(f)).astype(f)
    else:
        assert p["lm"] is None
    live = p["hyp_len"] >= 0
    got = scores.cpu().numpy()
    if alpha:
        total = total / np.power((np.maximum(p["hyp_len"], 0) + 1).astype(f), f(alpha))
    total = np.where(live, total, -np.inf).astype(f)
    order = np.argsort(-total.astype(np.float64), axis=1, kind="stable")
    want = np.take_along_axis(total, order, axis=1)
    if alpha:                                                    # (the power is the device's: an ulp of it may differ)
        np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=4 * np.finfo(f).eps)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        order = p["order"]
    else:
        assert np.array_equal(got, want) and np.array_equal(p["order"], order)
    tok = tokens.cpu().numpy()
    for b in range(tok.shape[0]):
        for r in range(K):
            h = _hyps(p, b, int(order[b, r])) or []
            assert tok[b, r].tolist() == h + [EOS] * (tok.shape[2] - len(h))
    best, best_score = net.recognize_two_pass(xs, ilens, K, ctc_weight=w, length_penalty=alpha, lm=lm if lmw else None,
                                              lm_weight=lmw)
    assert torch.equal(best, tokens[:, 0]) and torch.equal(best_score, scores[:, 0])


def test_weight_one_and_width_one_return_the_search(hb, tiny):
    net, lm, xs, ilens = tiny
    ids, sc = net.recognize_ctc_beams(xs, ilens, 4, nbest=True)
    top, top_sc = net.recognize_ctc_beams(xs, ilens, 4)
    assert top == [u[0] for u in ids] and top_sc == [u[0] for u in sc]
    assert all(len(u) >= 1 and all(a >= b for a, b in zip(s, s[1:])) for u, s in zip(ids, sc))
    tokens, scores = net.recognize_two_pass(xs, ilens, 4, ctc_weight=1.0, nbest=True)
    tok, got = tokens.cpu().numpy(), scores.cpu().numpy()
    for b, (u, s) in enumerate(zip(ids, sc)):
        for r, h in enumerate(u):
            assert tok[b, r].tolist() == h + [EOS] * (tok.shape[2] - len(h))
            assert got[b, r] == np.float32(s[r])
        assert np.isneginf(got[b, len(u):]).all()
    one, _ = net.recognize_ctc_beams(xs, ilens, 1)
    for w in (0.0, 0.5, 1.0):
        best, _ = net.recognize_two_pass(xs, ilens, 1, ctc_weight=w, lm=lm, lm_weight=0.3)
        for b, h in enumerate(one):
            assert best[b].tolist() == h + [EOS] * (best.shape[1] - len(h))


def test_refusals_come_before_any_launch(hb, tiny):
    import model as M
    import synth
    net, lm, xs, ilens = tiny
    plain = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY).cuda()
    hb.LAUNCHES.clear()
    for call in (lambda: plain.recognize_two_pass(xs, ilens, 4), lambda: plain.recognize_ctc_beams(xs, ilens, 4),
                 lambda: net.recognize_two_pass(xs, ilens, 0), lambda: net.recognize_two_pass(xs, ilens, 17),
                 lambda: net.recognize_two_pass(xs, ilens, 4, ctc_weight=1.5)):
        with pytest.raises(ValueError):
            call()
    other = M.LM(bos=1, eos=EOS, pad=0, labeldist=None, **dict(synth.TINY_LM, output_dim=synth.TINY["output_dim"] + 1,
                                                                 ls_weight=0.0)).cuda()
    with pytest.raises(ValueError):
        net.recognize_two_pass(xs, ilens, 4, lm=other, lm_weight=0.5)
    lm.eos = 3
    try:
        with pytest.raises(ValueError):
            net.recognize_two_pass(xs, ilens, 4, lm=lm, lm_weight=0.5)
    finally:
        lm.eos = EOS
    assert sum(hb.LAUNCHES.values()) == 0, dict(hb.LAUNCHES)


def test_solver_test_with_two_pass_decode(hb, tmp_path, monkeypatch):
    """Without the key (or with it false) Solver.test issues the launches it issued before; with it the lines are
    recognize_two_pass's; the key does not combine with ctc_greedy_decode or a model without the head."""
    import test_ctc_gpu as tc
    from dataloader import get_data_loader
    root = str(tmp_path)
    solver, dev = tc._solver(root, monkeypatch, ctc_weight=0.3)
    cfg = dict(solver.config)
    assert "two_pass_decode" not in cfg
    sd = {k: v.clone() for k, v in solver.model.state_dict().items()}
    jsd = {k: v.clone() for k, v in solver.judge.state_dict().items()}

    def run(**extra):
        solver.config = dict(cfg, **extra)
        hb.LAUNCHES.clear()
        solver.test(state_dict=sd, judge_state_dict=jsd if extra.get("lm_weight") else None)
        with open(os.path.join(root, "dev.txt")) as f:
            return f.read().splitlines(), dict(hb.LAUNCHES)

    def direct(K, **kw):
        loader = get_data_loader(solver._dataset("dev", None, sort=False), batch_size=1, shuffle=False, drop_last=False)
        solver.model.eval(), solver.judge.eval()
        preds, refs = [], []
        for batch in solver._feed(loader, sharded=False):
            xs, ilens, _ = batch
            p, _ = solver.model.recognize_two_pass(xs, ilens, K, **kw)
            preds += p.cpu().numpy().tolist()
            refs += batch.ys_host
        solver.model.train(), solver.judge.train()
        return solver.ind2sent(preds, refs)[1]

    for extra in (dict(), dict(beam_size=4, ctc_decode_weight=0.4, lm_weight=0.6)):
        run(**extra)                                              # (warm: the first call of a shape may plan its products)
        absent, n_absent = run(**extra)
        off, n_off = run(two_pass_decode=False, **extra)
        assert off == absent and n_off == n_absent and n_absent.get("ctc_beam", 0) == 0
    lines, n = run(two_pass_decode=True, beam_size=4, beam_length_penalty=0.5, ctc_decode_weight=0.4, lm_weight=0.6)
    assert n["ctc_beam"] == 4 and n.get("beam_step", 0) == 0 and n.get("beam_ctc_step", 0) == 0 and n.get("beam_lm_step", 0) == 0
    assert lines == direct(4, ctc_weight=0.4, length_penalty=0.5, lm=solver.judge, lm_weight=0.6)
    assert solver.judge.training and solver.model.training
    lines1, n1 = run(two_pass_decode=True, ctc_decode_weight=0.4)                 # beam_size 1: the search's best, rescored
    assert n1["ctc_beam"] == 4 and lines1 == direct(1, ctc_weight=0.4)
    # best-of-K CER on the device, as the beam-search path reports it
    run(two_pass_decode=True, beam_size=4, ctc_decode_weight=0.4, cer_on_gpu=True)
    assert solver.last_test["best_of_k_cer"] is not None and solver.last_test["best_of_k_cer"] <= solver.last_test["cer"]
    solver.config = dict(cfg, two_pass_decode=True, ctc_greedy_decode=True)
    with pytest.raises(ValueError):
        solver.test(state_dict=sd)
    plain, _ = tc._solver(os.path.join(root, "plain"), monkeypatch)
    plain.config = dict(plain.config, two_pass_decode=True)
    with pytest.raises(ValueError):
        plain.test(state_dict={k: v.clone() for k, v in plain.model.state_dict().items()})
