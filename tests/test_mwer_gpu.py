"""MWER training on the GPU: the two kernels of csrc/mwer.hip over a grid of shapes and inputs against the float64
restatement (tests/mwer_ref.py), per element; ops.mwer_loss against the same loss composed from ops.label_logprob and torch;
Decoder.score_hypotheses_grad against score_hypotheses; E2E.mwer_forward and the Solver's step end to end.

Allowance of the kernel grid, per output tensor (the project's rule): max(4 x the float32 restatement's
own error against float64 on the same input, 8 * 2^-24 x the tensor's largest magnitude).  Every case prints its worst error /
allowance with the `mwer-parity` tag (`pytest -s`; profiles/mwer_parity.txt holds one run)."""
import numpy as np
import pytest
import torch

import mwer_ref as R
import synth
from test_hip_parity import _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 2
OUTPUTS = ("loss", "risk", "post", "seq_logp", "dlogits")


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


# ------------------------------------------------------------------------------------------------ the kernel grid
_REFS = {}


def _refs(c):
    """The case, its float64 and float32 restatements: computed once, shared, left unchanged."""
    key = R.case_id(c)
    if key not in _REFS:
        case = R.make_case(c)
        args = (case["logits"], case["tokens"], case["npos"], case["err"], case["B"], case["scale"], case["g"])
        _REFS[key] = (case, R.run_f64(*args), R.run_f32(*args))
    return _REFS[key]


def _launch(hb, case):
    """asr_mwer_fwd_f32 + asr_mwer_bwd_f32 on the case.  The logits are a [L, R, V] view of a [L, R, V + 3] buffer whose extra
    columns, whose positions l >= n_r and whose unused rows are NaN: nothing of them may be read.  dlogits is NaN before the
    launch.  -> dict of CPU tensors."""
    B, K, L, V = case["B"], case["K"], case["L"], case["V"]
    Rr = B * K
    n = np.clip(case["npos"], 0, L)
    buf = torch.full((L, Rr, V + 3), float("nan"))
    buf[:, :, :V] = torch.from_numpy(case["logits"])
    buf[torch.from_numpy(np.arange(L)[:, None] >= n[None, :])] = float("nan")
    buf = buf.to(DEV)
    logits = buf[:, :, :V]
    tokens, npos, err = (torch.from_numpy(case[k]).to(DEV) for k in ("tokens", "npos", "err"))
    f32 = dict(device=DEV, dtype=torch.float32)
    out = dict(seq_logp=torch.full((Rr,), float("nan"), **f32), post=torch.full((Rr,), float("nan"), **f32),
               coef=torch.full((Rr,), float("nan"), **f32), risk=torch.full((B,), float("nan"), **f32),
               loss=torch.full((1,), float("nan"), **f32))
    ws = torch.full((L * Rr,), float("nan"), **f32)
    hb.mwer_fwd(logits, tokens, npos, err, B, case["scale"], out["seq_logp"], out["post"], out["coef"], out["risk"], out["loss"], ws)
    dz = torch.full((L, Rr, V), float("nan"), **f32)
    g = torch.tensor([case["g"]], **f32)
    hb.mwer_bwd(logits, tokens, npos, out["coef"], B, g, case["scale"], dz)
    out["dlogits"] = dz
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("c", R.GRID, ids=R.case_id)
def test_kernels_against_float64(hb, c):
    case, r64, r32 = _refs(c)
    got = _launch(hb, case)
    B, K, L, V = case["B"], case["K"], case["L"], case["V"]
    n = np.clip(case["npos"], 0, L)
    ratios = {}
    for name in OUTPUTS:
        g = got[name].numpy().astype(np.float64).reshape(r64[name].shape)
        assert np.isfinite(g).all(), name
        allow = R.allowance(r64[name], r32[name])
        err = float(np.abs(g - r64[name]).max())
        ratios[name] = err / allow if allow > 0 else (0.0 if err == 0 else float("inf"))
    print("mwer-parity %-46s worst error / allowance  %s" % (
        R.case_id(c), "  ".join("%s %.3f" % (k, ratios[k]) for k in OUTPUTS)))
    # masked positions, unused rows: exact zeros, bit for bit
    dz = got["dlogits"].numpy().view(np.uint32)
    masked = np.arange(L)[:, None] >= n[None, :]
    assert not dz[masked].any(), "a masked position of dlogits is not +0.0"
    unused = case["npos"] <= 0
    for name in ("seq_logp", "post", "coef"):
        assert not got[name].numpy().view(np.uint32)[unused].any(), name
    live_any = (case["npos"] > 0).reshape(B, K).any(1)
    assert not got["risk"].numpy().view(np.uint32)[~live_any].any()
    if c[7] == "equal" or K == 1:
        assert not (got["dlogits"].numpy() != 0).any() and float(got["loss"]) == 0.0
    if c[4] == "far":
        assert (got["post"].numpy() == 0).any() and (r64["post"] > 0).all(), "some posteriors are meant to underflow"
    for name in OUTPUTS:
        assert ratios[name] <= 1.0, "%s: %s is %.3f allowances off" % (R.case_id(c), name, ratios[name])


@pytest.mark.parametrize("c", [R.GRID[2], R.GRID[3], R.GRID[12]], ids=R.case_id)
def test_two_launches_give_the_same_bits(hb, c):
    case, _, _ = _refs(c)
    runs = []
    for det in (False, True, False, True):
        if det:
            with hb.deterministic():
                runs.append(_launch(hb, case))
        else:
            runs.append(_launch(hb, case))
    for other in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k].view(torch.int32), other[k].view(torch.int32)), k


def test_refusals_on_the_device(hb):
    import ops
    z = torch.zeros(2, 17, 5, device=DEV)
    tok = torch.zeros(2, 17, dtype=torch.long, device=DEV)
    n = torch.ones(17, dtype=torch.int32, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.mwer_loss(z, tok, n, n, 1.0, n_utts=1)                                # K = 17
    with pytest.raises(RuntimeError):
        ops.mwer_loss(z, tok, n, n, 1.0 / 3, n_utts=3)                            # 17 rows are not 3 x K


# ------------------------------------------------------------------------------------------------ node and model
def _tiny():
    """The tiny model of tests/test_beam_ctc_gpu.py (its _modules helper: output layer scaled, a CTC head), three references
    and a 4-best list from its own search with the last slot of utterance 0 marked unused."""
    import test_beam_ctc_gpu as tbc
    net, _, xs, ilens, L = tbc._modules((0, 0.0, 14))
    rs = np.random.RandomState(77)
    ys = [torch.from_numpy(rs.randint(3, synth.TINY["output_dim"], size=n)).cuda() for n in (5, 4, 3)]
    with torch.no_grad():
        enc_h, enc_lens = net.encoder(xs, ilens)
        tokens, _ = net.decoder.recognize_beams(enc_h, enc_lens, L, 4, nbest=True)
    hyp_len = ((tokens == EOS).int().cumsum(2) == 0).sum(2).int()
    hyp_len[0, 3] = -1
    return net, xs, ilens, ys, L, tokens, hyp_len


def _composed(ops, logits, tok_lb, npos, err, B):
    """The loss from existing parts: ops.label_logprob, then torch with autograd."""
    L, Rr, _ = logits.shape
    K = Rr // B
    logp = ops.label_logprob(logits, tok_lb)
    mask = torch.arange(L, device=DEV).unsqueeze(1) < npos.unsqueeze(0)
    s = torch.where(mask, logp, torch.zeros((), device=DEV)).sum(0).view(B, K)
    live = (npos > 0).view(B, K)
    post = torch.softmax(torch.where(live, s, torch.full_like(s, -float("inf"))), dim=1)
    e = err.view(B, K).float() * live
    d = torch.where(live, e - e.sum(1, keepdim=True) / live.sum(1, keepdim=True), torch.zeros_like(e))
    return (post * d).sum(1).sum() / B


def test_node_against_the_composition_from_existing_ops(hb):
    import ops
    net, xs, ilens, ys, L, tokens, hyp_len = _tiny()
    B, K = tokens.shape[:2]
    err = torch.tensor([3, 0, 5, 9, 1, 4, 2, 2, 6, 0, 1, 7], dtype=torch.int32, device=DEV)
    params = [p for p in net.parameters() if not any(p is q for q in net.ctc_lo.parameters())]
    res = []
    for fused in (True, False):
        net.zero_grad()
        enc_h, enc_lens = net.encoder(xs, ilens)
        _, logits, tok_lb, npos = net.decoder.score_hypotheses_grad(enc_h, enc_lens, tokens, hyp_len, scores=False)
        if fused:
            loss, parts = ops.mwer_loss(logits, tok_lb, npos, err, 1.0 / B)
            assert not any(v.requires_grad for v in parts.values()) and loss.requires_grad
        else:
            loss = _composed(ops, logits, tok_lb, npos, err, B)
        loss.backward()
        res.append((loss.detach().clone(), [p.grad.detach().clone() for p in params]))
    assert float(res[1][0]) != 0
    _close(res[0][0], res[1][0], what="loss")
    for (name, _), a, b in zip([(n, p) for n, p in net.named_parameters() if not n.startswith("ctc_lo")], res[0][1], res[1][1]):
        assert float(b.abs().max()) > 0, name
        _close(a, b, what=name)


# hb.LAUNCHES of Decoder.score_hypotheses on the 3 x 4 hypotheses of _tiny(), recorded on the commit before MWER training
SCORE_LAUNCHES = {"dec_fwd_step": 1}
# ... and the bits of its scores there
SCORE_BITS = [[-1078778162, -1068909274, -1066698134, -1078778162], [-1078843066, -1068907850, -1066722701, -1063609464],
              [-1078890168, -1068897036, -1066742093, -1063586960]]
# ... and of one Solver.sup_train_one_iteration on the tiny batch (test_deterministic_gpu._solver, dropout 0)
SUP_LAUNCHES = {"lstm_fwd_step": 2, "dec_fwd_step": 1, "dec_bwd_step": 1, "lstm_bwd_step": 2}


def test_scoring_pass_with_and_without_the_graph(hb):
    net, xs, ilens, ys, L, tokens, hyp_len = _tiny()
    with torch.no_grad():
        enc_h, enc_lens = net.encoder(xs, ilens)
    hb.LAUNCHES.clear()
    att, tok_out, mask = net.decoder.score_hypotheses(enc_h, enc_lens, tokens.int(), hyp_len)
    print("mwer-launches score_hypotheses %r" % (dict(hb.LAUNCHES),))
    assert dict(hb.LAUNCHES) == SCORE_LAUNCHES
    assert att.view(torch.int32).cpu().tolist() == SCORE_BITS
    att_g, logits, tok_lb, npos = net.decoder.score_hypotheses_grad(enc_h, enc_lens, tokens, hyp_len)
    assert att_g.requires_grad and logits.requires_grad
    _close(att_g, att, what="scores")
    assert torch.equal(tok_lb.t(), tok_out) and torch.equal(npos, torch.where(hyp_len.view(-1) >= 0, hyp_len.view(-1) + 1, 0).int())
    assert torch.equal(mask.sum(1).int(), hyp_len.view(-1).clamp(min=0) + 1)


def test_mwer_forward_end_to_end(hb):
    import parallel
    import utils
    net, xs, ilens, ys, L, _, _ = _tiny()
    net.train()
    B, K = len(ys), 4
    np.random.seed(3)
    hb.LAUNCHES.clear()
    loss = net.mwer_forward(xs, ilens, ys, K, ce_weight=0.01, max_dec_timesteps=L)
    assert hb.LAUNCHES["mwer"] == 2 and hb.LAUNCHES["beam_step"] > 0
    m = net.last_mwer
    tokens, hyp_len, err = m["tokens"].cpu().tolist(), m["hyp_len"].cpu().tolist(), m["err"].cpu().tolist()
    refs = [y.cpu().tolist() for y in ys]
    live = 0
    for b in range(B):
        for k in range(K):
            if hyp_len[b][k] < 0:
                continue
            live += 1
            hyp = tokens[b][k][:tokens[b][k].index(EOS)] if EOS in tokens[b][k] else tokens[b][k]
            assert len(hyp) == hyp_len[b][k]
            assert err[b * K + k] == utils.edit_distance(hyp, refs[b]), (b, k)
    assert live >= B and len(set(err)) > 1
    post = m["post"].view(B, K).double().cpu()
    assert float((post.sum(1) - 1).abs().max()) <= 4 * K * 2.0 ** -24
    assert float(post.view(-1)[m["hyp_len"].view(-1).cpu() < 0].abs().sum()) == 0
    np.random.seed(3)
    _, lp, _, _ = net(xs, ilens, ys)
    l_ce = parallel.local_loss(lp, dict(b_global=B))
    want = m["risk"].double().mean() + 0.01 * l_ce.detach().double()
    got = float(loss.detach())
    assert abs(got - float(want)) <= 1e-5 * abs(float(want)) + 1e-6, (got, float(want))
    # the gradient reaches the encoder and every decoder parameter
    net.zero_grad()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in net.encoder.parameters())
    # K = 1: nothing to rank - the loss is the cross-entropy term alone
    np.random.seed(3)
    one = net.mwer_forward(xs, ilens, ys, 1, ce_weight=0.01, max_dec_timesteps=L)
    assert float(net.last_mwer["mwer"]) == 0.0 and abs(float(one.detach()) - 0.01 * float(l_ce)) <= 1e-5 * abs(float(l_ce))


def _mwer_solver(tmp_path, monkeypatch, **over):
    import test_deterministic_gpu as td
    return td._solver(str(tmp_path), monkeypatch, synth.TINY, synth.TINY_LM, **over)


def _tiny_batch(dev):
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    tokens, lengths = R.fixed_hyps(ys, 4, 9, EOS)
    return (torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys],
            (torch.from_numpy(tokens).to(dev), torch.from_numpy(lengths).to(dev)))


def test_ten_steps_on_frozen_hypotheses_lower_the_risk(hb, tmp_path, monkeypatch):
    """Plain descent on a smooth function: the learning rate is the one at which the float64 oracle alone does it
    (tests/test_mwer_cpu.py)."""
    solver, dev = _mwer_solver(tmp_path, monkeypatch, mwer_beam=4, learning_rate=R.DESCENT_LR)
    xs, ilens, ys, hyps = _tiny_batch(dev)
    risks = []
    for _ in range(R.DESCENT_STEPS + 1):
        loss, risk = solver.mwer_train_one_iteration(xs, ilens, ys, hyps=hyps)
        risks.append(risk)
    solver.flush()
    risks = [float(r) for r in risks]
    print("mwer-descent mean risk over the steps: " + " ".join("%.5f" % r for r in risks))
    assert risks[-1] < risks[0] and risks[0] != 0
    with pytest.raises(ValueError, match="one process"):
        solver.world = 2
        solver.mwer_train_one_iteration(xs, ilens, ys, hyps=hyps)


def test_a_step_reproduces_bit_for_bit_in_deterministic_mode(hb, tmp_path, monkeypatch):
    import test_deterministic_gpu as td

    def steps(solver, dev):
        xs, ilens, ys, hyps = _tiny_batch(dev)
        loss, _ = solver.mwer_train_one_iteration(xs, ilens, ys, hyps=hyps)
        yield "mwer step", loss, solver.gen_opt
    td._run_twice(tmp_path, monkeypatch, synth.TINY, synth.TINY_LM, steps, dict(mwer_beam=4))


def test_supervised_step_launches_are_the_ones_before(hb, tmp_path, monkeypatch):
    solver, dev = _mwer_solver(tmp_path, monkeypatch)
    assert "mwer_beam" not in solver.config
    xs, ilens, ys, _ = _tiny_batch(dev)
    np.random.seed(4)
    hb.LAUNCHES.clear()
    solver.sup_train_one_iteration(xs, ilens, ys, 1.0)
    solver.flush()
    print("mwer-launches sup step %r" % (dict(hb.LAUNCHES),))
    assert "mwer" not in hb.LAUNCHES
    assert dict(hb.LAUNCHES) == SUP_LAUNCHES
