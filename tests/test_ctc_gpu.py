"""The CTC branch on the GPU: the loss kernels (csrc/ctc.hip) against torch.nn.functional.ctc_loss on the CPU in float64,
then the head in E2E, one Solver step and the checkpoint rule.

Tolerance of the kernel cases: none is written down here.  Every case also runs torch's float32 CPU ctc_loss on the same
inputs; the kernel's worst absolute error against float64 may be at most 4 x that float32 error (another summation order
inside the log-sum-exps, no more), with a floor of 8 fp32 ulps of the tensor's largest magnitude where the float32 error is
about zero.  Each case prints its two ratios (kernel error / allowance)."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

VOCABS = (2, 5, 34, 257)
# label counts per kernel path: up to 64 states one wave per utterance, up to 256 one workgroup with a state per thread,
# beyond that the states are strided over the threads.  2L + 1 straddles the wave at L = 31 / 32 and the workgroup at 127 / 128.
GROUPS = dict(wave=(31,), block=(32, 127), strided=(128, 200))


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _labels(rs, V, n, equal=False):
    if equal or V == 2:
        return [int(rs.randint(1, V))] * n
    return [int(v) for v in rs.randint(1, V, size=n)]


def _utterances(V, group, seed):
    """(frames, labels) per utterance: the small shapes of every group, then the group's own label counts at T' = 2L + 3."""
    rs = np.random.RandomState(seed)
    a = int(rs.randint(1, V))
    b = a % (V - 1) + 1 if V > 2 else a                     # another label where the vocabulary has one
    utts = [(1, []), (1, [a]), (17, []), (3, [a, a]), (2, [a, b] if b != a else [a]),
            (5, [a, a, a, b]),                                # infeasible: 4 labels + 2 repeats (3 where b == a) need > 5
            (29, _labels(rs, V, 13, equal=True))]             # all tokens equal: the longest run of the sorted position list
    for L in GROUPS[group]:
        utts.append((2 * L + 3, _labels(rs, V, L)))
    utts.append((2 * GROUPS[group][0] + 1, _labels(rs, V, GROUPS[group][0], equal=True)))    # T' = L + repeats + 2
    return utts


_CASES = {}


def _case(V, group, scale, extra=0):
    """Inputs and the CPU results (float64 checker, float32 yardstick) of one case, computed once.  extra: frames behind the
    longest utterance - the same utterances and logits on a time axis of max(t) + extra, which no utterance fills (a rank of
    a data-parallel step: the encoder is padded to the global T_max)."""
    key = (V, group, scale, extra)
    if key in _CASES:
        return _CASES[key]
    utts = _utterances(V, group, 100 + V)
    rs = np.random.RandomState(7 * V + len(group))
    B, T = len(utts), max(t for t, _ in utts)
    z = torch.from_numpy((scale * rs.normal(0, 1, size=(B, T, V))).astype(np.float32))
    if extra:
        z, T = torch.cat([z, torch.zeros(B, extra, V)], 1), T + extra
    lens = [t for t, _ in utts]
    for i, t in enumerate(lens):
        z[i, t:] = 0.0
    ylens = [len(y) for _, y in utts]
    ys = torch.tensor([v for _, y in utts for v in y], dtype=torch.long)
    g = torch.from_numpy(rs.uniform(-2, 2, size=B).astype(np.float32))
    g[1], g[-1] = 0.0, 1.0
    out = dict(z=z, lens=lens, ylens=ylens, ys=ys, g=g, B=B, T=T, V=V)
    for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
        zz = z.to(dt).clone().requires_grad_()
        nll = F.ctc_loss(F.log_softmax(zz, -1).transpose(0, 1), ys, torch.tensor(lens), torch.tensor(ylens), blank=0,
                         reduction="none", zero_infinity=True)
        (nll * g.to(dt)).sum().backward()
        out[name] = (nll.detach().double(), zz.grad.double())
    raw = F.ctc_loss(F.log_softmax(z.double(), -1).transpose(0, 1), ys, torch.tensor(lens), torch.tensor(ylens), blank=0,
                     reduction="none", zero_infinity=False)
    out["feasible"] = torch.isfinite(raw)
    assert int((~out["feasible"]).sum()) == 1 and bool(torch.isfinite(out["ref"][0]).all())
    _CASES[key] = out
    return out


def _run(hb, c, zero_infinity=True):
    """ops.ctc_loss on the case: the logits are a [B, T, V] view of a [B, T, V + 3] buffer (ld = V + 3) whose padding - the
    frames behind every length and the three extra columns - is NaN."""
    import ops
    B, T, V = c["B"], c["T"], c["V"]
    buf = torch.full((B, T, V + 3), float("nan"))
    for i, t in enumerate(c["lens"]):
        buf[i, :t, :V] = c["z"][i, :t]
    buf = buf.to(DEV).requires_grad_()
    nll = ops.ctc_loss(buf[:, :, :V], hb.to_device_i32(c["lens"], DEV), c["ys"].to(DEV), c["ylens"], zero_infinity)
    nll.backward(c["g"].to(DEV))
    return nll.detach().cpu(), buf.grad.cpu()


def _allowance(f32, ref):
    err32 = float((f32 - ref).abs().max())
    floor = 8.0 * float(np.spacing(np.float32(ref.abs().max())))
    return max(4.0 * err32, floor), err32


def _check(c, nll, grad, rows, what):
    V = c["V"]
    for i, t in enumerate(c["lens"]):
        assert bool((grad[i, t:] == 0).all()), "%s: utterance %d has a gradient behind its %d frames" % (what, i, t)
    assert bool((grad[:, :, V:] == 0).all())
    assert bool(torch.isfinite(nll[rows]).all()) and bool(torch.isfinite(grad[rows]).all()), what
    ref_n, ref_g = c["ref"]
    f32_n, f32_g = c["f32"]
    allow_n, e32n = _allowance(f32_n[rows], ref_n[rows])
    allow_g, e32g = _allowance(f32_g[rows], ref_g[rows])
    err_n = float((nll[rows].double() - ref_n[rows]).abs().max())
    err_g = float((grad[rows][:, :, :V].double() - ref_g[rows]).abs().max())
    print("ctc_parity %s: nll err %.3g (f32 cpu %.3g, allowed %.3g, ratio %.3f)  grad err %.3g (f32 cpu %.3g, allowed %.3g, "
          "ratio %.3f)  max|nll| %.4g" % (what, err_n, e32n, allow_n, err_n / allow_n, err_g, e32g, allow_g, err_g / allow_g,
                                          float(ref_n[rows].abs().max())))
    assert err_n <= allow_n, "%s: nll error %.3g above %.3g" % (what, err_n, allow_n)
    assert err_g <= allow_g, "%s: gradient error %.3g above %.3g" % (what, err_g, allow_g)


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("V", VOCABS)
def test_kernel_against_float64(hb, V, group):
    """T' = 1 with L in {0, 1}; L = 0 at T' = 17; tight T' = L + repeats; an infeasible row (loss 0, gradient 0 under
    zero_infinity); 2L + 1 on both sides of a wave and of a workgroup; ld = V + 3; NaN behind every length; all-equal labels;
    upstream gradients of both signs and 0."""
    c = _case(V, group, 3.0)
    nll, grad = _run(hb, c)
    bad = int((~c["feasible"]).nonzero()[0])
    assert float(nll[bad]) == 0.0 and bool((grad[bad] == 0).all())
    _check(c, nll, grad, torch.arange(c["B"]), "V=%d %s" % (V, group))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_time_axis_past_every_utterance(hb, group):
    """T = max(t) + 5: NaN behind every length, the five frames no utterance has included; ld = V + 3.  The allowance and the
    zero gradient behind every length as above, and the bits of the run at T = max(t): every sum of the kernels has one
    owner and the extent only changes strides."""
    c, short = _case(34, group, 3.0, extra=5), _case(34, group, 3.0)
    assert c["T"] == short["T"] + 5 and torch.equal(c["z"][:, :short["T"]], short["z"])
    nll, grad = _run(hb, c)
    assert grad.shape[1] == c["T"]
    _check(c, nll, grad, torch.arange(c["B"]), "V=34 %s T+5" % group)
    nll0, grad0 = _run(hb, short)
    assert torch.equal(nll, nll0), "nll differs from the run at T = max(t)"
    assert torch.equal(grad[:, :short["T"]], grad0), "the gradient differs from the run at T = max(t)"
    assert bool((grad[:, short["T"]:] == 0).all())
    print("ctc_parity V=34 %s T+5: bit-identical to T=%d" % (group, short["T"]))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_logits_scaled_by_50(hb, group):
    """Probabilities underflow in linear space (logits ~ 150 N(0, 1)): every output finite, same allowance."""
    c = _case(34, group, 150.0)
    nll, grad = _run(hb, c)
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(grad).all())
    _check(c, nll, grad, torch.arange(c["B"]), "V=34 %s x50" % group)


def test_infeasible_without_zero_infinity(hb):
    c = _case(34, "block", 3.0)
    nll, grad = _run(hb, c, zero_infinity=False)
    bad = ~c["feasible"]
    assert bool(torch.isinf(nll[bad]).all()) and bool((nll[bad] > 0).all())
    _check(c, nll, grad, c["feasible"].nonzero().flatten(), "V=34 block, zero_infinity off")


@pytest.mark.parametrize("det", [False, True])
def test_bit_reproducible(hb, det):
    c = _case(257, "strided", 3.0)
    with hb.deterministic(det):
        first, second = _run(hb, c), _run(hb, c)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1].nan_to_num(), second[1].nan_to_num()) and not bool(torch.isnan(first[1]).any())


def test_refused_shapes(hb):
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_ws_bytes(2, 10, 5, hb.CTC_MAX_LABELS + 1)
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_ws_bytes(2, 10, 1, 3)
    B, T, V, L = 3, 7, 5, 2
    assert hb.ctc_ws_bytes(B, T, V, L) >= 4 * (B * T * (2 * L + 2) + B * (L + V + 1))


# ------------------------------------------------------------------------------------------------ head and model
def _tiny(ctc_weight=None, seed=21):
    import model as M
    torch.manual_seed(seed)
    kw = {} if ctc_weight is None else dict(ctc_weight=ctc_weight)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw).to(DEV)
    weights = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    res = net.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys and all(k.startswith("ctc_lo.") for k in res.missing_keys)
    net.train()
    xs, ilens, ys = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    return net, torch.from_numpy(xs).to(DEV), ilens, [torch.from_numpy(y).to(DEV) for y in ys]


def _step(net, xs, ilens, ys):
    import parallel
    np.random.seed(5)
    _, lp, _, _ = net(xs, ilens, ys, tf_rate=1.0, loss_norm=len(ilens))
    loss = parallel.local_loss(lp, dict(b_global=len(ilens)))
    net.zero_grad()
    loss.backward()
    return lp, loss


def test_ctc_off_is_todays_model(hb):
    """(a) ctc_weight = 0: the reference's state_dict keys, no ctc_lo, and the bits of a model built without the argument
    (both steps in deterministic mode: outside it the fp32 atomics make no two runs of ANY model equal)."""
    off, xs, ilens, ys = _tiny(0.0)
    plain = _tiny(None)[0]
    assert not hasattr(off, "ctc_lo")
    assert list(off.state_dict()) == list(plain.state_dict()) and set(off.state_dict()) == set(synth.e2e_weights(synth.TINY, 11))
    with hb.deterministic():
        lp0, loss0 = _step(off, xs, ilens, ys)
        lp1, loss1 = _step(plain, xs, ilens, ys)
    assert getattr(lp0, "ctc_loss", None) is None
    assert torch.equal(loss0, loss1) and torch.equal(lp0, lp1)
    for (n, p), (_, q) in zip(off.named_parameters(), plain.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_joint_value(hb):
    """(b) the loss of the step = 0.7 L_att + 0.3 sum(nll) / B, L_att from the same forward's log_probs.  Allowance: L_att is
    an fp32 sum of B L <= 15 rounded terms, sum(nll) one of 3, the combination three more roundings - 32 fp32 ulps of the
    larger term covers it."""
    net, xs, ilens, ys = _tiny(0.3)
    assert tuple(net.ctc_lo.weight.shape) == (synth.TINY["output_dim"], synth.TINY["enc_hidden_dim"])
    lp, loss = _step(net, xs, ilens, ys)
    B = len(ilens)
    att = -float(lp.detach().double().sum()) / (B * lp.shape[1])
    ctc = float(lp.ctc_nll.detach().double().sum()) / B
    want = 0.7 * att + 0.3 * ctc
    assert ctc > 0 and np.isfinite(want)
    got = float(loss.detach())
    assert abs(got - want) <= 32 * 2.0 ** -23 * max(abs(att), abs(ctc)), (got, want)
    assert net.ctc_lo.weight.grad is not None and float(net.ctc_lo.weight.grad.abs().max()) > 0


def test_gradient_into_the_encoder(hb):
    """(c) d enc_h, d ctc_lo.weight, d ctc_lo.bias of sum(nll) / B alone against the float64 checker applied to the model's
    own enc_h: 1e-3 of each tensor's max."""
    net, xs, ilens, ys = _tiny(0.3)
    enc_h, _ = net.encoder(xs, ilens)
    e = enc_h.detach().clone().requires_grad_()
    net.zero_grad()
    B = len(ilens)
    (net.ctc_nll(e, ys).sum() / B).backward()
    lens = net.encoder.enc2.last_lens_dev.cpu().long()
    e64 = enc_h.detach().double().cpu().requires_grad_()
    w64 = net.ctc_lo.weight.detach().double().cpu().requires_grad_()
    b64 = net.ctc_lo.bias.detach().double().cpu().requires_grad_()
    logp = F.log_softmax(e64 @ w64.t() + b64, -1).transpose(0, 1)
    nll = F.ctc_loss(logp, torch.cat([y.cpu() for y in ys]), lens, torch.tensor([len(y) for y in ys]), blank=0,
                     reduction="none", zero_infinity=True)
    (nll.sum() / B).backward()
    for name, got, want in (("enc_h", e.grad, e64.grad), ("ctc_lo.weight", net.ctc_lo.weight.grad, w64.grad),
                            ("ctc_lo.bias", net.ctc_lo.bias.grad, b64.grad)):
        err, top = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        print("ctc head %s: err %.3g of max %.3g" % (name, err, top))
        assert top > 0 and err <= 1e-3 * top, name


def _solver(root, monkeypatch, **over):
    """The tiny Solver of tests/test_solver_gpu.py / test_deterministic_gpu.py with seeded weights; the CTC head (no fixture
    holds one) from a seeded torch generator."""
    import yaml
    from dataset import synthetic_utterances
    from solver import Solver
    t, l = synth.TINY, synth.TINY_LM
    nv = t["output_dim"]
    vocab = {s: i for i, s in enumerate(["<PAD>", "<BOS>", "<EOS>"] + ["s%d" % i for i in range(nv - 5)] + ["<space>", "<NOISE>"])}
    os.makedirs(root, exist_ok=True)
    for name, n, seed in (("train", 12, 1), ("dev", 4, 2)):
        with open(os.path.join(root, name + ".pkl"), "wb") as f:
            pickle.dump(synthetic_utterances(n, t["input_dim"], nv, 24, seed), f)
    with open(os.path.join(root, "vocab_dict.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(root, "non_lang_syms.pkl"), "wb") as f:
        pickle.dump(["<NOISE>", "<PAD>", "<BOS>", "<EOS>"], f)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "semi-supervised-asr_amd", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(logdir=os.path.join(root, "log"), model_dir=root, model_name="m", load_model_path=os.path.join(root, "m"),
               load_judge_path=os.path.join(root, "m"), dataset_root_dir=root, vocab_path=os.path.join(root, "vocab_dict.pkl"),
               non_lang_syms_path=os.path.join(root, "non_lang_syms.pkl"), labeled_set="train", unlabeled_speech_set="train",
               unlabeled_text_set="train", dev_set="dev", test_set="dev", max_dec_timesteps=8, batch_size=4,
               input_dim=t["input_dim"], enc_hidden_dim=t["enc_hidden_dim"], enc_n_layers=t["enc_n_layers"],
               subsample=t["subsample"], dropout_rate=0.0, dec_hidden_dim=t["dec_hidden_dim"], att_dim=t["att_dim"],
               conv_channels=t["conv_channels"], conv_kernel_size=t["conv_kernel_size"], att_odim=t["att_odim"],
               embedding_dim=t["embedding_dim"], ls_weight=t["ls_weight"], dis_embedding_dim=l["embedding_dim"],
               dis_hidden_dim=l["hidden_dim"], dis_dropout_rate=0.0, dis_layers=l["n_layers"], d_learning_rate=2e-4,
               learning_rate=5e-4, weight_decay=1e-6, max_grad_norm=5, min_feature_length=1, add_gaussian=False)
    cfg.update(over)
    monkeypatch.chdir(root)
    solver = Solver(cfg)
    dev = next(solver.model.parameters()).device
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        wm = synth.e2e_weights(t, 11)
        for k, v in solver.model.state_dict().items():
            v.copy_(torch.from_numpy(wm[k]) if k in wm else torch.empty(v.shape).uniform_(-0.25, 0.25, generator=gen))
    solver.model.decoder.labeldist = synth.labeldist(nv, 12)
    solver.model.decoder.vlabeldist = torch.from_numpy(np.asarray(solver.model.decoder.labeldist, dtype=np.float32)).to(dev)
    solver.model.decoder._dist_dev = {}
    solver.model.train()
    return solver, dev


def _sup_batch(dev):
    xs, ilens, ys = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    return torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys]


def test_one_train_step(hb, tmp_path, monkeypatch):
    """(d) one supervised step with ctc_weight = 0.3: finite loss, the head has moved, the abort latch is clear; the same
    step from the same state twice in deterministic mode leaves the same bits in every parameter."""
    after = []
    for run in range(2):
        solver, dev = _solver(str(tmp_path / ("run%d" % run)), monkeypatch, ctc_weight=0.3, deterministic=True)
        assert "ctc_lo.weight" in dict(solver.model.named_parameters())
        before = solver.model.ctc_lo.weight.detach().clone()
        hb.persist_clear_abort(dev)
        np.random.seed(4)
        xs, ilens, ys = _sup_batch(dev)
        loss = solver.sup_train_one_iteration(xs, ilens, ys, 1.0)
        solver.flush()
        assert np.isfinite(float(loss))
        assert not torch.equal(before, solver.model.ctc_lo.weight.detach())
        assert not hb.persist_aborted(dev)
        after.append({n: p.detach().clone() for n, p in solver.model.named_parameters()})
    for n in after[0]:
        assert torch.equal(after[0][n], after[1][n]), n


def test_checkpoint_without_the_head(hb, tmp_path, monkeypatch, capsys):
    """(e) an attention-only checkpoint into a model with the head: the rest loads, ctc_lo keeps its initialisation, and it
    says so; the optimiser state of such a run is refused."""
    solver, dev = _solver(str(tmp_path / "s"), monkeypatch, ctc_weight=0.3)
    head = {k: v.detach().clone() for k, v in solver.model.state_dict().items() if k.startswith("ctc_lo.")}
    assert sorted(head) == ["ctc_lo.bias", "ctc_lo.weight"]
    old = {k: torch.from_numpy(v) + 0.5 for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    path = str(tmp_path / "old")
    torch.save(old, path + ".ckpt")
    capsys.readouterr()
    solver.load_model(path, False)
    said = capsys.readouterr().out
    assert said.count("keeps its initialisation") == 1
    sd = solver.model.state_dict()
    for k, v in head.items():
        assert torch.equal(sd[k], v), k
    for k, v in old.items():
        assert torch.equal(sd[k].cpu(), v), k
    with pytest.raises(RuntimeError, match="CTC head"):
        solver.load_model(path, True)
