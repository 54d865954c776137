"""The star CTC loss on the GPU (csrc/ctc_star.hip) against its torch restatement (tests/ctc_star_ref.py) in
float64, then the penalty in E2E.

Tolerance of the kernel cases: none is written down here.  Every case also runs the restatement in float32 on the same
inputs; per element the kernel's error against float64 may be at most 4 x the float32 restatement's worst error (another
summation order inside the log-sum-exps, no more), with a floor of 8 fp32 ulps of the tensor's largest magnitude where the
float32 error is about zero - test_ctc_gpu's rule.  Each case prints a `ctc_star_parity` line with its two ratios
(profiles/ctc_star_parity.txt holds one run).

The dispatch boundaries are the header's (include/asr_hip.h, "Star CTC", max_label_len): S = 3 L + 2 states; one wave per
utterance up to 64 states (L <= 20), one workgroup with a state per thread up to 256 (L <= 84), states strided over the
threads beyond (L >= 85)."""
import numpy as np
import pytest
import torch

import ctc_star_ref as R
import poison as P
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")

VOCABS = (2, 5, 34, 257)
GROUPS = dict(wave=(20,), block=(21, 84), strided=(85, 130))
PENALTIES = (-INF, -5.0, -1.0, -0.25, 0.0)


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    assert 3 * 20 + 2 <= 64 < 3 * 21 + 2 and 3 * 84 + 2 <= 256 < 3 * 85 + 2
    return hip_backend


def _labels(rs, V, n, equal=False):
    if equal or V == 2:
        return [int(rs.randint(1, V))] * n
    return [int(v) for v in rs.randint(1, V, size=n)]


def _utterances(V, group, seed):
    """(frames, labels) per utterance - test_ctc_gpu._utterances restated: the small shapes of every group, then the group's
    own label counts at T' = 2L + 3."""
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


def _reference(z, lens, labels, pen, g):
    out = {}
    for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
        zz = z.to(dt).clone().requires_grad_()
        nll, _ = R.star_ctc_nll(zz, lens, labels, pen, zero_infinity=True)
        (nll * g.to(dt)).sum().backward()
        out[name] = (nll.detach().double(), zz.grad.double())
    return out


def _case(V, group, scale, extra=0, closed=False):
    """Inputs and the CPU results (float64 checker, float32 yardstick) of one case, computed once.  extra: frames behind the
    longest utterance.  closed: every penalty -inf (the plain CTC lattice); otherwise one of PENALTIES per row, each at least
    once."""
    key = (V, group, scale, extra, closed)
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
    labels = [y for _, y in utts]
    g = torch.from_numpy(rs.uniform(-2, 2, size=B).astype(np.float32))
    g[1], g[-1] = 0.0, 1.0
    order = rs.permutation(len(PENALTIES))
    pen = [-INF if closed else PENALTIES[order[i % len(PENALTIES)]] for i in range(B)]
    assert closed or set(pen) == set(PENALTIES)
    out = dict(z=z, lens=lens, labels=labels, ylens=[len(y) for y in labels], pen=pen, g=g, B=B, T=T, V=V,
               ys=torch.tensor([v for y in labels for v in y], dtype=torch.long))
    out.update(_reference(z, lens, labels, pen, g))
    _, out["feasible"] = R.star_ctc_nll(z.double(), lens, labels, pen, zero_infinity=False)
    # exactly one row is infeasible, under the reference alone, before the GPU runs
    assert int((~out["feasible"]).sum()) == 1 and not bool(out["feasible"][5])
    assert bool(torch.isfinite(out["ref"][0]).all()) and bool(torch.isfinite(out["ref"][1]).all())
    _CASES[key] = out
    return out


def _run(hb, c, zero_infinity=True, rows=None, pen=None, extra_cols=3):
    """ops.ctc_star_loss on the case (or on its `rows`, in that order): the logits are a [B, T, V] view of a [B, T, V + 3]
    buffer (ld = V + 3) whose padding - the frames behind every length and the three extra columns - is NaN."""
    import ops
    rows = list(range(c["B"])) if rows is None else list(rows)
    pen = c["pen"] if pen is None else pen
    T, V = c["T"], c["V"]
    buf = torch.full((len(rows), T, V + extra_cols), float("nan"))
    for r, i in enumerate(rows):
        buf[r, :c["lens"][i], :V] = c["z"][i, :c["lens"][i]]
    buf = buf.to(DEV).requires_grad_()
    ys = torch.tensor([v for i in rows for v in c["labels"][i]], dtype=torch.long)
    nll = ops.ctc_star_loss(buf[:, :, :V], hb.to_device_i32([c["lens"][i] for i in rows], DEV), ys.to(DEV),
                            [c["ylens"][i] for i in rows], torch.tensor([pen[i] for i in rows], dtype=torch.float32),
                            zero_infinity)
    nll.backward(c["g"][rows].to(DEV))
    return nll.detach().cpu(), buf.grad.cpu()


def _allowance(f32, ref, other32=0.0):
    err32 = max(float((f32 - ref).abs().max()), other32)
    floor = 8.0 * float(np.spacing(np.float32(ref.abs().max())))
    return max(4.0 * err32, floor), err32


def _check(c, nll, grad, rows, what, ref=None, other32=(0.0, 0.0)):
    V = c["V"]
    for i, t in enumerate(c["lens"]):
        assert bool((grad[i, t:] == 0).all()), "%s: utterance %d has a gradient behind its %d frames" % (what, i, t)
    assert bool((grad[:, :, V:] == 0).all())
    assert bool(torch.isfinite(nll[rows]).all()) and bool(torch.isfinite(grad[rows]).all()), what
    ref_n, ref_g = c["ref"] if ref is None else ref
    f32_n, f32_g = c["f32"]
    allow_n, e32n = _allowance(f32_n[rows], c["ref"][0][rows], other32[0])
    allow_g, e32g = _allowance(f32_g[rows], c["ref"][1][rows], other32[1])
    err_n = float((nll[rows].double() - ref_n[rows]).abs().max())
    err_g = float((grad[rows][:, :, :V].double() - ref_g[rows]).abs().max())
    print("ctc_star_parity %s: nll err %.3g (f32 cpu %.3g, allowed %.3g, ratio %.3f)  grad err %.3g (f32 cpu %.3g, allowed "
          "%.3g, ratio %.3f)  max|nll| %.4g" % (what, err_n, e32n, allow_n, err_n / allow_n, err_g, e32g, allow_g,
                                                err_g / allow_g, float(c["ref"][0][rows].abs().max())))
    assert err_n <= allow_n, "%s: nll error %.3g above %.3g" % (what, err_n, allow_n)
    assert err_g <= allow_g, "%s: gradient error %.3g above %.3g" % (what, err_g, allow_g)


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("V", VOCABS)
def test_kernel_against_float64(hb, V, group):
    """T' = 1 with L in {0, 1}; L = 0 at T' = 17; tight T' = L + repeats; an infeasible row (loss 0, gradient 0 under
    zero_infinity); 3L + 2 on both sides of a wave and of a workgroup; V = 2 (nb = x[1]); a penalty of {-inf, -5, -1, -0.25, 0}
    per row; ld = V + 3; NaN behind every length; all-equal labels; upstream gradients of both signs and 0."""
    c = _case(V, group, 3.0)
    nll, grad = _run(hb, c)
    bad = int((~c["feasible"]).nonzero()[0])
    assert float(nll[bad]) == 0.0 and bool((grad[bad] == 0).all())
    _check(c, nll, grad, torch.arange(c["B"]), "V=%d %s" % (V, group))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_time_axis_past_every_utterance(hb, group):
    """T = max(t) + 5: the same allowance, zeros behind every length, and the bits of the run at T = max(t)."""
    c, short = _case(34, group, 3.0, extra=5), _case(34, group, 3.0)
    assert c["T"] == short["T"] + 5 and torch.equal(c["z"][:, :short["T"]], short["z"]) and c["pen"] == short["pen"]
    nll, grad = _run(hb, c)
    assert grad.shape[1] == c["T"]
    _check(c, nll, grad, torch.arange(c["B"]), "V=34 %s T+5" % group)
    nll0, grad0 = _run(hb, short)
    assert torch.equal(nll, nll0), "nll differs from the run at T = max(t)"
    assert torch.equal(grad[:, :short["T"]], grad0), "the gradient differs from the run at T = max(t)"
    assert bool((grad[:, short["T"]:] == 0).all())


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


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_closed_rows_are_the_ctc_loss(hb, group):
    """penalty = -inf in every row: the star kernels against the float64 restatement (which test_ctc_star_cpu holds to
    F.ctc_loss), then against ops.ctc_loss on the GPU, same inputs, by the same rule.  There two kernels are compared, each
    with a float32 yardstick of its own - the restatement here, torch's float32 CPU ctc_loss for ops.ctc_loss
    (test_ctc_gpu) - and "the float32 reference's own error" is the larger of the two: torch's alpha-beta gradient in
    float32 is several times noisier than the restatement's autograd, and so, inside its own allowance, is csrc/ctc.hip's."""
    import ops
    import torch.nn.functional as F
    c = _case(34, group, 3.0, closed=True)
    nll, grad = _run(hb, c)
    rows = torch.arange(c["B"])
    _check(c, nll, grad, rows, "V=34 %s closed" % group)
    buf = torch.full((c["B"], c["T"], c["V"] + 3), float("nan"))
    for i, t in enumerate(c["lens"]):
        buf[i, :t, :c["V"]] = c["z"][i, :t]
    buf = buf.to(DEV).requires_grad_()
    plain = ops.ctc_loss(buf[:, :, :c["V"]], hb.to_device_i32(c["lens"], DEV), c["ys"].to(DEV), c["ylens"], True)
    plain.backward(c["g"].to(DEV))
    torch32 = []
    for dt in (torch.float64, torch.float32):
        zz = c["z"].to(dt).clone().requires_grad_()
        t_nll = F.ctc_loss(F.log_softmax(zz, -1).transpose(0, 1), c["ys"], torch.tensor(c["lens"]), torch.tensor(c["ylens"]),
                           blank=0, reduction="none", zero_infinity=True)
        (t_nll * c["g"].to(dt)).sum().backward()
        torch32.append((t_nll.detach().double(), zz.grad.double()))
    other32 = tuple(float((torch32[1][k] - torch32[0][k]).abs().max()) for k in (0, 1))
    _check(c, nll, grad, rows, "V=34 %s closed vs ops.ctc_loss" % group,
           ref=(plain.detach().cpu().double(), buf.grad.cpu()[:, :, :c["V"]].double()), other32=other32)


@pytest.mark.parametrize("det", [False, True])
def test_bit_reproducible(hb, det):
    c = _case(257, "strided", 3.0)
    with hb.deterministic(det):
        first, second = _run(hb, c), _run(hb, c)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1]) and not bool(torch.isnan(first[1]).any())


def test_batch_invariance(hb):
    """A row's nll and gradient have the same bits alone (another Lmax: another kernel for most rows), at another batch
    position (reversed order) and beside rows with other penalties."""
    c = _case(34, "strided", 3.0)
    B = c["B"]
    nll, grad = _run(hb, c)
    rev = list(range(B))[::-1]
    nll_r, grad_r = _run(hb, c, rows=rev)
    for r, i in enumerate(rev):
        assert torch.equal(nll_r[r], nll[i]) and torch.equal(grad_r[r], grad[i]), "moved: row %d" % i
    for i in range(B):
        n1, g1 = _run(hb, c, rows=[i])
        assert torch.equal(n1[0], nll[i]) and torch.equal(g1[0], grad[i]), "alone: row %d" % i
    for k in range(3):
        pen = c["pen"][1:] + c["pen"][:1]
        kept = list(range(k, B, 3))
        for i in kept:
            pen[i] = c["pen"][i]
        assert any(pen[i] != c["pen"][i] for i in range(B))
        n2, g2 = _run(hb, c, pen=pen)
        for i in kept:
            assert torch.equal(n2[i], nll[i]) and torch.equal(g2[i], grad[i]), "other penalties: row %d" % i
    print("ctc_star_parity batch invariance V=34 strided: %d rows alone, moved, beside other penalties: bit-identical" % B)


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_outputs_and_workspace(hb, pattern):
    """torch.empty & co (nll, dlogits, a fresh workspace) filled with the pattern, then the pooled workspace a first call left
    behind poisoned where it lay: the bits of the clean run.  The integer regions of the workspace (order, head) are written
    before they are read in the same call, as in csrc/ctc.hip: head is zeroed for all V entries and order filled for 0 .. L-1
    by the alpha kernel; the gradient kernel reads them in a later launch, for feasible rows only."""
    import ops
    c = _case(34, "block", 3.0)
    P.empty_pool()
    want = _run(hb, c)
    try:
        for variant in ("fresh", "leftover"):
            st = P.Stats()
            if variant == "fresh":
                P.empty_pool()
            else:
                assert any(k[0] == "ctc_star" and v for k, v in ops._POOL.free.items())
                assert P.poison_pool(pattern, st) > 0
            with P.poisoned(pattern, st):
                got = _run(hb, c)
            assert st.total > 0
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (variant, pattern)
    finally:
        P.empty_pool()


def test_refused_shapes(hb):
    import ops
    z = torch.zeros(1, 4, 5, device=DEV)
    one = hb.to_device_i32([4], DEV)
    lab = torch.ones(2, dtype=torch.long, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_star_loss(z, one, torch.ones(hb.CTC_STAR_MAX_LABELS + 1, dtype=torch.long, device=DEV),
                          [hb.CTC_STAR_MAX_LABELS + 1], -1.0)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_star_loss(z[:, :, :1], one, lab[:0], [0], -1.0)
    for bad in (0.5, float("nan"), torch.tensor([0.25]), torch.tensor([float("nan")]), torch.tensor([0.25], device=DEV)):
        with pytest.raises(ValueError):
            ops.ctc_star_loss(z, one, lab, [2], bad)
    # the workspace: 4-byte aligned and at least ctc_star_ws_bytes, checked before anything is launched
    need = hb.ctc_star_ws_bytes(1, 4, 5, 2)
    raw = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    offs, pen = hb.to_device_i32([0, 2], DEV), torch.full((1,), -1.0, device=DEV)
    nll, dz, g = torch.zeros(1, device=DEV), torch.zeros(1, 4, 5, device=DEV), torch.ones(1, device=DEV)
    before = dict(hb.LAUNCHES)
    for ws, nbytes in ((raw[1:], need), (raw[:need], need - 4)):
        with pytest.raises(RuntimeError):
            hb.ctc_star_loss_fwd(z, 5, one, lab, offs, 2, pen, True, nll, ws, ws_bytes=nbytes)
        with pytest.raises(RuntimeError):
            hb.ctc_star_loss_bwd(z, 5, one, lab, offs, 2, pen, True, g, ws, dz, 5, ws_bytes=nbytes)
    assert dict(hb.LAUNCHES) == before
    hb.ctc_star_loss_fwd(z, 5, one, lab, offs, 2, pen, True, nll, raw[:need])
    assert np.isfinite(float(nll))


# ------------------------------------------------------------------------------------------------ the model
TINY_ILENS, TINY_YLENS = [23, 17, 12], [4, 3, 2]     # 6, 5 and 3 encoder frames: every row has room for a star


def _tiny(seed=21, **kw):
    import model as M
    torch.manual_seed(seed)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw).to(DEV)
    weights = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    res = net.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys and all(k.startswith("ctc_lo.") for k in res.missing_keys)
    net.train()
    xs, ilens, ys = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], TINY_ILENS, TINY_YLENS, 13)
    return net, torch.from_numpy(xs).to(DEV), ilens, [torch.from_numpy(y).to(DEV) for y in ys]


def _step(net, xs, ilens, ys):
    import parallel
    np.random.seed(5)
    _, lp, _, _ = net(xs, ilens, ys, tf_rate=1.0, loss_norm=len(ilens))
    loss = parallel.local_loss(lp, dict(b_global=len(ilens)))
    net.zero_grad()
    loss.backward()
    return lp, loss


def _star_reference(net, enc_h, ys, penalty):
    """mean-free star nll [B] (float64, with autograd to e64 / w64 / b64) of the model's own encoder output"""
    lens = net.encoder.enc2.last_lens_dev.cpu().tolist()
    e64 = enc_h.detach().double().cpu().requires_grad_()
    w64 = net.ctc_lo.weight.detach().double().cpu().requires_grad_()
    b64 = net.ctc_lo.bias.detach().double().cpu().requires_grad_()
    nll, feasible = R.star_ctc_nll(e64 @ w64.t() + b64, lens, [y.cpu().tolist() for y in ys], [penalty] * len(ys))
    assert bool(feasible.all())
    return nll, e64, w64, b64


def test_key_absent_is_todays_model(hb):
    """ctc_star_penalty absent or None: the launches of the step, its loss and every gradient are those of a model built
    without the argument (deterministic mode: outside it no two runs of any model are equal), and no star kernel runs."""
    plain, xs, ilens, ys = _tiny(ctc_weight=0.3)
    none = _tiny(ctc_weight=0.3, ctc_star_penalty=None)[0]
    assert list(plain.state_dict()) == list(none.state_dict())
    counts = []
    with hb.deterministic():
        for net in (plain, none):
            before = dict(hb.LAUNCHES)
            lp, loss = _step(net, xs, ilens, ys)
            counts.append(({k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}, lp, loss))
    assert counts[0][0] == counts[1][0] and counts[0][0].get("ctc_loss") == 1 and "ctc_star_loss" not in counts[0][0]
    assert torch.equal(counts[0][2], counts[1][2]) and torch.equal(counts[0][1], counts[1][1])
    for (n, p), (_, q) in zip(plain.named_parameters(), none.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_joint_value_with_the_star_term(hb):
    """ctc_star_penalty = -0.5: the loss of the step = 0.7 L_att + 0.3 mean(star nll), L_att from the same forward's
    log_probs, the star term from the float64 restatement on the model's own encoder output and head.  Allowance: the 32
    fp32 ulps of test_ctc_gpu.test_joint_value for the sums, plus 1e-3 of the star term (the head's fp32 product
    against float64)."""
    net, xs, ilens, ys = _tiny(ctc_weight=0.3, ctc_star_penalty=-0.5)
    before = dict(hb.LAUNCHES)
    lp, loss = _step(net, xs, ilens, ys)
    assert hb.LAUNCHES["ctc_star_loss"] == before.get("ctc_star_loss", 0) + 1
    assert hb.LAUNCHES["ctc_star_loss_bwd"] == before.get("ctc_star_loss_bwd", 0) + 1
    assert hb.LAUNCHES["ctc_loss"] == before.get("ctc_loss", 0)
    enc_h, _ = net.encoder(xs, ilens)
    ref, _, _, _ = _star_reference(net, enc_h, ys, -0.5)
    B = len(ilens)
    att = -float(lp.detach().double().sum()) / (B * lp.shape[1])
    star = float(ref.detach().sum()) / B
    want = 0.7 * att + 0.3 * star
    got = float(loss.detach())
    err_rows = float((lp.ctc_nll.detach().double().cpu() - ref.detach()).abs().max())
    print("ctc_star model: loss %.6f want %.6f; star nll rows err %.3g of max %.3g" % (got, want, err_rows,
                                                                                       float(ref.detach().abs().max())))
    assert abs(got - want) <= 32 * 2.0 ** -23 * max(abs(att), abs(star)) + 0.3 * 1e-3 * abs(star), (got, want)
    assert err_rows <= 1e-3 * float(ref.detach().abs().max())
    assert net.ctc_lo.weight.grad is not None and float(net.ctc_lo.weight.grad.abs().max()) > 0
    # the penalty is a plain attribute: reassigned, the next step uses it
    net.ctc_star_penalty = -5.0
    lp2, _ = _step(net, xs, ilens, ys)
    ref2, _, _, _ = _star_reference(net, net.encoder(xs, ilens)[0], ys, -5.0)
    assert float((lp2.ctc_nll.detach().double().cpu() - ref2.detach()).abs().max()) <= 1e-3 * float(ref2.detach().abs().max())
    assert float(ref2.detach().sum()) > float(ref.detach().sum())


def test_gradient_into_the_encoder(hb):
    """d enc_h, d ctc_lo.weight, d ctc_lo.bias of mean(star nll) alone against the float64 restatement applied to the model's
    own enc_h: 1e-3 of each tensor's max."""
    net, xs, ilens, ys = _tiny(ctc_weight=0.3, ctc_star_penalty=-0.5)
    enc_h, _ = net.encoder(xs, ilens)
    e = enc_h.detach().clone().requires_grad_()
    net.zero_grad()
    B = len(ilens)
    (net.ctc_nll(e, ys).sum() / B).backward()
    ref, e64, w64, b64 = _star_reference(net, enc_h, ys, -0.5)
    (ref.sum() / B).backward()
    for name, got, want in (("enc_h", e.grad, e64.grad), ("ctc_lo.weight", net.ctc_lo.weight.grad, w64.grad),
                            ("ctc_lo.bias", net.ctc_lo.bias.grad, b64.grad)):
        err, top = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        print("ctc_star head %s: err %.3g of max %.3g" % (name, err, top))
        assert top > 0 and err <= 1e-3 * top, name


def test_eval_mode_runs_the_plain_loss(hb):
    import ops
    net, xs, ilens, ys = _tiny(ctc_weight=0.3, ctc_star_penalty=-0.5)
    net.eval()
    before = dict(hb.LAUNCHES)
    with torch.no_grad():
        enc_h, _ = net.encoder(xs, ilens)
        got = net.ctc_nll(enc_h, ys)
        assert hb.LAUNCHES["ctc_loss"] == before.get("ctc_loss", 0) + 1
        assert hb.LAUNCHES["ctc_star_loss"] == before.get("ctc_star_loss", 0)
        logits = ops.linear(enc_h.reshape(-1, enc_h.shape[2]), net.ctc_lo.weight, net.ctc_lo.bias).view(len(ys), enc_h.shape[1], -1)
        want = ops.ctc_loss(logits, net.encoder.enc2.last_lens_dev, torch.cat(ys).long(), [len(y) for y in ys], True)
    assert torch.equal(got, want)
    net.train()
    with torch.no_grad():
        star = net.ctc_nll(net.encoder(xs, ilens)[0], ys)
    assert hb.LAUNCHES["ctc_star_loss"] == before.get("ctc_star_loss", 0) + 1
    assert bool((star <= got).all()) and bool((star < got).any())


def test_star_penalty_without_the_ctc_branch_raises(hb):
    with pytest.raises(ValueError):
        _tiny(ctc_star_penalty=-0.5)
    with pytest.raises(ValueError):
        _tiny(ctc_weight=0.0, ctc_star_penalty=-0.5)
