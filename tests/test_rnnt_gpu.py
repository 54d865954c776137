"""The transducer head on the GPU (csrc/rnnt.hip): the joint and loss kernels per element against the float64
restatement of tests/rnnt_ref.py, then the head in E2E, greedy decoding and a Solver run.

Tolerance of the kernel cases: none is written down here.  Every case also runs the float32 restatement (the same
recurrences in the same order, numpy) on the same inputs; a tensor's worst absolute error against float64 may be at most
4 x that float32 error, with a floor of 8 x 2^-24 x the tensor's largest magnitude where the float32 error is about zero -
the form of profiles/frontend_parity.txt.  The allowance belongs to a tensor of the call (all utterances of a batch
together), not to an utterance's slice of it: a one-row slice such as the (1, 0) lattice of the ragged batch has a float32
error that is small by luck (the rounding of one log-sum-exp near 3, ulp 2.4e-7) and its floor is then below that rounding;
a first version of this file that split the allowance by utterance measured 1.16 on such a slice.  Each case prints one
`rnnt-parity` line: worst error / allowance per tensor.

Lattices (T_b, U_b).  The chains run one wave up to 64 label positions (U + 1 <= 64), 256 threads with a position per thread
up to 256, and positions strided over the workgroup beyond: (64, 63) | (65, 64) straddle the wave, (130, 129) runs three
waves wide along an anti-diagonal, (3, 257) has 258 positions - past the workgroup."""
import functools

import numpy as np
import pytest
import torch

import poison as P
import rnnt_ref as R
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

SMALL = ((1, 0), (1, 1), (7, 0), (2, 6), (5, 3))
LARGE = ((64, 63), (65, 64), (130, 129), (3, 257))


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


def _allowance(f32, ref):
    err32 = float(np.abs(f32.astype(np.float64) - ref).max()) if ref.size else 0.0
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return max(4.0 * err32, 8.0 * 2.0 ** -24 * scale)


class _Worst(object):
    """Worst element error / allowance per tensor of a call.  A tensor is what the call returns - nll [B], dlogits, Z, dPE,
    dPP of the whole batch, its valid elements gathered utterance by utterance - and has ONE allowance, from the float32
    restatement's worst error and the largest magnitude over the same elements."""

    def __init__(self):
        self.parts = {}

    def add(self, name, got, ref, f32):
        self.parts.setdefault(name, []).append((np.ravel(got).astype(np.float64), np.ravel(ref), np.ravel(f32)))

    def ratios(self):
        out = {}
        for name, parts in self.parts.items():
            got, ref, f32 = (np.concatenate([p[i] for p in parts]) for i in range(3))
            allow = _allowance(f32, ref)
            err = float(np.abs(got - ref).max()) if ref.size else 0.0
            out[name] = err / allow if allow > 0 else (0.0 if err == 0 else np.inf)
        return out

    def check(self, what):
        ratios = self.ratios()
        print("rnnt-parity %-34s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
        for name, r in ratios.items():
            assert r <= 1.0, "%s: %s error is %.3f of its allowance" % (what, name, r)


# ------------------------------------------------------------------------------------------------ loss
@functools.lru_cache(maxsize=None)
def _loss_case(lattices, V, seed=0, T=None):
    """Logits uniform in (-3, 3), labels uniform in [1, V), upstream gradients of both signs; the float64 and float32
    restatements per utterance, computed once."""
    rs = np.random.RandomState(1000 + 7 * V + seed + sum(t * 3 + u for t, u in lattices))
    B, T, U = len(lattices), T or max(t for t, _ in lattices), max(u for _, u in lattices)
    z = rs.uniform(-3, 3, (B, T, U + 1, V)).astype(np.float32)
    ys = [rs.randint(1, V, u).astype(np.int64) for _, u in lattices]
    g = (rs.uniform(0.5, 1.5, B) * rs.choice([-1.0, 1.0], B)).astype(np.float32)
    ref = [R.loss_and_grad(z[b, :t, :u + 1], ys[b], np.float64, g[b]) for b, (t, u) in enumerate(lattices)]
    f32 = [R.loss_and_grad(z[b, :t, :u + 1], ys[b], np.float32, g[b]) for b, (t, u) in enumerate(lattices)]
    return dict(lattices=lattices, B=B, T=T, U=U, V=V, z=z, ys=ys, g=g, ref=ref, f32=f32)


def _run_loss(hb, c, pad=3, lens=None, ys=None):
    """ops.rnnt_loss on the case.  pad > 0: the logits are a [B, T, U + 1, V] view of a [.., V + pad] buffer (ld = V + pad);
    the extra columns and every padded node hold NaN.  lens / ys: other frame counts / labels than the case's (the rows a
    test means the kernels to leave unscored)."""
    import ops
    B, T, U, V = c["B"], c["T"], c["U"], c["V"]
    lens = [t for t, _ in c["lattices"]] if lens is None else list(lens)
    ys = c["ys"] if ys is None else ys
    buf = torch.full((B, T, U + 1, V + pad), float("nan"))
    for b, (_, u) in enumerate(c["lattices"]):
        buf[b, :lens[b], :u + 1, :V] = torch.from_numpy(c["z"][b, :lens[b], :u + 1])
    buf = buf.to(DEV).requires_grad_()
    labels = torch.from_numpy(np.concatenate(ys) if ys else np.zeros(0, np.int64)).to(DEV)
    nll = ops.rnnt_loss(buf[..., :V], hb.to_device_i32(lens, DEV), labels, [u for _, u in c["lattices"]])
    nll.backward(torch.from_numpy(c["g"]).to(DEV))
    return nll.detach().cpu().numpy(), buf.grad.cpu().numpy()


def _check_loss(c, nll, grad, what, unscored=()):
    """unscored: rows the call was given no frame or a label outside [1, V) for - nll +inf, the gradient exact zeros."""
    V, w = c["V"], _Worst()
    assert np.isfinite(np.delete(nll, list(unscored))).all()
    for b, (t, u) in enumerate(c["lattices"]):
        if b in unscored:
            assert nll[b] == np.inf and (grad[b] == 0).all(), "%s: utterance %d was scored" % (what, b)
            continue
        valid = np.zeros(grad.shape[1:3], bool)
        valid[:t, :u + 1] = True
        assert (grad[b][~valid] == 0).all(), "%s: utterance %d has a gradient on a padded node" % (what, b)
        assert (grad[b][:, :, V:] == 0).all() and np.isfinite(grad[b]).all()
        w.add("nll", nll[b:b + 1], np.asarray([c["ref"][b][0]]), np.asarray([c["f32"][b][0]]))
        w.add("dlogits", grad[b, :t, :u + 1, :V], c["ref"][b][1], c["f32"][b][1])
    w.check(what)


@pytest.mark.parametrize("lattice", SMALL + LARGE)
def test_loss_one_utterance(hb, lattice):
    c = _loss_case((lattice,), 34)
    _check_loss(c, *_run_loss(hb, c), "loss T=%d U=%d V=34" % lattice)


@pytest.mark.parametrize("V", (3, 34, 65))
def test_loss_ragged_batch(hb, V):
    """B = 5, padded nodes on both axes; V below, inside and across a 64-lane row; ld = V + 3."""
    c = _loss_case(SMALL, V)
    _check_loss(c, *_run_loss(hb, c), "loss ragged B=5 V=%d" % V)


def test_loss_contiguous_and_across_the_wave(hb):
    """ld = V, and a ragged batch whose longest row is past one wave of label positions while the others are not."""
    c = _loss_case(((65, 64), (5, 3), (1, 0), (64, 63)), 5)
    _check_loss(c, *_run_loss(hb, c, pad=0), "loss ragged wide V=5 ld=V")


def test_loss_is_bit_reproducible(hb):
    c = _loss_case(SMALL + ((65, 64),), 34)
    for det in (False, True):
        with hb.deterministic(det):
            a, b = _run_loss(hb, c), _run_loss(hb, c)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        first = a if not det else first
        assert np.array_equal(a[0], first[0]) and np.array_equal(a[1], first[1])       # ... and the same in both modes


# A time axis longer than every utterance of the call - what a rank of a data-parallel step hands the head, its encoder
# padded to the global T_max: (lattices, T, V of the loss, J of the joint).  The kernels give every sum one owner and the
# extent only changes strides, so the results on the frames the shorter extent has are the SAME BITS.
LONG_AXIS = ((SMALL, 12, 34, 32), (((64, 63), (5, 3)), 70, 5, 32), (((1, 0),), 9, 34, 32), (((3, 257),), 4, 5, 32))
_LONG_IDS = ["small-T12", "wave-T70", "one-node-T9", "strided-T4"]


def _trimmed(c, *keys):
    """The case on the extent of its longest utterance: the same inputs, the extra frames cut off."""
    tmax = max(t for t, _ in c["lattices"])
    assert tmax < c["T"]
    return dict(c, T=tmax, **{k: np.ascontiguousarray(c[k][:, :tmax]) for k in keys})


@pytest.mark.parametrize("pad", (3, 0))
@pytest.mark.parametrize("lattices,T,V,J", LONG_AXIS, ids=_LONG_IDS)
def test_loss_time_axis_past_every_utterance(hb, lattices, T, V, J, pad):
    """NaN on every frame t >= T_b, the extra ones included: the float64 restatement under the file's allowance, exact zeros in
    dlogits on all of them (_check_loss), and the bits of the same lattices at T = max T_b."""
    c = _loss_case(lattices, V, T=T)
    nll, grad = _run_loss(hb, c, pad=pad)
    assert grad.shape[1] == T
    what = "loss %s T=%d V=%d ld=V+%d" % (lattices if len(lattices) < 3 else "SMALL", T, V, pad)
    _check_loss(c, nll, grad, what)
    short = _trimmed(c, "z")
    nll0, grad0 = _run_loss(hb, short, pad=pad)
    assert np.array_equal(nll, nll0), "%s: nll differs from the run at T = %d" % (what, short["T"])
    assert np.array_equal(grad[:, :short["T"]], grad0), "%s: dlogits differs from the run at T = %d" % (what, short["T"])
    assert (grad[:, short["T"]:] == 0).all()
    print("rnnt-parity %-34s bit-identical to T=%d" % (what, short["T"]))


@pytest.mark.parametrize("kind", ("no frame", "label V", "label 0"))
def test_loss_leaves_one_row_unscored(hb, kind):
    """A batch of three whose middle row cannot be scored - T_b = 0, or a label outside [1, V): that row's nll is +inf and its
    gradient exact zeros (rnnt_alpha_kernel leaves log P at -inf, rnnt_grad_kernel writes zeros without reading alpha or
    beta), the other rows stay within the allowance.  No host check refuses such a row: the lengths and the labels are on
    the device."""
    c = _loss_case(((4, 2), (3, 3), (2, 1)), 34)
    lens, ys = [t for t, _ in c["lattices"]], [y.copy() for y in c["ys"]]
    if kind == "no frame":
        lens[1] = 0
    else:
        ys[1][1] = c["V"] if kind == "label V" else 0
    nll, grad = _run_loss(hb, c, lens=lens, ys=ys)
    _check_loss(c, nll, grad, "loss B=3, row 1: %s" % kind, unscored=(1,))


# ------------------------------------------------------------------------------------------------ joint
@functools.lru_cache(maxsize=None)
def _joint_case(lattices, J, T=None):
    rs = np.random.RandomState(2000 + J + sum(t * 3 + u for t, u in lattices))
    B, T, U = len(lattices), T or max(t for t, _ in lattices), max(u for _, u in lattices)
    pe = rs.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32)
    pp = rs.uniform(-1.5, 1.5, (B, U + 1, J)).astype(np.float32)
    dz = rs.uniform(-1, 1, (B, T, U + 1, J)).astype(np.float32)
    ref, f32 = [], []
    for dt, out in ((np.float64, ref), (np.float32, f32)):
        for b, (t, u) in enumerate(lattices):
            z = R.joint(pe[b, :t], pp[b, :u + 1], dt)
            out.append((z,) + R.joint_bwd(dz[b, :t, :u + 1], z, dt))
    return dict(lattices=lattices, B=B, T=T, U=U, J=J, pe=pe, pp=pp, dz=dz, ref=ref, f32=f32)


def _run_joint(hb, c):
    """ops.rnnt_joint and its backward; the upstream gradient holds NaN on every padded node (they are never read)."""
    import ops
    pe, pp = torch.from_numpy(c["pe"]).to(DEV).requires_grad_(), torch.from_numpy(c["pp"]).to(DEV).requires_grad_()
    z = ops.rnnt_joint(pe, pp, hb.to_device_i32([t for t, _ in c["lattices"]], DEV), [u for _, u in c["lattices"]])
    got_z = z.detach().cpu().numpy().copy()
    dz = torch.full(tuple(c["dz"].shape), float("nan"))
    for b, (t, u) in enumerate(c["lattices"]):
        dz[b, :t, :u + 1] = torch.from_numpy(c["dz"][b, :t, :u + 1])
    z.backward(dz.to(DEV))
    return got_z, pe.grad.cpu().numpy(), pp.grad.cpu().numpy()


def _check_joint(c, z, dpe, dpp, what):
    w = _Worst()
    for b, (t, u) in enumerate(c["lattices"]):
        valid = np.zeros(z.shape[1:3], bool)
        valid[:t, :u + 1] = True
        assert (z[b][~valid] == 0).all(), "%s: Z of utterance %d is not zero on a padded node" % (what, b)
        assert (dpe[b, t:] == 0).all() and (dpp[b, u + 1:] == 0).all() and np.isfinite(dpe).all() and np.isfinite(dpp).all()
        for name, got, k in (("Z", z[b, :t, :u + 1], 0), ("dPE", dpe[b, :t], 1), ("dPP", dpp[b, :u + 1], 2)):
            w.add(name, got, c["ref"][b][k], c["f32"][b][k])
    w.check(what)


@pytest.mark.parametrize("J", (4, 32, 260))
def test_joint_ragged_batch(hb, J):
    c = _joint_case(SMALL, J)
    _check_joint(c, *_run_joint(hb, c), "joint ragged B=5 J=%d" % J)


@pytest.mark.parametrize("lattice", SMALL + LARGE)
def test_joint_one_utterance(hb, lattice):
    c = _joint_case((lattice,), 32)
    _check_joint(c, *_run_joint(hb, c), "joint T=%d U=%d J=32" % lattice)


@pytest.mark.parametrize("lattices,T,V,J", LONG_AXIS, ids=_LONG_IDS)
def test_joint_time_axis_past_every_utterance(hb, lattices, T, V, J):
    """PE rows and NaN upstream gradients on frames that belong to no utterance: exact zeros in Z and dPE on every frame
    t >= T_b (_check_joint), the allowance, and the bits of the same lattices at T = max T_b."""
    c = _joint_case(lattices, J, T=T)
    z, dpe, dpp = _run_joint(hb, c)
    assert z.shape[1] == T and dpe.shape[1] == T
    what = "joint %s T=%d J=%d" % (lattices if len(lattices) < 3 else "SMALL", T, J)
    _check_joint(c, z, dpe, dpp, what)
    short = _trimmed(c, "pe", "dz")
    z0, dpe0, dpp0 = _run_joint(hb, short)
    n = short["T"]
    assert np.array_equal(z[:, :n], z0) and np.array_equal(dpe[:, :n], dpe0) and np.array_equal(dpp, dpp0), what
    assert (z[:, n:] == 0).all() and (dpe[:, n:] == 0).all()
    print("rnnt-parity %-34s bit-identical to T=%d" % (what, n))


def test_joint_is_bit_reproducible(hb):
    c = _joint_case(SMALL + ((65, 64),), 32)
    a, b = _run_joint(hb, c), _run_joint(hb, c)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refused_before_anything_is_written(hb):
    import ops
    pe, pp = torch.zeros(1, 2, 6, device=DEV), torch.zeros(1, 3, 6, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.rnnt_joint(pe, pp, hb.to_device_i32([2], DEV), [2])
    z = torch.full((1, 2, 3, 6), 7.0, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        hb.rnnt_joint_fwd(pe, pp, hb.to_device_i32([2], DEV), hb.to_device_i32([0, 2], DEV), z)
    assert bool((z == 7.0).all())
    with pytest.raises(hb.UnsupportedShape):
        ops.rnnt_loss(torch.zeros(1, 2, 3, 1, device=DEV), hb.to_device_i32([2], DEV), torch.ones(2, dtype=torch.long, device=DEV), [2])


# ------------------------------------------------------------------------------------------------ poisoned buffers
@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_buffers(hb, pattern):
    """The loss and the joint on the ragged batch, from an empty pool and from the leftover of a larger call in the same
    capacity class of the pool, filled with the pattern where it lay: bit-identical to the clean run.  The workspaces hold
    floats only (no integer region), and no kernel indexes by anything read from them."""
    import ops
    lc, jc = _loss_case(SMALL, 34), _joint_case(SMALL, 32)
    P.empty_pool()
    clean = _run_loss(hb, lc) + _run_joint(hb, jc)
    big_l, big_j = _loss_case(((40, 6),), 34, seed=1), _joint_case(((36, 6),), 32)
    cap = ops._row_capacity
    words = lambda c: (hb.rnnt_ws_bytes(c["B"], c["T"], c["U"], 4, c["V"]) + 3) // 4
    zn = lambda c: c["B"] * c["T"] * (c["U"] + 1) * c["J"]
    assert words(big_l) > words(lc) and cap(words(big_l)) == cap(words(lc))
    assert zn(big_j) > zn(jc) and cap(zn(big_j)) == cap(zn(jc))
    for variant in ("empty pool", "leftover"):
        P.empty_pool()
        st = P.Stats()
        if variant == "leftover":
            _run_loss(hb, big_l), _run_joint(hb, big_j)
            assert P.poison_pool(pattern, st) >= 2
        with P.poisoned(pattern, st):
            got = _run_loss(hb, lc) + _run_joint(hb, jc)
        assert st.total > 0
        for name, a, b in zip(("nll", "dlogits", "Z", "dPE", "dPP"), clean, got):
            assert np.array_equal(a, b), "%s differs under %s / %s" % (name, pattern, variant)
        print("rnnt-poison %-5s %-10s %s; bit-identical" % (pattern, variant, st.line()))


# ------------------------------------------------------------------------------------------------ head and model
def _tiny(seed=21, **kw):
    import model as M
    torch.manual_seed(seed)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw).to(DEV)
    weights = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    res = net.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("ctc_lo.", "rnnt.")) for k in res.missing_keys)
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


@pytest.mark.parametrize("ctc_weight", (None, 0.3))
def test_weight_zero_launches_the_parent_model(hb, ctc_weight):
    """The attention-only and the CTC-only model: built with rnnt_weight = 0 they give the loss and gradient bits of a model
    built without the argument (deterministic mode: outside it the fp32 atomics make no two runs of any model equal)."""
    kw = {} if ctc_weight is None else dict(ctc_weight=ctc_weight)
    off, xs, ilens, ys = _tiny(rnnt_weight=0.0, **kw)
    plain = _tiny(**kw)[0]
    assert not hasattr(off, "rnnt") and list(off.state_dict()) == list(plain.state_dict())
    before = dict(hb.LAUNCHES)
    with hb.deterministic():
        lp0, loss0 = _step(off, xs, ilens, ys)
        lp1, loss1 = _step(plain, xs, ilens, ys)
    assert not any(k.startswith("rnnt") for k in hb.LAUNCHES if hb.LAUNCHES[k] != before.get(k, 0))
    assert getattr(lp0, "rnnt_loss", None) is None
    assert torch.equal(loss0, loss1) and torch.equal(lp0, lp1)
    for (n, p), (_, q) in zip(off.named_parameters(), plain.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_three_term_loss_value(hb):
    """loss = 0.3 L_att + 0.2 sum(nll_ctc) / B + 0.5 sum(nll_rnnt) / B from the same forward; 32 fp32 ulps of the largest
    term cover the sums' and the combination's roundings."""
    net, xs, ilens, ys = _tiny(rnnt_weight=0.5, ctc_weight=0.2, rnnt_joint_dim=32)
    lp, loss = _step(net, xs, ilens, ys)
    B = len(ilens)
    att = -float(lp.detach().double().sum()) / (B * lp.shape[1])
    ctc, rnnt = float(lp.ctc_nll.detach().double().sum()) / B, float(lp.rnnt_nll.detach().double().sum()) / B
    want = 0.3 * att + 0.2 * ctc + 0.5 * rnnt
    assert rnnt > 0 and abs(float(loss.detach()) - want) <= 32 * 2.0 ** -23 * max(abs(att), abs(ctc), abs(rnnt)), (float(loss), want)
    for n, p in net.rnnt.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n


def test_head_gradients_against_float64(hb):
    """d enc_h and every parameter gradient of the head for sum(nll) / B alone, against autograd through the torch float64
    restatement fed the model's own enc_h: the project's gradient gate, worst element <= 1e-3 of its tensor's largest."""
    net, xs, ilens, ys = _tiny(rnnt_weight=0.5, ctc_weight=0.2, rnnt_joint_dim=32)
    enc_h, _ = net.encoder(xs, ilens)
    e = enc_h.detach().clone().requires_grad_()
    net.zero_grad()
    B = len(ilens)
    nll = net.rnnt_nll(e, ys)
    (nll.sum() / B).backward()
    lens = net.encoder.enc2.last_lens_dev.cpu().tolist()
    e64 = enc_h.detach().double().cpu().requires_grad_()
    p64 = {k: v.detach().double().cpu().requires_grad_() for k, v in net.rnnt.state_dict().items()}
    assert set(p64) == set(R.HEAD_KEYS)
    want = R.torch_head_nll(p64, e64, lens, [y.cpu().tolist() for y in ys], net.rnnt.bos)
    (want.sum() / B).backward()
    err = float((nll.detach().double().cpu() - want.detach()).abs().max())
    print("rnnt head nll: err %.3g of max %.3g" % (err, float(want.detach().abs().max())))
    assert err <= 1e-3 * float(want.detach().abs().max())
    got = dict(net.rnnt.named_parameters())
    for name, g, w in [("enc_h", e.grad, e64.grad)] + [(k, got[k].grad, p64[k].grad) for k in R.HEAD_KEYS]:
        err, top = float((g.double().cpu() - w).abs().max()), float(w.abs().max())
        print("rnnt head %s: err %.3g of max %.3g" % (name, err, top))
        assert top > 0 and err <= 1e-3 * top, name


# ------------------------------------------------------------------------------------------------ greedy decoding
@pytest.mark.parametrize("name", sorted(R.DECODE_CASES))
def test_greedy_decode(hb, name):
    """TransducerHead.greedy on the margin-checked inputs (test_rnnt_cpu.py holds the margin, and that the cases hit
    max_symbols, the length cap, T_b = 1 and rows that finish at different iterations): tokens and lengths exactly, scores
    within the allowance (the float32 restatement walks the same path)."""
    import model as M
    p, enc_h, lens, max_symbols, max_len = R.decode_case(name)
    d = R.DECODE_DIMS
    head = M.TransducerHead(d["V"], d["E"], d["P"], d["H"], d["J"], bos=1).to(DEV)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    with torch.no_grad():
        out, n, score = head.greedy(torch.from_numpy(enc_h).to(DEV), hb.to_device_i32(lens, DEV), max_symbols, max_len)
    out, n, score = out.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    assert out.shape == (len(lens), max_len)
    ref = [R.greedy(p, enc_h[b, :t], 1, max_symbols, max_len) for b, t in enumerate(lens)]
    f32 = [R.greedy(p, enc_h[b, :t], 1, max_symbols, max_len, dt=np.float32) for b, t in enumerate(lens)]
    for b, r in enumerate(ref):
        assert int(n[b]) == len(r["tokens"]) and out[b, :n[b]].tolist() == r["tokens"], (name, b, out[b], r["tokens"])
    w = _Worst()
    w.add("score", score, np.asarray([r["score"] for r in ref]), np.asarray([r["score"] for r in f32], np.float32))
    w.check("greedy %s" % name)


def test_recognize_rnnt(hb):
    """E2E.recognize_rnnt: id lists in recognize_ctc's layout, the device tensors in last_rnnt, and the rows of the head's
    own greedy on the model's encoder output; at most max_symbols x frames and max_dec_timesteps tokens per row."""
    net, xs, ilens, ys = _tiny(rnnt_weight=0.5, rnnt_joint_dim=32)
    net.eval()
    ids = net.recognize_rnnt(xs, ilens, max_symbols=2, max_dec_timesteps=5)
    last = net.last_rnnt
    assert len(ids) == len(ilens) and all(isinstance(r, list) for r in ids)
    frames = net.encoder.enc2.last_lens_dev.cpu().tolist()
    for b, row in enumerate(ids):
        assert len(row) == int(last["lengths"][b]) <= min(5, 2 * frames[b]) and all(1 <= k < synth.TINY["output_dim"] for k in row)
        assert last["tokens"][b, :len(row)].tolist() == row
    assert bool(torch.isfinite(last["scores"]).all()) and bool((last["scores"] <= 0).all())
    with torch.no_grad():
        enc_h, _ = net.encoder(xs, ilens)
        out, n, score = net.rnnt.greedy(enc_h, net.encoder.enc2.last_lens_dev, 2, 5)
    assert torch.equal(out, last["tokens"]) and torch.equal(n, last["lengths"])


def test_overfit_and_solver_test(hb, tmp_path, monkeypatch, capsys):
    """Four utterances, a tiny model, 40 supervised steps with rnnt_weight = 0.5: L_rnnt ends below where it started,
    validation reports val_rnnt_loss, and Solver.test with rnnt_greedy_decode runs and reports a CER."""
    import test_ctc_gpu as TC
    solver, dev = TC._solver(str(tmp_path / "s"), monkeypatch, rnnt_weight=0.5, rnnt_joint_dim=32, learning_rate=5e-3)
    assert hasattr(solver.model, "rnnt")
    xs, ilens, ys = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], [12, 11, 9, 6], [4, 3, 3, 2], 17)
    xs, ys = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]

    def l_rnnt():
        solver.model.eval()
        with torch.no_grad():
            _, lp, _, _ = solver.model(xs, ilens, ys=ys)
        solver.model.train()
        return float(lp.rnnt_loss)

    first = l_rnnt()
    np.random.seed(4)
    for _ in range(40):
        loss = solver.sup_train_one_iteration(xs, ilens, ys, 1.0)
    solver.flush()
    last = l_rnnt()
    print("rnnt overfit: L_rnnt %.4f -> %.4f after 40 steps" % (first, last))
    assert np.isfinite(float(loss)) and last < first and not hb.persist_aborted(dev)
    capsys.readouterr()
    solver.validation()
    assert solver.val_rnnt_loss is not None and "val_rnnt_loss=" in capsys.readouterr().out
    solver.config["rnnt_greedy_decode"] = True
    cer = solver.test(state_dict={k: v.clone() for k, v in solver.model.state_dict().items()})
    assert np.isfinite(cer) and cer >= 0 and solver.last_test["cer"] == cer
    assert "CER=" in capsys.readouterr().out
    solver.config["beam_size"] = 4
    with pytest.raises(ValueError, match="does not combine"):
        solver.test(state_dict=solver.model.state_dict())


def test_checkpoint_without_the_head(hb, tmp_path, monkeypatch, capsys):
    """A checkpoint without the head loads into a model with it (the head keeps its initialisation); its optimiser state
    does not."""
    import test_ctc_gpu as TC
    solver, dev = TC._solver(str(tmp_path / "s"), monkeypatch, rnnt_weight=0.3, rnnt_joint_dim=32)
    head = {k: v.detach().clone() for k, v in solver.model.state_dict().items() if k.startswith("rnnt.")}
    assert len(head) == len(R.HEAD_KEYS)
    old = {k: torch.from_numpy(v) + 0.5 for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    path = str(tmp_path / "old")
    torch.save(old, path + ".ckpt")
    capsys.readouterr()
    solver.load_model(path, False)
    assert capsys.readouterr().out.count("keeps its initialisation") == 1
    sd = solver.model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in head.items()) and all(torch.equal(sd[k].cpu(), v) for k, v in old.items())
    with pytest.raises(RuntimeError, match="transducer head"):
        solver.load_model(path, True)
