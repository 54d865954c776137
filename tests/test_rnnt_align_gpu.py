"""Transducer forced alignment on the GPU (csrc/rnnt_align.hip, ops.rnnt_align, E2E.align_rnnt, Solver.align_rnnt)
against the float64 restatement tests/rnnt_align_ref.py.

Grid: the lattices (T_b, U_b) of tests/test_rnnt_gpu.py - (64, 63) | (65, 64) straddle the wave of label positions, (130, 129)
runs three waves wide along an anti-diagonal and two back-pointer words past the first, (3, 257) is past the workgroup
(positions strided) - each alone and in a ragged batch of five, at V = 3, 34, 65 with ld = V + 3 and NaN on every padded node
and in the extra columns.  The back-pointers have ONE storage path (the workspace), so the grid has no case for a switch.

Tolerance: none is written down here.  score, token_logp and blank_logp of a call are one tensor each (all utterances
together) with the allowance of tests/test_rnnt_gpu.py: 4 x the float32 restatement's worst error, with a floor of
8 x 2^-24 x the tensor's largest magnitude.  emit_frame and frame_labels must EQUAL the float64 path: every case is decisive
(tests/test_rnnt_align_cpu.py holds that), none is left out.  Each case prints one `rnnt-align-parity` line: worst error /
allowance per tensor."""
import numpy as np
import pytest
import torch

import poison as P
import rnnt_align_ref as A
import rnnt_ref as R
from test_rnnt_align_cpu import check_structure

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("score", "emit_frame", "token_logp", "frame_labels", "blank_logp")


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


def _logits(c, pad, lens=None):
    """The case's logits as a [B, T, U + 1, V] view of a [.., V + pad] buffer: NaN in the extra columns and on every node
    off an utterance's lattice (lens: other frame counts than the case's)."""
    lat, V = c["lattices"], c["V"]
    B, T, U = len(lat), max(t for t, _ in lat), max(u for _, u in lat)
    buf = torch.full((B, T, U + 1, V + pad), float("nan"))
    for b, x in enumerate(c["utts"]):
        n = x["T"] if lens is None else lens[b]
        buf[b, :n, :x["U"] + 1, :V] = torch.from_numpy(x["z"][:n])
    return buf.to(DEV)[..., :V]


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS}


def _run(hb, c, pad=3, lens=None, ys=None):
    """ops.rnnt_align on the case -> the outputs on the host.  lens / ys: other frame counts / labels than the case's (the
    rows a test means the kernels to leave unaligned)."""
    import ops
    ys = [x["y"] for x in c["utts"]] if ys is None else ys
    z = _logits(c, pad, lens).requires_grad_()                  # (forward only: accepted, nothing recorded)
    labels = torch.from_numpy(np.concatenate(ys).astype(np.int64)).to(DEV)
    frame_lens = hb.to_device_i32([x["T"] for x in c["utts"]] if lens is None else list(lens), DEV)
    res = ops.rnnt_align(z, frame_lens, labels, [len(y) for y in ys])
    assert not res.score.requires_grad and res.score.grad_fn is None
    assert res.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(y) for y in ys])]).tolist()
    return _host(res)


def _rows(c, out):
    """The outputs utterance by utterance: (b, utterance, score, emit_frame, token_logp, frame_labels, blank_logp)."""
    o = 0
    for b, x in enumerate(c["utts"]):
        sl = slice(o, o + x["U"])
        yield b, x, out["score"][b], out["emit_frame"][sl], out["token_logp"][sl], out["frame_labels"][b], out["blank_logp"][b]
        o += x["U"]


def _check(c, out, what, nll=None):
    """Per element against float64 under the case's allowances, the integer outputs exactly, the structural identities,
    score = the sum of its parts, the padding; nll: ops.rnnt_loss on the same logits - the bound."""
    worst = dict(score=0.0, token_logp=0.0, blank_logp=0.0, parts=0.0)
    allow = c["allow"]
    for b, x, score, emit, tlp, fl, bl in _rows(c, out):
        T, U, r = x["T"], x["U"], x["ref"]
        assert (fl[T:] == -1).all() and (bl[T:] == 0).all(), "%s: utterance %d behind its %d frames" % (what, b, T)
        check_structure(emit, fl[:T], T, U)
        assert emit.tolist() == r["emit_frame"].tolist(), "%s: utterance %d (gap %.3g)" % (what, b, r["gap"])
        assert fl[:T].tolist() == r["frame_labels"].tolist(), "%s: utterance %d" % (what, b)
        assert np.isfinite(score) and np.isfinite(tlp).all() and np.isfinite(bl).all()
        worst["score"] = max(worst["score"], abs(float(score) - float(r["score"])) / allow["score"])
        if U:
            worst["token_logp"] = max(worst["token_logp"], float(np.abs(tlp.astype(np.float64) - r["token_logp"]).max()) / allow["token_logp"])
        worst["blank_logp"] = max(worst["blank_logp"], float(np.abs(bl[:T].astype(np.float64) - r["blank_logp"]).max()) / allow["blank_logp"])
        parts = float(tlp.astype(np.float64).sum() + bl[:T].astype(np.float64).sum())
        worst["parts"] = max(worst["parts"], abs(parts - float(score)) / allow["score"])
        if nll is not None:
            assert float(score) <= -float(nll[b]) + allow["score"], "%s: utterance %d beats the likelihood" % (what, b)
            if U == 0 or T == 1:
                assert abs(float(score) + float(nll[b])) <= allow["score"], "%s: utterance %d has one path" % (what, b)
    print("rnnt-align-parity %-28s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for name, ratio in worst.items():
        assert ratio <= 1.0, "%s: %s error is %.3f of its allowance" % (what, name, ratio)


def _what(lattices, V):
    return ("T=%d U=%d" % lattices[0] if len(lattices) == 1 else "ragged B=%d to T=%d U=%d" % (
        len(lattices), max(t for t, _ in lattices), max(u for _, u in lattices))) + " V=%d" % V


@pytest.mark.parametrize("lattices,V", A.GRID, ids=lambda v: str(v).replace(" ", ""))
def test_align_against_float64(hb, lattices, V):
    import ops
    c = A.case(lattices, V)
    out = _run(hb, c)
    labels = torch.from_numpy(np.concatenate([x["y"] for x in c["utts"]])).to(DEV)
    nll = ops.rnnt_loss(_logits(c, 3), hb.to_device_i32([t for t, _ in lattices], DEV), labels, [u for _, u in lattices])
    _check(c, out, _what(lattices, V), nll=nll.cpu().numpy())


def test_contiguous_logits(hb):
    c = A.case(A.SMALL, 34)
    _check(c, _run(hb, c, pad=0), "ragged B=5 V=34 ld=V")


@pytest.mark.parametrize("T,U", [(5, 3), (65, 64)])
def test_tie_rule_on_the_device(hb, T, U):
    """All-zero logits: every path ties exactly, in fp32 too.  The blank predecessor wins: every label at frame 0, and the
    score is the float32 restatement's to the bit."""
    import ops
    V = 5
    z, y = np.zeros((T, U + 1, V), np.float32), np.arange(U, dtype=np.int64) % (V - 1) + 1
    res = ops.rnnt_align(torch.from_numpy(z).to(DEV)[None], hb.to_device_i32([T], DEV), torch.from_numpy(y).to(DEV), [U])
    out, r32 = _host(res), A.viterbi(z, y, np.float32)
    assert out["emit_frame"].tolist() == [0] * U == r32["emit_frame"].tolist()
    assert out["frame_labels"][0].tolist() == [U] * T
    assert out["score"].view(np.int32)[0] == np.float32(r32["score"]).view(np.int32), (out["score"][0], r32["score"])


def _same_bits(a, b, what):
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), "%s: %s differs" % (what, k)


def _row_of(c, out, b):
    """Utterance b's slice of a batch's outputs, in the shapes of a run of that utterance alone."""
    _, x, score, emit, tlp, fl, bl = list(_rows(c, out))[b]
    return dict(score=np.asarray([score]), emit_frame=emit, token_logp=tlp, frame_labels=fl[None, :x["T"]], blank_logp=bl[None, :x["T"]])


@pytest.mark.parametrize("lattices,V", [(A.BATCHES[0], 34), (A.BATCHES[1], 3)], ids=["small-V34", "large-V3"])
def test_same_bits_in_every_run_and_for_a_row_alone(hb, lattices, V):
    c = A.case(lattices, V)
    for det in (False, True):
        with hb.deterministic(det):
            a, again = _run(hb, c), _run(hb, c)
        _same_bits(a, again, "two calls")
        first = a if not det else first
        _same_bits(a, first, "deterministic mode")
    for b, lat in enumerate(lattices):
        alone = _run(hb, A.case((lat,), V))
        _same_bits(_row_of(c, a, b), alone, "T=%d U=%d alone / in the batch" % lat)
        assert (a["frame_labels"][b, lat[0]:] == -1).all() and (a["blank_logp"][b, lat[0]:] == 0).all()


def test_rows_that_cannot_be_aligned(hb):
    """A batch of six whose rows 1, 2, 4 and 5 cannot be aligned - no frame, a label V, a label 0, more labels than the
    launch holds (that one needs hb.rnnt_align: ops sizes the launch by the longest row): score -inf, emit_frame -1,
    token_logp -inf, frame_labels -1, blank_logp 0 for those rows alone; rows 0 and 3 have the bits of a run without them."""
    import ops
    lattices, V = ((4, 2), (3, 3), (2, 1), (5, 3), (3, 2), (2, 3)), 34
    c = A.case(lattices, V)
    lens = [4, 0, 2, 5, 3, 2]
    ys = [x["y"].copy() for x in c["utts"]]
    ys[2][0], ys[4][1] = V, 0
    ys[5] = np.concatenate([ys[5], [1, 2]])                    # five labels on a launch for three
    counts = [len(y) for y in ys]
    offs = np.concatenate([[0], np.cumsum(counts)])
    B, T, U, total = len(lattices), 5, 3, int(offs[-1])
    z = _logits(c, 3, lens)
    i32, f32 = dict(device=DEV, dtype=torch.int32), dict(device=DEV, dtype=torch.float32)
    res = ops.RnntAlignment(score=torch.empty(B, **f32), emit_frame=torch.empty(total, **i32), token_logp=torch.empty(total, **f32),
                            frame_labels=torch.empty(B, T, **i32), blank_logp=torch.empty(B, T, **f32))
    ws = torch.empty(hb.rnnt_align_ws_bytes(B, T, U, V) // 4, **f32)
    hb.rnnt_align(z, z.stride(2), hb.to_device_i32(lens, DEV), torch.from_numpy(np.concatenate(ys)).to(DEV),
                  hb.to_device_i32(offs.tolist(), DEV), res.score, res.emit_frame, res.token_logp, res.frame_labels, res.blank_logp, ws)
    out = _host(res)
    for b in (1, 2, 4, 5):
        sl = slice(offs[b], offs[b + 1])
        assert np.isneginf(out["score"][b]) and (out["emit_frame"][sl] == -1).all() and np.isneginf(out["token_logp"][sl]).all()
        assert (out["frame_labels"][b] == -1).all() and (out["blank_logp"][b] == 0).all()
    good = A.case((lattices[0], lattices[3]), V)
    alone = _run(hb, good)
    _check(good, alone, "the rows that can be aligned")
    for k, b in enumerate((0, 3)):
        sl = slice(offs[b], offs[b + 1])
        got = dict(score=out["score"][b:b + 1], emit_frame=out["emit_frame"][sl], token_logp=out["token_logp"][sl],
                   frame_labels=out["frame_labels"][b:b + 1, :lens[b]], blank_logp=out["blank_logp"][b:b + 1, :lens[b]])
        _same_bits(got, _row_of(good, alone, k), "row %d beside rows that cannot be aligned" % b)
    # through ops: the kinds it can express
    via_ops = _run(hb, A.case(lattices[:5], V), lens=lens[:5], ys=ys[:5])
    assert np.isneginf(via_ops["score"][[1, 2, 4]]).all() and np.array_equal(via_ops["score"][[0, 3]], out["score"][[0, 3]])


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_buffers(hb, pattern):
    """The ragged batches (one wave; three waves and strided positions, two back-pointer words) with every torch.empty of the
    call - outputs and workspace - filled with the pattern, from an emptied pool and behind a larger call whose freed
    memory the allocator hands back: bit-identical to the clean run.  The workspace's back-pointer words are integers in a
    float tensor; the backtrace reads only the words its chain wrote (rnnt_align_chain_kernel, `only words the chain has
    written`), and its steps are bounded by the lattice whatever a word holds."""
    cases = [A.case(A.BATCHES[0], 34), A.case(A.BATCHES[1], 3)]
    big = A.case(((40, 6), (7, 0)), 34)
    P.empty_pool()
    clean = [_run(hb, c) for c in cases]
    for variant in ("empty pool", "leftover"):
        P.empty_pool()
        st = P.Stats()
        if variant == "leftover":
            _run(hb, big)
            P.poison_pool(pattern, st)
        with P.poisoned(pattern, st):
            got = [_run(hb, c) for c in cases]
        assert st.total > 0
        for c, a, b in zip(cases, clean, got):
            _same_bits(a, b, "%s / %s" % (pattern, variant))
        print("rnnt-align-poison %-5s %-10s %s; bit-identical" % (pattern, variant, st.line()))


def test_launches_and_refused_shapes(hb):
    import ops
    c = A.case(A.SMALL, 34)
    before = dict(hb.LAUNCHES)
    _run(hb, c)
    assert {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)} == {"rnnt_align": 1, "rnnt_align_launch": 2}
    lens, one = hb.to_device_i32([2], DEV), torch.ones(2, dtype=torch.long, device=DEV)
    with pytest.raises(hb.UnsupportedShape):
        ops.rnnt_align(torch.zeros(1, 2, 3, 1, device=DEV), lens, one, [2])
    with pytest.raises(ValueError):
        ops.rnnt_align(torch.zeros(1, 2, 4, 5, device=DEV), lens, one, [2])            # four label positions for two labels
    with pytest.raises(ValueError):
        ops.rnnt_align(torch.zeros(1, 2, 3, 5, device=DEV), lens, one[:1], [2])


# ------------------------------------------------------------------------------------------------ model and solver
def _head_logits(p, enc_h, T, y, bos):
    """TransducerHead.logits of one utterance from the head's parameters, in the dtype of `p` (tests/rnnt_ref.py's cell)."""
    h = c = enc_h.new_zeros(p["lstm.weight_hh_l0"].shape[1])
    hs = []
    for tok in [bos] + y:
        h, c = R._cell(p, tok, h, c, torch)
        hs.append(h)
    pe = enc_h[:T] @ p["lin_enc.weight"].t() + p["lin_enc.bias"]
    pp = torch.stack(hs) @ p["lin_pred.weight"].t()
    return (torch.tanh(pe[:, None, :] + pp[None, :, :]) @ p["lin_out.weight"].t() + p["lin_out.bias"]).numpy()


def _tiny(**kw):
    import test_rnnt_gpu as TR
    net, xs, ilens, ys = TR._tiny(**kw)
    net.eval()
    return net, xs, ilens, ys


def test_model_align_rnnt(hb):
    """E2E.align_rnnt on the tiny model: the float64 restatement of the head from the model's own weights and encoder
    output - scores within the allowance (the float32 restatement is the same head in torch float32), frames exact (the
    inputs are decisive: asserted); two calls give the same bits; one record per utterance in forward's layout."""
    net, xs, ilens, ys = _tiny(rnnt_weight=0.5, rnnt_joint_dim=32)
    hb.LAUNCHES.clear()
    out = net.align_rnnt(xs, ilens, ys)
    assert hb.LAUNCHES["rnnt_align"] == 1
    res = net.last_rnnt_alignment
    assert net.align_rnnt(xs, ilens, ys) == out
    _same_bits(_host(res), _host(net.last_rnnt_alignment), "two calls")
    with torch.no_grad():
        enc_h, _ = net.encoder(xs, ilens)
    frames = net.encoder.enc2.last_lens_dev.cpu().tolist()
    assert frames == [-(-n // net.time_reduction) for n in ilens] == [o["frames"] for o in out]
    ref, f32 = [], []
    for dt, rows in ((torch.float64, ref), (torch.float32, f32)):
        p = {k: v.detach().to(dt).cpu() for k, v in net.rnnt.state_dict().items()}
        e = enc_h.detach().to(dt).cpu()
        for b, y in enumerate(ys):
            y = y.cpu().tolist()
            rows.append(A.viterbi(_head_logits(p, e[b], frames[b], y, net.rnnt.bos), y, np.float64 if dt == torch.float64 else np.float32))
    allow = A.allowance([r["score"] for r in f32], [r["score"] for r in ref])
    assert all(r["gap"] > 2.0 * allow for r in ref), ([r["gap"] for r in ref], allow)
    worst = 0.0
    for b, (o, r) in enumerate(zip(out, ref)):
        assert o["tokens"] == ys[b].cpu().tolist() and o["frame"] == r["emit_frame"].tolist(), b
        assert res.frame_labels[b, :frames[b]].cpu().tolist() == r["frame_labels"].tolist()
        worst = max(worst, abs(o["score"] - float(r["score"])) / allow)
        np.testing.assert_allclose(o["confidence"], np.exp(r["token_logp"]), rtol=1e-3)
        assert all(0.0 < v <= 1.0 for v in o["confidence"])
    print("rnnt-align-parity %-28s score %.3f" % ("tiny model", worst))
    assert worst <= 1.0
    # a row that cannot be aligned: the blank as a label (an index the embedding holds, so the prediction network runs)
    bad = net.align_rnnt(xs, ilens, ys[:-1] + [torch.zeros_like(ys[-1])])[-1]
    assert bad["score"] == -np.inf and set(bad["frame"]) == {-1} and set(bad["confidence"]) == {0.0}


def test_model_without_the_head(hb):
    net, xs, ilens, ys = _tiny(ctc_weight=0.3)
    hb.LAUNCHES.clear()
    with pytest.raises(ValueError, match="transducer head"):
        net.align_rnnt(xs, ilens, ys)
    assert not hb.LAUNCHES                                                   # before any launch


def test_ctc_align_beside_the_transducer_head(hb):
    """A model with both heads: E2E.align returns the CTC head's alignment - what tests/test_ctc_align_gpu.py holds it to -
    and the same records before and after align_rnnt."""
    import test_ctc_align_gpu as TA
    net, xs, ilens, ys = _tiny(rnnt_weight=0.4, ctc_weight=0.3, rnnt_joint_dim=32)
    before = net.align(xs, ilens, ys)
    ctc = net.last_alignment
    net.align_rnnt(xs, ilens, ys)
    assert net.align(xs, ilens, ys) == before
    assert set(before[0]) == {"tokens", "first", "last", "confidence", "score", "frames"}
    with torch.no_grad():
        logits, _, _ = net._ctc_logits(xs, ilens, "test")
    z = logits.cpu().numpy()
    frames = net.encoder.enc2.last_lens_dev.cpu().tolist()
    utts = [(frames[b], ys[b].cpu().tolist()) for b in range(len(ilens))]
    TA._check(dict(z=z, utts=utts, V=z.shape[2], **TA._restated(z, utts)), ctc, "both heads")


def test_solver_align_rnnt(hb, tmp_path, monkeypatch):
    import test_ctc_gpu as TC
    solver, dev = TC._solver(str(tmp_path), monkeypatch, rnnt_weight=0.3, rnnt_joint_dim=32)
    assert solver.model.training
    records = solver.align_rnnt()
    assert solver.model.training                                             # the mode it was called in
    symbols = {i: s for s, i in solver.vocab.items()}
    want = [[symbols[int(i)] for i in y.reshape(-1).tolist()] for _, _, ys in solver._feed(solver.dev_loader, sharded=False) for y in ys]
    assert len(records) == 4 == len(want) and [r["tokens"] for r in records] == want      # the loader's count and order
    for rec in records:
        assert set(rec) == {"tokens", "frame", "confidence", "score", "frames"}
        assert len(rec["tokens"]) == len(rec["frame"]) == len(rec["confidence"]) and np.isfinite(rec["score"]) and rec["score"] < 0
        assert rec["frame"] == sorted(rec["frame"]) and all(0 <= f < rec["frames"] for f in rec["frame"])
        assert all(0.0 < v <= 1.0 for v in rec["confidence"])
    solver.model.eval()
    assert [r["tokens"] for r in solver.align_rnnt(solver.dev_loader)] == want and not solver.model.training
    solver.model.train()
