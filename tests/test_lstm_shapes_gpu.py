"""The LSTM sequence kernels (csrc/lstm_persist.hip, csrc/lstm.hip) through ops.lstm_layer against a float64 restatement of
the same operation (O.lstm_direction per direction, gradients by autograd), across what the launchers dispatch on: the
five compiled widths and the widths without an instantiation, the three arithmetics and the `+gather` flag, the 4- / 8- /
16-row groups and the consecutive launches over row blocks they lead to, the two memory layouts (time-major padded and
packed rows), recurrences of hundreds of steps, and gate pre-activations far inside the saturated range of
asr_fast_sigmoid / asr_fast_tanh.  Every case names the hb.LAUNCHES keys it must leave behind, so a silent change of
dispatch fails; y, dx and every parameter gradient are held to the float64 reference tensor-wide, y and dx also within
each utterance (y: and each direction's half of the feature axis) against that utterance's own scale, and the padding
frames / padding rows of y and dx hold exact zeros whatever the upstream gradient holds there.

dx is the sum of both directions' input gradients and has no halves: it is checked per utterance.  The exemption cap
counts an utterance as exempt when any of its parts is (y of either direction, dx).

    python tests/test_lstm_shapes_gpu.py --record [--out FILE]

writes, per case, the error of the GPU against float64 beside the error of the same restatement evaluated in fp32 on the
CPU, and the launch keys taken (profiles/lstm_shapes_parity.jsonl)."""
import functools
import json
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "semi-supervised-asr_amd"), os.path.join(_ROOT, "tests", "golden")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu

# The limits the project holds the LSTM to (test_lstm_persistent_path, _packed_lstm_case in tests/test_hip_parity.py):
# relative to the largest reference value of the tensor, plus ATOL - or, per utterance, relative to that utterance's own
# largest reference value plus 8 fp32 ulps of the tensor's largest (the floor of _allowance in tests/test_ctc_gpu.py).
RTOL_Y = 1e-4
RTOL_GRAD = 1e-3
RTOL_GRAD_BF16X3_LONG = 5e-3         # bf16x3 on recurrences longer than LONG_T steps: what test_big_configs_gpu.py records at cfg-5
LONG_T = 64
ATOL = 1e-5
EXEMPT_BELOW = 1e-4                  # an utterance whose own reference maximum is below this share of the tensor's: its gradient
EXEMPT_ONE_IN = 10                   # vanished under saturation; at most one utterance in EXEMPT_ONE_IN of a case

PNAMES = ("w_ih", "w_hh", "b_ih", "b_hh")
PERSIST_WIDTHS = (128, 256, 320, 512, 640)


def _gpu():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------------------ cases
# Dispatch (csrc/lstm_persist.hip: rows_per_group, fwd_rows16, bwd_kernel_kind; hip_backend.lstm_seq_fwd / lstm_seq_bwd):
#   rows per XCD group: 4 while B <= 4 * (8 / ndir), else 8; a launch covers rows * (8 / ndir) utterances, further ones follow
#   in consecutive launches; the forward at H = 512 in a split-bf16 arithmetic takes 16 rows per group for every block of
#   16 * (8 / ndir) utterances still left.
#   backward kernel `kind`:          H = 128, 256, 512            H = 320                 H = 640
#     f32                            gathered dG, fp32 operands   the same                none (the forward declines too)
#     bf16x6                         exchanged, dW_hh unfused     the same                its own exchanged kernel, unfused
#     bf16x3                         exchanged, dW_hh fused       gathered, two terms     none
#     bf16x3+gather                  gathered, two terms          the same                none
#     bf16x6+gather                  gathered, three terms        the same                none
#                                    (none at H = 512: 171 KB of LDS)
#   any other width: per-step kernels both ways.
# fwd / bwd: "persist" or "step" - hb.count_path increments LAUNCHES["lstm_fwd_" + fwd] and LAUNCHES["lstm_bwd_" + bwd] once
# per call of the sequence operator (not once per row block, and once whether asr_lstm_seq_bwd_persist_w or, after it
# declined, asr_lstm_seq_bwd_persist ran).
# dw: what asr_lstm_bwd_persist_fuses_dw(H, arith) must answer for the case - -1 no persistent backward, 0 the exchanged
# kernel that leaves dW_hh to the caller, 1 a kernel that sums dW_hh itself.
BWD_KINDS = {"step": -1, "exchanged-unfused": 0, "exchanged": 1, "gathered-f32": 1, "gathered-split": 1}


def _c(tag, H, B, T, ndir=2, arith="bf16x6", layout="tm", fwd="persist", kind="exchanged-unfused", I=24, sub=1, lens=None,
       sat=False, seed=0):
    name = "%s-H%d-B%d-T%d-%s-%s-%s" % (tag, H, B, T, "bi" if ndir == 2 else "uni", arith, layout)
    if I != 24:
        name += "-I%d" % I
    bwd = "step" if kind == "step" else "persist"
    return pytest.param(dict(name=name, H=H, B=B, T=T, ndir=ndir, arith=arith, layout=layout, fwd=fwd, bwd=bwd, kind=kind,
                             I=I, sub=sub, lens=lens, sat=sat, seed=seed), id=name)


CASES = []
# row-group boundaries at H = 512, bidirectional: 4 | 8 rows per group, a second launch of one row, the 16-row forward block
# with and without a remainder behind it - in both layouts
for _B, _tag in ((16, "last-4-row-groups"), (17, "first-8-row-groups"), (32, "one-full-launch"), (33, "one-row-second-launch"),
                 (63, "below-16-row-forward"), (64, "16-row-forward"), (65, "16-row-forward-and-one-row")):
    for _layout in ("tm", "packed"):
        CASES.append(_c(_tag, 512, _B, 5, layout=_layout, sub=2))
# ... unidirectional: 4 | 8 rows at 32 | 33, a second launch at 64 | 65, the 16-row forward at 127 | 128
for _B, _tag in ((32, "last-4-row-groups"), (33, "first-8-row-groups"), (64, "one-full-launch"), (65, "one-row-second-launch"),
                 (127, "below-16-row-forward"), (128, "16-row-forward")):
    CASES.append(_c(_tag, 512, _B, 4, ndir=1))
# two-term products: the 16-row forward with NT = 2, the exchanged backward with NT = 2 and a one-row second launch
CASES += [_c("16-row-forward-two-terms", 512, 65, 5, arith="bf16x3", kind="exchanged"),
          _c("one-row-second-launch-two-terms", 512, 33, 5, arith="bf16x3", kind="exchanged")]
# widths x arithmetics
for _H in (128, 256):
    CASES += [_c("width", _H, 9, 6, arith="bf16x6", kind="exchanged-unfused"),
              _c("width", _H, 9, 6, arith="bf16x3", kind="exchanged"),
              _c("width", _H, 9, 6, arith="f32", kind="gathered-f32"),
              _c("width", _H, 9, 6, arith="bf16x3+gather", kind="gathered-split"),
              _c("width", _H, 9, 6, arith="bf16x6+gather", kind="gathered-split")]
CASES += [_c("width", 320, 9, 6, arith="bf16x6", kind="exchanged-unfused"),
          _c("width-no-two-term-exchange", 320, 9, 6, arith="bf16x3", kind="gathered-split"),
          _c("width", 320, 9, 6, arith="f32", kind="gathered-f32"),
          _c("width", 512, 9, 6, arith="f32", kind="gathered-f32"),
          _c("width", 512, 9, 6, arith="bf16x3+gather", kind="gathered-split"),
          _c("width-backward-declines-171KB-LDS", 512, 9, 6, arith="bf16x6+gather", kind="step"),
          _c("judge-width", 640, 9, 6, ndir=1, arith="bf16x6", kind="exchanged-unfused"),
          _c("judge-width-backward-declines", 640, 9, 6, ndir=1, arith="bf16x3", kind="step"),
          _c("judge-width-both-decline", 640, 9, 6, ndir=1, arith="f32", fwd="step", kind="step")]
# no instantiation of the persistent kernels: per-step both ways
for _H in (16, 48, 192, 384):
    for _B in (5, 33):
        CASES.append(_c("no-instantiation", _H, _B, 6, fwd="step", kind="step"))
# long recurrences, ragged
CASES += [_c("long", 128, 3, 300, arith="bf16x6", kind="exchanged-unfused"),
          _c("long", 128, 3, 300, arith="f32", kind="gathered-f32"),
          _c("long", 128, 3, 300, arith="bf16x3", kind="exchanged"),
          _c("long-most-rows-finished", 512, 4, 200, arith="bf16x6", layout="packed", sub=2, lens=[200, 131, 2, 1]),
          _c("long-most-rows-finished", 512, 4, 200, arith="f32", kind="gathered-f32", layout="packed", sub=2, lens=[200, 131, 2, 1]),
          _c("long-judge-width", 640, 2, 120, ndir=1, arith="bf16x6")]
# saturated gates
for _H in (128, 512):
    CASES += [_c("saturated", _H, 6, 7, arith="bf16x6", sat=True), _c("saturated", _H, 6, 7, arith="f32", kind="gathered-f32", sat=True)]
# degenerate shapes
for _H in (512, 16):
    _kw = dict(fwd="step", kind="step") if _H == 16 else {}
    CASES += [_c("one-step", _H, 1, 1, **_kw), _c("one-step", _H, 2, 1, **_kw), _c("one-step", _H, 17, 1, **_kw),
              _c("all-lengths-one", _H, 5, 3, lens=[1] * 5, **_kw), _c("one-utterance", _H, 1, 9, **_kw)]
CASES += [_c("feature-width-input", 128, 9, 6, I=80), _c("narrow-input", 128, 9, 6, I=4)]


def _want(case):
    return {"lstm_fwd_" + case["fwd"]: 1, "lstm_bwd_" + case["bwd"]: 1}


def _rtol_grad(case):
    return RTOL_GRAD_BF16X3_LONG if case["arith"].startswith("bf16x3") and case["T"] > LONG_T else RTOL_GRAD


# ----------------------------------------------------------------------------------------------------------- inputs
def _lens(case, g):
    B, T = case["B"], case["T"]
    if case["lens"] is not None:
        lens = list(case["lens"])
    else:
        lens = [int(v) for v in torch.randint(1, T + 1, (B,), generator=g)]
        lens[0] = T
        if B >= 3:
            lens[-1] = 1
        lens = sorted(lens, reverse=True)
    assert len(lens) == B and lens[0] == max(lens) and (B < 3 or T == 1 or min(lens) == 1 or case["lens"] is not None)
    return lens


@functools.lru_cache(maxsize=None)
def _inputs_of(name):
    return _inputs(CASE_BY_NAME[name])


def _inputs(case):
    """fp32 inputs on the CPU: x [B, T, I] zero behind each length, the torch-layout parameters per direction, the upstream
    gradient dy [B, T, ndir H] with noise on the padding frames too.  Saturated cases: inputs scaled so that W_ih x has a
    standard deviation near 8, and one gate column in five with a bias drawn at a standard deviation of 45."""
    H, B, T, I, ndir = (case[k] for k in ("H", "B", "T", "I", "ndir"))
    g = torch.Generator().manual_seed(7919 * H + 131 * B + 17 * T + 3 * I + ndir + 100003 * case["seed"])
    lens = _lens(case, g)
    k = 1.0 / np.sqrt(H)
    x = torch.randn(B, T, I, generator=g)
    if case["sat"]:
        x = x * float(8.0 / (k * np.sqrt(I / 3.0)))
    for b, n in enumerate(lens):
        x[b, n:] = 0.0
    prm = []
    for d in range(ndir):
        prm += [torch.empty(4 * H, I).uniform_(-k, k, generator=g), torch.empty(4 * H, H).uniform_(-k, k, generator=g),
                torch.empty(4 * H).uniform_(-k, k, generator=g), torch.empty(4 * H).uniform_(-k, k, generator=g)]
        if case["sat"]:
            wide = (torch.rand(4 * H, generator=g) < 0.2).float()
            prm[-2] = prm[-2] + wide * torch.randn(4 * H, generator=g) * 45.0
    dy = torch.randn(B, T, ndir * H, generator=g)
    return dict(x=x, lens=lens, prm=prm, dy=dy, seed_pad=int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))


# -------------------------------------------------------------------------------------------------------- reference
def _reference(case, inp, dtype):
    """O.lstm_direction per direction in `dtype` on the CPU, gradients of (y * dy).sum() by autograd -> y [B, T, ndir H], dx
    [B, T, I], prm = the gradients in the order of the parameters."""
    p = [t.detach().to(dtype).requires_grad_(True) for t in inp["prm"]]
    xc = inp["x"].detach().to(dtype).requires_grad_(True)
    y = torch.cat([O.lstm_direction(xc, inp["lens"], *p[4 * d:4 * d + 4], reverse=(d == 1)) for d in range(case["ndir"])], 2)
    grads = torch.autograd.grad((y * inp["dy"].to(dtype)).sum(), [xc] + p)
    return dict(y=y.detach(), dx=grads[0], prm=list(grads[1:]))


@functools.lru_cache(maxsize=None)
def _references_of(name):
    """(float64 checker, fp32 yardstick) of a case: computed once, shared, never modified."""
    case = CASE_BY_NAME[name]
    inp = _inputs_of(name)
    return _reference(case, inp, torch.float64), _reference(case, inp, torch.float32)


def _preactivations(case, inp, ref):
    """The gate pre-activations of the live frames in float64, from the reference's own outputs: W_ih x_t + b + W_hh h_prev."""
    H, T = case["H"], case["T"]
    x = inp["x"].double()
    out = []
    for d in range(case["ndir"]):
        w_ih, w_hh, b_ih, b_hh = (t.double() for t in inp["prm"][4 * d:4 * d + 4])
        h = ref["y"][:, :, d * H:(d + 1) * H]
        prev = torch.zeros_like(h)
        if T > 1:
            if d == 0:
                prev[:, 1:] = h[:, :-1]
            else:
                prev[:, :-1] = h[:, 1:]
        pre = x @ w_ih.t() + b_ih + b_hh + prev @ w_hh.t()
        for b, n in enumerate(inp["lens"]):
            out.append(pre[b, :n].reshape(-1))
    return torch.cat(out)


def _saturation_ok(case, inp, ref):
    """About a tenth of the pre-activations beyond +-30, a few (at least three, under 3 %) beyond +-90."""
    pre = _preactivations(case, inp, ref).abs()
    beyond30, beyond90 = float((pre > 30).double().mean()), int((pre > 90).sum())
    return 0.05 <= beyond30 <= 0.2 and 3 <= beyond90 <= 0.03 * pre.numel(), (beyond30, beyond90, pre.numel())


# -------------------------------------------------------------------------------------------------------------- GPU
def _run_gpu(case, inp, dev):
    """ops.lstm_layer + backward in the case's arithmetic and layout -> y, dx in the padded [B, T, .] form, the parameter
    gradients, `pad` = the largest magnitude on a padding frame / padding row of y and dx, and the lstm_* LAUNCHES left."""
    import ops
    import hip_backend as hb
    H, B, T, ndir = (case[k] for k in ("H", "B", "T", "ndir"))
    lens = inp["lens"]
    both = case["fwd"] == "persist" and case["bwd"] == "persist"
    gp = [p.to(dev).requires_grad_(True) for p in inp["prm"]]
    g = torch.Generator().manual_seed(inp["seed_pad"])
    with hb.arith(case["arith"]):
        hb.LAUNCHES.clear()
        if case["layout"] == "tm":
            xg = inp["x"].to(dev).requires_grad_(True)
            lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)

            def run():
                got = ops.lstm_layer(xg.transpose(0, 1), lens_dev, gp, ndir)
                got.backward(inp["dy"].transpose(0, 1).contiguous().to(dev))
                return got
            if both:
                with hb.require_persistent():
                    got = run()
            else:
                got = run()
            y, dx = got.detach().transpose(0, 1).cpu(), xg.grad.cpu()
            pad = 0.0
            for b, n in enumerate(lens):
                if n < T:
                    pad = max(pad, float(y[b, n:].abs().max()), float(dx[b, n:].abs().max()))
        else:
            layout = hb.RowLayout(lens, [case["sub"]], dev)
            rows = hb.LayerRows(layout, 0)
            assert all(int(e) > n for e, n in zip(layout.ext[0], lens)) and rows.R == int(layout.ext[0].sum())
            xp = hb.rows_pack(inp["x"].to(dev), rows).requires_grad_(True)
            dyp = torch.randn(rows.R, ndir * H, generator=g)           # noise on the padding rows: must reach no gradient
            for b, n in enumerate(lens):
                r0 = int(layout.base[0][b])
                dyp[r0:r0 + n] = inp["dy"][b, :n]

            def run():
                got = ops.lstm_layer(xp, None, gp, ndir, rows=rows)
                got.backward(dyp.to(dev))
                return got
            if both:
                with hb.require_persistent():
                    got = run()
            else:
                got = run()
            yp, dxp = got.detach().cpu(), xp.grad.cpu()
            y, dx = torch.zeros(B, T, ndir * H), torch.zeros(B, T, case["I"])
            pad = 0.0
            for b, n in enumerate(lens):
                r0, e = int(layout.base[0][b]), int(layout.ext[0][b])
                y[b, :n], dx[b, :n] = yp[r0:r0 + n], dxp[r0:r0 + n]
                pad = max(pad, float(yp[r0 + n:r0 + e].abs().max()), float(dxp[r0 + n:r0 + e].abs().max()))
        torch.cuda.synchronize()
        ran = {k: v for k, v in hb.LAUNCHES.items() if k.startswith("lstm_") and v}
    assert not hb.persist_aborted(dev), (case["name"], ran, hb.persist_abort_code(dev))
    return dict(y=y, dx=dx, prm=[p.grad.detach().cpu() for p in gp], pad=pad), ran


# ----------------------------------------------------------------------------------------------------------- errors
def _units(case, lens):
    """The parts the per-utterance check looks at: (tensor, utterance, label, feature slice)."""
    H = case["H"]
    for b in range(len(lens)):
        for d in range(case["ndir"]):
            yield "y", b, "y/utt%d/dir%d" % (b, d), slice(d * H, (d + 1) * H)
        yield "dx", b, "dx/utt%d" % b, slice(None)


def _errors(case, lens, out, ref):
    """-> {name: (error, allowance, scale)} tensor-wide for y, dx and d<parameter><direction>; {label: (error, allowance,
    scale)} of every part of _units that is not exempt; the utterances with an exempt part.  Errors are absolute, `scale` is
    the largest reference magnitude of the tensor / the part."""
    rg = _rtol_grad(case)
    wide, parts, exempt = {}, {}, set()

    def whole(name, got, want, rtol):
        scale = float(want.abs().max())
        wide[name] = (float((got.double() - want.double()).abs().max()), rtol * scale + ATOL, scale)

    whole("y", out["y"], ref["y"], RTOL_Y)
    whole("dx", out["dx"], ref["dx"], rg)
    for i, (a, b) in enumerate(zip(out["prm"], ref["prm"])):
        whole("d%s%d" % (PNAMES[i % 4], i // 4), a, b, rg)
    for tensor, b, label, cols in _units(case, lens):
        n = lens[b]
        want = ref[tensor][b, :n, cols].double()
        got = out[tensor][b, :n, cols].double()
        top, scale = wide[tensor][2], float(want.abs().max())
        if scale < EXEMPT_BELOW * top:
            exempt.add(b)
            continue
        floor = 8.0 * float(np.spacing(np.float32(top)))
        parts[label] = (float((got - want).abs().max()), (RTOL_Y if tensor == "y" else rg) * scale + floor, scale)
    return wide, parts, exempt


def _worst(parts, prefix):
    """The part of y or dx that uses the largest share of its allowance: (label, error, allowance, scale)."""
    sel = [(k,) + v for k, v in parts.items() if k.startswith(prefix)]
    return max(sel, key=lambda r: r[1] / r[2]) if sel else None


def _cap_ok(case, exempt):
    return EXEMPT_ONE_IN * len(exempt) <= case["B"]


def _finite(out):
    return all(bool(torch.isfinite(t).all()) for t in [out["y"], out["dx"]] + out["prm"])


def _over(wide, parts):
    bad = {k: "%.3g > %.3g (scale %.3g)" % v for k, v in wide.items() if not v[0] <= v[1]}
    bad.update({k: "%.3g > %.3g (scale %.3g)" % v for k, v in parts.items() if not v[0] <= v[1]})
    return bad


def _check(case, inp, out, ref, what):
    """The numeric part of a case, for the GPU's results or (the CPU companion) the fp32 restatement's."""
    assert _finite(out), "%s [%s]: an output is not finite" % (case["name"], what)
    wide, parts, exempt = _errors(case, inp["lens"], out, ref)
    assert _cap_ok(case, exempt), "%s [%s]: utterances %s of %d are exempt, more than one in %d" % (
        case["name"], what, sorted(exempt), case["B"], EXEMPT_ONE_IN)
    print("%s [%s] %s | worst parts: %s" % (case["name"], what, " ".join("%s=%.2e" % (k, v[0] / max(v[2], 1e-300)) for k, v in wide.items()),
                                         " ".join("%s=%.2e of %.2e" % w[:3] for w in (_worst(parts, "y"), _worst(parts, "dx")) if w)))
    bad = _over(wide, parts)
    assert not bad, "%s [%s]: against float64, over the limit (y %g, gradients %g of the largest reference value): %s" % (
        case["name"], what, RTOL_Y, _rtol_grad(case), bad)
    return wide, parts, exempt


CASE_BY_NAME = {prm.values[0]["name"]: prm.values[0] for prm in CASES}
assert len(CASE_BY_NAME) == len(CASES)


@pytest.mark.parametrize("case", CASES)
def test_lstm_shapes_against_float64(case):
    """ops.lstm_layer, forward and backward, on the kernels the case names - LAUNCHES must equal the case's keys, the
    persistent kernels must not have aborted - against the float64 restatement: y, dx and all eight (four) parameter
    gradients tensor-wide; y per utterance and direction and dx per utterance against their own scale; exact zeros on
    the padding frames (time-major) / the padding rows of every block (packed).  Saturated cases assert first, on the
    reference's own pre-activations, that the gates do saturate."""
    dev = _gpu()
    import hip_backend as hb
    assert hb.USE_PERSIST and not hb.DETERMINISTIC[0]
    inp = _inputs_of(case["name"])
    ref, _ = _references_of(case["name"])
    if case["sat"]:
        ok, seen = _saturation_ok(case, inp, ref)
        assert ok, "%s: share beyond +-30, count beyond +-90, of: %s" % (case["name"], seen)
    hb.persist_clear_abort(dev)
    try:
        out, ran = _run_gpu(case, inp, dev)
    except RuntimeError as exc:
        if "HIP error" in str(exc) or "illegal memory access" in str(exc) or re.search(r"failed with code [1-9]", str(exc)):
            # a device fault is a finding of its own: nothing more is started on that device by this session
            pytest.exit("%s: the device faulted: %s" % (case["name"], exc), returncode=3)
        raise
    assert ran == _want(case), "%s: the kernels that ran %s are not the ones this shape must take %s" % (case["name"], ran, _want(case))
    assert out["pad"] == 0.0, "%s: y or dx holds %g on a padding frame / row" % (case["name"], out["pad"])
    _check(case, inp, out, ref, "GPU")


# ----------------------------------------------------------------------------------------------------------- record
def _record(path):
    """Per case one JSON line: the launch keys, and {tensor or worst part: [GPU against float64, fp32 on the CPU against
    float64]} as shares of the largest reference value of that tensor / part."""
    dev = _gpu()
    import hip_backend as hb
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed = 0
    with open(path, "w") as f:
        for prm in CASES:
            case = prm.values[0]
            inp = _inputs(case)
            t0 = time.time()
            ref, ref32 = _reference(case, inp, torch.float64), _reference(case, inp, torch.float32)
            t_ref = time.time() - t0
            hb.persist_clear_abort(dev)
            t0 = time.time()
            out, ran = _run_gpu(case, inp, dev)
            t_gpu = time.time() - t0
            wide, parts, exempt = _errors(case, inp["lens"], out, ref)
            wide32, parts32, _ = _errors(case, inp["lens"], ref32, ref)
            err = {k: [float("%.3g" % (v[0] / max(v[2], 1e-300))), float("%.3g" % (wide32[k][0] / max(v[2], 1e-300)))]
                   for k, v in wide.items()}
            worst = {}
            for prefix in ("y", "dx"):
                w = _worst(parts, prefix)
                if w is not None:
                    worst[w[0]] = [float("%.3g" % (w[1] / w[3])), float("%.3g" % (parts32[w[0]][0] / w[3])),
                                   float("%.3g" % (w[2] / w[3]))]
            ok = (ran == _want(case) and out["pad"] == 0.0 and _finite(out) and _cap_ok(case, exempt)
                  and not _over(wide, parts))
            failed += not ok
            rec = dict(case=case["name"], kind=case["kind"], ran=sorted(ran), ok=bool(ok), rtol_grad=_rtol_grad(case),
                       exempt=sorted(exempt), padding=out["pad"], err=err, worst_utterance=worst)
            print("%s reference %.2f s, GPU %.2f s%s" % (case["name"], t_ref, t_gpu, "" if ok else "   <-- NOT OK"))
            f.write(json.dumps(rec) + "\n")
            f.flush()
    print("%s written, %d record(s) over a limit or off their path" % (path, failed))
    return failed


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_lstm_shapes_gpu.py --record [--out FILE]")
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lstm_shapes_parity.jsonl")
    sys.exit(1 if _record(dest) else 0)
