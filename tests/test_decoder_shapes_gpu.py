"""The decoder sequence kernels (csrc/dec_persist.hip, csrc/decoder.hip, csrc/feedback.hip) against a float64 restatement of
the same operation, across the four dimensions the launchers dispatch on: conv channels C, conv half-width K, encoder
frames T' and, free-running, the vocabulary V.  Every case names the hb.LAUNCHES key each direction must take, so a
silent change of dispatch fails; every output and gradient is held to the float64 reference tensor-wide and, for the
per-utterance tensors, within each utterance against that utterance's own scale.

    python tests/test_decoder_shapes_gpu.py --record [--out FILE]

writes, per case and path, the error of the GPU against float64 beside the error of the same reference evaluated in fp32
on the CPU (profiles/decoder_shapes_parity.jsonl)."""
import json
import os
import re
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "semi-supervised-asr_amd"), os.path.join(_ROOT, "tests", "golden")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu

# The limits the project holds the decoder to (test_decoder_persistent_path, the d512 oracle tests, BASELINE.json's gate),
# relative to the largest reference value of the tensor - or, per utterance, of that utterance's part of it.
RTOL_OUT = 2e-4
RTOL_GRAD = 1e-3

E_DIM = 128
NAMES = ("P", "Q", "emb_w", "w_ih", "w_hh", "b_ih", "b_hh", "wdec", "convw", "watt", "gvec", "bo", "w_out", "b_out")
PER_UTT = {"logits": 1, "ws": 1, "P": 0, "Q": 0}        # the utterance axis of the tensors that have one


def _gpu():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------------------ cases
# Teacher-forced.  With DP_NT = 512, T'p = T' rounded up to a multiple of 4 (csrc/dec_persist.hip, dec_fwd_persist_impl /
# dec_bwd_persist_impl):
#   forward : C <= 12;  4 rows per group while T' <= 128 and C T'p <= 1024, else 2 rows per group while T' <= 256 and
#             C T'p <= 3072
#   backward: C <= 16;  4 rows per group under the same condition, else 2 rows per group while T' <= 256, C T'p <= 2560 and
#             bwd_lds_plan(T', C, K) <= 160 KB (it is, for every case below: the largest are (8, 128, 100) in the 4-row
#             geometry with 162 420 bytes and (10, 256, 100) in the 2-row geometry with 155 964)
# fwd / bwd: the key that must run when the persistent kernel of that direction is asked for.
def _tf(C, Tp, K, fwd, bwd, dim=512, B=5, L=3, drop=True):
    name = "C%d-T%d-K%d" % (C, Tp, K) + ("-B%d" % B if B != 5 else "") + ("-w%d" % dim if dim != 512 else "")
    return pytest.param(dict(name=name, dim=dim, B=B, C=C, Tp=Tp, K=K, L=L, V=34, drop=drop, kind="teacher", fwd=fwd, bwd=bwd),
                        id=name)


TEACHER_CASES = [
    # the 4-row geometry at its real extent: T' > 100, T' not a multiple of 4, one channel, an odd channel count
    _tf(8, 128, 100, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(8, 125, 100, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(4, 128, 100, "dec_fwd_persist", "dec_bwd_persist", drop=False),
    _tf(1, 128, 3, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(3, 127, 5, "dec_fwd_persist", "dec_bwd_persist"),
    # both sides of C T'p = 1024 and of T' = 128
    _tf(8, 129, 100, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(10, 100, 100, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(10, 101, 100, "dec_fwd_persist", "dec_bwd_persist", drop=False),
    _tf(12, 84, 10, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(12, 85, 10, "dec_fwd_persist", "dec_bwd_persist"),
    # the limits of the 2-row geometry: the backward's C T'p = 2560, the forward's 3072, K = 100 with T' = 256
    _tf(12, 212, 10, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(12, 213, 10, "dec_fwd_persist", "dec_bwd_step"),
    _tf(12, 256, 100, "dec_fwd_persist", "dec_bwd_step"),
    _tf(10, 256, 100, "dec_fwd_persist", "dec_bwd_persist", drop=False),
    # channels the forward declines: the per-step forward feeds the persistent backward; the per-step backward at its CMAX
    _tf(13, 64, 10, "dec_fwd_step", "dec_bwd_persist"),
    _tf(16, 64, 10, "dec_fwd_step", "dec_bwd_persist"),
    _tf(16, 160, 10, "dec_fwd_step", "dec_bwd_persist"),
    _tf(16, 161, 10, "dec_fwd_step", "dec_bwd_step"),
    # beyond both
    _tf(10, 257, 100, "dec_fwd_step", "dec_bwd_step"),
    # one-tap and three-tap filters
    _tf(8, 128, 0, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(10, 60, 1, "dec_fwd_persist", "dec_bwd_persist"),
    _tf(10, 96, 0, "dec_fwd_persist", "dec_bwd_persist", drop=False),
    # a second launch of one row, in each geometry (32 / 16 rows per launch)
    _tf(8, 128, 100, "dec_fwd_persist", "dec_bwd_persist", B=33, drop=False),
    _tf(10, 130, 100, "dec_fwd_persist", "dec_bwd_persist", B=17),
    # the other instantiation
    _tf(8, 128, 100, "dec_fwd_persist", "dec_bwd_persist", dim=320),
    _tf(12, 213, 10, "dec_fwd_persist", "dec_bwd_step", dim=320, drop=False),
    _tf(16, 64, 10, "dec_fwd_step", "dec_bwd_persist", dim=320),
]


# Free-running.  The forward with the feedback inside the kernel takes V <= 64, the backward of the smooth feedback V <= 36
# (its W_out slice sits in LDS); between them the persistent forward is followed by the per-step backward and
# asr_dec_feedback_bwd.  A greedy sequence has no gradient through its feedback: the plain persistent backward runs it.
def _fr(kind, V, C, Tp, K, fwd, bwd, L=4, drop=True, seed=0):
    name = "%s-V%d-C%d-T%d-K%d" % (kind, V, C, Tp, K)
    return pytest.param(dict(name=name, dim=512, B=5, C=C, Tp=Tp, K=K, L=L, V=V, drop=drop, kind=kind, fwd=fwd, bwd=bwd,
                             seed=seed), id=name)


FREE_CASES = [
    _fr("smooth", 5, 10, 60, 100, "dec_free_persist", "dec_bwd_persist", drop=False),
    _fr("smooth", 36, 10, 60, 100, "dec_free_persist", "dec_bwd_persist"),
    _fr("smooth", 37, 10, 60, 100, "dec_free_persist", "dec_bwd_step"),
    _fr("smooth", 64, 10, 60, 100, "dec_free_persist", "dec_bwd_step"),
    _fr("smooth", 65, 10, 60, 100, "dec_free_step", "dec_bwd_step"),
    _fr("smooth", 36, 10, 130, 100, "dec_free_persist", "dec_bwd_persist"),
    _fr("smooth", 37, 10, 130, 100, "dec_free_persist", "dec_bwd_step", drop=False),
    _fr("greedy", 37, 8, 128, 100, "dec_free_persist", "dec_bwd_persist"),
]


# ----------------------------------------------------------------------------------------------------------- inputs
def _inputs(case):
    """fp32 inputs on the CPU, drawn as the existing decoder tests draw theirs (ragged w0 lengths in [T'/2, T'])."""
    B, Tp, L, V, C, K = (case[k] for k in ("B", "Tp", "L", "V", "C", "K"))
    D = A = Od = case["dim"]
    free = case["kind"] != "teacher"
    g = torch.Generator().manual_seed(1009 * C + 31 * Tp + 7 * K + B + V + case["dim"] + 100003 * case.get("seed", 0))
    sc0 = 1.0 / np.sqrt(D)
    sco = 0.3 if free else sc0

    def rnd(*sh, sc=1.0):
        return torch.randn(*sh, generator=g) * sc

    x = dict(P=rnd(B, Tp, A, sc=0.5), Q=rnd(B, Tp, Od, sc=0.5), emb_w=rnd(V, E_DIM, sc=0.5),
             w_ih=rnd(4 * D, E_DIM + Od, sc=sc0), w_hh=rnd(4 * D, D, sc=sc0), b_ih=rnd(4 * D, sc=sc0),
             b_hh=rnd(4 * D, sc=sc0), wdec=rnd(A, D, sc=sc0), convw=rnd(C, 1, 1, 2 * K + 1, sc=0.1),
             watt=rnd(A, C, sc=0.3), gvec=rnd(1, A, sc=sc0), bo=rnd(Od, sc=sc0), w_out=rnd(V, D + Od, sc=sco),
             b_out=rnd(V, sc=sco))
    lens = torch.randint(max(1, Tp // 2), Tp + 1, (B,), generator=g)
    w0 = torch.zeros(B, Tp)
    for b in range(B):
        w0[b, :lens[b]] = 1.0 / float(lens[b])
    x["w0"] = w0
    x["tokens"] = None if free else torch.randint(0, V, (B, L), generator=g)
    x["xmask"] = (torch.rand(L, B, Od + E_DIM, generator=g) > 0.3).float() / 0.7 if case["drop"] else None
    x["dlog"] = rnd(L, B, V)
    x["dws"] = rnd(L, B, Tp, sc=0.1)
    return x


# -------------------------------------------------------------------------------------------------------- reference
def _reference(case, x, dtype):
    """Decoder.forward's loop (model.py:324-351) on the operands ops.decoder_sequence takes, in `dtype` on the CPU:
    O.lstm_cell and the arithmetic of O.attloc_step with st.pre = P and the context output w @ Q + bo (model.py:362-363:
    P = mlp_enc(enc), Q = enc @ mlp_o.weight^T).  The dropout mask of the cell input is the explicit xmask, laid out
    (ctx | emb) where the cell input is (emb | ctx).  -> logits [L, B, V], ws [L, B, T'], pred [L, B], {name: gradient} of
    (logits * dlog).sum() + (ws * dws).sum()."""
    p = {k: x[k].detach().to(dtype).requires_grad_(True) for k in NAMES}
    L, kind = case["L"], case["kind"]
    B, Tp, _ = p["P"].shape
    D, Od = p["w_hh"].shape[1], p["Q"].shape[2]
    C, K = p["convw"].shape[0], (p["convw"].shape[-1] - 1) // 2
    xmask = None if x["xmask"] is None else x["xmask"].to(dtype)
    z = torch.zeros(B, D, dtype=dtype)
    c = torch.zeros(B, D, dtype=dtype)
    ctx = torch.zeros(B, Od, dtype=dtype)
    w = x["w0"].to(dtype)
    filt = p["convw"].reshape(C, 1, 2 * K + 1)
    logits, ws, preds = [], [], []
    logit = None
    for s in range(L):
        if kind == "teacher":
            emb = p["emb_w"][x["tokens"][:, s]]
        elif s == 0:
            emb = p["emb_w"][torch.full((B,), 1, dtype=torch.long)]           # <BOS> = 1
        elif kind == "smooth":
            emb = torch.softmax(3.0 * logit, dim=-1) @ p["emb_w"]
        else:
            emb = p["emb_w"][preds[-1]]
        cell_in = torch.cat([emb, ctx], dim=1)
        if xmask is not None:
            cell_in = cell_in * torch.cat([xmask[s][:, Od:], xmask[s][:, :Od]], dim=1)
        z, c = O.lstm_cell(cell_in, z, c, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
        conv = F.conv1d(w.unsqueeze(1), filt, padding=K)                      # [B, C, T']
        loc = conv.transpose(1, 2) @ p["watt"].t()
        dec = (z @ p["wdec"].t()).unsqueeze(1)
        e = (torch.tanh(p["P"] + dec + loc) @ p["gvec"].t()).squeeze(2)
        w = torch.softmax(2.0 * e, dim=1)                                     # over all T' frames
        ctx = torch.bmm(w.unsqueeze(1), p["Q"]).squeeze(1) + p["bo"]
        logit = torch.cat([z, ctx], dim=1) @ p["w_out"].t() + p["b_out"]
        logits.append(logit)
        ws.append(w)
        preds.append(logit.detach().argmax(-1))
    logits, ws = torch.stack(logits), torch.stack(ws)
    loss = (logits * x["dlog"].to(dtype)).sum() + (ws * x["dws"].to(dtype)).sum()
    grads = torch.autograd.grad(loss, [p[k] for k in NAMES])
    return logits.detach(), ws.detach(), torch.stack(preds), dict(zip(NAMES, grads))


def _margin_ok(logits):
    """The condition on a free-running case's inputs: at every (step, utterance) the two largest float64 logits lie further
    apart than 1e-3 of the row's largest logit, so that no fp32 evaluation may pick another token."""
    top = logits.topk(2, dim=-1).values
    return bool(((top[..., 0] - top[..., 1]) > 1e-3 * logits.abs().amax(-1)).all())


# -------------------------------------------------------------------------------------------------------------- GPU
def _run_gpu(case, x, dev, fused, persist_fwd, persist_bwd):
    """ops.decoder_sequence + backward with the given path switches -> logits, ws, pred, gradients, the LAUNCHES it left."""
    import ops
    import hip_backend as hb
    old = hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD
    hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = fused, persist_fwd, persist_bwd
    try:
        par = {k: x[k].to(dev).requires_grad_(True) for k in NAMES}
        tokens = None if x["tokens"] is None else x["tokens"].to(dev)
        xmask = None if x["xmask"] is None else x["xmask"].to(dev)
        opts = dict(L=case["L"], tokens=tokens, tf_flags=None, smooth=case["kind"] == "smooth", smooth_scaling=3.0,
                    sample=False, scaling=2.0, xmask=xmask, bos=1)
        hb.LAUNCHES.clear()
        logits, ws, pred = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"], par["b_ih"],
                                                par["b_hh"], par["wdec"], par["convw"], par["watt"], par["gvec"], par["bo"],
                                                par["w_out"], par["b_out"], x["w0"].to(dev), opts)
        ((logits * x["dlog"].to(dev)).sum() + (ws * x["dws"].to(dev)).sum()).backward()
        torch.cuda.synchronize()
        ran = dict(hb.LAUNCHES)
        assert not hb.persist_aborted(dev), (case["name"], ran, hb.persist_abort_code(dev))
        return logits.detach().cpu(), ws.detach().cpu(), pred.cpu(), {k: par[k].grad.detach().cpu() for k in NAMES}, ran
    finally:
        hb.USE_FEEDBACK_KERNEL, hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = old


def _paths(case):
    """[(label, (fused, persistent forward, persistent backward), LAUNCHES that must result)]"""
    if case["kind"] == "teacher":
        return [("fwd=%d bwd=%d" % (pf, pb), (True, pf, pb),
                 {case["fwd"] if pf else "dec_fwd_step": 1, case["bwd"] if pb else "dec_bwd_step": 1})
                for pf, pb in ((False, False), (True, False), (False, True), (True, True))]
    return [("per-step", (True, False, False), {"dec_free_step": 1, "dec_bwd_step": 1}),
            ("persistent", (True, True, True), {case["fwd"]: 1, case["bwd"]: 1})]


# ----------------------------------------------------------------------------------------------------------- errors
def _rel(got, want):
    """Largest error over the largest reference value, of the whole tensor."""
    want = want.double()
    return float((got.double() - want).abs().max()) / max(1e-30, float(want.abs().max()))


def _rel_per_utterance(got, want, axis):
    """Largest over the utterances of: the largest error within utterance b over that utterance's own largest reference value
    (an error confined to one row of a group cannot hide behind another row's scale)."""
    want = want.double().transpose(0, axis).flatten(1)
    got = got.double().transpose(0, axis).flatten(1)
    return float(((got - want).abs().amax(1) / want.abs().amax(1).clamp_min(1e-30)).max())


def _errors(out, ref):
    """{tensor name: error}: outputs under their names, gradients as d<name>, per-utterance figures with a /utt suffix."""
    lg, ws, _, gr = out
    lr, wr, _, rr = ref
    err = {"logits": _rel(lg, lr), "ws": _rel(ws, wr)}
    err["logits/utt"] = _rel_per_utterance(lg, lr, PER_UTT["logits"])
    err["ws/utt"] = _rel_per_utterance(ws, wr, PER_UTT["ws"])
    for k in NAMES:
        err["d" + k] = _rel(gr[k], rr[k])
    for k in ("P", "Q"):
        err["d%s/utt" % k] = _rel_per_utterance(gr[k], rr[k], PER_UTT[k])
    return err


def _limit(name):
    return RTOL_OUT if name.split("/")[0] in ("logits", "ws") else RTOL_GRAD


def _check(case, label, out, ref, ran, want):
    assert ran == want, "%s [%s]: the kernels that ran %s are not the ones this shape must take %s" % (case["name"], label, ran, want)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all(), (case["name"], label)
    if case["kind"] != "teacher":
        assert torch.equal(out[2], ref[2]), "%s [%s]: hypotheses differ" % (case["name"], label)
    err = _errors(out, ref)
    print("%s [%s] %s" % (case["name"], label, " ".join("%s=%.2e" % kv for kv in err.items())))
    bad = {k: v for k, v in err.items() if not v <= _limit(k)}
    assert not bad, "%s [%s]: against float64, over the limit (%g outputs, %g gradients): %s" % (
        case["name"], label, RTOL_OUT, RTOL_GRAD, bad)
    return err


def _case(case):
    dev = _gpu()
    import hip_backend as hb
    x = _inputs(case)
    ref = _reference(case, x, torch.float64)
    if case["kind"] != "teacher":
        assert _margin_ok(ref[0]), "%s: the inputs leave two logits of a row within 1e-3 of its largest: pick another seed" % case["name"]
    hb.persist_clear_abort(dev)
    for label, flags, want in _paths(case):
        try:
            out = _run_gpu(case, x, dev, *flags)
        except RuntimeError as exc:
            if "HIP error" in str(exc) or "illegal memory access" in str(exc) or re.search(r"failed with code [1-9]", str(exc)):
                # a device fault is a finding of its own: nothing more is started on that device by this session
                pytest.exit("%s [%s]: the device faulted: %s" % (case["name"], label, exc), returncode=3)
            raise
        _check(case, label, out[:4], ref, out[4], want)


@pytest.mark.parametrize("case", TEACHER_CASES)
def test_teacher_forced_decoder_shapes_against_float64(case):
    """Teacher-forced sequences at widths 512 (320 where named), E = 128, L = 3, B = 5 (33 / 17 where named) over (C, T', K):
    all four combinations of the persistent forward / backward, each against the float64 reference - logits, attention
    weights and every gradient tensor-wide, logits / ws / dP / dQ also per utterance - and each on the kernels the case
    names (the `_step` key where the launcher must decline although asked)."""
    _case(case)


@pytest.mark.parametrize("case", FREE_CASES)
def test_free_running_decoder_shapes_against_float64(case):
    """Free-running sequences (smooth feedback softmax(3 logit) @ E; greedy) over the vocabulary: the per-step kernels with
    the fused feedback kernel, then the persistent kernels, each against the float64 reference; the hypotheses equal it
    exactly (the inputs keep the two largest logits of every row apart, asserted on the CPU first)."""
    _case(case)


# ----------------------------------------------------------------------------------------------------------- record
def _record(path):
    """Per case and path, one JSON line: the kernels that ran and {tensor: [GPU against float64, fp32 on the CPU against
    float64]}."""
    dev = _gpu()
    import hip_backend as hb
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    failed = 0
    with open(path, "w") as f:
        for prm in TEACHER_CASES + FREE_CASES:
            case = prm.values[0]
            x = _inputs(case)
            t0 = time.time()
            ref = _reference(case, x, torch.float64)
            t_ref = time.time() - t0
            cpu32 = _errors(_reference(case, x, torch.float32), ref)
            hb.persist_clear_abort(dev)
            for label, flags, want in _paths(case):
                t0 = time.time()
                out = _run_gpu(case, x, dev, *flags)
                t_gpu = time.time() - t0
                gpu = _errors(out[:4], ref)
                ok = out[4] == want and all(v <= _limit(k) for k, v in gpu.items())
                failed += not ok
                rec = dict(case=case["name"], kind=case["kind"], path=label, ran=sorted(out[4]), ok=bool(ok),
                           err={k: [float("%.3g" % gpu[k]), float("%.3g" % cpu32[k])] for k in gpu})
                if case["kind"] != "teacher":
                    rec["hypotheses_equal"] = bool(torch.equal(out[2], ref[2]))
                print("%s [%s] reference %.2f s, GPU %.2f s" % (case["name"], label, t_ref, t_gpu))
                f.write(json.dumps(rec) + "\n")
                f.flush()
    print("%s written, %d record(s) over a limit or off their path" % (path, failed))
    return failed


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_decoder_shapes_gpu.py --record [--out FILE]")
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decoder_shapes_parity.jsonl")
    sys.exit(1 if _record(dest) else 0)
