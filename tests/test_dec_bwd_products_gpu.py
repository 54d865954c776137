"""The products of the persistent decoder backward (csrc/dec_persist.hip, dec_persist_bwd_kernel: the two conv-backward
Toeplitz products and the dX product dgates . W_cat) at the loop edges of those phases: conv channels C in {1, 8, 10}, conv
half width K in {1, 7, 100} (100 = DP_KMAX; K >= T' lets every tap reach the zero padding), encoder frames T' in
{3, 16, 17, 100} (one part, a part boundary, cfg-2) with 4 rows per group and {129, 200} with 2, B in {1, 4, 5, 32}
(a partly filled group, a full one, one row into the second), L in {1, 2, 9}, widths 512 and 320 (cfg-1), E = 128, ragged
initial attention weights with one utterance of length 1.

Each case drives ops.decoder_sequence (teacher-forced) forward and backward with the persistent kernels required and
asserted through hb.LAUNCHES, and compares EVERY gradient the operator returns - dP, dQ, d(embedding), dW_ih, dW_hh, db_ih,
db_hh (the parts of dW_cat), dW_dec, d(conv weights), dW_att, dgvec, dbo, dW_out, db_out - per element against the float64
restatement below.  The operator has no length argument and no differentiable initial state: its softmax spans all T'
frames, z_0 = c_0 = ctx_0 = 0 and w0 is not differentiated, so there is neither a padded position nor an initial-state
gradient among its results; the ragged part of a case is w0.

Allowance (the rule of tests/test_lstm_shapes_gpu.py): the same restatement is evaluated in fp32 on the CPU; the GPU's
largest error against float64 over the tensor's largest magnitude may be at most RATIO_MAX = 16 times the fp32
restatement's (floored at 2^-24, the rounding of the result itself).  profiles/dec_bwd_products_parity.jsonl holds the
ratios of the commit before the products were rewritten ("parent") and after ("head"); where the parent's ratio of a tensor
already exceeds 16, the bound of that tensor is twice the parent's ratio.  The last two cases run the cfg-2 widths in
hb.arith("f32") and "bf16x3": the arithmetic switch only reaches the GEMMs outside the kernel (the embedding columns of dX
among them), so they show that the unchanged products still join the rewritten ones.

    python tests/test_dec_bwd_products_gpu.py --record LABEL --out FILE     # one JSON line per case: {tensor: ratio}
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (_ROOT, os.path.join(_ROOT, "semi-supervised-asr_amd"), os.path.join(_ROOT, "tests", "golden")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

RATIO_MAX = 16.0
FLOOR = 2.0 ** -24
E_DIM = 128
V = 34
NAMES = ("P", "Q", "emb_w", "w_ih", "w_hh", "b_ih", "b_hh", "wdec", "convw", "watt", "gvec", "bo", "w_out", "b_out")
PARITY = os.path.join(_ROOT, "profiles", "dec_bwd_products_parity.jsonl")


def _c(C, K, Tp, B, L, dim=512, drop=True, arith=None):
    name = "C%d-K%d-T%d-B%d-L%d" % (C, K, Tp, B, L) + ("-w%d" % dim if dim != 512 else "") + \
        ("" if drop else "-nodrop") + ("-%s" % arith if arith else "")
    return pytest.param(dict(name=name, C=C, K=K, Tp=Tp, B=B, L=L, dim=dim, drop=drop, arith=arith), id=name)


CASES = [
    # 4 rows per group (T' <= 128, C T'p <= 1024)
    _c(1, 1, 3, 1, 1), _c(1, 7, 16, 4, 2), _c(1, 100, 17, 5, 2), _c(1, 100, 100, 5, 2),
    _c(8, 1, 16, 5, 2), _c(8, 7, 17, 4, 9), _c(8, 100, 3, 5, 2), _c(8, 100, 100, 32, 2), _c(8, 7, 100, 5, 1),
    _c(10, 1, 100, 5, 2), _c(10, 7, 3, 4, 2), _c(10, 100, 16, 1, 9), _c(10, 100, 17, 5, 2), _c(10, 100, 100, 32, 9),
    _c(10, 7, 100, 4, 2), _c(10, 100, 100, 5, 2, drop=False),
    # 2 rows per group (T' > 128)
    _c(1, 1, 129, 1, 2), _c(8, 7, 129, 4, 2), _c(10, 100, 129, 5, 2), _c(10, 100, 200, 32, 2), _c(8, 100, 200, 5, 9),
    _c(1, 100, 200, 4, 1), _c(10, 7, 200, 5, 2), _c(10, 1, 200, 1, 1),
    # the cfg-1 widths
    _c(10, 100, 100, 4, 2, dim=320), _c(8, 7, 17, 5, 9, dim=320), _c(10, 100, 200, 5, 2, dim=320), _c(1, 1, 3, 1, 1, dim=320),
    # the other arithmetics of the GEMMs around the kernel, cfg-2 widths
    _c(10, 100, 100, 5, 2, arith="f32"), _c(10, 100, 100, 5, 2, arith="bf16x3"),
]


def _inputs(case):
    """fp32 inputs on the CPU.  w0 is uniform over the first len_b frames of utterance b; the last utterance has length 1."""
    B, Tp, L, C, K = (case[k] for k in ("B", "Tp", "L", "C", "K"))
    D = A = Od = case["dim"]
    g = torch.Generator().manual_seed(7919 * C + 131 * Tp + 17 * K + 3 * B + L + case["dim"])
    sc0 = 1.0 / np.sqrt(D)

    def rnd(*sh, sc=1.0):
        return torch.randn(*sh, generator=g) * sc

    x = dict(P=rnd(B, Tp, A, sc=0.5), Q=rnd(B, Tp, Od, sc=0.5), emb_w=rnd(V, E_DIM, sc=0.5),
             w_ih=rnd(4 * D, E_DIM + Od, sc=sc0), w_hh=rnd(4 * D, D, sc=sc0), b_ih=rnd(4 * D, sc=sc0),
             b_hh=rnd(4 * D, sc=sc0), wdec=rnd(A, D, sc=sc0), convw=rnd(C, 1, 1, 2 * K + 1, sc=0.1),
             watt=rnd(A, C, sc=0.3), gvec=rnd(1, A, sc=sc0), bo=rnd(Od, sc=sc0), w_out=rnd(V, D + Od, sc=sc0),
             b_out=rnd(V, sc=sc0))
    lens = torch.randint(max(1, Tp // 2), Tp + 1, (B,), generator=g)
    if B > 1:
        lens[B - 1] = 1
    w0 = torch.zeros(B, Tp)
    for b in range(B):
        w0[b, :lens[b]] = 1.0 / float(lens[b])
    x["w0"] = w0
    x["tokens"] = torch.randint(0, V, (B, L), generator=g)
    x["xmask"] = (torch.rand(L, B, Od + E_DIM, generator=g) > 0.3).float() / 0.7 if case["drop"] else None
    x["dlog"] = rnd(L, B, V)
    x["dws"] = rnd(L, B, Tp, sc=0.1)
    return x


def _reference(case, x, dtype):
    """The teacher-forced decoder loop on the operands of ops.decoder_sequence, in `dtype` on the CPU: LSTM cell on
    (embedding | context) under the explicit dropout mask (laid out (ctx | emb)), location-aware attention with P and the
    context output w @ Q + bo, softmax(2 e) over all T' frames.  -> {name: gradient} of (logits dlog).sum() + (ws dws).sum()."""
    p = {k: x[k].detach().to(dtype).requires_grad_(True) for k in NAMES}
    L = case["L"]
    B, Tp, _ = p["P"].shape
    D, Od = p["w_hh"].shape[1], p["Q"].shape[2]
    C, K = p["convw"].shape[0], (p["convw"].shape[-1] - 1) // 2
    xmask = None if x["xmask"] is None else x["xmask"].to(dtype)
    z = torch.zeros(B, D, dtype=dtype)
    c = torch.zeros(B, D, dtype=dtype)
    ctx = torch.zeros(B, Od, dtype=dtype)
    w = x["w0"].to(dtype)
    filt = p["convw"].reshape(C, 1, 2 * K + 1)
    logits, ws = [], []
    for s in range(L):
        cell_in = torch.cat([p["emb_w"][x["tokens"][:, s]], ctx], dim=1)
        if xmask is not None:
            cell_in = cell_in * torch.cat([xmask[s][:, Od:], xmask[s][:, :Od]], dim=1)
        gates = cell_in @ p["w_ih"].t() + p["b_ih"] + z @ p["w_hh"].t() + p["b_hh"]
        gi, gf, gg, go = gates.chunk(4, dim=1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        z = torch.sigmoid(go) * torch.tanh(c)
        conv = F.conv1d(w.unsqueeze(1), filt, padding=K)                      # [B, C, T']
        loc = conv.transpose(1, 2) @ p["watt"].t()
        dec = (z @ p["wdec"].t()).unsqueeze(1)
        e = (torch.tanh(p["P"] + dec + loc) @ p["gvec"].t()).squeeze(2)
        w = torch.softmax(2.0 * e, dim=1)
        ctx = torch.bmm(w.unsqueeze(1), p["Q"]).squeeze(1) + p["bo"]
        logits.append(torch.cat([z, ctx], dim=1) @ p["w_out"].t() + p["b_out"])
        ws.append(w)
    loss = (torch.stack(logits) * x["dlog"].to(dtype)).sum() + (torch.stack(ws) * x["dws"].to(dtype)).sum()
    return dict(zip(NAMES, torch.autograd.grad(loss, [p[k] for k in NAMES])))


def _run_gpu(case, x, dev):
    """ops.decoder_sequence + backward, persistent kernels required -> {name: gradient}, the LAUNCHES it left."""
    import contextlib
    import ops
    import hip_backend as hb
    old = hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD
    hb.USE_PERSIST_DEC = hb.USE_PERSIST_DEC_BWD = True
    try:
        with (hb.arith(case["arith"]) if case["arith"] else contextlib.nullcontext()):
            par = {k: x[k].to(dev).requires_grad_(True) for k in NAMES}
            xmask = None if x["xmask"] is None else x["xmask"].to(dev)
            opts = dict(L=case["L"], tokens=x["tokens"].to(dev), tf_flags=None, smooth=False, smooth_scaling=3.0,
                        sample=False, scaling=2.0, xmask=xmask, bos=1)
            hb.persist_clear_abort(dev)
            hb.LAUNCHES.clear()
            logits, ws, _ = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"], par["b_ih"],
                                                 par["b_hh"], par["wdec"], par["convw"], par["watt"], par["gvec"], par["bo"],
                                                 par["w_out"], par["b_out"], x["w0"].to(dev), opts)
            ((logits * x["dlog"].to(dev)).sum() + (ws * x["dws"].to(dev)).sum()).backward()
            torch.cuda.synchronize()
        ran = dict(hb.LAUNCHES)
        assert not hb.persist_aborted(dev), (case["name"], ran, hb.persist_abort_code(dev))
        return {k: par[k].grad.detach().cpu() for k in NAMES}, ran
    finally:
        hb.USE_PERSIST_DEC, hb.USE_PERSIST_DEC_BWD = old


def _rel(got, want):
    """Largest error of any element over the largest reference magnitude of the tensor."""
    want = want.double()
    return float((got.double() - want).abs().max()) / max(1e-30, float(want.abs().max()))


def _ratios(case, dev):
    """-> {d<name>: (GPU error against float64) / max(fp32 restatement's error against float64, 2^-24)}, the GPU gradients."""
    x = _inputs(case)
    ref = _reference(case, x, torch.float64)
    cpu32 = _reference(case, x, torch.float32)
    try:
        got, ran = _run_gpu(case, x, dev)
    except RuntimeError as exc:
        if "HIP error" in str(exc) or "illegal memory access" in str(exc):
            pytest.exit("%s: the device faulted: %s" % (case["name"], exc), returncode=3)      # nothing more runs on it
        raise
    assert ran.get("dec_fwd_persist") == 1 and ran.get("dec_bwd_persist") == 1 and \
        not any(k.endswith("_step") for k in ran), "%s: not the persistent path: %s" % (case["name"], ran)
    out = {}
    for k in NAMES:
        assert got[k].shape == ref[k].shape and torch.isfinite(got[k]).all(), (case["name"], k)
        out["d" + k] = _rel(got[k], ref[k]) / max(_rel(cpu32[k], ref[k]), FLOOR)
    return out, got


def _parent_ratios():
    """{case name: {tensor: ratio}} of the commit before the rewrite, from profiles/dec_bwd_products_parity.jsonl."""
    out = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            for line in f:
                rec = json.loads(line)
                if rec.get("commit") == "parent":
                    out[rec["case"]] = rec["ratio"]
    return out


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.mark.parametrize("case", CASES)
def test_decoder_backward_products_against_float64(case, dev):
    """Every gradient of the teacher-forced decoder sequence on the persistent kernels, per element against float64: at most
    16 times the error of the fp32 restatement (twice the parent commit's recorded ratio where that already exceeds 16)."""
    ratio, _ = _ratios(case, dev)
    parent = _parent_ratios().get(case["name"], {})
    print("%s %s" % (case["name"], " ".join("%s=%.2f" % kv for kv in ratio.items())))
    bad = {}
    for k, v in ratio.items():
        bound = 2.0 * parent[k] if parent.get(k, 0.0) > RATIO_MAX else RATIO_MAX
        if not v <= bound:
            bad[k] = (v, bound)
    assert not bad, "%s: error against float64 over (ratio to the fp32 restatement's, bound): %s" % (case["name"], bad)


def _record(label, path):
    import __graft_entry__ as entry
    entry.build()
    dev_ = torch.device("cuda")
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        for prm in CASES:
            case = prm.values[0]
            ratio, _ = _ratios(case, dev_)
            f.write(json.dumps(dict(commit=label, case=case["name"], ratio={k: float("%.3g" % v) for k, v in ratio.items()})) + "\n")
            f.flush()
            print(label, case["name"], "max ratio %.2f (%s)" % (max(ratio.values()), max(ratio, key=ratio.get)))


if __name__ == "__main__":
    if "--record" not in sys.argv or "--out" not in sys.argv:
        sys.exit("usage: python tests/test_dec_bwd_products_gpu.py --record LABEL --out FILE")
    _record(sys.argv[sys.argv.index("--record") + 1], sys.argv[sys.argv.index("--out") + 1])
