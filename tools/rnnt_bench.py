"""Measures the transducer head on one GPU, alternating the sides of every comparison in one process:

    op      ops.rnnt_joint (forward + backward), ops.rnnt_loss forward, and forward + backward, at B = 32, T = 100, U = 100,
            V = 34, J = 256, beside a reference loss: torchaudio.functional.rnnt_loss when torchaudio is importable,
            otherwise a torch composition (log_softmax, then logaddexp over the anti-diagonals); the record says which
    decode  TransducerHead.greedy at B in {1, 32}
    step    the cfg-2 supervised step (bench.py's Solver and batch) with rnnt_weight 0 and --rnnt-weight, alternating

Appends one JSON line per measurement to profiles/rnnt_bench.jsonl: medians over --rounds windows, every window kept."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def _append(path, rec):
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def _alternate(args, sides, calls):
    windows = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            for _ in range(args.warmup):
                fn()
            windows[k].append(_window(fn, calls))
    out = {}
    for k, w in windows.items():
        med = statistics.median(w)
        out["ms_" + k] = round(med, 4)
        out["windows_ms_" + k] = [round(v, 4) for v in w]
        out["spread_" + k] = round((max(w) - min(w)) / med, 4)
    return out


def _torch_rnnt(logits, flens, ys):
    """The reference composition: log_softmax, alpha over the anti-diagonals with torch.logaddexp, one utterance at a time
    batched over the diagonal's nodes."""
    lp = torch.log_softmax(logits, -1)
    out = []
    for b, y in enumerate(ys):
        T, U = flens[b], len(y)
        blank = lp[b, :T, :U + 1, 0]
        lab = lp[b, :T, :U, :].gather(2, y.view(1, U, 1).expand(T, U, 1)).squeeze(2) if U else lp.new_zeros(T, 0)
        ninf = lp.new_full((1,), float("-inf"))
        alpha = lp.new_zeros(1)                              # diagonal 0: node (0, 0)
        lo_prev = 0
        for d in range(1, T + U):
            lo, hi = max(0, d - (T - 1)), min(U, d)
            u = torch.arange(lo, hi + 1, device=lp.device)
            t = d - u
            padded = torch.cat([ninf, alpha, ninf])          # alpha of diagonal d - 1 at u - lo_prev + 1
            up = padded[u - lo_prev + 1] + blank[(t - 1).clamp(min=0), u]
            left = padded[u - lo_prev] + (lab[t, (u - 1).clamp(min=0)] if U else ninf)
            up = torch.where(t > 0, up, ninf)
            left = torch.where(u > 0, left, ninf)
            alpha, lo_prev = torch.logaddexp(up, left), lo
        out.append(-(alpha[-1] + blank[T - 1, U]))
    return torch.stack(out)


def bench_op(args, hb, ops):
    dev = torch.device("cuda")
    B, T, U, V, J = args.B, args.T, args.U, args.V, args.J
    rs = np.random.RandomState(7)
    flens = [T] + rs.randint(T // 2, T + 1, B - 1).tolist()
    ulens = [U] + rs.randint(U // 2, U + 1, B - 1).tolist()
    ys = [torch.from_numpy(rs.randint(1, V, n)).to(dev) for n in ulens]
    packed, lens_dev = torch.cat(ys), hb.to_device_i32(flens, dev)
    gen = torch.Generator().manual_seed(5)
    pe = torch.randn(B, T, J, generator=gen).to(dev).requires_grad_()
    pp = torch.randn(B, U + 1, J, generator=gen).to(dev).requires_grad_()
    dz = torch.randn(B, T, U + 1, J, generator=gen).to(dev)
    z = (3.0 * torch.randn(B, T, U + 1, V, generator=gen)).to(dev).requires_grad_()
    g = torch.ones(B, device=dev)

    def joint():
        pe.grad = pp.grad = None
        ops.rnnt_joint(pe, pp, lens_dev, ulens).backward(dz)

    def loss_fwd():
        with torch.no_grad():
            ops.rnnt_loss(z, lens_dev, packed, ulens)

    def loss_both():
        z.grad = None
        ops.rnnt_loss(z, lens_dev, packed, ulens).backward(g)
    try:
        import torchaudio.functional as TAF
        ref_name = "torchaudio.functional.rnnt_loss"
        lens_t, ulens_t = torch.tensor(flens, dtype=torch.int32, device=dev), torch.tensor(ulens, dtype=torch.int32, device=dev)
        targets = torch.zeros(B, U, dtype=torch.int32, device=dev)
        for b, y in enumerate(ys):
            targets[b, :len(y)] = y.int()

        def ref_both():
            z.grad = None
            TAF.rnnt_loss(z, targets, lens_t, ulens_t, blank=0, reduction="none").backward(g)
    except ImportError:
        ref_name = "torch composition (log_softmax + logaddexp over anti-diagonals)"

        def ref_both():
            z.grad = None
            _torch_rnnt(z, flens, ys).backward(g)
    shape = dict(B=B, T=T, U=U, V=V, J=J, rounds=args.rounds, calls_per_window=args.calls)
    _append(args.out, dict(tool="tools/rnnt_bench.py op", call="rnnt_joint forward + backward", z_bytes=4 * B * T * (U + 1) * J,
                           **shape, **_alternate(args, dict(hip=joint), args.calls)))
    _append(args.out, dict(tool="tools/rnnt_bench.py op", call="rnnt_loss forward", ws_bytes=hb.rnnt_ws_bytes(B, T, U, J, V),
                           **shape, **_alternate(args, dict(hip=loss_fwd), args.calls)))
    ref_calls = max(1, args.calls // 20)
    rec = _alternate(args, dict(hip=loss_both), args.calls)
    rec.update(_alternate(args, dict(ref=ref_both), ref_calls))
    _append(args.out, dict(tool="tools/rnnt_bench.py op", call="rnnt_loss forward + backward", reference=ref_name,
                           ref_calls_per_window=ref_calls, ratio_ref_over_hip=round(rec["ms_ref"] / rec["ms_hip"], 3), **shape, **rec))


def bench_decode(args, hb):
    import model as M
    dev = torch.device("cuda")
    torch.manual_seed(3)
    head = M.TransducerHead(args.V, 128, 512, 512, args.J, bos=1).to(dev)
    for B in (1, 32):
        enc_h = torch.randn(B, args.T, 512, device=dev)
        lens_dev = hb.to_device_i32([args.T] * B, dev)

        def decode():
            with torch.no_grad():
                head.greedy(enc_h, lens_dev, 3, args.decode_len)
        _append(args.out, dict(tool="tools/rnnt_bench.py decode", call="TransducerHead.greedy", B=B, T=args.T, V=args.V, J=args.J,
                               max_symbols=3, max_len=args.decode_len, iterations=args.T + args.decode_len, rounds=args.rounds,
                               calls_per_window=args.decode_calls, **_alternate(args, dict(hip=decode), args.decode_calls)))


def bench_step(args, hb, synth, bench):
    import model as M
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="rnnt_cost_")
    spec = bench.CONFIGS["cfg2"]
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    xs, lens, ys = synth.ragged_batch(B, T, c["input_dim"], c["output_dim"], 1234)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    plain_weights = synth.e2e_weights

    def with_head(cfg, seed):                 # (bench.make_solver loads synth.e2e_weights strictly: no fixture holds a head)
        w = plain_weights(cfg, seed)
        torch.manual_seed(seed + 1)
        head = M.TransducerHead(cfg["output_dim"], cfg["embedding_dim"], cfg["dec_hidden_dim"], cfg["enc_hidden_dim"], args.J, 1)
        w.update({"rnnt." + k: v.detach().numpy() for k, v in head.state_dict().items()})
        return w
    solvers = {}
    for mode, w in (("off", 0.0), ("on", args.rnnt_weight)):
        synth.e2e_weights = with_head if w > 0 else plain_weights
        try:
            solvers[mode] = bench.make_solver(c, B, T, os.path.join(tmp, mode), **(dict(rnnt_weight=w, rnnt_joint_dim=args.J) if w else {}))
        finally:
            synth.e2e_weights = plain_weights
    windows, launches, loss = {"off": [], "on": []}, {}, {}
    for _ in range(args.rounds):
        for mode in ("off", "on"):
            sv = solvers[mode]
            with contextlib.redirect_stdout(sys.stderr):
                for _ in range(args.warmup):
                    sv.sup_train_one_iteration(xs_d, lens, ys_d, 1.0)
                sv.flush()
                hb.LAUNCHES.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    last = sv.sup_train_one_iteration(xs_d, lens, ys_d, 1.0)
                sv.flush()
                torch.cuda.synchronize()
            windows[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
            launches[mode] = {k: v // args.steps for k, v in sorted(hb.LAUNCHES.items())}
            loss[mode] = float(last)
    med = {m: statistics.median(w) for m, w in windows.items()}
    _append(args.out, dict(
        tool="tools/rnnt_bench.py step", config="cfg2", call="Solver.sup_train_one_iteration",
        workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T), rnnt_weight=args.rnnt_weight, rnnt_joint_dim=args.J,
        rounds=args.rounds, steps_per_window=args.steps, ms_per_step_off=round(med["off"], 3), ms_per_step_on=round(med["on"], 3),
        added_ms=round(med["on"] - med["off"], 3), cost_ratio=round(med["on"] / med["off"], 4),
        windows_ms_off=[round(w, 3) for w in windows["off"]], windows_ms_on=[round(w, 3) for w in windows["on"]],
        sequence_op_paths=launches, last_loss=loss, arith=hb.arith_name()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="op,decode,step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="op: calls per window")
    ap.add_argument("--decode-calls", type=int, default=3)
    ap.add_argument("--decode-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20, help="step: train steps per window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rnnt-weight", type=float, default=0.3)
    for name, val in (("B", 32), ("T", 100), ("U", 100), ("V", 34), ("J", 256)):
        ap.add_argument("--" + name, type=int, default=val)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "rnnt_bench.py measures on the GPU"
    what = args.what.split(",")
    if "op" in what:
        bench_op(args, hb, ops)
    if "decode" in what:
        bench_decode(args, hb)
    if "step" in what:
        bench_step(args, hb, synth, bench)


if __name__ == "__main__":
    main()
