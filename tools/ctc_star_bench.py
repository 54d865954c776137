"""What the star CTC loss costs, two measurements, each ALTERNATING its two sides in one process behind warm-up:

  op    ops.ctc_star_loss forward + backward (csrc/ctc_star.hip: five launches) against ops.ctc_loss forward + backward
        (csrc/ctc.hip: four) of the same tree on the same logits, at B = 32, T' = 100, V = 34 with ragged frame lengths
        and ragged label counts up to 40, every utterance feasible; the star side at penalty -0.5.
  step  Solver.sup_train_one_iteration at cfg-2 with ctc_weight 0.3, with and without `ctc_star_penalty: -0.5`
        (bench.make_solver: the benchmark's model and batch), in the manner of tools/ctc_bench.py.

Both append one JSON line to profiles/ctc_star_bench.jsonl.  Wall clock around windows that end in a device synchronise;
the median window of each side and the spread of each side's own windows (max - min over the median: a difference inside
it is not one)."""
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


def _spread(w, med):
    return round((max(w) - min(w)) / med, 4)


def bench_op(args, hb, ops):
    dev = torch.device("cuda")
    B, Tp, V, lmax = 32, 100, 34, 40
    rs = np.random.RandomState(1234)
    ylens = [int(n) for n in rs.randint(8, lmax + 1, size=B)]
    ylens[0] = lmax
    flens = [int(n) for n in rs.randint(60, Tp + 1, size=B)]
    flens[0] = Tp
    flens = [max(t, 2 * n + 1) for t, n in zip(flens, ylens)]           # every utterance feasible, repeats or not
    assert max(flens) == Tp and max(ylens) == lmax
    packed = torch.from_numpy(np.concatenate([rs.randint(1, V, size=n) for n in ylens]).astype(np.int64)).to(dev)
    z = (3.0 * torch.randn(B, Tp, V, generator=torch.Generator().manual_seed(5))).to(dev).requires_grad_()
    lens_dev = hb.to_device_i32(flens, dev)
    pen = torch.full((B,), args.penalty, device=dev)
    g = torch.ones(B, device=dev)

    def star():
        z.grad = None
        ops._CtcStarLoss.apply(z, lens_dev, packed, ylens, pen, True).backward(g)

    def plain():
        z.grad = None
        ops.ctc_loss(z, lens_dev, packed, ylens, True).backward(g)
    star()
    plain()
    nll_star = ops.ctc_star_loss(z.detach(), lens_dev, packed, ylens, args.penalty, False)
    nll_ctc = ops.ctc_loss(z.detach(), lens_dev, packed, ylens, False)
    assert bool(torch.isfinite(nll_ctc).all()) and bool((nll_star <= nll_ctc).all())
    windows = {"star": [], "ctc": []}
    for _ in range(args.rounds):
        for side, fn in (("star", star), ("ctc", plain)):
            for _ in range(args.warmup):
                fn()
            windows[side].append(_window(fn, args.calls))
    med = {k: statistics.median(w) for k, w in windows.items()}
    _append(args.out, dict(
        tool="tools/ctc_star_bench.py op", B=B, T_out=Tp, V=V, max_label_len=lmax, mean_label_len=round(float(np.mean(ylens)), 1),
        penalty=args.penalty, call="forward + backward", rounds=args.rounds, calls_per_window=args.calls,
        ms_star=round(med["star"], 4), ms_ctc=round(med["ctc"], 4), ratio_star_over_ctc=round(med["star"] / med["ctc"], 3),
        windows_ms_star=[round(w, 4) for w in windows["star"]], windows_ms_ctc=[round(w, 4) for w in windows["ctc"]],
        spread_star=_spread(windows["star"], med["star"]), spread_ctc=_spread(windows["ctc"], med["ctc"]),
        states_star=3 * lmax + 2, states_ctc=2 * lmax + 1, mean_nll_star=round(float(nll_star.mean()), 3),
        mean_nll_ctc=round(float(nll_ctc.mean()), 3), ws_bytes_star=hb.ctc_star_ws_bytes(B, Tp, V, lmax),
        ws_bytes_ctc=hb.ctc_ws_bytes(B, Tp, V, lmax)))


def bench_step(args, hb, synth, bench):
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="ctc_star_cost_")
    spec = bench.CONFIGS["cfg2"]
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    xs, lens, ys = synth.ragged_batch(B, T, c["input_dim"], c["output_dim"], 1234)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    plain_weights = synth.e2e_weights

    def with_head(cfg, seed):                 # (bench.make_solver loads synth.e2e_weights strictly: no fixture holds a head)
        w = plain_weights(cfg, seed)
        rs = np.random.RandomState(seed + 1)
        k = 1.0 / np.sqrt(cfg["enc_hidden_dim"])
        w["ctc_lo.weight"] = rs.uniform(-k, k, size=(cfg["output_dim"], cfg["enc_hidden_dim"])).astype(np.float32)
        w["ctc_lo.bias"] = rs.uniform(-k, k, size=(cfg["output_dim"],)).astype(np.float32)
        return w
    solvers = {}
    synth.e2e_weights = with_head
    try:
        for mode, over in (("ctc", {}), ("star", dict(ctc_star_penalty=args.penalty))):
            solvers[mode] = bench.make_solver(c, B, T, os.path.join(tmp, mode), ctc_weight=args.ctc_weight, **over)
    finally:
        synth.e2e_weights = plain_weights
    windows, launches, loss = {"ctc": [], "star": []}, {}, {}
    for _ in range(args.rounds):
        for mode in ("ctc", "star"):
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
            launches[mode] = {k: v // args.steps for k, v in sorted(hb.LAUNCHES.items()) if k.startswith("ctc")}
            loss[mode] = float(last)
    med = {m: statistics.median(w) for m, w in windows.items()}
    _append(args.out, dict(
        tool="tools/ctc_star_bench.py step", config="cfg2", call="Solver.sup_train_one_iteration",
        workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T), ctc_weight=args.ctc_weight, penalty=args.penalty,
        rounds=args.rounds, steps_per_window=args.steps, ms_per_step_ctc=round(med["ctc"], 3),
        ms_per_step_star=round(med["star"], 3), added_ms=round(med["star"] - med["ctc"], 3),
        cost_ratio=round(med["star"] / med["ctc"], 4), windows_ms_ctc=[round(w, 3) for w in windows["ctc"]],
        windows_ms_star=[round(w, 3) for w in windows["star"]], spread_ctc=_spread(windows["ctc"], med["ctc"]),
        spread_star=_spread(windows["star"], med["star"]), ctc_launches_per_step=launches, last_loss=loss,
        arith=hb.arith_name(), persistent_after=bool(hb.USE_PERSIST and hb.USE_PERSIST_DEC)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="op,step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="op: forward + backward calls per window")
    ap.add_argument("--steps", type=int, default=20, help="step: train steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--penalty", type=float, default=-0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_star_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "ctc_star_bench.py measures on the GPU"
    what = args.what.split(",")
    if "op" in what:
        bench_op(args, hb, ops)
    if "step" in what:
        bench_step(args, hb, synth, bench)


if __name__ == "__main__":
    main()
