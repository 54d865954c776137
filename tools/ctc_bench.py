"""What the CTC branch costs, two measurements, each ALTERNATING its two sides in one process behind warm-up:

  op    ops.ctc_loss forward + backward (csrc/ctc.hip: four launches) against torch-ROCm's log_softmax + F.ctc_loss forward +
        backward on the same device and the same logits, at the decoder-side shapes of cfg-2 (B = 32, T' = 100, V = 34) and
        cfg-5 (B = 8, T' = 200): frame lengths = the encoder's output lengths of synth.ragged_batch, label lengths as synth
        draws them (0.125 of the input frames = the output frames: most utterances are at or past the edge of feasibility,
        where both sides still run the whole recursion) and, as a second line, half of that (every utterance feasible).
        Appends one JSON line per shape and label setting to profiles/ctc_bench.jsonl.
  step  Solver.sup_train_one_iteration at cfg-2 with ctc_weight 0 and 0.3 (bench.make_solver: the benchmark's model and
        batch), in the manner of tools/det_cost.py.  Appends one JSON line to profiles/ctc_cost.jsonl.

Wall clock around windows that end in a device synchronise; the median window of each side and the spread of each side's
own windows (max - min over the median: a difference inside it is not one)."""
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
import torch.nn.functional as F

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


def bench_op(args, hb, ops, synth, bench):
    dev = torch.device("cuda")
    for name in ("cfg2", "cfg5"):
        spec = bench.CONFIGS[name]
        c, B, T = spec["model"], spec["batch"], spec["frames"]
        V = c["output_dim"]
        _, ilens, ys = synth.ragged_batch(B, T, c["input_dim"], V, 1234)
        sub = 2 ** sum(1 for s in c["subsample"] if s > 1)
        flens = [(n + sub - 1) // sub for n in ilens]
        Tp = max(flens)
        for labels in ("synth", "half"):
            yl = [y if labels == "synth" else y[:max(1, len(y) // 2)] for y in ys]
            ylens = [len(y) for y in yl]
            packed = torch.from_numpy(np.concatenate(yl)).to(dev)
            z = (3.0 * torch.randn(B, Tp, V, generator=torch.Generator().manual_seed(5))).to(dev).requires_grad_()
            lens_dev = hb.to_device_i32(flens, dev)
            lens_t, ylens_t = torch.tensor(flens), torch.tensor(ylens)
            g = torch.ones(B, device=dev)

            def ours():
                z.grad = None
                ops.ctc_loss(z, lens_dev, packed, ylens, True).backward(g)

            def theirs():
                z.grad = None
                F.ctc_loss(F.log_softmax(z, -1).transpose(0, 1), packed, lens_t, ylens_t, blank=0, reduction="none",
                           zero_infinity=True).backward(g)
            ours()
            nll = ops.ctc_loss(z.detach(), lens_dev, packed, ylens, False)
            feasible = int(torch.isfinite(nll).sum())
            windows = {"hip": [], "torch": []}
            for _ in range(args.rounds):
                for side, fn in (("hip", ours), ("torch", theirs)):
                    for _ in range(args.warmup):
                        fn()
                    windows[side].append(_window(fn, args.calls))
            med = {k: statistics.median(w) for k, w in windows.items()}
            _append(args.out_op, dict(
                tool="tools/ctc_bench.py op", shape=name, B=B, T_out=Tp, V=V, labels=labels, max_label_len=max(ylens),
                feasible_utterances=feasible, call="forward + backward", rounds=args.rounds, calls_per_window=args.calls,
                ms_hip=round(med["hip"], 4), ms_torch_rocm=round(med["torch"], 4), ratio_torch_over_hip=round(med["torch"] / med["hip"], 3),
                windows_ms_hip=[round(w, 4) for w in windows["hip"]], windows_ms_torch=[round(w, 4) for w in windows["torch"]],
                spread_hip=round((max(windows["hip"]) - min(windows["hip"])) / med["hip"], 4),
                spread_torch=round((max(windows["torch"]) - min(windows["torch"])) / med["torch"], 4),
                ws_bytes=hb.ctc_ws_bytes(B, Tp, V, max(ylens))))


def bench_step(args, hb, synth, bench):
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="ctc_cost_")
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
    for mode, w in (("off", 0.0), ("on", args.ctc_weight)):
        synth.e2e_weights = with_head if w > 0 else plain_weights
        try:
            solvers[mode] = bench.make_solver(c, B, T, os.path.join(tmp, mode), ctc_weight=w)
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
    _append(args.out_step, dict(
        tool="tools/ctc_bench.py step", config="cfg2", call="Solver.sup_train_one_iteration",
        workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T), ctc_weight=args.ctc_weight, rounds=args.rounds,
        steps_per_window=args.steps, ms_per_step_off=round(med["off"], 3), ms_per_step_on=round(med["on"], 3),
        added_ms=round(med["on"] - med["off"], 3), cost_ratio=round(med["on"] / med["off"], 4),
        windows_ms_off=[round(w, 3) for w in windows["off"]], windows_ms_on=[round(w, 3) for w in windows["on"]],
        spread_off=round((max(windows["off"]) - min(windows["off"])) / med["off"], 4),
        spread_on=round((max(windows["on"]) - min(windows["on"])) / med["on"], 4),
        sequence_op_paths=launches, last_loss=loss, arith=hb.arith_name(),
        persistent_after=bool(hb.USE_PERSIST and hb.USE_PERSIST_DEC)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="op,step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="op: forward + backward calls per window")
    ap.add_argument("--steps", type=int, default=20, help="step: train steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--out-op", default=os.path.join(ROOT, "profiles", "ctc_bench.jsonl"))
    ap.add_argument("--out-step", default=os.path.join(ROOT, "profiles", "ctc_cost.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "ctc_bench.py measures on the GPU"
    what = args.what.split(",")
    if "op" in what:
        bench_op(args, hb, ops, synth, bench)
    if "step" in what:
        bench_step(args, hb, synth, bench)


if __name__ == "__main__":
    main()
