"""What deterministic mode costs: Solver.sup_train_one_iteration at cfg-2 (32 utterances of 80x800) and cfg-5
(8 of 80x1600), the mode off and on ALTERNATING in one process - two Solvers per configuration (bench.make_solver: the
benchmark's model, weights and batch), `--rounds` rounds of (off, on), each a window of `--steps` steps behind `--warmup`
warm-up steps of that mode, wall clock around a window that ends in flush + device synchronise.  Reports per configuration
the median window of each mode, the spread of each mode's own windows (max - min, as a share of the median: a difference
inside it is not one), and the sequence-operator paths a step of each mode took.  Appends one JSON line per configuration
to --out (default profiles/deterministic_cost.jsonl)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deterministic_cost.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import hip_backend as hb
    import synth
    assert torch.cuda.is_available(), "det_cost.py measures on the GPU"
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="det_cost_")
    for name in args.configs.split(","):
        spec = bench.CONFIGS[name]
        c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
        xs, lens, ys = synth.ragged_batch(B, T, c["input_dim"], c["output_dim"], 1234)
        xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
        solvers = {mode: bench.make_solver(c, B, T, os.path.join(tmp, name + "_" + mode), deterministic=(mode == "on"))
                   for mode in ("off", "on")}
        windows, paths, loss = {"off": [], "on": []}, {}, {}
        for rnd in range(args.rounds):
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
                paths[mode] = {k: v // args.steps for k, v in sorted(hb.LAUNCHES.items())}
                loss[mode] = float(last)
        med = {m: statistics.median(w) for m, w in windows.items()}
        rec = dict(tool="tools/det_cost.py", config=name, call="Solver.sup_train_one_iteration",
                   workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T), rounds=args.rounds, steps_per_window=args.steps,
                   ms_per_step_off=round(med["off"], 3), ms_per_step_on=round(med["on"], 3),
                   cost_ratio=round(med["on"] / med["off"], 3),
                   windows_ms_off=[round(w, 3) for w in windows["off"]], windows_ms_on=[round(w, 3) for w in windows["on"]],
                   spread_off=round((max(windows["off"]) - min(windows["off"])) / med["off"], 4),
                   spread_on=round((max(windows["on"]) - min(windows["on"])) / med["on"], 4),
                   sequence_op_paths=paths, last_loss=loss, arith=hb.arith_name(),
                   persistent_after=bool(hb.USE_PERSIST and hb.USE_PERSIST_DEC))
        line = json.dumps(rec)
        print(line)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del solvers, xs_d, ys_d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
