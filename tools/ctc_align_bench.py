"""What CTC forced alignment and best-path decoding cost, each measurement ALTERNATING its two sides in one
process behind warm-up, medians of the windows as tools/ctc_bench.py takes them:

  align   asr_ctc_align_f32 (csrc/ctc_align.hip: the frame log-sum-exps, then chain + backtrace + outputs in one launch)
          against asr_ctc_loss_fwd (csrc/ctc.hip: the same chain with logsumexp on it), both on buffers allocated once, at the
          decoder-side shapes of cfg-2 (B = 32, T' = 100, V = 34) and cfg-5 (B = 8, T' = 200, V = 34) with full-length
          utterances and T' / 2 labels each (every row feasible);
  greedy  asr_ctc_greedy_f32 (argmax, collapse and compaction in one launch) against torch-ROCm's logits.argmax(-1) (the
          argmax alone) on the same logits.

Appends one JSON line per shape to profiles/ctc_align_bench.jsonl.  Wall clock around windows that end in a device
synchronise; the spread of each side's own windows (max - min over the median) says what a difference is worth."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("cfg2", 32, 100, 34), ("cfg5", 8, 200, 34))


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def _alternate(args, sides):
    windows = {name: [] for name, _ in sides}
    for _ in range(args.rounds):
        for name, fn in sides:
            for _ in range(args.warmup):
                fn()
            windows[name].append(_window(fn, args.calls))
    med = {k: statistics.median(w) for k, w in windows.items()}
    spread = {k: (max(w) - min(w)) / med[k] for k, w in windows.items()}
    return windows, med, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    assert torch.cuda.is_available(), "ctc_align_bench.py measures on the GPU"
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name, B, T, V in SHAPES:
        L = T // 2
        rs = np.random.RandomState(1234)
        labels = torch.from_numpy(rs.randint(1, V, size=B * L)).to(dev)
        offs = hb.to_device_i32([i * L for i in range(B + 1)], dev)
        lens = hb.to_device_i32([T] * B, dev)
        z = (3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(5))).to(dev)
        i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
        path, score = torch.empty(B, T, **i32), torch.empty(B, **f32)
        first, last, tlp = torch.empty(B * L, **i32), torch.empty(B * L, **i32), torch.empty(B * L, **f32)
        ws_a = torch.empty((hb.ctc_align_ws_bytes(B, T, V, L) + 3) // 4, **f32)
        ws_l = torch.empty((hb.ctc_ws_bytes(B, T, V, L) + 3) // 4, **f32)
        nll = torch.empty(B, **f32)
        ids, n, ft = torch.empty(B, T, **i32), torch.empty(B, **i32), torch.empty(B, T, **i32)

        def align():
            hb.ctc_align(z, lens, labels, offs, L, path, score, first, last, tlp, ws_a)

        def loss_fwd():
            hb.ctc_loss_fwd(z, V, lens, labels, offs, L, False, nll, ws_l)

        def greedy():
            hb.ctc_greedy(z, lens, ids, n, ft)

        def argmax():
            z.argmax(-1)
        align(), loss_fwd(), greedy()
        torch.cuda.synchronize()
        feasible = int(torch.isfinite(score).sum())
        assert feasible == B == int(torch.isfinite(nll).sum())
        assert bool((score <= -nll).all())                      # the best alignment is one of those the loss sums
        assert torch.equal(ft.long(), z.argmax(-1))
        wa, ma, sa = _alternate(args, (("align", align), ("loss_fwd", loss_fwd)))
        wg, mg, sg = _alternate(args, (("greedy", greedy), ("argmax", argmax)))
        rec = dict(tool="tools/ctc_align_bench.py", shape=name, B=B, T_out=T, V=V, labels_per_utterance=L,
                   feasible_utterances=feasible, rounds=args.rounds, calls_per_window=args.calls,
                   ms_align=round(ma["align"], 4), ms_ctc_loss_fwd=round(ma["loss_fwd"], 4),
                   ratio_align_over_loss_fwd=round(ma["align"] / ma["loss_fwd"], 3),
                   spread_align=round(sa["align"], 4), spread_loss_fwd=round(sa["loss_fwd"], 4),
                   windows_ms_align=[round(w, 4) for w in wa["align"]], windows_ms_loss_fwd=[round(w, 4) for w in wa["loss_fwd"]],
                   ms_greedy=round(mg["greedy"], 4), ms_torch_argmax=round(mg["argmax"], 4),
                   ratio_greedy_over_argmax=round(mg["greedy"] / mg["argmax"], 3),
                   spread_greedy=round(sg["greedy"], 4), spread_argmax=round(sg["argmax"], 4),
                   windows_ms_greedy=[round(w, 4) for w in wg["greedy"]], windows_ms_argmax=[round(w, 4) for w in wg["argmax"]],
                   back_pointers="lds" if hb.ctc_align_ws_bytes(B, T, V, L) == 8 * ((B * T + 63) // 64 * 64) else "workspace",
                   ws_bytes_align=hb.ctc_align_ws_bytes(B, T, V, L), ws_bytes_loss=hb.ctc_ws_bytes(B, T, V, L))
        line = json.dumps(rec)
        print(line)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
