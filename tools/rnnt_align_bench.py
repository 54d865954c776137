"""What transducer forced alignment costs: asr_transducer_align_f32 (csrc/rnnt_align.hip: the node pass, then
chain + backtrace + outputs in one launch) against asr_rnnt_loss_fwd_f32 (csrc/rnnt.hip: the node log-sum-exps, then the same
chain with logaddexp on it) on the same inputs, ALTERNATING the two sides in one process behind warm-up, medians of the
windows as tools/ctc_align_bench.py takes them.  No time is promised: the loss forward is the yardstick.

Shape: B = 32, T = 100, U = 100 with the rows ragged down to half of both, V = 34.  Buffers are allocated once.

Appends one JSON line to profiles/rnnt_align_bench.jsonl.  Wall clock around windows that end in a device synchronise; the
spread of each side's own windows (max - min over the median) says what a difference is worth."""
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

B, T, U, V = 32, 100, 100, 34


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
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_align_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    assert torch.cuda.is_available(), "rnnt_align_bench.py measures on the GPU"
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rs = np.random.RandomState(1234)
    frames = [T] + [int(n) for n in rs.randint(T // 2, T + 1, size=B - 1)]
    counts = [U] + [int(n) for n in rs.randint(U // 2, U + 1, size=B - 1)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).tolist()
    labels = torch.from_numpy(rs.randint(1, V, size=offsets[-1])).to(dev)
    offs, lens = hb.to_device_i32(offsets, dev), hb.to_device_i32(frames, dev)
    z = (3.0 * torch.randn(B, T, U + 1, V, generator=torch.Generator().manual_seed(5))).to(dev)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    score, nll = torch.empty(B, **f32), torch.empty(B, **f32)
    emit, tlp = torch.empty(offsets[-1], **i32), torch.empty(offsets[-1], **f32)
    fl, bl = torch.empty(B, T, **i32), torch.empty(B, T, **f32)
    ws_a = torch.empty((hb.rnnt_align_ws_bytes(B, T, U, V) + 3) // 4, **f32)
    ws_l = torch.empty((hb.rnnt_ws_bytes(B, T, U, 4, V) + 3) // 4, **f32)

    def align():
        hb.rnnt_align(z, V, lens, labels, offs, score, emit, tlp, fl, bl, ws_a)

    def loss_fwd():
        hb.rnnt_loss_fwd(z, V, lens, labels, offs, nll, ws_l)

    align(), loss_fwd()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(nll).all())
    assert bool((score <= -nll).all())                          # the best alignment is one of those the loss sums
    parts = torch.stack([tlp[offsets[b]:offsets[b + 1]].double().sum() + bl[b].double().sum() for b in range(B)])
    assert float((parts - score.double()).abs().max()) < 1e-2   # score = the sum of its parts
    w, m, s = _alternate(args, (("align", align), ("loss_fwd", loss_fwd)))
    rec = dict(tool="tools/rnnt_align_bench.py", B=B, T=T, U=U, V=V, frames_min=min(frames), labels_min=min(counts),
               labels_total=offsets[-1], rounds=args.rounds, calls_per_window=args.calls,
               ms_align=round(m["align"], 4), ms_rnnt_loss_fwd=round(m["loss_fwd"], 4),
               ratio_align_over_loss_fwd=round(m["align"] / m["loss_fwd"], 3),
               spread_align=round(s["align"], 4), spread_loss_fwd=round(s["loss_fwd"], 4),
               windows_ms_align=[round(x, 4) for x in w["align"]], windows_ms_loss_fwd=[round(x, 4) for x in w["loss_fwd"]],
               ws_bytes_align=hb.rnnt_align_ws_bytes(B, T, U, V), ws_bytes_loss=hb.rnnt_ws_bytes(B, T, U, 4, V))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
