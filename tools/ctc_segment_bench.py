#!/usr/bin/env python
"""Times asr_ctc_segment_f32 (csrc/ctc_segment.hip) and writes profiles/ctc_segment_bench.jsonl (needs a GPU):
  same    the entry with free_ends = 0 against asr_ctc_align_f32 on the same inputs at B = 32, T' = 100, V = 34, 40 labels
          per row, the two alternating in one process
  long    long recordings with free ends: B in {1, 8}, T' = 7 500, V = 34, 200 utterances, per frame and in total, at 8 000
          labels (more labels than frames: the chain runs to the end and finds no alignment, so no backtrace and no output
          passes run) and at 7 000 labels (feasible: chain, backtrace and outputs); and the same call with frame_lens = 1
          (the lse launch and the kernel's setup alone).  The backtrace and output passes are at most the difference of the
          two label counts' times
Every figure is the median over --reps timed calls (hip events around one call, workspace and outputs allocated before),
after --warmup calls."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out)), float(np.min(out))


def segment_call(hb, z, lens, ys, s, lmax, free_ends, window=30):
    """One hb.ctc_segment call on the tensors of an ops.ctc_segment result `s`, with a workspace of its own."""
    B, T, V = z.shape
    ws = torch.empty((hb.ctc_segment_ws_bytes(B, T, V, lmax) + 3) // 4, device=z.device)
    return lambda: hb.ctc_segment(z, lens, ys, s.offsets, lmax, free_ends, s.utt_offsets, s.rec_utts, window, s.path, s.score,
                                  s.first, s.last, s.token_logp, s.utt_begin, s.utt_end, s.utt_logp, s.utt_conf, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_segment_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import ops
    dev = "cuda"
    rs = np.random.RandomState(0)
    rows = []

    def inputs(B, T, V, L, n_utts):
        z = torch.from_numpy(rs.normal(0, 1, size=(B, T, V)).astype(np.float32)).to(dev)
        ys = torch.from_numpy(rs.randint(1, V, size=B * L)).to(dev)
        cuts = [L // n_utts + (1 if i < L % n_utts else 0) for i in range(n_utts)]
        return z, hb.to_device_i32([T] * B, dev), ys, [cuts] * B

    # the entry without free ends against the alignment entry, alternating
    B, T, V, L = 32, 100, 34, 40
    z, lens, ys, utts = inputs(B, T, V, L, 4)
    a, s = ops.ctc_align(z, lens, ys, [L] * B), ops.ctc_segment(z, lens, ys, utts, free_ends=False)
    assert torch.equal(a.path, s.path) and torch.equal(a.token_logp, s.token_logp) and bool(torch.isfinite(a.score).all())
    ws_a = torch.empty((hb.ctc_align_ws_bytes(B, T, V, L) + 3) // 4, device=dev)
    ali = lambda: hb.ctc_align(z, lens, ys, a.offsets, L, a.path, a.score, a.first, a.last, a.token_logp, ws_a)   # noqa: E731
    seg = segment_call(hb, z, lens, ys, s, L, False)
    ta, ts = [], []
    for _ in range(5):
        ta.append(timed(ali, args.warmup, args.reps)[0])
        ts.append(timed(seg, args.warmup, args.reps)[0])
    rows.append(dict(case="same", B=B, T=T, V=V, L=L, align_us=float(np.median(ta)), segment_free0_us=float(np.median(ts)),
                     align_us_per_frame=float(np.median(ta)) / T, segment_us_per_frame=float(np.median(ts)) / T,
                     ratio=float(np.median(ts)) / float(np.median(ta)), rounds=5, reps=args.reps))
    # long recordings
    for B in (1, 8):
        for L in (8000, 7000):
            T, V = 7500, 34
            z, lens, ys, utts = inputs(B, T, V, L, 200)
            s = ops.ctc_segment(z, lens, ys, utts, free_ends=True)
            feasible = bool(torch.isfinite(s.score).all())
            assert feasible == (L == 7000)
            med, best = timed(segment_call(hb, z, lens, ys, s, L, True), 2, max(5, args.reps // 3))
            one = hb.to_device_i32([1] * B, dev)                                   # (no chain, no backtrace)
            med_rest, _ = timed(segment_call(hb, z, one, ys, s, L, True), 2, max(5, args.reps // 3))
            rows.append(dict(case="long", B=B, T=T, V=V, L=L, utterances=200, feasible=feasible, total_us=med, best_us=best,
                             us_per_frame=med / T, frame_lens_1_us=med_rest,
                             ratio_per_frame_to_align=(med / T) / rows[0]["align_us_per_frame"],
                             ws_bytes=hb.ctc_segment_ws_bytes(B, T, V, L)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r, sort_keys=True) + "\n")
            print(json.dumps(r, sort_keys=True))


if __name__ == "__main__":
    main()
