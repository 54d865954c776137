"""Joint CTC-attention beam-search timing, modelled on tools/beam_bench.py --lm: milliseconds per decoded
batch for the plain search and the joint one (ctc_decode_weight 0.3), alternating in one process, at DESIGN 4.8's set-up -
cfg-2 decoder widths (D = A = O = 512, E = 128, 10 channels of kernel 201), T' = 100, V = 50, L = 230, the <EOS> bias pushed
down, B in {1, 32} x K in {1, 4, 8}, the ragged lengths of tools/beam_bench.py.  The CTC logits come from a seeded head on
the encoder frames, scaled down so that no prefix dies before its frames run out.

A prefix longer than its utterance's T_b frames has CTC probability 0, so the joint search of an utterance ends after at most
T_b + 1 steps while the plain one, with <EOS> suppressed, runs all L: the two are compared per step actually run
(`steps`), `ctc_us_per_step` = joint ms / joint steps - plain ms / plain steps.  One JSON line per (B, K, method); --out appends
them to a file.  Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/beam_ctc_bench.py --profile` the joint search
of one case (B = 32, K = 4) runs once, for the kernel shares."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--profile", action="store_true", help="the joint search of one case (B = 32, K = 4), for a rocprofv3 run")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import model as M
    import synth
    V, L, Tp = 50, 230, 100
    cfg = dict(synth.CFG2, output_dim=V)
    w = synth.e2e_weights(cfg, 99)
    w["decoder.output_layer.bias"][2] -= 30.0
    net = M.E2E(labeldist=synth.labeldist(V, 5), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    head = torch.from_numpy((np.random.RandomState(7).randn(V, 512) * 0.02).astype(np.float32)).cuda()
    cases = [(32, 4)] if args.profile else [(B, K) for B in (1, 32) for K in (1, 4, 8)]
    for B, K in cases:
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]
        lens_dev = hb.to_device_i32(lens, "cuda")
        ctc_logits = (enc @ head.t()).contiguous()

        def plain():
            return net.decoder.recognize_beams(enc, lens, L, K)[0]

        def joint():
            return net.decoder.recognize_beams(enc, lens, L, K, ctc_logits=ctc_logits, ctc_lens=lens_dev,
                                               ctc_decode_weight=args.ctc_weight)[0]

        methods = (("beam_ctc", joint),) if args.profile else (("beam", plain), ("beam_ctc", joint))
        times = {m: [] for m, _ in methods}
        for _, fn in methods:                                  # warm-up
            fn()
        torch.cuda.synchronize()
        hb.LAUNCHES.clear()
        reps = 1 if args.profile else args.reps
        for _ in range(reps):                                  # alternating: both see the same clocks and neighbours
            for m, fn in methods:
                times[m].append(_timed(fn))
        med, steps = {}, {}
        for m, _ in methods:
            med[m] = float(np.median(times[m]))
            steps[m] = hb.LAUNCHES[m + "_step"] // reps
            rec = dict(K=K, B=B, L=L, Tp=Tp, V=V, method=m, ms_per_batch=round(med[m], 3),
                       ms_all=[round(t, 3) for t in times[m]], steps=steps[m], us_per_step=round(1e3 * med[m] / max(1, steps[m]), 2),
                       launches_per_step=round(hb.LAUNCHES[m + "_launch"] / max(1, hb.LAUNCHES[m + "_step"]), 3))
            if m == "beam_ctc":
                rec["ctc_weight"] = args.ctc_weight
                if "beam" in med:
                    rec["ctc_us_per_step"] = round(1e3 * (med[m] / max(1, steps[m]) - med["beam"] / max(1, steps["beam"])), 2)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
