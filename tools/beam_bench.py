"""Beam-search decode timing: milliseconds per decoded batch for greedy (Decoder.forward, ys=None) and for
Decoder.recognize_beams with K in {1, 4, 8}, B in {1, 32}, at cfg-2 decoder widths (D = A = O = 512, E = 128, 10
channels of kernel 201), T' = 100, V = 50, L = 230 steps.  The output layer's <EOS> bias is pushed down so that every
decode runs all L steps (the worst case, the same work for every method).  Prints one JSON line per case with the
launches per beam step.  Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/beam_bench.py --profile` one case
(B = 32, K = 4) runs once, for the kernel shares."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="one case (B = 32, K = 4), for a rocprofv3 run")
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
    cases = [(32, 4)] if args.profile else [(B, K) for B in (1, 32) for K in ("greedy", 1, 4, 8)]
    for B, K in cases:
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]

        def run():
            with torch.no_grad():
                if K == "greedy":
                    return net.decoder(enc, lens, ys=None, max_dec_timesteps=L)[2]
                return net.decoder.recognize_beams(enc, lens, L, K)[0]

        run()
        torch.cuda.synchronize()
        hb.LAUNCHES.clear()
        times = []
        for _ in range(1 if args.profile else args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        rec = dict(method="greedy" if K == "greedy" else "beam", K=None if K == "greedy" else K, B=B, L=L, Tp=Tp, V=V,
                   ms_per_batch=round(float(np.median(times)), 3), ms_all=[round(t, 3) for t in times])
        if K != "greedy":
            rec["steps"] = hb.LAUNCHES["beam_step"] // len(times)
            rec["launches_per_step"] = round(hb.LAUNCHES["beam_launch"] / max(1, hb.LAUNCHES["beam_step"]), 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
