"""Beam-search decode timing: milliseconds per decoded batch for greedy (Decoder.forward, ys=None) and for
Decoder.recognize_beams with K in {1, 4, 8}, B in {1, 32}, at cfg-2 decoder widths (D = A = O = 512, E = 128, 10
channels of kernel 201), T' = 100, V = 50, L = 230 steps.  The output layer's <EOS> bias is pushed down so that every
decode runs all L steps (the worst case, the same work for every method).  Prints one JSON line per case with the
launches per beam step.  Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/beam_bench.py --profile` one case
(B = 32, K = 4) runs once, for the kernel shares.

--lm: shallow fusion with the cfg-4 judge (2 x 640 LSTM, E = 256).  Per (B, K) three lines from the same
process: "beam" (the plain search), "beam_lm" (the fused search) and "lm_forward_step" - one LM.forward_step call per
step on the same B*K rows, the only way to compute the LM's part without the fused kernels (its state is not permuted and
nothing is selected: a lower bound of that composition).  `lm_us_per_step` of the fused line is (fused - plain) / L.
With --profile the one case is the fused search.  --lm-micro times asr_lm_step_f32 alone (R = 4 and 128, one layer at
H = In = 640: 13.1 MB of weights per call) for its achieved weight bandwidth.

--ngram / --word-lm: a 3-gram automaton over the V tokens, or a lexicon of a few thousand words with a bigram word
LM, inside the search.  Per (B, K), B in {1, 32} and K in {4, 8}, two lines from the same process, the plain search ("beam")
and the fused one ("beam_ngram" / "beam_word_lm"), their calls alternating; `select_us_per_step` of the fused line is
(fused - plain) / L, the cost of the fused select over the plain select.  With --profile the one case is the fused search."""
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
    ap.add_argument("--lm", action="store_true", help="shallow fusion with the cfg-4 judge: plain, fused, LM.forward_step")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lm-micro", action="store_true", help="asr_lm_step_f32 alone: time and weight bandwidth")
    ap.add_argument("--ngram", action="store_true", help="a 3-gram LM inside the search: plain and fused, alternating")
    ap.add_argument("--word-lm", action="store_true", help="a lexicon and word LM inside the search: plain and fused, alternating")
    ap.add_argument("--table-lm-weight", type=float, default=0.5)
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
    lm = None
    if args.lm or args.lm_micro:
        lm_cfg = dict(synth.CFG_JUDGE, output_dim=V)
        lm_cfg.pop("ls_weight")
        lm = M.LM(bos=1, eos=2, pad=0, ls_weight=0.0, labeldist=None, **lm_cfg).cuda()
        lm.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lm_weights(lm_cfg, 77).items()})
        lm.eval()
    if args.lm_micro:
        return lm_micro(hb, lm)
    if args.lm:
        return lm_cases(args, hb, net, lm, V, L, Tp)
    if args.ngram or args.word_lm:
        return table_lm_cases(args, hb, net, V, L, Tp)
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


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def lm_cases(args, hb, net, lm, V, L, Tp):
    cases = [(32, 4)] if args.profile else [(B, K) for B in (1, 32) for K in (1, 4, 8)]
    reps = 1 if args.profile else args.reps
    for B, K in cases:
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]
        emb = lm.embedding(torch.full((B * K,), lm.bos, dtype=torch.long, device="cuda")).unsqueeze(1)

        def plain():
            return net.decoder.recognize_beams(enc, lens, L, K)[0]

        def fused():
            return net.decoder.recognize_beams(enc, lens, L, K, lm=lm, lm_weight=args.lm_weight)[0]

        def forward_steps():
            z = c = None
            for _ in range(L):
                logit, z, c = lm.forward_step(emb, z, c)
            return logit

        base = dict(K=K, B=B, L=L, Tp=Tp, V=V)
        med = {}
        for method, fn in (("beam_lm", fused),) if args.profile else (("beam", plain), ("beam_lm", fused),
                                                                       ("lm_forward_step", forward_steps)):
            hb.LAUNCHES.clear()
            times = _timed(fn, reps)
            med[method] = float(np.median(times))
            rec = dict(base, method=method, ms_per_batch=round(med[method], 3), ms_all=[round(t, 3) for t in times])
            key = {"beam": "beam", "beam_lm": "beam_lm"}.get(method)
            if key:
                rec["steps"] = hb.LAUNCHES[key + "_step"] // (len(times) + 1)
                rec["launches_per_step"] = round(hb.LAUNCHES[key + "_launch"] / max(1, hb.LAUNCHES[key + "_step"]), 3)
            if method == "beam_lm" and "beam" in med:
                rec["lm_weight"] = args.lm_weight
                rec["lm_us_per_step"] = round(1e3 * (med["beam_lm"] - med["beam"]) / L, 2)
            if method == "lm_forward_step":
                rec["lm_us_per_step"] = round(1e3 * med[method] / L, 2)
            print(json.dumps(rec), flush=True)


def table_lm_cases(args, hb, net, V, L, Tp):
    from ngram import NgramLM
    from word_lm import WordLM
    rs = np.random.RandomState(3)
    space = V - 1
    if args.ngram:
        text = [[int(c) for c in rs.randint(3, V, size=rs.randint(5, 40))] for _ in range(400)]
        kw = dict(ngram=NgramLM.estimate(text, 3, V, 1, 2), ngram_weight=args.table_lm_weight, ngram_bonus=0.2)
        method = "beam_ngram"
    else:
        words = [[int(c) for c in rs.randint(3, space, size=rs.randint(1, 7))] for _ in range(3000)]
        text = []
        for _ in range(1500):
            row = []
            for i in rs.randint(len(words), size=rs.randint(2, 9)):
                row += words[i] + [space]
            text.append(row[:-1])
        kw = dict(word_lm=WordLM.estimate(text, space, 2, V=V, bos=1, eos=2), word_lm_weight=args.table_lm_weight, word_bonus=0.2)
        method = "beam_word_lm"
    cases = [(32, 4)] if args.profile else [(B, K) for B in (1, 32) for K in (4, 8)]
    reps = 1 if args.profile else args.reps
    for B, K in cases:
        ers = np.random.RandomState(B)
        enc = torch.from_numpy(ers.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]
        fns = dict(beam=lambda: net.decoder.recognize_beams(enc, lens, L, K)[0],
                   fused=lambda: net.decoder.recognize_beams(enc, lens, L, K, **kw)[0])
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        times = dict(beam=[], fused=[])
        steps = {}
        for _ in range(reps):                                    # alternating: both see the same clocks
            for name in (("fused",) if args.profile else ("beam", "fused")):
                hb.LAUNCHES.clear()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fns[name]()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
                steps[name] = (hb.LAUNCHES["beam_step"], round(hb.LAUNCHES["beam_launch"] / max(1, hb.LAUNCHES["beam_step"]), 3))
        med = {k: float(np.median(v)) for k, v in times.items() if v}
        for name in med:
            rec = dict(method="beam" if name == "beam" else method, K=K, B=B, L=L, Tp=Tp, V=V, ms_per_batch=round(med[name], 3),
                       ms_all=[round(t, 3) for t in times[name]], steps=steps[name][0], launches_per_step=steps[name][1])
            if name == "fused" and "beam" in med:
                rec["select_us_per_step"] = round(1e3 * (med["fused"] - med["beam"]) / L, 2)
            print(json.dumps(rec), flush=True)


def lm_micro(hb, lm):
    H = lm.hidden_dim
    layer = lm.LSTM.direction_params(1)                       # H -> H: 4H x 2H fp32 weights
    for R in (4, 128):
        st = hb.LmStepState(R, torch.zeros(4, H, device="cuda"), [layer])
        st.xin[0].normal_()
        n = 200

        def run():
            for _ in range(n):
                st.step()

        times = _timed(run, 5)
        us = 1e3 * float(np.median(times)) / n
        mb = 4 * H * 2 * H * 4 / 1e6
        print(json.dumps(dict(method="asr_lm_step_f32", R=R, H=H, In=H, us_per_call=round(us, 2), weight_MB=round(mb, 2),
                              weight_GBps=round(mb / us * 1e3, 1), back_to_back_calls=n)), flush=True)


if __name__ == "__main__":
    main()
