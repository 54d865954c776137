"""What two-pass decoding costs, every measurement ALTERNATING its sides in one process behind warm-up, in
windows that end in a device synchronise, medians and spreads (max - min over the median) of the windows as
tools/ctc_align_bench.py takes them.  The set-up is DESIGN 4.8's / tools/beam_ctc_bench.py's: cfg-2 decoder widths (D = A = O
= 512, E = 128, 10 channels of kernel 201), T' = 100, V = 50, the ragged lengths of tools/beam_bench.py, the CTC logits from a
seeded head on the encoder frames; B in {1, 32} x K in {4, 8}.  Everything starts behind the encoder, on both sides.

  search    asr_ctc_beam_f32 (csrc/ctc_beam.hip: the frame log-sum-exps, then every frame, the ranking and the backtrace in one
            launch) on buffers allocated once, against asr_ctc_loss_fwd (csrc/ctc.hip), which walks a chain of the same length
            (T' / 2 labels per utterance); plus the search alone at K = 1, 2, 4, 8, 16 (B = 32): what grows with K is the select
            (K rounds) and the candidate walk (K entries), what does not is the rest of a frame
  two_pass  Decoder.rescore_ctc_beams (the search, one teacher-forced decoder pass over B K rows, the combination) against the
            yardstick Decoder.recognize_beams with ctc_decode_weight (the joint search of DESIGN 4.15) at the same B and K
  with_lm   the same two with the judge LM (cfg-2's judge widths): one LM.forward over the B K rows against shallow fusion
            inside the joint search

Appends one JSON line per (B, K) to profiles/two_pass_bench.jsonl."""
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


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def _alternate(sides, rounds, calls, warmup):
    windows = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            for _ in range(warmup):
                fn()
            windows[name].append(_window(fn, calls))
    med = {k: statistics.median(w) for k, w in windows.items()}
    spread = {k: (max(w) - min(w)) / med[k] for k, w in windows.items()}
    return windows, med, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per window of the search alone")
    ap.add_argument("--decode-calls", type=int, default=3, help="calls per window of a whole decode")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_pass_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import model as M
    import synth
    assert torch.cuda.is_available(), "two_pass_bench.py measures on the GPU"
    dev = torch.device("cuda")
    V, L, Tp = 50, 230, 100
    cfg = dict(synth.CFG2, output_dim=V)
    w = synth.e2e_weights(cfg, 99)
    w["decoder.output_layer.bias"][2] -= 30.0
    net = M.E2E(labeldist=synth.labeldist(V, 5), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    lm_cfg = dict(synth.CFG_JUDGE, output_dim=V)
    lm_cfg.pop("ls_weight")
    lm = M.LM(bos=1, eos=2, pad=0, ls_weight=0.0, labeldist=None, **lm_cfg).cuda()
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lm_weights(lm_cfg, 77).items()})
    lm.eval()
    head = torch.from_numpy((np.random.RandomState(7).randn(V, 512) * 0.02).astype(np.float32)).cuda()
    dec = net.decoder
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)

    def search_sides(B, K, z, lens_dev):
        hyp, hyp_len, score = torch.empty(B, K, Tp, **i32), torch.empty(B, K, **i32), torch.empty(B, K, **f32)
        ws = torch.empty((hb.ctc_beam_ws_bytes(B, Tp, V, K) + 3) // 4, **f32)
        return (lambda: hb.ctc_beam(z, lens_dev, K, hyp, hyp_len, score, ws)), (hyp, hyp_len, score)

    for B in (1, 32):
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]
        lens_dev = hb.to_device_i32(lens, dev)
        z = (enc @ head.t()).contiguous()
        nl = Tp // 2 - 20
        labels = torch.from_numpy(np.random.RandomState(1234).randint(1, V, size=B * nl)).to(dev)
        offs = hb.to_device_i32([i * nl for i in range(B + 1)], dev)
        ws_l = torch.empty((hb.ctc_ws_bytes(B, Tp, V, nl) + 3) // 4, **f32)
        nll = torch.empty(B, **f32)

        def loss_fwd():
            hb.ctc_loss_fwd(z, V, lens_dev, labels, offs, nl, False, nll, ws_l)
        for K in (4, 8):
            search, outs = search_sides(B, K, z, lens_dev)
            search(), loss_fwd()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(nll).all()) and bool((outs[1][:, 0] >= 0).all())
            live = float((outs[1] >= 0).float().mean())

            def two_pass(lm_=None):
                return dec.rescore_ctc_beams(enc, lens, z, lens_dev, K, ctc_weight=args.ctc_weight, lm=lm_,
                                             lm_weight=args.lm_weight if lm_ is not None else 0.0)[0]

            def joint(lm_=None):
                return dec.recognize_beams(enc, lens, L, K, ctc_logits=z, ctc_lens=lens_dev, ctc_decode_weight=args.ctc_weight,
                                           lm=lm_, lm_weight=args.lm_weight if lm_ is not None else 0.0)[0]
            ws_, ms, ss = _alternate((("search", search), ("loss_fwd", loss_fwd)), args.rounds, args.calls, args.warmup)
            hb.LAUNCHES.clear()
            wd, md, sd = _alternate((("two_pass", two_pass), ("joint", joint)), args.rounds, args.decode_calls, args.warmup)
            joint_steps = hb.LAUNCHES["beam_ctc_step"] // (args.rounds * (args.decode_calls + args.warmup))
            wl, ml, sl = _alternate((("two_pass_lm", lambda: two_pass(lm)), ("joint_lm", lambda: joint(lm))), args.rounds,
                                    args.decode_calls, args.warmup)
            r4 = lambda x: round(x, 4)                                                          # noqa: E731
            rec = dict(tool="tools/two_pass_bench.py", B=B, K=K, T_out=Tp, V=V, ctc_weight=args.ctc_weight,
                       lm_weight=args.lm_weight, rounds=args.rounds, calls_per_window=args.calls,
                       decode_calls_per_window=args.decode_calls, live_share_of_slots=r4(live),
                       ms_search=r4(ms["search"]), ms_ctc_loss_fwd=r4(ms["loss_fwd"]),
                       ratio_search_over_loss_fwd=round(ms["search"] / ms["loss_fwd"], 3),
                       us_per_frame_search=round(1e3 * ms["search"] / Tp, 3),
                       spread_search=r4(ss["search"]), spread_loss_fwd=r4(ss["loss_fwd"]),
                       windows_ms_search=[r4(x) for x in ws_["search"]],
                       ms_two_pass=r4(md["two_pass"]), ms_joint_beam=r4(md["joint"]), joint_beam_steps=joint_steps,
                       ratio_joint_over_two_pass=round(md["joint"] / md["two_pass"], 3),
                       spread_two_pass=r4(sd["two_pass"]), spread_joint_beam=r4(sd["joint"]),
                       windows_ms_two_pass=[r4(x) for x in wd["two_pass"]], windows_ms_joint_beam=[r4(x) for x in wd["joint"]],
                       ms_two_pass_lm=r4(ml["two_pass_lm"]), ms_joint_beam_lm=r4(ml["joint_lm"]),
                       ratio_joint_lm_over_two_pass_lm=round(ml["joint_lm"] / ml["two_pass_lm"], 3),
                       spread_two_pass_lm=r4(sl["two_pass_lm"]), spread_joint_beam_lm=r4(sl["joint_lm"]),
                       windows_ms_two_pass_lm=[r4(x) for x in wl["two_pass_lm"]],
                       windows_ms_joint_beam_lm=[r4(x) for x in wl["joint_lm"]],
                       ws_bytes_search=hb.ctc_beam_ws_bytes(B, Tp, V, K))
            if B == 32 and K == 8:                            # the search alone over the beam widths
                sides = []
                for k2 in (1, 2, 4, 8, 16):
                    sides.append(("K%d" % k2, search_sides(B, k2, z, lens_dev)[0]))
                _, mk, sk = _alternate(tuple(sides), args.rounds, args.calls, args.warmup)
                rec["ms_search_by_K"] = {k: r4(v) for k, v in mk.items()}
                rec["spread_search_by_K"] = {k: r4(v) for k, v in sk.items()}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
