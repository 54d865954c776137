"""What the n-gram LM costs, every measurement ALTERNATING its sides in one process behind warm-up, in windows
that end in a device synchronise, medians and spreads (max - min over the median) of the windows, as tools/two_pass_bench.py
takes them - and at its shapes: B in {1, 32} x K in {4, 8}, T' = 100, V = 50, the cfg-2 decoder behind the search, a 4-gram
from NgramLM.estimate on synthetic text.

  plain      asr_ctc_beam_f32 of this tree - and, with --parent-lib (the parent commit's libasr_hip.so, built apart), the same
             entry of that library on the same buffers, alternating: the LM = false instantiations must not have moved
  fused      asr_ctc_beam_lm_f32 against the plain search, us per frame
  score      asr_ngram_score_f32 alone, on the plain search's list (B K rows of T' ids); plain + score is what rescoring a
             list costs, to hold against fused
  two_pass   Decoder.rescore_ctc_beams with and without the n-gram LM

Appends one JSON line per (B, K) to profiles/ngram_bench.jsonl."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def synthetic_text(V, n, seed):
    """Label sequences with structure an n-gram can learn: a random first-order chain over the labels 3 .. V - 1."""
    rs = np.random.RandomState(seed)
    labels = np.arange(3, V)
    trans = rs.dirichlet(np.full(len(labels), 0.05), size=len(labels))
    out = []
    for _ in range(n):
        c, seq = rs.randint(len(labels)), []
        for _ in range(rs.randint(5, 40)):
            seq.append(int(labels[c]))
            c = rs.choice(len(labels), p=trans[c])
        out.append(seq)
    return out


def main():
    from two_pass_bench import _alternate
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per window of a search or the scoring kernel")
    ap.add_argument("--decode-calls", type=int, default=3, help="calls per window of a whole two-pass decode")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ngram-weight", type=float, default=0.5)
    ap.add_argument("--ngram-bonus", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libasr_hip.so of the parent commit: the plain search of both, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import model as M
    import synth
    from ngram import NgramLM
    assert torch.cuda.is_available(), "ngram_bench.py measures on the GPU"
    dev = torch.device("cuda")
    V, Tp = 50, 100
    cfg = dict(synth.CFG2, output_dim=V)
    w = synth.e2e_weights(cfg, 99)
    net = M.E2E(labeldist=synth.labeldist(V, 5), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    dec = net.decoder
    head = torch.from_numpy((np.random.RandomState(7).randn(V, 512) * 0.02).astype(np.float32)).cuda()
    lm = NgramLM.estimate(synthetic_text(V, 2000, 11), 4, V, 1, 2)
    table = lm.to(dev)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.asr_ctc_beam_f32.argtypes = hb.load().asr_ctc_beam_f32.argtypes
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    r4 = lambda x: round(x, 4)                                                                  # noqa: E731
    for B in (1, 32):
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens = [Tp - (b * 37) % 40 for b in range(B)]
        lens_dev = hb.to_device_i32(lens, dev)
        z = (enc @ head.t()).contiguous()
        for K in (4, 8):
            hyp, hyp_len = torch.empty(B, K, Tp, **i32), torch.empty(B, K, **i32)
            score, ctc, lms = (torch.empty(B, K, **f32) for _ in range(3))
            ws = torch.empty((hb.ctc_beam_ws_bytes(B, Tp, V, K) + 3) // 4, **f32)
            ns = torch.empty(B * K, **f32)

            def plain():
                hb.ctc_beam(z, lens_dev, K, hyp, hyp_len, score, ws)

            def plain_parent():
                rc = parent.asr_ctc_beam_f32(B, Tp, V, K, hb.ptr(z), V, hb.ptr(lens_dev), hb.ptr(hyp), hb.ptr(hyp_len), hb.ptr(score),
                                             hb.ptr(ws), hb.stream())
                assert rc == 0

            def fused():
                hb.ctc_beam_lm(z, lens_dev, K, table, args.ngram_weight, args.ngram_bonus, True, hyp, hyp_len, score, ctc, lms, ws)
            plain()
            torch.cuda.synchronize()
            list_hyp, list_len = hyp.view(B * K, Tp).clone(), hyp_len.view(-1).clone()
            plain_bits = score.clone()

            def rescore():
                hb.ngram_score(table, list_hyp, list_len, ns)

            def two_pass(with_lm):
                extra = dict(ngram=lm, ngram_weight=args.ngram_weight, ngram_bonus=args.ngram_bonus) if with_lm else {}
                return dec.rescore_ctc_beams(enc, lens, z, lens_dev, K, ctc_weight=0.3, **extra)[0]
            rec = dict(tool="tools/ngram_bench.py", B=B, K=K, T_out=Tp, V=V, order=lm.order, states=table.S,
                       ngram_weight=args.ngram_weight, ngram_bonus=args.ngram_bonus, rounds=args.rounds,
                       calls_per_window=args.calls, decode_calls_per_window=args.decode_calls)
            if parent is not None:
                plain_parent()
                torch.cuda.synchronize()
                rec["parent_bits_equal"] = bool(torch.equal(plain_bits, score))
                wp, mp, sp = _alternate((("plain", plain), ("parent", plain_parent)), args.rounds, args.calls, args.warmup)
                rec.update(ms_plain_ab=r4(mp["plain"]), ms_plain_parent=r4(mp["parent"]),
                           ratio_plain_over_parent=round(mp["plain"] / mp["parent"], 4),
                           spread_plain_ab=r4(sp["plain"]), spread_plain_parent=r4(sp["parent"]),
                           windows_ms_plain_ab=[r4(x) for x in wp["plain"]], windows_ms_plain_parent=[r4(x) for x in wp["parent"]])
            wf, mf, sf = _alternate((("plain", plain), ("fused", fused), ("score", rescore)), args.rounds, args.calls, args.warmup)
            wt, mt, st = _alternate((("two_pass", lambda: two_pass(False)), ("two_pass_ngram", lambda: two_pass(True))),
                                    args.rounds, args.decode_calls, args.warmup)
            rec.update(ms_plain=r4(mf["plain"]), ms_fused=r4(mf["fused"]), ms_ngram_score=r4(mf["score"]),
                       us_per_frame_plain=round(1e3 * mf["plain"] / Tp, 3), us_per_frame_fused=round(1e3 * mf["fused"] / Tp, 3),
                       ratio_fused_over_plain=round(mf["fused"] / mf["plain"], 3),
                       ratio_fused_over_plain_plus_score=round(mf["fused"] / (mf["plain"] + mf["score"]), 3),
                       spread_plain=r4(sf["plain"]), spread_fused=r4(sf["fused"]), spread_ngram_score=r4(sf["score"]),
                       windows_ms_plain=[r4(x) for x in wf["plain"]], windows_ms_fused=[r4(x) for x in wf["fused"]],
                       ms_two_pass=r4(mt["two_pass"]), ms_two_pass_ngram=r4(mt["two_pass_ngram"]),
                       ratio_two_pass_ngram_over_two_pass=round(mt["two_pass_ngram"] / mt["two_pass"], 3),
                       spread_two_pass=r4(st["two_pass"]), spread_two_pass_ngram=r4(st["two_pass_ngram"]))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
