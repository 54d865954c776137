"""Measures the transducer beam search on one GPU beside the greedy decoder of the same tree, alternating the
sides in one process: TransducerHead.beam at B in {1, 32}, T' = 100, L = 100, V = 34, J = 256, K in {1, 4, 8}, plain and with
a 3-gram table, and TransducerHead.greedy (max_symbols 3, the same T' and L) as the yardstick.

Appends one JSON line per (B, K, LM) to profiles/rnnt_beam_bench.jsonl: medians over --rounds windows, every window kept,
ms per call, microseconds per iteration (T' + L of them) and launches per iteration.

--word-lm measures the search with a lexicon and a word LM inside instead: per (B, K) the plain search, the
search with the 3-gram table and the search with a random word 3-gram over a few hundred words (tests/word_lm_ref.py's
recipe), alternating in one process; one line per (B, K) with what = "rnnt_wbeam"."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--word-lm", action="store_true", help="plain, n-gram and word-LM search of the same tree, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_beam_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import model as M
    import ngram
    T, L, V, J, E, P, H = 100, 100, 34, 256, 256, 320, 320
    torch.manual_seed(0)
    head = M.TransducerHead(V, E, P, H, J, bos=1).to("cuda")
    rs = np.random.RandomState(0)
    lm = ngram.NgramLM.estimate([[int(t) for t in rs.randint(3, V, rs.randint(2, 30))] for _ in range(400)], 3, V, 1, 2)
    if args.word_lm:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import word_lm_ref
        words = [tuple(int(c) for c in rs.randint(1, V - 1, rs.randint(1, 6))) for _ in range(300)]
        wlm = word_lm_ref.random_word_lm(V, 3, 1, extra_words=words)
        table = wlm.compile()
        for B in (1, 32):
            enc_h = torch.randn(B, T, H, device="cuda")
            lens = hb.to_device_i32([T] * B, "cuda")
            for K in (1, 4, 8):
                sides = dict(plain=lambda: head.beam(enc_h, lens, K, L),
                             ngram=lambda: head.beam(enc_h, lens, K, L, ngram=lm, ngram_weight=0.5, ngram_bonus=0.5),
                             word_lm=lambda: head.beam(enc_h, lens, K, L, word_lm=wlm, word_lm_weight=0.5, word_bonus=0.5))
                windows = {k: [] for k in sides}
                with torch.no_grad():
                    before = hb.LAUNCHES["rnnt_wbeam_launch"]
                    sides["word_lm"]()
                    launches = hb.LAUNCHES["rnnt_wbeam_launch"] - before
                    for _ in range(args.rounds):
                        for k, fn in sides.items():
                            for _ in range(args.warmup):
                                fn()
                            windows[k].append(_window(fn, args.calls))
                rec = dict(what="rnnt_wbeam", B=B, T=T, L=L, V=V, J=J, K=K, lexicon_words=len(wlm.lexicon), word_states=table.S,
                           word_arcs=table.A, trie_nodes=table.N, launches=launches,
                           launches_per_iteration=round((launches - 2) / (T + L), 3))
                for k, w in windows.items():
                    med = statistics.median(w)
                    rec.update({"ms_" + k: round(med, 4), "windows_ms_" + k: [round(v, 4) for v in w],
                                "spread_" + k: round((max(w) - min(w)) / med, 4)})
                rec["word_lm_minus_plain_ms"] = round(rec["ms_word_lm"] - rec["ms_plain"], 4)
                rec["ngram_minus_plain_ms"] = round(rec["ms_ngram"] - rec["ms_plain"], 4)
                line = json.dumps(rec)
                print(line)
                os.makedirs(os.path.dirname(args.out), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        return
    for B in (1, 32):
        enc_h = torch.randn(B, T, H, device="cuda")
        lens = hb.to_device_i32([T] * B, "cuda")
        for K in (1, 4, 8):
            for fused in (False, True):
                kw = dict(ngram=lm, ngram_weight=0.5, ngram_bonus=0.5) if fused else {}
                sides = dict(beam=lambda: head.beam(enc_h, lens, K, L, **kw), greedy=lambda: head.greedy(enc_h, lens, 3, L))
                before = hb.LAUNCHES["rnnt_beam_launch"]
                with torch.no_grad():
                    sides["beam"]()
                    launches = hb.LAUNCHES["rnnt_beam_launch"] - before
                    windows = {k: [] for k in sides}
                    for _ in range(args.rounds):
                        for k, fn in sides.items():
                            for _ in range(args.warmup):
                                fn()
                            windows[k].append(_window(fn, args.calls))
                rec = dict(what="rnnt_beam", B=B, T=T, L=L, V=V, J=J, K=K, ngram=fused, launches=launches,
                           launches_per_iteration=round((launches - 2) / (T + L), 3))
                for k, w in windows.items():
                    med = statistics.median(w)
                    rec.update({"ms_" + k: round(med, 4), "windows_ms_" + k: [round(v, 4) for v in w],
                                "spread_" + k: round((max(w) - min(w)) / med, 4), "us_per_iteration_" + k: round(med * 1e3 / (T + L), 2)})
                line = json.dumps(rec)
                print(line)
                os.makedirs(os.path.dirname(args.out), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
