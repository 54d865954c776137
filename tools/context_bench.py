"""What contextual biasing costs inside the CTC prefix beam search, at the shapes of tools/ngram_bench.py (B in
{1, 32}, K in {4, 8}, T' = 100, V = 50): alternating windows of calls that end in a device synchronise, medians and spreads
(max - min over the median) of the windows, as tools/two_pass_bench.py takes them.
    context-alone search      against the plain search      (alternating)
    n-gram + context search   against the n-gram search     (alternating)
    the scoring kernel alone  (asr_context_score_f32 over the B K hypotheses of the plain search)
for phrase lists of 10 and 1000 phrases, one list shared by the batch and one list per utterance.
--parent-lib PATH: the plain and the n-gram search of the parent commit's library beside this one's, alternating - the
existing instantiations did not move, in time; the margin is the windows' own spread in the same run.
Appends one JSON line per (B, K, phrases, shared) to profiles/context_bench.jsonl."""
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


def phrase_list(V, n, seed):
    """n phrases of 2 .. 6 labels drawn from ngram_bench's synthetic text, so that the search meets them."""
    from ngram_bench import synthetic_text
    rs = np.random.RandomState(seed)
    out = []
    for seq in synthetic_text(V, n, seed):
        at = rs.randint(0, max(1, len(seq) - 6))
        out.append(seq[at:at + rs.randint(2, 7)])
    return out


def main():
    from ngram_bench import synthetic_text
    from two_pass_bench import _alternate
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ctx-weight", type=float, default=1.0)
    ap.add_argument("--boost", type=float, default=1.5)
    ap.add_argument("--parent-lib", default=None, help="libasr_hip.so of the parent commit: its plain and n-gram search, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    from context import ContextBatch, ContextGraph
    from ngram import NgramLM
    assert torch.cuda.is_available(), "context_bench.py measures on the GPU"
    dev = torch.device("cuda")
    V, Tp = 50, 100
    head = torch.from_numpy((np.random.RandomState(7).randn(V, 512) * 0.02).astype(np.float32)).cuda()
    lm = NgramLM.estimate(synthetic_text(V, 2000, 11), 4, V, 1, 2)
    table = lm.to(dev)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.asr_ctc_beam_f32.argtypes = hb.load().asr_ctc_beam_f32.argtypes
        parent.asr_ctc_beam_lm_f32.argtypes = hb.load().asr_ctc_beam_lm_f32.argtypes
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    r4 = lambda x: round(x, 4)                                                                  # noqa: E731
    built = {}
    for B in (1, 32):
        rs = np.random.RandomState(B)
        enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
        lens_dev = hb.to_device_i32([Tp - (b * 37) % 40 for b in range(B)], dev)
        z = (enc @ head.t()).contiguous()
        for K in (4, 8):
            hyp, hyp_len = torch.empty(B, K, Tp, **i32), torch.empty(B, K, **i32)
            score, ctc, lms, cxs = (torch.empty(B, K, **f32) for _ in range(4))
            ws = torch.empty((hb.ctc_beam_ws_bytes(B, Tp, V, K) + 3) // 4, **f32)
            ns = torch.empty(B * K, **f32)

            def plain():
                hb.ctc_beam(z, lens_dev, K, hyp, hyp_len, score, ws)

            def ngram():
                hb.ctc_beam_lm(z, lens_dev, K, table, 0.5, 0.5, True, hyp, hyp_len, score, ctc, lms, ws)

            def plain_parent():
                assert parent.asr_ctc_beam_f32(B, Tp, V, K, hb.ptr(z), V, hb.ptr(lens_dev), hb.ptr(hyp), hb.ptr(hyp_len),
                                               hb.ptr(score), hb.ptr(ws), hb.stream()) == 0

            def ngram_parent():
                assert parent.asr_ctc_beam_lm_f32(B, Tp, V, K, hb.ptr(z), V, hb.ptr(lens_dev), table.S, hb.ptr(table.logp),
                                                  hb.ptr(table.nxt), int(table.start), int(table.eos), 0.5, 0.5, hb.ptr(hyp),
                                                  hb.ptr(hyp_len), hb.ptr(score), hb.ptr(ctc), hb.ptr(lms), hb.ptr(ws), hb.stream()) == 0
            plain()
            torch.cuda.synchronize()
            list_hyp, list_len = hyp.view(B * K, Tp).clone(), hyp_len.view(-1).clone()
            base = dict(tool="tools/context_bench.py", B=B, K=K, T_out=Tp, V=V, ctx_weight=args.ctx_weight, boost=args.boost,
                        rounds=args.rounds, calls_per_window=args.calls)
            if parent is not None:
                bits = score.clone()
                plain_parent()
                torch.cuda.synchronize()
                base["parent_bits_equal"] = bool(torch.equal(bits, score))
                wp, mp, sp = _alternate((("plain", plain), ("plain_parent", plain_parent), ("ngram", ngram),
                                         ("ngram_parent", ngram_parent)), args.rounds, args.calls, args.warmup)
                base.update(ms_plain_ab=r4(mp["plain"]), ms_plain_parent=r4(mp["plain_parent"]),
                            ratio_plain_over_parent=r4(mp["plain"] / mp["plain_parent"]), spread_plain_ab=r4(sp["plain"]),
                            spread_plain_parent=r4(sp["plain_parent"]), ms_ngram_ab=r4(mp["ngram"]),
                            ms_ngram_parent=r4(mp["ngram_parent"]), ratio_ngram_over_parent=r4(mp["ngram"] / mp["ngram_parent"]),
                            spread_ngram_ab=r4(sp["ngram"]), spread_ngram_parent=r4(sp["ngram_parent"]))
            for n_phrases in (10, 1000):
                for shared in (True, False):
                    if (B, n_phrases, shared) not in built:            # (compiled once per list, not per beam width)
                        if shared:
                            context = ContextGraph(phrase_list(V, n_phrases, 5), boost=args.boost, V=V)
                        else:
                            context = ContextBatch([ContextGraph(phrase_list(V, n_phrases, 100 + b), boost=args.boost, V=V)
                                                    for b in range(B)], list(range(B)))
                        built[(B, n_phrases, shared)] = context.to(dev)
                    ctab = built[(B, n_phrases, shared)]
                    rows = torch.arange(B, **i32).repeat_interleave(K) if not shared else torch.zeros(B * K, **i32)

                    def ctx_alone():
                        hb.ctc_beam_ctx(z, lens_dev, K, ctab, args.ctx_weight, None, 0.0, 0.0, True, hyp, hyp_len, score, ctc, None,
                                        cxs, ws)

                    def ctx_ngram():
                        hb.ctc_beam_ctx(z, lens_dev, K, ctab, args.ctx_weight, table, 0.5, 0.5, True, hyp, hyp_len, score, ctc, lms,
                                        cxs, ws)

                    def scorer():
                        hb.context_score(ctab, list_hyp, list_len, ns, graph_of=rows)
                    _, m, s = _alternate((("plain", plain), ("ctx", ctx_alone), ("ngram", ngram), ("ngram_ctx", ctx_ngram),
                                          ("score", scorer)), args.rounds, args.calls, args.warmup)
                    rec = dict(base, phrases=n_phrases, shared=shared, states=ctab.N, arcs=ctab.A,
                               ms_plain=r4(m["plain"]), ms_ctx=r4(m["ctx"]), ms_ngram=r4(m["ngram"]), ms_ngram_ctx=r4(m["ngram_ctx"]),
                               ms_context_score=r4(m["score"]), us_per_frame_plain=round(1e3 * m["plain"] / Tp, 3),
                               us_per_frame_ctx=round(1e3 * m["ctx"] / Tp, 3), us_per_frame_ngram=round(1e3 * m["ngram"] / Tp, 3),
                               us_per_frame_ngram_ctx=round(1e3 * m["ngram_ctx"] / Tp, 3),
                               ratio_ctx_over_plain=round(m["ctx"] / m["plain"], 3),
                               ratio_ngram_ctx_over_ngram=round(m["ngram_ctx"] / m["ngram"], 3),
                               spread_plain=r4(s["plain"]), spread_ctx=r4(s["ctx"]), spread_ngram=r4(s["ngram"]),
                               spread_ngram_ctx=r4(s["ngram_ctx"]), spread_context_score=r4(s["score"]))
                    line = json.dumps(rec)
                    print(line, flush=True)
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
