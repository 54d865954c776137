"""What the word-level LM and lexicon cost, every measurement ALTERNATING its sides in one process behind
warm-up, in windows that end in a device synchronise, medians and spreads (max - min over the median) of the windows, as
tools/ngram_bench.py takes them: B in {1, 32} x K in {4, 8}, T' = 100, V = 34 (a character vocabulary), the cfg-2 decoder
behind the search, a word 3-gram (NgramLM.estimate over synthetic word sequences) over a synthetic lexicon of 20 000 and of
1 000 words, a character 4-gram for the char-LM side.

  plain / char_lm    asr_ctc_beam_f32 and asr_ctc_beam_lm_f32 of this tree - and, with --parent-lib (the parent commit's
                     libasr_hip.so, built apart), the same entries of that library on the same buffers, alternating, outputs
                     compared bit for bit: the existing instantiations must not have moved
  word_lm            asr_ctc_beam_wlm_f32 with lexicon_only off and on, us per frame against the two above
  score              asr_word_lm_score_f32 alone, on the plain search's list (B K rows of T' ids)
  two_pass           Decoder.rescore_ctc_beams without and with the word LM

Appends one JSON line per (lexicon, B, K) to profiles/word_lm_bench.jsonl."""
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

SPACE, FIRST_LETTER = 3, 4


def synthetic_word_lm(V, n_words, order, seed, n_sentences=3000):
    """A lexicon of n_words random spellings over the letters and a Witten-Bell model over Zipf-drawn word sequences with
    first-order structure (a word's successor is drawn near it), so that bigram and trigram contexts repeat."""
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM, W_FIRST
    rs = np.random.RandomState(seed)
    spell = set()
    while len(spell) < n_words:
        spell.add(tuple(int(c) for c in rs.randint(FIRST_LETTER, V, size=rs.randint(2, 9))))
    lex = Lexicon(sorted(spell), None, SPACE, 1, 2, V=V)
    p = 1.0 / np.arange(1, n_words + 1)
    p /= p.sum()
    text = []
    for _ in range(n_sentences):
        w, row = int(rs.choice(n_words, p=p)), []
        for _ in range(rs.randint(3, 12)):
            row.append(W_FIRST + w)
            w = (w + int(rs.choice(8))) % n_words if rs.rand() < 0.7 else int(rs.choice(n_words, p=p))
        text.append(row)
    return WordLM(NgramLM.estimate(text, order, W_FIRST + n_words, 1, 2), lex)


def main():
    from two_pass_bench import _alternate
    from ngram_bench import synthetic_text
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per window of a search or the scoring kernel")
    ap.add_argument("--decode-calls", type=int, default=3, help="calls per window of a whole two-pass decode")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--bonus", type=float, default=0.5)
    ap.add_argument("--lexicons", type=int, nargs="+", default=[20000, 1000])
    ap.add_argument("--parent-lib", default=None, help="libasr_hip.so of the parent commit: the plain and char-LM searches of both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_lm_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import model as M
    import synth
    from ngram import NgramLM
    assert torch.cuda.is_available(), "word_lm_bench.py measures on the GPU"
    dev = torch.device("cuda")
    V, Tp = 34, 100
    cfg = dict(synth.CFG2, output_dim=V)
    w = synth.e2e_weights(cfg, 99)
    net = M.E2E(labeldist=synth.labeldist(V, 5), **cfg).cuda()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    net.eval()
    dec = net.decoder
    head = torch.from_numpy((np.random.RandomState(7).randn(V, 512) * 0.02).astype(np.float32)).cuda()
    char_lm = NgramLM.estimate(synthetic_text(V, 2000, 11), 4, V, 1, 2)
    char_table = char_lm.to(dev)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.asr_ctc_beam_f32.argtypes = hb.load().asr_ctc_beam_f32.argtypes
        parent.asr_ctc_beam_lm_f32.argtypes = hb.load().asr_ctc_beam_lm_f32.argtypes
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    r4 = lambda x: round(x, 4)                                                                  # noqa: E731
    for n_lex in args.lexicons:
        wlm = synthetic_word_lm(V, n_lex, 3, 5)
        table = wlm.to(dev)
        for B in (1, 32):
            rs = np.random.RandomState(B)
            enc = torch.from_numpy(rs.randn(B, Tp, 512).astype(np.float32)).cuda()
            lens = [Tp - (b * 37) % 40 for b in range(B)]
            lens_dev = hb.to_device_i32(lens, dev)
            z = (enc @ head.t()).contiguous()
            for K in (4, 8):
                hyp, hyp_len, nws = torch.empty(B, K, Tp, **i32), torch.empty(B, K, **i32), torch.empty(B, K, **i32)
                score, ctc, lms = (torch.empty(B, K, **f32) for _ in range(3))
                ws = torch.empty((hb.ctc_beam_ws_bytes(B, Tp, V, K) + 3) // 4, **f32)
                ns, nn = torch.empty(B * K, **f32), torch.empty(B * K, **i32)

                def plain():
                    hb.ctc_beam(z, lens_dev, K, hyp, hyp_len, score, ws)

                def char():
                    hb.ctc_beam_lm(z, lens_dev, K, char_table, args.weight, args.bonus, True, hyp, hyp_len, score, ctc, lms, ws)

                def plain_parent():
                    assert parent.asr_ctc_beam_f32(B, Tp, V, K, hb.ptr(z), V, hb.ptr(lens_dev), hb.ptr(hyp), hb.ptr(hyp_len),
                                                   hb.ptr(score), hb.ptr(ws), hb.stream()) == 0

                def char_parent():
                    assert parent.asr_ctc_beam_lm_f32(B, Tp, V, K, hb.ptr(z), V, hb.ptr(lens_dev), char_table.S, hb.ptr(char_table.logp),
                                                      hb.ptr(char_table.nxt), char_table.start, char_table.eos, args.weight, args.bonus,
                                                      hb.ptr(hyp), hb.ptr(hyp_len), hb.ptr(score), hb.ptr(ctc), hb.ptr(lms), hb.ptr(ws),
                                                      hb.stream()) == 0

                def word(lexicon_only):
                    hb.ctc_beam_wlm(z, lens_dev, K, table, args.weight, args.bonus, True, lexicon_only, hyp, hyp_len, score, ctc, lms,
                                    nws, ws)

                def bits(fn):
                    fn()
                    torch.cuda.synchronize()
                    return [t.clone() for t in (hyp, hyp_len, score, ctc, lms)]
                plain_bits = bits(plain)
                list_hyp, list_len = hyp.view(B * K, Tp).clone(), hyp_len.view(-1).clone()

                def rescore():
                    hb.word_lm_score(table, list_hyp, list_len, ns, nn)

                def two_pass(with_lm):
                    extra = dict(word_lm=wlm, word_lm_weight=args.weight, word_bonus=args.bonus) if with_lm else {}
                    return dec.rescore_ctc_beams(enc, lens, z, lens_dev, K, ctc_weight=0.3, **extra)[0]
                rec = dict(tool="tools/word_lm_bench.py", lexicon=n_lex, B=B, K=K, T_out=Tp, V=V, order=wlm.order, states=table.S,
                           arcs=table.A, trie_nodes=table.N, weight=args.weight, bonus=args.bonus, rounds=args.rounds,
                           calls_per_window=args.calls, decode_calls_per_window=args.decode_calls)
                if parent is not None:
                    char_bits = bits(char)
                    rec["parent_plain_bits_equal"] = all(torch.equal(a, b) for a, b in zip(plain_bits[:3], bits(plain_parent)[:3]))
                    rec["parent_char_lm_bits_equal"] = all(torch.equal(a, b) for a, b in zip(char_bits, bits(char_parent)))
                    wp, mp, sp = _alternate((("plain", plain), ("plain_parent", plain_parent), ("char_lm", char),
                                             ("char_lm_parent", char_parent)), args.rounds, args.calls, args.warmup)
                    for k in mp:
                        rec["ms_ab_" + k], rec["spread_ab_" + k] = r4(mp[k]), r4(sp[k])
                        rec["windows_ms_ab_" + k] = [r4(x) for x in wp[k]]
                    rec["ratio_plain_over_parent"] = round(mp["plain"] / mp["plain_parent"], 4)
                    rec["ratio_char_lm_over_parent"] = round(mp["char_lm"] / mp["char_lm_parent"], 4)
                sides = (("plain", plain), ("char_lm", char), ("word_lm", lambda: word(False)), ("word_lm_lexicon_only", lambda: word(True)),
                         ("score", rescore))
                wf, mf, sf = _alternate(sides, args.rounds, args.calls, args.warmup)
                wt, mt, st = _alternate((("two_pass", lambda: two_pass(False)), ("two_pass_word_lm", lambda: two_pass(True))),
                                        args.rounds, args.decode_calls, args.warmup)
                for k in mf:
                    rec["ms_" + k], rec["spread_" + k] = r4(mf[k]), r4(sf[k])
                    rec["windows_ms_" + k] = [r4(x) for x in wf[k]]
                for k in ("plain", "char_lm", "word_lm", "word_lm_lexicon_only"):
                    rec["us_per_frame_" + k] = round(1e3 * mf[k] / Tp, 3)
                rec.update(ratio_word_lm_over_plain=round(mf["word_lm"] / mf["plain"], 3),
                           ratio_word_lm_over_char_lm=round(mf["word_lm"] / mf["char_lm"], 3),
                           ms_two_pass=r4(mt["two_pass"]), ms_two_pass_word_lm=r4(mt["two_pass_word_lm"]),
                           ratio_two_pass_word_lm_over_two_pass=round(mt["two_pass_word_lm"] / mt["two_pass"], 3),
                           spread_two_pass=r4(st["two_pass"]), spread_two_pass_word_lm=r4(st["two_pass_word_lm"]))
                line = json.dumps(rec)
                print(line, flush=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
