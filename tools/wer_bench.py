"""WER scoring: three scorers on the same pairs, in one process.  Per case B utterances x K hypotheses whose
references are transcripts of tests/golden/synth.py's text generator (learnable_corpus: words of letters joined by <space>,
now and then a <NOISE>) at WSJ-like sizes - 8 .. 28 words of 1 .. 9 letters, about 100 tokens -, hypotheses derived from them
with ~5 % of the tokens (spaces included) substituted / inserted / deleted and followed by <EOS> padding:
  host_ms        utils.calculate_wer on the rendered strings (the host's Levenshtein loop over the words)
  device_ms      utils.calculate_wer_ids on the id lists: padding, one upload, one launch, one read-back - wall clock
  token_us       asr_edit_distance_i32 alone on resident operands (what CER costs on these pairs)
  word_us        asr_word_edit_distance_i32 alone on the same operands
token_us and word_us are medians of windows that alternate between the two kernels behind a warm-up, each window
`--kernel-reps` launches between device events; word_over_token is their ratio.  Cases: B x K = 32 x 1, 32 x 8, 333 x 4
(the size of WSJ's eval92).  Every case first checks the three scorers against each other.
With --step also one MWER train step at cfg-2 (bench.py's model, batch 32, 800 frames), K = 4, with `mwer_unit` token and word
on the same solver, alternating.  Prints one JSON line per record and appends it to --out (default profiles/wer_bench.jsonl)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ((32, 1), (32, 8), (333, 4))          # (utterances, hypotheses each)


def make_pairs(n_utt, k, vocab, seed, err=0.05, tail=20):
    """-> (hyp id lists [n_utt * k] with <EOS> and a padded tail, ref id lists [n_utt], ref_index)."""
    import synth
    corpus = synth.learnable_corpus(n_utt, seed, input_dim=1, words=(8, 28), word_len=(1, 9), hold=(1, 1))
    refs = [corpus[u]["token_ids"] for u in sorted(corpus)]
    rs = np.random.RandomState(seed + 1)
    kept = [i for s, i in vocab.items() if s not in ("<PAD>", "<BOS>", "<EOS>")]
    eos = vocab["<EOS>"]
    hyps = []
    for ref in refs:
        for _ in range(k):
            hyp = []
            for t in ref:
                u = rs.uniform()
                if u < err / 3:
                    continue                                             # deletion
                hyp.append(int(kept[rs.randint(len(kept))]) if u < 2 * err / 3 else t)
                if u > 1 - err / 3:
                    hyp.append(int(kept[rs.randint(len(kept))]))         # insertion
            hyps.append(hyp + [eos] * tail)
    return hyps, refs, [b for b in range(n_utt) for _ in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time the MWER train step with both units")
    ap.add_argument("--step-calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wer_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import synth
    import utils
    from mwer_bench import _alternate
    assert torch.cuda.is_available(), "wer_bench.py measures on the GPU"
    vocab, nls = synth.wsj_vocab(), list(synth.NON_LANG_SYMS)
    eos, space, dev = vocab["<EOS>"], vocab["<space>"], torch.device("cuda")
    table = torch.from_numpy(utils.cer_token_table(vocab, nls)).to(dev)
    r4 = lambda x: round(x, 4)                                           # noqa: E731

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for n_utt, k in CASES:
        hyps, refs, index = make_pairs(n_utt, k, vocab, seed=100 * n_utt + k)
        hyp_s = utils.to_sents(utils.remove_pad_eos(hyps, eos=eos), vocab, nls)
        ref_s = utils.to_sents(refs, vocab, nls)
        ref_s = [ref_s[i] for i in index]

        def host():
            return utils.calculate_wer(hyp_s, ref_s)

        def device():
            return utils.calculate_wer_ids(hyps, refs, vocab, nls, eos, dev, ref_index=index)

        want, (got, dist, ref_n) = host(), device()                      # (also the warm-up)
        assert got == want and dist == [utils.edit_distance(h.split(), r.split()) for h, r in zip(hyp_s, ref_s)], (got, want)
        torch.cuda.synchronize()
        host_ms, device_ms = [], []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host()
            host_ms.append(1e3 * (time.perf_counter() - t0))
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device()                                                     # (ends with the read-back: synchronous)
            device_ms.append(1e3 * (time.perf_counter() - t0))
        # the two kernels alone, on the same resident operands
        n = len(hyps)
        d_hyp = torch.tensor([h + [eos] * (max(map(len, hyps)) - len(h)) for h in hyps], dtype=torch.int32, device=dev)
        d_ref = torch.tensor([r + [0] * (max(map(len, refs)) - len(r)) for r in refs], dtype=torch.int32, device=dev)
        d_len = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
        d_idx = torch.tensor(index, dtype=torch.int32, device=dev)
        out_t = torch.empty(3, n, dtype=torch.int32, device=dev)
        out_w = torch.empty(3, n, dtype=torch.int32, device=dev)

        def token():
            hb.edit_distance(d_hyp, d_ref, d_len, ref_index=d_idx, eos=eos, skip=table, out=out_t)

        def word():
            hb.word_edit_distance(d_hyp, d_ref, d_len, space, ref_index=d_idx, eos=eos, skip=table, out=out_w)

        token()
        word()
        assert out_w[0].tolist() == dist and out_w[2].tolist() == ref_n
        assert out_t[0].tolist() == [utils.edit_distance(h, r) for h, r in zip(hyp_s, ref_s)]
        w, m, s = _alternate((("token", token), ("word", word)), args.rounds, args.kernel_reps, args.warmup)
        emit(dict(tool="tools/wer_bench.py", what="scoring", pairs=n, utterances=n_utt, K=k,
                  tokens_per_reference=r4(float(np.mean([len(r) for r in refs]))), words_per_reference=r4(sum(ref_n) / float(n)),
                  columns=[int(d_hyp.shape[1]), int(d_ref.shape[1])], wer=round(want, 6),
                  host_ms=round(float(np.median(host_ms)), 3), device_ms=round(float(np.median(device_ms)), 3),
                  host_over_device=round(float(np.median(host_ms)) / float(np.median(device_ms)), 1),
                  token_us=round(1e3 * m["token"], 2), word_us=round(1e3 * m["word"], 2),
                  word_over_token=round(m["word"] / m["token"], 3), rounds=args.rounds, launches_per_window=args.kernel_reps,
                  spread={k_: r4(v) for k_, v in s.items()}, windows_us={k_: [round(1e3 * x, 2) for x in v] for k_, v in w.items()},
                  host_ms_all=[round(t, 3) for t in host_ms], device_ms_all=[round(t, 3) for t in device_ms]))
    if not args.step:
        return

    import bench
    K = 4
    spec = bench.CONFIGS["cfg2"]
    cfg = dict(spec["model"])
    torch.manual_seed(1000)
    np.random.seed(1000)
    solver = bench.make_solver(cfg, spec["batch"], spec["frames"], os.path.join(tempfile.mkdtemp(prefix="wer_bench_"), "main"),
                               mwer_beam=K, mwer_ce_weight=0.01)
    xs, lens, ys = synth.ragged_batch(spec["batch"], spec["frames"], cfg["input_dim"], cfg["output_dim"], 1234)
    xs_d = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    ys_d = [torch.from_numpy(y).to(dev) for y in ys]
    word_id = solver.mwer_unit_config(dict(mwer_unit="word"), solver.vocab)
    err = {}

    def step(unit_space):
        def run():
            solver.mwer_space = unit_space                               # what `mwer_unit` sets when the solver is built
            solver.model.space_id = unit_space
            solver.mwer_train_one_iteration(xs_d, lens, ys_d)
            solver.flush()
        return run
    sides = (("token", step(None)), ("word", step(word_id)))
    for name, fn in sides:
        fn()
        err[name] = float(solver.model.last_mwer["err"].float().mean())
    w, m, s = _alternate(sides, args.rounds, args.step_calls, 2)
    emit(dict(tool="tools/wer_bench.py", what="mwer train step", config="cfg2", B=len(lens), K=K, frames=spec["frames"],
              rounds=args.rounds, calls_per_window=args.step_calls, ms_step_token=r4(m["token"]), ms_step_word=r4(m["word"]),
              word_over_token=round(m["word"] / m["token"], 4), mean_err={k_: r4(v) for k_, v in err.items()},
              parent_ms_mwer_step=24.8844, parent_record="profiles/mwer_bench.jsonl, `train step`",
              spread={k_: r4(v) for k_, v in s.items()}, windows_ms={k_: [r4(x) for x in v] for k_, v in w.items()}))


if __name__ == "__main__":
    main()
