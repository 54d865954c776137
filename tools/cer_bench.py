"""CER scoring: the host's Levenshtein loop against the edit-distance kernel, in one process on the same
pairs.  Per case N (hypothesis, reference) pairs of about `chars` characters over the WSJ character inventory, hypotheses
derived from the references with ~15 % substitutions / insertions / deletions and followed by <EOS> padding, as a decode
leaves them:
  host_ms    utils.calculate_cer on the rendered strings (remove_pad_eos + to_sents are not timed: both routes need them for
             the hypothesis file)
  device_ms  utils.calculate_cer_ids on the id lists: padding, one upload, one launch, one read-back - wall clock, the
             device idle before and after
  kernel_us  asr_edit_distance_i32 alone on operands already on the device (events around `--kernel-reps` launches)
Cases: 32 x 60, 32 x 100, 32 x 230 characters; 256 pairs (B = 32 utterances x K = 8 hypotheses, through ref_index) x 100;
503 x 100 (the size of WSJ's dev93).  Every case first checks that the two routes return the same CER and distances.
Prints one JSON line per case and appends it to --out (default profiles/cer_bench.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((32, 1, 60), (32, 1, 100), (32, 1, 230), (32, 8, 100), (503, 1, 100))     # (utterances, hypotheses each, characters)


def make_pairs(n_utt, k, chars, vocab, seed, err=0.15, tail=20):
    """-> (hyp id lists [n_utt * k] with <EOS> and a padded tail, ref id lists [n_utt], ref_index or None)."""
    rs = np.random.RandomState(seed)
    kept = [i for s, i in vocab.items() if s not in ("<PAD>", "<BOS>", "<EOS>")]      # <NOISE> included: scoring strips it
    eos = vocab["<EOS>"]
    refs, hyps = [], []
    for _ in range(n_utt):
        ref = [int(kept[j]) for j in rs.randint(0, len(kept), size=int(rs.randint(chars - chars // 10, chars + 1)))]
        refs.append(ref)
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
    return hyps, refs, ([b for b in range(n_utt) for _ in range(k)] if k > 1 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cer_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import synth
    import utils
    vocab, nls = synth.wsj_vocab(), list(synth.NON_LANG_SYMS)
    eos, dev = vocab["<EOS>"], torch.device("cuda")
    table = torch.from_numpy(utils.cer_token_table(vocab, nls)).to(dev)
    for n_utt, k, chars in CASES:
        hyps, refs, index = make_pairs(n_utt, k, chars, vocab, seed=chars + n_utt + k)
        hyp_s = utils.to_sents(utils.remove_pad_eos(hyps, eos=eos), vocab, nls)
        ref_s = utils.to_sents(refs, vocab, nls)
        ref_s = [ref_s[i] for i in index] if index is not None else ref_s

        def host():
            return utils.calculate_cer(hyp_s, ref_s)

        def device():
            return utils.calculate_cer_ids(hyps, refs, vocab, nls, eos, dev, ref_index=index)

        want, (got, dist, _) = host(), device()                     # (also the warm-up)
        assert got == want and dist == [utils.edit_distance(h, r) for h, r in zip(hyp_s, ref_s)], (got, want)
        torch.cuda.synchronize()
        host_ms, device_ms = [], []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host()
            host_ms.append(1e3 * (time.perf_counter() - t0))
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device()                                                # (ends with the read-back: synchronous)
            device_ms.append(1e3 * (time.perf_counter() - t0))
        # the kernel alone
        n = len(hyps)
        d_hyp = torch.tensor([h + [eos] * (max(map(len, hyps)) - len(h)) for h in hyps], dtype=torch.int32, device=dev)
        d_ref = torch.tensor([r + [0] * (max(map(len, refs)) - len(r)) for r in refs], dtype=torch.int32, device=dev)
        d_len = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
        d_idx = torch.tensor(index, dtype=torch.int32, device=dev) if index is not None else None
        out = torch.empty(3, n, dtype=torch.int32, device=dev)

        def kernel():
            hb.edit_distance(d_hyp, d_ref, d_len, ref_index=d_idx, eos=eos, skip=table, out=out)

        kernel()
        assert out[0].tolist() == dist
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_reps):
            kernel()
        b.record()
        b.synchronize()
        rec = dict(pairs=n, utterances=n_utt, K=k, chars=chars, cer=round(want, 6),
                   host_ms=round(float(np.median(host_ms)), 3), device_ms=round(float(np.median(device_ms)), 3),
                   kernel_us=round(1e3 * a.elapsed_time(b) / args.kernel_reps, 2),
                   host_ms_all=[round(t, 3) for t in host_ms], device_ms_all=[round(t, 3) for t in device_ms])
        rec["speedup"] = round(rec["host_ms"] / rec["device_ms"], 1)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
