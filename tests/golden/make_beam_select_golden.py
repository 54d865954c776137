"""Record the attention beam search's select variants that beam_plain_select.npz does not cover (csrc/beam.hip: the judge,
the CTC prefix score, both, and the plain select at the largest candidate list), on the GPU, with the library as it is
built in this checkout:

    python tests/golden/make_beam_select_golden.py        -> tests/golden/beam_select_variants.npz

Only this project's own results are written: per case the outputs of one select and of the backtrack after it, and one
checksum per input array.  tests/test_beam_ngram_gpu.py runs record() again and compares the two at 0 ulp, so the file is
recorded BEFORE a change that must keep the bits, and never after it."""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, V, L, EOS, SEED = 3, 34, 6, 2, 77
STEPS = (("mid", 3), ("last", L - 1))
# (variant, K): K = 4 and 16 give the candidate lists M = 8 and M = 32; the plain select at K = 4 is beam_plain_select.npz
CASES = [("plain", 16)] + [(v, K) for v in ("lm", "ctc", "ctc_lm") for K in (4, 16)]
LM_WEIGHT, CTC_WEIGHT, LENGTH_PENALTY = 0.4, 0.3, 0.5


class _Psi:
    """What select_ctc reads of a CtcPrefixState: no prefix kernel runs."""

    def __init__(self, psi, psi_prev):
        self.psi, self.psi_prev = psi, psi_prev


def inputs(K):
    """logits, scores of test_beam_gpu._select_case; finite judge logits, psi and psi_prev from a fixed generator."""
    import test_beam_gpu as tb
    logits, scores = tb._select_case(K, V, EOS, SEED)
    rs = np.random.RandomState(1000 + K)
    lm_logits = (rs.randn(B * K, V) * 3).astype(np.float32)
    psi = (-rs.rand(B * K, V) * 6).astype(np.float32)
    psi_prev = (-rs.rand(B * K) * 6).astype(np.float32)
    return dict(logits=logits, scores=scores, lm_logits=lm_logits, psi=psi, psi_prev=psi_prev)


def _crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def record(hb):
    """-> {name: array}: for every case and step the select's and the backtrack's outputs (fin and fin_score rows from nfin on
    are zeroed: they are not written), and `in_K<K>_<array>` checksums of the inputs."""
    out = {}
    for variant, K in CASES:
        inp = inputs(K)
        for k, a in inp.items():
            out["in_K%d_%s" % (K, k)] = _crc(a)
        dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in inp.items()}
        z = dev["logits"].reshape(B * K, V)
        for step, t in STEPS:
            s = hb.BeamSearch(B, K, V, L, EOS, "cuda")
            s.scores.copy_(dev["scores"])
            s.tok_hist.zero_()
            s.bp_hist.zero_()
            for i in range(t):                                               # a history for the backtrack to follow
                s.tok_hist[i] = 3 + i
            if variant == "plain":
                s.select(z, t)
            elif variant == "lm":
                s.select_lm(z, dev["lm_logits"], LM_WEIGHT, t)
            else:
                s.select_ctc(z, _Psi(dev["psi"], dev["psi_prev"]), CTC_WEIGHT, t,
                             lm_logits=dev["lm_logits"] if variant == "ctc_lm" else None, lm_weight=LM_WEIGHT)
            toks, sc, lens = s.backtrack(LENGTH_PENALTY)
            torch.cuda.synchronize()
            nf = s.nfin.cpu().numpy()
            fin, fin_score = s.fin.cpu().numpy(), s.fin_score.cpu().numpy()
            for b in range(B):
                fin[b, nf[b]:] = 0
                fin_score[b, nf[b]:] = 0
            name = "%s_K%d_%s_" % (variant, K, step)
            out.update({name + "tok": s.tok_hist[t].cpu().numpy(), name + "bp": s.bp_hist[t].cpu().numpy(),
                        name + "scores": s.scores.cpu().numpy(), name + "nfin": nf, name + "fin": fin,
                        name + "fin_score": fin_score, name + "out_tok": toks.cpu().numpy(), name + "out_score": sc.cpu().numpy(),
                        name + "out_len": lens.cpu().numpy()})
    return out


def bits(a):
    """An array as raw words: equal bits, not equal values (NaN, -0)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    import hip_backend
    rec = record(hip_backend)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "beam_select_variants.npz")
    np.savez_compressed(path, **rec)
    print("beam_select_variants: %d arrays, %d bytes -> %s" % (len(rec), os.path.getsize(path), path))
