"""Bit-level record of the sequence kernels (csrc/ctc.hip, ctc_align.hip, ctc_beam.hip, ctc_prefix.hip, beam.hip, mwer.hip,
rnnt_beam.hip; the searches also with an n-gram LM and with a lexicon and word LM inside):

    python tools/seq_bits.py dump OUT.npz         fixed-seed inputs through every kernel, instantiation and switch -> all outputs
    python tools/seq_bits.py compare A.npz B.npz  exit 1 unless both hold the same arrays, equal as raw 32-bit words

Run `dump` in two checkouts (each in its own process) and `compare` anywhere: the kernels promise the same bits in every run, so
a change that is meant to keep behaviour must compare equal.  Only entry points of ops / hip_backend are used."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


WORDS = ((2,), (3,), (4, 2), (2, 3, 4))      # the lexicon, <space> = 1: the nodes "4" and "2 3" end no word


def _char_lm(V):
    """A token 3-gram (bos 1, eos 2) estimated from fixed-seed text over a few labels of a vocabulary of V."""
    from ngram import NgramLM
    rs = np.random.RandomState(11)
    return NgramLM.estimate([[int(t) for t in rs.randint(3, min(V, 12), rs.randint(2, 12))] for _ in range(200)], 3, V, 1, 2)


def _word_lm(V):
    """A word 3-gram over WORDS, estimated from fixed-seed word sequences, behind their lexicon in a vocabulary of V."""
    from ngram import NgramLM
    from word_lm import Lexicon, WordLM, W_FIRST
    rs = np.random.RandomState(12)
    text = [[W_FIRST + int(w) for w in rs.randint(0, len(WORDS), rs.randint(1, 8))] for _ in range(100)]
    return WordLM(NgramLM.estimate(text, 3, W_FIRST + len(WORDS), 1, 2), Lexicon(list(WORDS), None, 1, None, None, V=V))


def dump(path):
    import torch
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import ops
    dev, out = torch.device("cuda"), {}
    rng = np.random.RandomState(20240611)

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            out["%s.%d" % (name, i)] = t.detach().cpu().contiguous().numpy().view(np.uint32 if t.element_size() == 4 else np.uint8)

    def logits(*shape):
        return torch.from_numpy((3.0 * rng.randn(*shape)).astype(np.float32)).to(dev)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    def labels(V, lens, rep=False):
        seqs = [list(rng.randint(1, V, size=n)) for n in lens]
        if rep:
            seqs[2][1] = seqs[2][0]
        return torch.tensor([x for s in seqs for x in s] or [], dtype=torch.int64, device=dev)

    # CTC loss and alignment: one wave / 256 threads, one state each / eight states a thread; align: back-pointers outside LDS
    chains = [("w64", 4, 12, 5, (12, 9, 12, 3), (0, 3, 5, 5)), ("t256", 2, 140, 9, (140, 117), (100, 37)),
              ("ns8", 1, 300, 9, (300,), (130,)), ("bpws", 1, 370, 3, (370,), (200,))]
    for name, B, T, V, flens, llens in chains:
        z, lab = logits(B, T, V), labels(V, llens, rep=name == "w64")
        if name != "bpws":
            for zi in (True, False):
                zz = z.clone().requires_grad_(True)
                nll = ops.ctc_loss(zz, i32(flens), lab, list(llens), zero_infinity=zi)
                nll.backward(torch.linspace(0.5, 1.5, B, device=dev))
                keep("ctc_%s_zi%d" % (name, zi), nll, zz.grad)
        a = ops.ctc_align(z, i32(flens), lab, list(llens))
        keep("align_" + name, a.path, a.score, a.first, a.last, a.token_logp)
    for V in (2, 70):
        keep("greedy_v%d" % V, *ops.ctc_greedy(logits(3, 65, V), i32((65, 40, 1))))
    # prefix beam search: one wave, four waves, tokens behind the staged ones, history in the workspace, an empty utterance
    # - and the same searches with the n-gram LM and with the lexicon and word LM inside: eos term on / off, lexicon_only off / on
    rng2 = np.random.RandomState(20250307)                          # (the later cases' inputs stay what they were)
    beams = [("k1", 2, 20, 5, 1, (20, 13)), ("k4", 2, 20, 5, 4, (20, 13)), ("v300", 2, 20, 300, 4, (20, 0)),
             ("v1100", 1, 6, 1100, 2, (6,)), ("k16", 1, 300, 5, 16, (300,)), ("k2", 2, 20, 5, 2, (20, 13)), ("k8", 2, 20, 5, 8, (20, 13))]
    full = cut = 0                                                  # lexicon_only: utterances that kept K hypotheses / lost some
    for name, B, T, V, K, flens in beams:
        z = logits(B, T, V) if name not in ("k2", "k8") else torch.from_numpy((3.0 * rng2.randn(B, T, V)).astype(np.float32)).to(dev)
        keep("ctc_beam_" + name, *ops.ctc_beam(z, i32(flens), K))
        char, word = _char_lm(V), _word_lm(V)
        for eos in (1, 0):
            keep("ctc_beam_lm_%s_e%d" % (name, eos), *ops.ctc_beam(z, i32(flens), K, ngram=char, ngram_weight=0.6, ngram_bonus=0.4,
                                                                    eos_term=bool(eos)))
            for lo in (0, 1):
                res = ops.ctc_beam(z, i32(flens), K, word_lm=word, word_lm_weight=0.6, word_bonus=0.4, eos_term=bool(eos),
                                   lexicon_only=bool(lo))
                keep("ctc_beam_wlm_%s_e%d_lo%d" % (name, eos, lo), *res)
                n_hyp = (res[1] >= 0).sum(1).tolist()
                if not lo:                                          # the scorer on the search's own list, unused slots included
                    keep("word_lm_score_%s_e%d" % (name, eos), *ops.word_lm_score(word, res[0].view(B * K, T), res[1].view(-1),
                                                                                  eos_term=bool(eos), per_word=True))
                    whole = n_hyp
                else:
                    # utterances of at least 13 frames and K <= 8 whose free search filled its K slots: the walk of the lexicon
                    # (three first letters, each with a continuation or <space>) fills a beam of 8 within two frames, so a
                    # list shorter than K there is the tail's doing - an entry whose pending node ends no word
                    seen = [n for n, w_, f in zip(n_hyp, whole, flens) if f >= 13 and K <= 8 and w_ == K]
                    full, cut = full + sum(n == K for n in seen), cut + sum(n < K for n in seen)
    out["ctc_beam_lexicon_only_counts.0"] = np.array([full, cut], dtype=np.uint32)
    # the transducer search: plain, n-gram and word LM, one wave of entries and several, a short and an empty utterance
    B, T, L, J, V, E = 3, 6, 5, 64, 34, 8
    r = lambda *s, k=1.0: torch.from_numpy((k * rng2.randn(*s)).astype(np.float32)).to(dev)     # noqa: E731
    head = (r(B, T, J), i32((6, 3, 0)), r(4 * E, 2 * E, k=0.5), r(4 * E, k=0.1), r(J, E, k=0.5), r(V, J, k=0.5), r(V, k=0.1), r(V, E), 33)
    char, word = _char_lm(V), _word_lm(V)
    for K in (1, 4, 16):
        keep("rnnt_beam_k%d" % K, *ops.rnnt_beam(*head, K, L))
        for eos in (1, 0):
            keep("rnnt_beam_lm_k%d_e%d" % (K, eos), *ops.rnnt_beam(*head, K, L, ngram=char, ngram_weight=0.6, ngram_bonus=0.4,
                                                                    eos_term=bool(eos)))
            for lo in (0, 1):
                keep("rnnt_beam_wlm_k%d_e%d_lo%d" % (K, eos, lo), *ops.rnnt_beam(
                    *head, K, L, word_lm=word, word_lm_weight=0.6, word_bonus=0.4, eos_term=bool(eos), lexicon_only=bool(lo)))
    # BeamSearch.select / select_lm / select_ctc with the prefix scorer beside it: init, then three steps
    B, V, Tp, eos = 2, 70, 70, 1
    for K in (1, 4):
        ctc_z, flens = logits(B, Tp, V), i32((70, 51))
        for kind in ("plain", "lm", "ctc", "ctc_lm"):
            bs = hb.BeamSearch(B, K, V, 8, eos, dev)
            if K > 1:
                bs.scores[1, K - 1] = float("-inf")
                bs.scores[0, 1] = -0.5
            st = hb.CtcPrefixState(bs, ctc_z, flens, blank=0, lens_host=[70, 51]) if kind.startswith("ctc") else None
            for t in range(3):
                z, lm = logits(B * K, V), logits(B * K, V)
                if t == 1:
                    z[0] = float("-inf")
                if st is not None:
                    st.score()
                    keep("prefix_k%d_%s_t%d" % (K, kind, t), st.psi, st.state, st.last, st.psi_prev, st.lse)
                    bs.select_ctc(z, st, 0.3, t, lm_logits=lm if kind == "ctc_lm" else None, lm_weight=0.4)
                    st.advance(t)
                elif kind == "lm":
                    bs.select_lm(z, lm, 0.4, t)
                else:
                    bs.select(z, t)
                keep("select_k%d_%s_t%d" % (K, kind, t), bs.scores, bs.tok_hist[:t + 1], bs.bp_hist[:t + 1], bs.nfin, bs.done)
            if st is not None:
                keep("prefix_k%d_%s_end" % (K, kind), st.state, st.last, st.psi_prev)
    # MWER: ragged npos, an unused slot
    B, K, L, V = 2, 4, 6, 70
    z = logits(L, B * K, V).requires_grad_(True)
    tok = torch.from_numpy(rng.randint(0, V, size=(L, B * K))).to(dev)
    loss, parts = ops.mwer_loss(z, tok, i32((6, 3, 0, 5, 1, 6, 4, 2)), i32((2, 0, 9, 1, 3, 3, 0, 5)), 1.0 / B, n_utts=B)
    loss.backward()
    keep("mwer", loss, parts["seq_logp"], parts["post"], parts["risk"], parts["coef"], z.grad)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("seq_bits: %d arrays -> %s" % (len(out), path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
        print("%-34s %-14s %s" % (k, "x".join(map(str, a[k].shape)), "PASS" if same else "DIFFER"))
        if not same:
            bad.append(k)
    cases = sorted({k.split(".")[0] for k in a.files})
    for name, f in (("A", a), ("B", b)):
        if "ctc_beam_lexicon_only_counts.0" in f.files:
            print("%s: ctc_beam with lexicon_only: %d utterances kept K hypotheses, %d lost entries in the tail"
                  % ((name,) + tuple(f["ctc_beam_lexicon_only_counts.0"])))
    print("%d cases, %d arrays: %s" % (len(cases), len(a.files), "PASS" if not bad else "FAIL (%s)" % ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
