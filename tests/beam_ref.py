"""CPU restatement of beam-search decoding (Decoder.recognize_beams) for the tests: float64, built on the
oracle's lstm_cell / attloc_step.

`select` is one step's candidate ranking and fairseq walk, `search` the whole per-utterance search over any step
function, `decode` the search over the decoder of a state dict.  Each step also reports its decision margin: the
smallest of the score gaps that decided it (rank K-1 / K: which <EOS> finish; rank 2K-1 / 2K: which candidates are
looked at; the K-th / (K+1)-th non-<EOS> candidate: which beams stay live) - a hypothesis computed in other arithmetic
can only differ where one of them is within that arithmetic's error."""
import numpy as np
import torch

from oracle import asr_oracle as O


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def rank(scores, logp):
    """Flat candidate scores [K*V] (-inf for dead beams) and their order: score desc, lower flat index on ties."""
    scores = np.asarray(scores)
    cand = np.where(np.isfinite(scores)[:, None], scores[:, None] + logp, -np.inf).ravel()
    order = np.argsort(-cand, kind="stable")
    return cand, order


def select(scores, logp, eos):
    """One step for one utterance.  scores [K] (-inf: dead beam), logp [K, V].
    -> dict(tok [K], bp [K], scores [K], finished [(source beam, score)], nlive, margin)."""
    K, V = logp.shape
    cand, order = rank(scores, logp)
    top = [int(i) for i in order[:2 * K] if np.isfinite(cand[i])]
    tok, bp = np.full(K, eos, dtype=np.int64), np.zeros(K, dtype=np.int64)
    new = np.full(K, -np.inf, dtype=cand.dtype)
    finished, nlive, noneos = [], 0, []
    for r, idx in enumerate(top):
        k, v = divmod(idx, V)
        if v == eos:
            if r < K:
                finished.append((k, cand[idx]))
        elif nlive < K:
            tok[nlive], bp[nlive], new[nlive] = v, k, cand[idx]
            nlive += 1
    # decision margin
    srt = cand[order]

    def gap(r):
        if r + 1 >= len(srt) or not np.isfinite(srt[r + 1]):
            return np.inf
        return float(srt[r] - srt[r + 1])

    noneos = [float(cand[i]) for i in order[:2 * K + 1] if np.isfinite(cand[i]) and int(i) % V != eos]
    margin = min(gap(K - 1), gap(2 * K - 1))
    if len(noneos) > K:
        margin = min(margin, noneos[K - 1] - noneos[K])
    return dict(tok=tok, bp=bp, scores=new, finished=finished, nlive=nlive, margin=margin)


def search(step, K, V, L, eos, length_penalty=0.0):
    """step(t, parents [K], tokens [K]) -> logits [K, V] of the beams after the reorder (t = 0: parents 0, tokens None
    = <BOS>).  -> dict(hyps [(tokens, key, length)] ranked (at most K), margins per step, steps)."""
    scores = np.full(K, -np.inf)
    scores[0] = 0.0
    paths = [[] for _ in range(K)]
    parents, toks = np.zeros(K, dtype=np.int64), None
    fin, margins = [], []            # fin: (tokens, score, length) in the order of finishing
    t = 0
    for t in range(L):
        logits = np.asarray(step(t, parents, toks), dtype=np.float64)
        sel = select(scores, log_softmax(logits), eos)
        margins.append(sel["margin"])
        for k, sc in sel["finished"]:
            fin.append((paths[k] + [eos], float(sc), t + 1))
        paths = [paths[sel["bp"][j]] + [int(sel["tok"][j])] if j < sel["nlive"] else [] for j in range(K)]
        scores = sel["scores"]
        if t == L - 1 and len(fin) < K:
            for j in range(sel["nlive"]):
                fin.append((paths[j], float(scores[j]), t + 1))
        if len(fin) >= K or t == L - 1 or sel["nlive"] == 0:
            break
        parents, toks = sel["bp"], sel["tok"]
    keys = [sc / (float(n) ** length_penalty) if length_penalty else sc for _, sc, n in fin]
    order = sorted(range(len(fin)), key=lambda i: (-keys[i], i))
    hyps = [(fin[i][0], keys[i], fin[i][2]) for i in order[:K]]
    # the ranking itself is a decision too: the gap between the best two keys
    rank_margin = keys[order[0]] - keys[order[1]] if len(order) > 1 else np.inf
    return dict(hyps=hyps, margins=margins, rank_margin=rank_margin, steps=t + 1)


def decode(sd, enc_pad, enc_len, max_dec_timesteps, K, length_penalty=0.0, bos=O.BOS, eos=O.EOS):
    """Beam search over the decoder of state dict `sd` for each utterance of enc_pad [B, T', enc] (softmax over all T'
    frames, F1; temperature 2.0, F4).  -> list of search() results."""
    sd = {k: (v.detach().double() if torch.is_tensor(v) else v) for k, v in sd.items()}
    enc_pad = torch.as_tensor(enc_pad).double()
    emb_w = sd["decoder.embedding.weight"]
    w_out, b_out = sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"]
    cell = [sd["decoder.LSTMCell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    D = cell[1].shape[1]
    Od = sd["attention.mlp_o.weight"].shape[0]
    V = w_out.shape[0]
    out = []
    for b in range(enc_pad.shape[0]):
        enc = enc_pad[b:b + 1].expand(K, -1, -1).contiguous()
        lens = [int(enc_len[b])] * K
        st = O.AttState()
        state = dict(z=enc.new_zeros(K, D), c=enc.new_zeros(K, D), ctx=enc.new_zeros(K, Od), w=None)

        def step(t, parents, toks, state=state, enc=enc, lens=lens, st=st):
            idx = torch.as_tensor(parents, dtype=torch.long)
            if t > 0:
                for n in ("z", "c", "ctx", "w"):
                    state[n] = state[n][idx]
            tk = torch.full((K,), bos, dtype=torch.long) if toks is None else torch.as_tensor(toks, dtype=torch.long)
            x = torch.cat([emb_w[tk], state["ctx"]], dim=-1)
            state["z"], state["c"] = O.lstm_cell(x, state["z"], state["c"], *cell)
            state["ctx"], state["w"] = O.attloc_step(sd, st, enc, lens, state["z"], state["w"])
            return (torch.cat([state["z"], state["ctx"]], dim=-1) @ w_out.t() + b_out).numpy()

        out.append(search(step, K, V, max_dec_timesteps, eos, length_penalty))
    return out
