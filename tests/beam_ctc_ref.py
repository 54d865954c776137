"""CPU restatement of joint CTC-attention beam search for the tests: the CTC prefix score of Watanabe et al.
2017 from its recurrences, and the search of beam_ref / beam_lm_ref with that term added.

`log_probs` is x[t][v] = logits - logsumexp over the valid frames; `prefix_init`, `prefix_scores`, `prefix_advance` are the
state of the empty prefix, the scores psi(g c) of every one-token extension and the state of an extended prefix - in the
dtype of x, so that the same code is the float64 checker and the float32 yardstick of the kernel tests.  `search` is
beam_lm_ref.search with the CTC term (LM optional), `decode` the search over a decoder state dict, the weights of a CTC
head and, optionally, an LM state dict.  With ctc_weight = 0 the search is beam_ref's / beam_lm_ref's, operation for
operation."""
import numpy as np
import torch

import beam_lm_ref
import beam_ref
from oracle import asr_oracle as O

BLANK = 0


def log_probs(logits):
    """[T, V] raw logits of the valid frames -> x[t][v] = logits[t][v] - logsumexp_v logits[t], in the dtype of `logits`."""
    z = np.asarray(logits)
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True, dtype=z.dtype)))).astype(z.dtype)


def prefix_init(x, blank=BLANK):
    """The empty prefix: r_n = -inf, r_b[t] = sum_{tau <= t} x[tau][blank], psi_prev = 0, no last token."""
    T = x.shape[0]
    return dict(r_n=np.full(T, -np.inf, dtype=x.dtype), r_b=np.cumsum(x[:, blank], dtype=x.dtype), last=-1,
                psi_prev=x.dtype.type(0))


def _phi(st, c):
    return st["r_b"] if c == st["last"] else np.logaddexp(st["r_n"], st["r_b"])


def prefix_scores(st, x, eos, blank=BLANK):
    """psi [V]: psi(g c) = p0 (+) (+)_{t >= 1} (phi[t-1] + x[t][c]); psi(g <EOS>) = r_n[T-1] (+) r_b[T-1]; psi(g blank) = -inf."""
    T, V = x.shape
    both = np.logaddexp(st["r_n"], st["r_b"])
    phi = np.repeat(both[:, None], V, axis=1)
    if st["last"] >= 0:
        phi[:, st["last"]] = st["r_b"]
    psi = x[0].copy() if st["last"] < 0 else np.full(V, -np.inf, dtype=x.dtype)
    for t in range(1, T):
        psi = np.logaddexp(psi, phi[t - 1] + x[t])
    psi[eos] = both[T - 1]
    psi[blank] = -np.inf
    return psi.astype(x.dtype)


def prefix_advance(st, x, c, psi, blank=BLANK):
    """The state of g c from the state of g (psi: prefix_scores of g, for psi_prev)."""
    T = x.shape[0]
    phi = _phi(st, c)
    n, b = np.empty(T, dtype=x.dtype), np.empty(T, dtype=x.dtype)
    n[0] = x[0, c] if st["last"] < 0 else -np.inf
    b[0] = -np.inf
    for t in range(1, T):
        n[t] = np.logaddexp(n[t - 1], phi[t - 1]) + x[t, c]
        b[t] = np.logaddexp(n[t - 1], b[t - 1]) + x[t, blank]
    return dict(r_n=n, r_b=b, last=int(c), psi_prev=psi[c])


def ctc_term(psi, psi_prev):
    """psi - psi_prev with -inf where psi is -inf (also under a psi_prev of -inf: such a candidate never enters)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(psi), -np.inf, psi - psi_prev)


def search(step, K, V, L, eos, x, ctc_weight, lm_weight=None, length_penalty=0.0):
    """step(t, parents [K], tokens [K]) -> logits [K, V] (lm_weight None) or (logits, lm_logits); x [T, V]: log_probs of the
    utterance's CTC logits.  beam_ref.search on (1 - w) logp + w (psi - psi_prev) (+ lm_weight logp_lm); w = 0: no CTC term.
    -> dict(hyps [(tokens, key, length)] ranked, margins per step, rank_margin, steps)."""
    scores = np.full(K, -np.inf)
    scores[0] = 0.0
    paths = [[] for _ in range(K)]
    parents, toks = np.zeros(K, dtype=np.int64), None
    fin, margins = [], []
    states = [prefix_init(x) for _ in range(K)] if ctc_weight else None
    t = 0
    for t in range(L):
        out = step(t, parents, toks)
        logits, lm_logits = out if lm_weight is not None else (out, None)
        fused = beam_ref.log_softmax(logits)
        if ctc_weight:
            psis = [prefix_scores(states[k], x, eos) if np.isfinite(scores[k]) else np.full(V, -np.inf) for k in range(K)]
            term = np.stack([ctc_term(psis[k], states[k]["psi_prev"]) for k in range(K)])
            fused = (1.0 - ctc_weight) * fused + ctc_weight * term
        if lm_weight is not None:
            fused = fused + lm_weight * beam_ref.log_softmax(lm_logits)
        sel = beam_ref.select(scores, fused, eos)
        margins.append(sel["margin"])
        for k, sc in sel["finished"]:
            fin.append((paths[k] + [eos], float(sc), t + 1))
        paths = [paths[sel["bp"][j]] + [int(sel["tok"][j])] if j < sel["nlive"] else [] for j in range(K)]
        if ctc_weight:
            states = [prefix_advance(states[sel["bp"][j]], x, int(sel["tok"][j]), psis[sel["bp"][j]]) if j < sel["nlive"]
                      else states[j] for j in range(K)]
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
    rank_margin = keys[order[0]] - keys[order[1]] if len(order) > 1 else np.inf
    return dict(hyps=hyps, margins=margins, rank_margin=rank_margin, steps=t + 1)


def decode(sd, ctc_w, ctc_b, enc_pad, enc_len, max_dec_timesteps, K, ctc_weight, lm_sd=None, lm_weight=0.0,
           length_penalty=0.0, bos=O.BOS, eos=O.EOS):
    """Beam search over the decoder of state dict `sd` for each utterance of enc_pad [B, T', enc], every candidate scored
    jointly with the CTC head (ctc_w [V, enc], ctc_b [V]) on the utterance's enc_len[b] valid frames and, with lm_sd, the LM.
    The decoder and LM steps are beam_ref.decode's / beam_lm_ref.decode's.  -> list of search() results."""
    dbl = lambda d: {k: (v.detach().double() if torch.is_tensor(v) else torch.as_tensor(v).double())  # noqa: E731
                     for k, v in d.items()}
    sd = dbl(sd)
    lm_sd = dbl(lm_sd) if lm_sd is not None else None
    enc_pad = torch.as_tensor(enc_pad).double()
    ctc_w, ctc_b = torch.as_tensor(ctc_w).double(), torch.as_tensor(ctc_b).double()
    emb_w = sd["decoder.embedding.weight"]
    w_out, b_out = sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"]
    cell = [sd["decoder.LSTMCell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    D = cell[1].shape[1]
    Od = sd["attention.mlp_o.weight"].shape[0]
    V = w_out.shape[0]
    if lm_sd is not None:
        lm_emb = lm_sd["embedding.weight"]
        n_lm, H = len(beam_lm_ref.lm_layers(lm_sd)), lm_sd["LSTM.weight_hh_l0"].shape[1]
    out = []
    for b in range(enc_pad.shape[0]):
        enc = enc_pad[b:b + 1].expand(K, -1, -1).contiguous()
        lens = [int(enc_len[b])] * K
        x = log_probs((enc_pad[b, :lens[0]] @ ctc_w.t() + ctc_b).numpy())
        st = O.AttState()
        state = dict(z=enc.new_zeros(K, D), c=enc.new_zeros(K, D), ctx=enc.new_zeros(K, Od), w=None)
        if lm_sd is not None:
            state.update(lh=enc.new_zeros(n_lm, K, H), lc=enc.new_zeros(n_lm, K, H))

        def step(t, parents, toks, state=state, enc=enc, lens=lens, st=st):
            idx = torch.as_tensor(parents, dtype=torch.long)
            if t > 0:
                for n in ("z", "c", "ctx", "w"):
                    state[n] = state[n][idx]
                if lm_sd is not None:
                    state["lh"], state["lc"] = state["lh"][:, idx], state["lc"][:, idx]
            tk = torch.full((K,), bos, dtype=torch.long) if toks is None else torch.as_tensor(toks, dtype=torch.long)
            xin = torch.cat([emb_w[tk], state["ctx"]], dim=-1)
            state["z"], state["c"] = O.lstm_cell(xin, state["z"], state["c"], *cell)
            state["ctx"], state["w"] = O.attloc_step(sd, st, enc, lens, state["z"], state["w"])
            logits = (torch.cat([state["z"], state["ctx"]], dim=-1) @ w_out.t() + b_out).numpy()
            if lm_sd is None:
                return logits
            lm_logits, state["lh"], state["lc"] = beam_lm_ref.lm_step(lm_sd, lm_emb[tk], state["lh"], state["lc"])
            return logits, lm_logits.numpy()

        out.append(search(step, K, V, max_dec_timesteps, eos, x, ctc_weight, lm_weight if lm_sd is not None else None,
                          length_penalty))
    return out
