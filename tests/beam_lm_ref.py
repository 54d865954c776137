"""CPU restatement of beam search with shallow LM fusion for the tests: float64, the LM step on the oracle's
lstm_cell, the ranking and the walk on beam_ref.select over logp_asr + lm_weight * logp_lm.

`lm_step` is one step of the stacked LSTM + output layer of an LM state dict, `search` the per-utterance search over a
step function that returns both models' logits, `decode` the search over a decoder state dict and an LM state dict.
Margins, hypotheses and keys are reported as beam_ref.search reports them; with lm_weight = 0 they are beam_ref's."""
import numpy as np
import torch

import beam_ref
from oracle import asr_oracle as O


def lm_layers(lm_sd):
    """[(w_ih, w_hh, b_ih, b_hh)] of an LM state dict, bottom layer first."""
    out, l = [], 0
    while "LSTM.weight_ih_l%d" % l in lm_sd:
        out.append(tuple(lm_sd["LSTM.%s_l%d" % (n, l)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        l += 1
    return out


def lm_step(lm_sd, x, h, c):
    """x [R, E] (embedded tokens), h / c [n_layers, R, H] -> (logits [R, V], h, c); eval arithmetic, any float dtype."""
    new_h, new_c = [], []
    for l, cell in enumerate(lm_layers(lm_sd)):
        hl, cl = O.lstm_cell(x, h[l], c[l], *cell)
        new_h.append(hl)
        new_c.append(cl)
        x = hl
    return x @ lm_sd["output_layer.weight"].t() + lm_sd["output_layer.bias"], torch.stack(new_h), torch.stack(new_c)


def search(step, K, V, L, eos, lm_weight, length_penalty=0.0):
    """step(t, parents [K], tokens [K]) -> (logits [K, V], lm_logits [K, V]) of the beams after the reorder (t = 0:
    parents 0, tokens None = <BOS>).  beam_ref.search on the fused log-probabilities:
    -> dict(hyps [(tokens, key, length)] ranked (at most K), margins per step, rank_margin, steps)."""
    scores = np.full(K, -np.inf)
    scores[0] = 0.0
    paths = [[] for _ in range(K)]
    parents, toks = np.zeros(K, dtype=np.int64), None
    fin, margins = [], []
    t = 0
    for t in range(L):
        logits, lm_logits = step(t, parents, toks)
        fused = beam_ref.log_softmax(logits) + lm_weight * beam_ref.log_softmax(lm_logits)
        sel = beam_ref.select(scores, fused, eos)
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
    rank_margin = keys[order[0]] - keys[order[1]] if len(order) > 1 else np.inf
    return dict(hyps=hyps, margins=margins, rank_margin=rank_margin, steps=t + 1)


def decode(sd, lm_sd, enc_pad, enc_len, max_dec_timesteps, K, lm_weight, length_penalty=0.0, bos=O.BOS, eos=O.EOS):
    """Beam search over the decoder of state dict `sd`, every candidate rescored by the LM of state dict `lm_sd` (keys of
    model.LM), for each utterance of enc_pad [B, T', enc].  The decoder step is beam_ref.decode's; the LM consumes the
    same token through its own embedding and carries h, c per beam.  -> list of search() results."""
    dbl = lambda d: {k: (v.detach().double() if torch.is_tensor(v) else torch.as_tensor(v).double())  # noqa: E731
                     for k, v in d.items()}
    sd, lm_sd = dbl(sd), dbl(lm_sd)
    enc_pad = torch.as_tensor(enc_pad).double()
    emb_w, lm_emb = sd["decoder.embedding.weight"], lm_sd["embedding.weight"]
    w_out, b_out = sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"]
    cell = [sd["decoder.LSTMCell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    D = cell[1].shape[1]
    Od = sd["attention.mlp_o.weight"].shape[0]
    V = w_out.shape[0]
    n_lm, H = len(lm_layers(lm_sd)), lm_sd["LSTM.weight_hh_l0"].shape[1]
    out = []
    for b in range(enc_pad.shape[0]):
        enc = enc_pad[b:b + 1].expand(K, -1, -1).contiguous()
        lens = [int(enc_len[b])] * K
        st = O.AttState()
        state = dict(z=enc.new_zeros(K, D), c=enc.new_zeros(K, D), ctx=enc.new_zeros(K, Od), w=None,
                     lh=enc.new_zeros(n_lm, K, H), lc=enc.new_zeros(n_lm, K, H))

        def step(t, parents, toks, state=state, enc=enc, lens=lens, st=st):
            idx = torch.as_tensor(parents, dtype=torch.long)
            if t > 0:
                for n in ("z", "c", "ctx", "w"):
                    state[n] = state[n][idx]
                state["lh"], state["lc"] = state["lh"][:, idx], state["lc"][:, idx]
            tk = torch.full((K,), bos, dtype=torch.long) if toks is None else torch.as_tensor(toks, dtype=torch.long)
            x = torch.cat([emb_w[tk], state["ctx"]], dim=-1)
            state["z"], state["c"] = O.lstm_cell(x, state["z"], state["c"], *cell)
            state["ctx"], state["w"] = O.attloc_step(sd, st, enc, lens, state["z"], state["w"])
            lm_logits, state["lh"], state["lc"] = lm_step(lm_sd, lm_emb[tk], state["lh"], state["lc"])
            return (torch.cat([state["z"], state["ctx"]], dim=-1) @ w_out.t() + b_out).numpy(), lm_logits.numpy()

        out.append(search(step, K, V, max_dec_timesteps, eos, lm_weight, length_penalty))
    return out


def find_seeds(make_case, cases, tries, margin, min_steps):
    """The seed search of tests/test_beam_lm_gpu.py, restated so that it can be run again: for every case the first
    candidate in `tries` for which the restatement alone meets both conditions of the end-to-end test - at least
    (4B + 4) // 5 utterances with a smallest decision margin above `margin`, and one of them running >= min_steps steps.
    make_case(case, candidate) -> list of search() results.  -> {case: (candidate, margins, steps)}."""
    found = {}
    for case in cases:
        for cand in tries:
            res = make_case(case, cand)
            ok = [r for r in res if min(r["margins"]) > margin]
            if len(ok) >= (4 * len(res) + 4) // 5 and any(r["steps"] >= min_steps for r in ok):
                found[case] = (cand, [min(r["margins"]) for r in res], [r["steps"] for r in res])
                break
    return found
