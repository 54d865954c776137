"""Restatements of the transducer head (csrc/rnnt.hip) that need no GPU.

    joint, joint_bwd, loss_and_grad    numpy, in the dtype asked for: float64 is the reference, float32 - the same recurrences
                                       in the same order - is the yardstick of the GPU tests' allowance
    brute_force_nll                    every alignment path enumerated
    torch_nll, torch_head_nll          differentiable torch float64: the loss alone, and the whole head (embedding, LSTM,
                                       the three products, tanh, loss) so that head and model gradients come from autograd
    greedy                             the greedy decoder (lower index on ties, max_symbols per frame, a length cap)
    decode_case                        the decode inputs of the GPU tests, made here so that the CPU test can hold their
                                       top-two logit margin

One utterance at a time: logits [T, U + 1, V] over the utterance's own lattice, labels [U] in [1, V), blank = 0."""
import itertools

import numpy as np
import torch


def _lse_rows(z, dt):
    mx = z.max(-1)
    return (mx + np.log(np.exp(z - mx[..., None]).sum(-1, dtype=dt), dtype=dt)).astype(dt)


def _lae(a, b, dt):
    m = a if a > b else b
    if m == -np.inf:
        return dt(-np.inf)
    return dt(m + np.log(np.exp(dt(a - m), dtype=dt) + np.exp(dt(b - m), dtype=dt), dtype=dt))


def joint(pe, pp, dt=np.float64):
    """pe [T, J], pp [U + 1, J] -> Z [T, U + 1, J]."""
    return np.tanh(pe.astype(dt)[:, None, :] + pp.astype(dt)[None, :, :], dtype=dt)


def joint_bwd(dz, z, dt=np.float64):
    """-> (dpe [T, J], dpp [U + 1, J]): dz (1 - z^2) summed over u, resp. t, in ascending order."""
    dz, z = dz.astype(dt), z.astype(dt)
    d = dz * (dt(1) - z * z)
    dpe, dpp = np.zeros(d.shape[::2], dt), np.zeros(d.shape[1:], dt)
    for u in range(d.shape[1]):
        dpe += d[:, u]
    for t in range(d.shape[0]):
        dpp += d[t]
    return dpe, dpp


def loss_and_grad(logits, labels, dt=np.float64, g=1.0):
    """-> (nll, dlogits [T, U + 1, V]) of one utterance; the analytic gradient of the header, times g."""
    z = np.asarray(logits).astype(dt)
    T, U1, V = z.shape
    U = U1 - 1
    labels = [int(v) for v in labels]
    assert len(labels) == U and all(1 <= v < V for v in labels) and T >= 1
    lse = _lse_rows(z, dt)
    lb = z[:, :, 0] - lse                                           # lp_blank(t, u)
    ly = np.full((T, U1), -np.inf, dt)                              # lp_{y_{u+1}}(t, u)
    for u in range(U):
        ly[:, u] = z[:, u, labels[u]] - lse[:, u]
    ninf = dt(-np.inf)
    alpha = np.full((T, U1), ninf, dt)
    for d in range(T + U):
        for u in range(max(0, d - (T - 1)), min(U, d) + 1):
            t = d - u
            if d == 0:
                alpha[t, u] = 0
                continue
            up = dt(alpha[t - 1, u] + lb[t - 1, u]) if t > 0 else ninf
            left = dt(alpha[t, u - 1] + ly[t, u - 1]) if u > 0 else ninf
            alpha[t, u] = _lae(up, left, dt)
    logp = dt(alpha[T - 1, U] + lb[T - 1, U])
    beta = np.full((T, U1), ninf, dt)
    for d in range(T - 1 + U, -1, -1):
        for u in range(max(0, d - (T - 1)), min(U, d) + 1):
            t = d - u
            if t == T - 1 and u == U:
                beta[t, u] = lb[t, u]
                continue
            down = dt(beta[t + 1, u] + lb[t, u]) if t < T - 1 else ninf
            right = dt(beta[t, u + 1] + ly[t, u]) if u < U else ninf
            beta[t, u] = _lae(down, right, dt)
    gamma = np.exp((alpha + beta) - logp, dtype=dt)
    dz = np.exp(z - lse[..., None], dtype=dt) * gamma[..., None]
    bnext = np.concatenate([beta[1:], np.full((1, U1), ninf, dt)], 0)       # beta(t + 1, u); beta(T, U) = 0
    bnext[T - 1, U] = 0
    dz[:, :, 0] -= np.exp(((alpha + lb) + bnext) - logp, dtype=dt)
    for u in range(U):
        dz[:, u, labels[u]] -= np.exp(((alpha[:, u] + ly[:, u]) + beta[:, u + 1]) - logp, dtype=dt)
    return dt(-logp), (dt(g) * dz).astype(dt)


def brute_force_nll(logits, labels):
    """-log of the sum over every alignment: T - 1 blanks and U labels in any order, then the closing blank."""
    z = np.asarray(logits, np.float64)
    T, U1, V = z.shape
    U = U1 - 1
    lp = z - _lse_rows(z, np.float64)[..., None]
    total = 0.0
    for where in itertools.combinations(range(T - 1 + U), U):       # the moves that emit a label
        t = u = 0
        s = 0.0
        for m in range(T - 1 + U):
            if m in where:
                s += lp[t, u, int(labels[u])]
                u += 1
            else:
                s += lp[t, u, 0]
                t += 1
        total += np.exp(s + lp[T - 1, U, 0])
    return -np.log(total)


def torch_nll(logits, labels):
    """Differentiable float64 loss of one utterance: logits [T, U + 1, V] (a torch double tensor)."""
    T, U1, _ = logits.shape
    U = U1 - 1
    lp = torch.log_softmax(logits, -1)
    alpha = {(0, 0): lp.new_zeros(())}
    for d in range(1, T + U):
        for u in range(max(0, d - (T - 1)), min(U, d) + 1):
            t = d - u
            terms = []
            if t > 0:
                terms.append(alpha[(t - 1, u)] + lp[t - 1, u, 0])
            if u > 0:
                terms.append(alpha[(t, u - 1)] + lp[t, u - 1, int(labels[u - 1])])
            alpha[(t, u)] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return -(alpha[(T - 1, U)] + lp[T - 1, U, 0])


HEAD_KEYS = ("embedding.weight", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
             "lin_enc.weight", "lin_enc.bias", "lin_pred.weight", "lin_out.weight", "lin_out.bias")


def _cell(p, tok, h, c, lib):
    """One LSTM step (torch's gate order i, f, g, o) on numpy arrays or torch tensors."""
    g = p["lstm.weight_ih_l0"] @ p["embedding.weight"][int(tok)] + p["lstm.bias_ih_l0"] + p["lstm.weight_hh_l0"] @ h + \
        p["lstm.bias_hh_l0"]
    H = h.shape[0]
    sig = (lambda x: 1 / (1 + lib.exp(-x)))
    i, f, gg, o = sig(g[:H]), sig(g[H:2 * H]), lib.tanh(g[2 * H:3 * H]), sig(g[3 * H:])
    c2 = f * c + i * gg
    return o * lib.tanh(c2), c2


def torch_head_nll(p, enc_h, frame_lens, ys, bos):
    """The whole head in differentiable float64: p the head's parameters (HEAD_KEYS, torch double), enc_h [B, T, H] ->
    nll [B]."""
    out = []
    for b, y in enumerate(ys):
        T, y = int(frame_lens[b]), [int(v) for v in y]
        h = c = enc_h.new_zeros(p["lstm.weight_hh_l0"].shape[1])
        hs = []
        for tok in [bos] + y:
            h, c = _cell(p, tok, h, c, torch)
            hs.append(h)
        pe = enc_h[b, :T] @ p["lin_enc.weight"].t() + p["lin_enc.bias"]
        pp = torch.stack(hs) @ p["lin_pred.weight"].t()
        z = torch.tanh(pe[:, None, :] + pp[None, :, :])
        out.append(torch_nll(z @ p["lin_out.weight"].t() + p["lin_out.bias"], y))
    return torch.stack(out)


def greedy(p, enc_h, bos, max_symbols, max_len, dt=np.float64):
    """Greedy decoding of one utterance: p the head's parameters (numpy), enc_h [T, H].  The argmax takes the lower index on
    ties; a frame emits at most max_symbols tokens, the utterance max_len.  -> dict(tokens, score: the sum of the tokens'
    log-probabilities, margin: the least top-two logit gap of any step, iterations: the iteration after which the row was
    done, hit_max / hit_cap: whether a frame ran into max_symbols / the utterance into max_len)."""
    p = {k: np.asarray(v).astype(dt) for k, v in p.items()}
    pe = np.asarray(enc_h).astype(dt) @ p["lin_enc.weight"].T + p["lin_enc.bias"]
    T = pe.shape[0]
    zero = np.zeros(p["lstm.weight_hh_l0"].shape[1], dt)
    h, c = _cell(p, bos, zero, zero, np)
    pp = p["lin_pred.weight"] @ h
    t = nf = 0
    toks, score, margin, done_at, hit_max = [], dt(0), np.inf, None, False
    for it in range(T + max_len):
        if t >= T or len(toks) >= max_len:
            done_at = it if done_at is None else done_at
            continue
        if nf >= max_symbols:
            t, nf, hit_max = t + 1, 0, True
            continue
        lg = p["lin_out.weight"] @ np.tanh(pe[t] + pp, dtype=dt) + p["lin_out.bias"]
        k = int(np.argmax(lg))
        top = np.sort(lg)
        margin = min(margin, float(top[-1] - top[-2]))
        if k == 0:
            t, nf = t + 1, 0
            continue
        toks.append(k)
        score = dt(score + (lg[k] - (lg.max() + np.log(np.exp(lg - lg.max()).sum(dtype=dt), dtype=dt))))
        nf += 1
        h, c = _cell(p, k, h, c, np)
        pp = p["lin_pred.weight"] @ h
    return dict(tokens=toks, score=float(score), margin=margin, iterations=done_at if done_at is not None else T + max_len,
                hit_max=hit_max, hit_cap=len(toks) >= max_len)


def head_params(V, E, P, H, J, seed, blank_bias=0.0, scale=1.0):
    """Seeded float32 parameters of a TransducerHead (HEAD_KEYS)."""
    rs = np.random.RandomState(seed)
    shapes = {"embedding.weight": (V, E), "lstm.weight_ih_l0": (4 * P, E), "lstm.weight_hh_l0": (4 * P, P),
              "lstm.bias_ih_l0": (4 * P,), "lstm.bias_hh_l0": (4 * P,), "lin_enc.weight": (J, H), "lin_enc.bias": (J,),
              "lin_pred.weight": (J, P), "lin_out.weight": (V, J), "lin_out.bias": (V,)}
    p = {k: (scale * rs.uniform(-1, 1, s)).astype(np.float32) for k, s in shapes.items()}
    p["lin_out.bias"][0] += np.float32(blank_bias)
    return p


DECODE_DIMS = dict(V=9, E=16, P=16, H=16, J=32)
# name -> (parameter seed, blank bias, frames per row, max_symbols, max_len)
DECODE_CASES = dict(
    mixed=(3, 1.0, (6, 4, 1, 3), 3, 8),          # rows of different lengths finish at different iterations; a row with T_b = 1
    eager=(5, -4.0, (5, 2, 1), 2, 5),            # the blank is unlikely: frames run into max_symbols, rows into the length cap
)


def decode_case(name):
    """-> (parameters, enc_h [B, T, H] float32 zero-padded, frame lengths, max_symbols, max_len)."""
    seed, blank_bias, lens, max_symbols, max_len = DECODE_CASES[name]
    d = DECODE_DIMS
    p = head_params(d["V"], d["E"], d["P"], d["H"], d["J"], seed, blank_bias)
    rs = np.random.RandomState(seed + 100)
    enc_h = np.zeros((len(lens), max(lens), d["H"]), np.float32)
    for b, n in enumerate(lens):
        enc_h[b, :n] = rs.uniform(-1, 1, (n, d["H"]))
    return p, enc_h, list(lens), max_symbols, max_len
