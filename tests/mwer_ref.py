"""The MWER loss of csrc/mwer.hip restated without the product: in float64 on torch with plain autograd (the checker), and in
float32 on numpy with the header's summation orders (the yardstick whose own error against float64 sizes the allowances of
tests/test_mwer_gpu.py).  Also the inputs of the kernel grid, the fixed hypotheses of the end-to-end tests, and the whole MWER
step of the tiny model on the CPU oracle in float64 (the learning rate of the descent test is chosen on it).  No GPU code.

Rows are r = b K + k; logits [L, R, V]; tokens [L, R]; npos [R] (<= 0: an unused slot); err [R]; see include/asr_hip.h."""
import numpy as np
import torch

U = 2.0 ** -24                 # unit roundoff of float32


def loss_f64(logits, tokens, npos, err, B, scale):
    """logits: a float64 [L, R, V] tensor (with or without requires_grad; positions the loss does not read may hold anything
    finite) -> dict(loss, risk [B], post [R], seq_logp [R], coef [R]); `loss` carries the graph."""
    L, R, V = logits.shape
    K = R // B
    tokens, npos = torch.as_tensor(tokens).long(), torch.as_tensor(npos).long()
    errf = torch.as_tensor(err).double().view(B, K)
    n = npos.clamp(min=0, max=L)
    lp = torch.log_softmax(logits, -1).gather(-1, tokens.unsqueeze(-1)).squeeze(-1)              # [L, R]
    mask = torch.arange(L).unsqueeze(1) < n.unsqueeze(0)
    s = torch.where(mask, lp, torch.zeros((), dtype=logits.dtype)).sum(0)
    live = (npos > 0).view(B, K)
    any_live = live.any(1, keepdim=True)
    s2 = s.view(B, K)
    m = torch.where(live, s2, torch.full_like(s2, -float("inf"))).max(1, keepdim=True).values.detach()
    m = torch.where(any_live, m, torch.zeros_like(m))
    e = torch.where(live, torch.exp(torch.where(live, s2, m) - m), torch.zeros_like(s2))
    z = e.sum(1, keepdim=True)
    post = e / torch.where(any_live, z, torch.ones_like(z))
    wbar = (errf * live).sum(1, keepdim=True) / live.sum(1, keepdim=True).clamp(min=1)
    d = torch.where(live, errf - wbar, torch.zeros_like(errf))
    risk = (post * d).sum(1)
    coef = post.detach() * (d - risk.detach().unsqueeze(1))
    return dict(loss=scale * risk.sum(), risk=risk.detach(), post=post.detach().reshape(R),
                seq_logp=torch.where(live.reshape(R), s.detach(), torch.zeros_like(s.detach())), coef=coef.reshape(R))


def run_f64(logits, tokens, npos, err, B, scale, g=1.0):
    """The float64 checker with its gradient: logits any float array [L, R, V] -> dict of float64 numpy arrays, `dlogits`
    (the gradient of g * loss) among them."""
    z = torch.as_tensor(np.asarray(logits, dtype=np.float64)).clone().requires_grad_()
    out = loss_f64(z, tokens, npos, err, B, scale)
    (out["loss"] * g).backward()
    res = {k: v.detach().numpy().astype(np.float64) for k, v in out.items()}
    res["dlogits"] = z.grad.numpy()
    return res


def run_f32(logits, tokens, npos, err, B, scale, g=1.0):
    """The same formulas in float32 arithmetic, every sum in the header's order (l, then k, then b ascending; the sum over V
    is numpy's) -> dict of float32 arrays, dlogits from the closed form."""
    f = np.float32
    z = np.asarray(logits, dtype=f)
    L, R, V = z.shape
    K = R // B
    tokens, npos, err = np.asarray(tokens), np.asarray(npos), np.asarray(err)
    n = np.clip(npos, 0, L)
    mx = z.max(-1, keepdims=True)
    ex = np.exp(z - mx, dtype=f)
    se = ex.sum(-1, keepdims=True, dtype=f)
    lse = (mx + np.log(se, dtype=f))[..., 0]
    soft = ex / se
    lp = np.take_along_axis(z, tokens[..., None], -1)[..., 0] - lse
    s = np.zeros(R, dtype=f)
    for l in range(L):
        s = np.where(l < n, (s + lp[l]).astype(f), s)
    post, coef, risk = np.zeros(R, dtype=f), np.zeros(R, dtype=f), np.zeros(B, dtype=f)
    for b in range(B):
        rows = [b * K + k for k in range(K) if npos[b * K + k] > 0]
        if not rows:
            continue
        m = max(s[r] for r in rows)
        wbar = f(f(sum(int(err[r]) for r in rows)) / f(len(rows)))
        zs = f(0)
        for r in rows:
            zs = f(zs + np.exp(f(s[r] - m), dtype=f))
        inv = f(f(1) / zs)
        rb = f(0)
        for r in rows:
            post[r] = f(np.exp(f(s[r] - m), dtype=f) * inv)
            rb = f(rb + f(post[r] * f(f(err[r]) - wbar)))
        for r in rows:
            coef[r] = f(post[r] * f(f(f(err[r]) - wbar) - rb))
        risk[b] = rb
    tot = f(0)
    for b in range(B):
        tot = f(tot + risk[b])
    onehot = np.zeros_like(z)
    np.put_along_axis(onehot, tokens[..., None], f(1), -1)
    gr = (f(g) * f(scale) * coef).astype(f)
    dz = (gr[None, :, None] * (onehot - soft)).astype(f)
    dz[np.arange(L)[:, None] >= n[None, :]] = 0
    return dict(loss=np.asarray(f(scale) * tot, dtype=f), risk=risk, post=post, seq_logp=s, coef=coef, dlogits=dz)


def allowance(ref64, own32):
    """The project's rule for one output tensor: max(4 x the float32 restatement's own error against
    float64 on the same input, 8 * 2^-24 x the tensor's largest magnitude)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    e32 = float(np.max(np.abs(np.asarray(own32, dtype=np.float64) - ref64))) if ref64.size else 0.0
    return max(4.0 * e32, 8.0 * U * float(np.max(np.abs(ref64))) if ref64.size else 0.0)


# ------------------------------------------------------------------------------------------------ the kernel grid
# (B, K, L, V, logits, npos, slots, errs): a dozen combinations of B in {1, 3}, K in {1, 2, 4, 16}, L in {1, 2, 9, 65},
# V in {3, 34, 65, 130} - both sides of the 64-lane boundary.
#   logits  normal: N(0, 1) * 3;  spread: uniform over +-80;  far: the sequence scores of an utterance lie far apart (a bias on
#           the hypothesis' own tokens that grows with k), so the posteriors of the later slots underflow to 0
#   npos    random: 1 .. L;  one: 1 everywhere (only <EOS>);  full: L everywhere
#   slots   all: every slot live;  holes: utterance 0 has an unused slot in the middle and at the end, utterance 1 (where there
#           is one) a single live slot, utterance 2 none
#   errs    random | equal (every hypothesis of an utterance as wrong as the others: dlogits is exactly 0)
GRID = [
    (1, 1, 1, 3, "normal", "random", "all", "random"),
    (3, 2, 2, 34, "normal", "random", "all", "random"),
    (3, 4, 9, 65, "normal", "random", "holes", "random"),
    (1, 16, 65, 130, "normal", "random", "all", "random"),
    (3, 16, 9, 3, "spread", "random", "holes", "random"),
    (3, 4, 65, 34, "far", "random", "all", "random"),
    (1, 2, 9, 130, "normal", "one", "all", "random"),
    (3, 4, 2, 65, "spread", "full", "all", "random"),
    (3, 4, 9, 34, "normal", "random", "all", "equal"),
    (3, 16, 2, 130, "spread", "random", "holes", "random"),
    (1, 4, 1, 65, "normal", "random", "holes", "random"),
    (3, 2, 65, 3, "normal", "full", "all", "random"),
    (3, 4, 65, 130, "spread", "random", "holes", "random"),
    (3, 1, 9, 34, "normal", "random", "all", "random"),
]


def case_id(c):
    return "B%d-K%d-L%d-V%d-%s-%s-%s-%s" % c


def make_case(c):
    """-> dict(B, K, L, V, logits fp32 [L, R, V], tokens int64 [L, R], npos int32 [R], err int32 [R], scale, g)."""
    B, K, L, V, kind, npos_kind, slots, errs = c
    R = B * K
    rs = np.random.RandomState(1000 * B + 100 * K + 10 * L + V + len(kind) + len(npos_kind))
    tokens = rs.randint(0, V, size=(L, R)).astype(np.int64)
    if kind == "spread":
        z = rs.uniform(-80, 80, size=(L, R, V))
    else:
        z = 3.0 * rs.normal(0, 1, size=(L, R, V))
    if kind == "far":
        bias = np.tile(-2.5 * np.arange(K), B)              # per position: slot k ends about 160 k below slot 0 at L = 65 -
                                                            # under float32's smallest number, far above float64's
        np.put_along_axis(z, tokens[..., None], np.take_along_axis(z, tokens[..., None], -1) + bias[None, :, None], -1)
    npos = {"random": rs.randint(1, L + 1, size=R), "one": np.ones(R, dtype=np.int64),
            "full": np.full(R, L)}[npos_kind].astype(np.int32)
    if kind == "far":
        npos[:] = L
    if slots == "holes":
        live = np.ones((B, K), dtype=bool)
        if K >= 3:
            live[0, 1] = False
        if K >= 2:
            live[0, K - 1] = False
        if B >= 2:
            live[1, :] = False
            live[1, min(1, K - 1)] = True
        if B >= 3:
            live[2, :] = False
        npos = np.where(live.reshape(R), npos, np.where(np.arange(R) % 2 == 0, 0, -1)).astype(np.int32)
    err = rs.randint(0, 12, size=R).astype(np.int32)
    if errs == "equal":
        err = np.repeat(rs.randint(0, 12, size=B), K).astype(np.int32)
    return dict(B=B, K=K, L=L, V=V, logits=z.astype(np.float32), tokens=tokens, npos=npos, err=err, scale=1.0 / B, g=0.7)


# ------------------------------------------------------------------------------------------------ the tiny model's step
def fixed_hyps(ys, K, V, eos, seed=5):
    """K hypotheses per utterance, made from the reference without any search: the reference itself, then copies with a
    substitution / a deletion / an insertion / a random sequence, in turn.  -> (tokens int64 [B, K, T] <EOS>-padded, lengths
    int32 [B, K]) as numpy arrays, T = the longest + 1."""
    rs = np.random.RandomState(seed)
    hyps = []
    for y in ys:
        y = [int(v) for v in y]
        row = [list(y)]
        for k in range(1, K):
            h = list(y)
            kind = k % 4
            pos = int(rs.randint(0, max(len(h), 1)))
            tok = int(rs.randint(3, V))
            if kind == 1 and h:
                h[pos] = tok if tok != h[pos] else 3 + (tok - 2) % (V - 3)
            elif kind == 2 and len(h) > 1:
                del h[pos]
            elif kind == 3:
                h.insert(pos, tok)
            else:
                h = [int(v) for v in rs.randint(3, V, size=max(1, len(y) - 1))]
            row.append(h)
        hyps.append(row)
    T = max(len(h) for row in hyps for h in row) + 1
    tokens = np.full((len(ys), K, T), eos, dtype=np.int64)
    lengths = np.zeros((len(ys), K), dtype=np.int32)
    for b, row in enumerate(hyps):
        for k, h in enumerate(row):
            tokens[b, k, :len(h)] = h
            lengths[b, k] = len(h)
    return tokens, lengths


def oracle_step_loss(O, sd, cfg, xs, ilens, ys, hyp_tokens, hyp_len, ce_weight, eos=2):
    """E2E.mwer_forward with given hypotheses on the CPU oracle `O` (oracle.asr_oracle), in the dtype of `sd` (dropout 0):
    encoder once, the teacher-forced decoder over the B K rows (no label smoothing), the risk loss, + ce_weight times the
    supervised loss -mean(log-probs).  -> (loss with the graph, mean risk as a float)."""
    B, K, T = hyp_tokens.shape
    R = B * K
    enc_h, enc_lens = O.encoder_forward(sd, xs, ilens, cfg["enc_n_layers"], cfg["subsample"], 0.0, True, None)
    rep = enc_h.unsqueeze(1).expand(B, K, enc_h.shape[1], enc_h.shape[2]).reshape(R, enc_h.shape[1], enc_h.shape[2])
    len_rep = [int(l) for l in enc_lens for _ in range(K)]
    rows = [torch.as_tensor(hyp_tokens[b, k, :int(hyp_len[b, k])]).long() for b in range(B) for k in range(K)]
    logits, _, _, _ = O.decoder_forward(sd, rep, len_rep, rows, label_smoothing=False, training=True,
                                        olength_override=T + 1)
    tok_out = O.pad_ragged([torch.cat([r, r.new_tensor([eos])]) for r in rows], eos)
    tok_out = torch.nn.functional.pad(tok_out, (0, T + 1 - tok_out.shape[1]), value=eos)
    err = np.array([O.levenshtein([int(v) for v in rows[b * K + k]], [int(v) for v in ys[b]]) for b in range(B) for k in range(K)])
    out = loss_f64(logits.transpose(0, 1), tok_out.t(), hyp_len.reshape(R) + 1, err, B, 1.0 / B)
    loss = out["loss"]
    if ce_weight > 0:
        _, lp, _, _ = O.decoder_forward(sd, enc_h, enc_lens, ys, training=True, ls_weight=cfg.get("ls_weight", 0.0),
                                        labeldist=cfg.get("labeldist"))
        loss = loss + ce_weight * (-lp.mean())
    return loss, float(out["risk"].mean())


DESCENT_LR = 2e-3              # ten clipped Adam steps at this rate lower the tiny model's mean risk on the float64 oracle
DESCENT_STEPS = 10
