"""The three-term training loss of a model with the CTC and the transducer head, restated without a GPU:

    (1 - w_c - w_r) L_att + w_c sum(nll_ctc) / B + w_r sum(nll_rnnt) / B

Encoder and attention decoder are oracle/asr_oracle.py's on leaves of the dtype asked for (float64 is the reference, float32
the yardstick where a gate has to be derived), the CTC term is torch.nn.functional.ctc_loss on enc_h @ ctc_lo (blank = 0,
zero_infinity), the transducer term rnnt_ref.torch_head_nll; autograd gives every parameter's gradient.

A rank's loss under data parallelism (parallel.sup_local_loss) is the same three terms over the rank's rows of the strided
shard, the encoder padded to the GLOBAL T_max, the decoder run for the GLOBAL olength, every term divided by the GLOBAL batch
size (L_att by B_global x olength_global): `rows=` below.  The rank-local losses then sum to the full-batch one
(tests/test_heads_sharded_cpu.py holds that for this file before it judges the kernels).

The batch and the model of the sharded tests are made here, so that the CPU and the GPU file use the same ones."""
import numpy as np
import torch
import torch.nn.functional as F

import rnnt_ref as R
import synth
from oracle import asr_oracle as O

ILENS, YLENS = [11, 10, 9, 6, 5, 3], [4, 2, 3, 2, 3, 2]          # test_sharded_equals_full_batch_on_gpu's batch
WORLDS = (1, 2, 3, 4, 7)
WEIGHTS = dict(ctc_weight=0.2, rnnt_weight=0.5, rnnt_joint_dim=32)
BOS = 1


def batch(cfg=synth.TINY):
    """-> (xs [B, T, D] float32 numpy, ilens, ys: list of int64 numpy)."""
    return synth.batch(cfg["input_dim"], cfg["output_dim"], ILENS, YLENS, 13)


def labeldist(cfg=synth.TINY):
    return synth.labeldist(cfg["output_dim"], 12)


def tiny_net(cfg=synth.TINY, seed=21):
    """The model of the sharded tests on the CPU, in train mode: encoder and decoder from synth.e2e_weights(cfg, 11), the two
    heads as torch initialises them under `seed` (test_rnnt_gpu._tiny's order of calls)."""
    import model as M
    torch.manual_seed(seed)
    net = M.E2E(labeldist=labeldist(cfg), **cfg, **WEIGHTS)
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()}, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("ctc_lo.", "rnnt.")) for k in res.missing_keys)
    net.train()
    return net


def leaves(net, dtype=torch.float64):
    """{parameter name: a leaf of `dtype`} for every parameter of the model (named_parameters: each tensor once)."""
    return {n: p.detach().cpu().to(dtype).clone().requires_grad_() for n, p in net.named_parameters()}


def _oracle_state(p):
    sd = {k: v for k, v in p.items() if not k.startswith(("ctc_lo.", "rnnt."))}
    for k in list(sd):
        if k.startswith("attention."):                               # one tensor under both names
            sd["decoder." + k] = sd[k]
    return sd


def shard_rows(n, rank, world):
    """The rows of a length-sorted batch of n that rank `rank` of `world` owns (parallel.shard_indices, restated)."""
    return [i for i in range(n) if i % world == rank]


def loss(p, cfg, xs, ilens, ys, rows=None):
    """-> (loss, dict(att, ctc_nll [b], rnnt_nll [b], enc_lens, t_out)) of the rows `rows` of the batch (default: all of them)
    in the dtype of the leaves `p`; None for no rows.  xs numpy [B, T, D], ys a list of int arrays."""
    B = len(ilens)
    rows = list(range(B)) if rows is None else list(rows)
    if not rows:
        return None, None
    dtype = next(iter(p.values())).dtype
    t_max, olength = int(max(ilens)), max(len(y) for y in ys) + 1
    total = O.padded_lengths(t_max, cfg["enc_n_layers"], cfg["subsample"])
    x = torch.from_numpy(np.ascontiguousarray(xs[rows])).to(dtype)
    il, yl = [int(ilens[i]) for i in rows], [torch.as_tensor(np.asarray(ys[i]), dtype=torch.long) for i in rows]
    enc_h, enc_lens, (_, lp, _, _) = O.e2e_forward_with_encoder(
        _oracle_state(p), dict(cfg, labeldist=labeldist(cfg)), x, il, yl, tf_rate=1.0, total_length=total,
        olength_override=olength)
    assert lp.shape == (len(rows), olength) and enc_h.shape[1] == total[-1]
    att = -lp.sum() / (B * olength)
    logp = F.log_softmax(enc_h @ p["ctc_lo.weight"].t() + p["ctc_lo.bias"], -1).transpose(0, 1)
    ctc = F.ctc_loss(logp, torch.cat(yl), torch.tensor(enc_lens), torch.tensor([int(y.numel()) for y in yl]), blank=0,
                     reduction="none", zero_infinity=True)
    head = {k: p["rnnt." + k] for k in R.HEAD_KEYS}
    rnnt = R.torch_head_nll(head, enc_h, enc_lens, [y.tolist() for y in yl], BOS)
    wc, wr = WEIGHTS["ctc_weight"], WEIGHTS["rnnt_weight"]
    total_loss = (1.0 - wc - wr) * att + wc * (ctc.sum() / B) + wr * (rnnt.sum() / B)
    return total_loss, dict(att=att.detach(), ctc_nll=ctc.detach(), rnnt_nll=rnnt.detach(), enc_lens=enc_lens, t_out=total[-1])


def loss_and_grads(p, cfg, xs, ilens, ys, world=1):
    """The step over `world` ranks, one after another: -> (the sum of the rank-local losses, {name: the sum of the rank-local
    gradients}, the per-rank parts - None for an empty shard).  world = 1 is the full batch."""
    names = list(p)
    total, grads, parts = 0.0, {n: torch.zeros_like(p[n]) for n in names}, []
    for rank in range(world):
        l, part = loss(p, cfg, xs, ilens, ys, shard_rows(len(ilens), rank, world))
        parts.append(part)
        if l is None:
            continue
        for n, g in zip(names, torch.autograd.grad(l, [p[n] for n in names])):
            grads[n] += g
        total = total + l.detach()
    return total, grads, parts
