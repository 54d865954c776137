"""Utterance-level data parallelism + the flat-buffer optimiser.

The reference has no distributed code; this is the new component the north star
asks for: one process per GPU, the global minibatch sharded by utterance, ONE all-reduce (RCCL over
xGMI; backend "nccl" on ROCm) of a single flat fp32 gradient buffer per step, issued after backward
and before the clip, then an identical fused clip+Adam step on every rank.

Exact-parity rules under sharding are host-side only:
  * strided shard (rank r gets global rows r, r+W, ...) keeps every shard length-sorted;
  * every shard is padded to the GLOBAL T_max and decodes the GLOBAL olength (the unmasked softmax
    and unmasked mean make results depend on both);
  * local loss = -sum_local(log_probs) / (B_global * olength_global), so the all-reduced SUM of
    gradients equals the single-process gradient;
  * every rank consumes the numpy RNG identically (teacher-forcing draws; input noise is drawn for
    the global batch), seeded once by the Solver.
The three step kinds of the reference share these rules (`sup_local_loss`, `ssl_local_loss`,
`judge_local_loss` below; solver.py:375-378, 460-483, 288-291).  The semi-supervised loss
-sum(p_LM * log p * mask) / sum(mask) is normalised by the GLOBAL hypothesis-token count, which only exists on
the devices after the free-running decode: it is summed over ranks by ONE 4-byte all-reduce, issued asynchronously
right after the unlabeled decode and waited for after the labeled forward pass (it overlaps the judge and that
pass); the gradient exchange itself stays the single flat-buffer all-reduce.  Scalars for logging ride in four
spare floats at the end of that buffer (`FlatBuffers.aux`).
"""
import ctypes
import math

import os

import numpy as np
import torch
import torch.distributed as dist


# ------------------------------------------------------------------------------ sharding (host)
def shard_indices(n, rank, world):
    """Strided assignment: rows rank, rank+world, ... of a length-sorted global batch."""
    return list(range(rank, n, world))


_SHARD_INDEX = {}


def _shard_index_tensor(n, rank, world, device):
    """The strided row indices as a tensor on `device`, built once per (batch size, rank, world): indexing with a Python
    list uploads a fresh index tensor from pageable memory every step."""
    key = (n, rank, world, str(device))
    if key not in _SHARD_INDEX:
        _SHARD_INDEX[key] = torch.arange(rank, max(n, rank), world, device=device)      # empty for rank >= n
    return _SHARD_INDEX[key]


class LocalShard(object):
    """This rank's rows of a global batch together with the global constants the exact-parity rules need - what
    shard_batch() returns, made by the input pipeline (feed.DeviceFeed) instead of on the device: under data parallelism
    a rank then pads and uploads ITS rows only.  Accepted wherever a step takes the global batch tensor.
      xs     [b_local, T_max_global, D] (None for a text batch), ilens / ys: this rank's rows (lists; ys None for speech)
      info   b_global, t_max (global padded length), olength (global max label length + 1), text_norm (global sum of
             len + 5: the judge's normaliser)"""
    __slots__ = ("xs", "ilens", "ys", "info")

    def __init__(self, xs, ilens, ys, info):
        self.xs, self.ilens, self.ys, self.info = xs, ilens, ys, info

    @property
    def device(self):
        t = self.xs if self.xs is not None else (self.ys[0] if self.ys else None)
        return t.device if t is not None else None


def shard_batch(xs, ilens, ys, rank, world):
    """(xs [B,T,D] zero-padded to the global T_max, ilens desc, ys list) -> this rank's rows.
    xs keeps the global padded length; returns (xs_r, ilens_r, ys_r, info) where info carries the
    global constants every rank needs (B_global, T_max, olength).  A LocalShard passes through."""
    if isinstance(xs, LocalShard):
        return xs.xs, list(xs.ilens), xs.ys, xs.info
    info = dict(b_global=len(ilens), t_max=int(max(ilens)),
                olength=(max(int(y.shape[0]) for y in ys) + 1) if ys is not None else None)
    if world == 1:
        return xs, list(ilens), ys, info
    idx = shard_indices(len(ilens), rank, world)
    xs_r = xs[_shard_index_tensor(len(ilens), rank, world, xs.device)] if torch.is_tensor(xs) else xs[idx]
    return xs_r, [ilens[i] for i in idx], ([ys[i] for i in idx] if ys is not None else None), info


def local_loss(log_probs, info):
    """-sum over this shard / (B_global * olength_global)  (solver.py:377 is the W=1 case).  The product's decoder hands the
    sum along with the log-probabilities (`fused_sum`, accumulated by the kernel that made them): one multiply is left."""
    want = -1.0 / float(info["b_global"] * log_probs.shape[1])
    loss = getattr(log_probs, "fused_loss", None)
    if loss is not None:                     # the kernel scaled its sum already (Decoder.forward, loss_norm)
        have = log_probs.fused_loss_scale
        return joint_loss(loss if abs(have - want) <= 1e-12 * abs(want) else loss * (want / have), log_probs, info)
    total = getattr(log_probs, "fused_sum", None)
    if total is None:
        total = log_probs.sum()
    return joint_loss(total * want, log_probs, info)


def joint_loss(att, log_probs, info):
    """(1 - w) L_att + w L_ctc when the forward carried a CTC term along (E2E(ctc_weight > 0) sets, on its log-probs,
    ctc_loss = this shard's sum of per-utterance CTC nll / ctc_norm, ctc_norm = the number of utterances it divided by, and
    ctc_weight = w); the attention loss alone otherwise.  L_ctc is normalised per utterance by the GLOBAL batch size, like
    L_att, so the rank-local joint losses sum to the single-process one."""
    ctc = getattr(log_probs, "ctc_loss", None)
    rnnt = getattr(log_probs, "rnnt_loss", None)
    if ctc is None and rnnt is None:
        return att
    w, want = 0.0, float(info["b_global"])
    if ctc is not None:
        w, have = float(log_probs.ctc_weight), float(log_probs.ctc_norm)
        if have != want:
            ctc = ctc * (have / want)
    if rnnt is None:
        return (1.0 - w) * att + w * ctc
    # the transducer term (E2E(rnnt_weight > 0)) rides the same way: (1 - w_ctc - w_rnnt) L_att + w_ctc L_ctc +
    # w_rnnt L_rnnt, L_rnnt normalised per utterance by the global batch size
    wr, have = float(log_probs.rnnt_weight), float(log_probs.rnnt_norm)
    if have != want:
        rnnt = rnnt * (have / want)
    loss = (1.0 - w - wr) * att + wr * rnnt
    return loss if ctc is None else loss + w * ctc


_ONE = {}


def backward(loss):
    """loss.backward() without the fill launch of its seed: a device scalar's d(loss)/d(loss) = 1 is a cached tensor."""
    if loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32:
        one = _ONE.get(loss.device)
        if one is None:
            one = _ONE[loss.device] = torch.ones((), device=loss.device, dtype=torch.float32)
        loss.backward(gradient=one)
    else:
        loss.backward()


def world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def padded_lengths(t_max, n_layers, subsample):
    """Padded time extent entering each encoder layer (+ the output extent); model.padded_lengths without the
    kernel imports."""
    out = [int(t_max)]
    for i in range(n_layers):
        out.append((out[-1] + 1) // 2 if subsample[i] > 1 else out[-1])
    return out


def global_sum_async(t, group=None):
    """In-place SUM of a small tensor over the ranks; returns a handle with .wait() (None in a single process)."""
    if world() <= 1:
        return None
    return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True)


def skip_decoder_draws(steps):
    """A rank whose shard is empty still consumes the teacher-forcing draws of the step (model.py:328: one per decoder
    step), so that every rank's numpy stream stays aligned."""
    for _ in range(int(steps)):
        np.random.random_sample()


def sup_local_loss(model_fwd, xs, ilens, ys, tf_rate, rank, world_size, n_layers, subsample):
    """Supervised step (solver.py:375-378) on this rank's shard -> local loss (None for an empty shard)."""
    xs_r, il_r, ys_r, info = shard_batch(xs, ilens, ys, rank, world_size)
    if not il_r:
        skip_decoder_draws(info["olength"])
        return None
    extra = dict(loss_norm=info["b_global"]) if getattr(model_fwd, "accepts_loss_norm", False) else {}
    _, log_probs, _, _ = model_fwd(xs_r, il_r, ys_r, tf_rate=tf_rate, sample=False,
                                   total_length=padded_lengths(info["t_max"], n_layers, subsample),
                                   olength=info["olength"], **extra)
    return local_loss(log_probs, info)


def ssl_local_loss(model_fwd, judge_probs, lab, unlab, rank, world_size, eos, unsup_weight, proportion, smooth,
                   scaling, n_layers, subsample, group=None):
    """Generator step of the semi-supervised training (solver.py:460-483) on this rank's shards of the labeled and
    the unlabeled global batch.  model_fwd has E2E.forward's signature (+ total_length / olength), judge_probs maps
    a hypothesis [b, L] (int64) to the judge's per-token probabilities [b, L] (no gradient flows through it: the
    hypothesis is discrete).  Returns (local loss or None, (unsup_local, sup_local)); the three SUM over ranks to
    the single-process values, and the all-reduced gradient of the local losses is the single-process gradient."""
    lab_xs, lab_ilens, lab_ys = lab
    unlab_xs, unlab_ilens = unlab
    u_xs, u_il, _, u_info = shard_batch(unlab_xs, unlab_ilens, None, rank, world_size)
    t_pad = u_info["t_max"] if isinstance(unlab_xs, LocalShard) else unlab_xs.shape[1]
    steps = int(t_pad * proportion)                       # global padded length (solver.py:467)
    dev = unlab_xs.device if (torch.is_tensor(unlab_xs) or isinstance(unlab_xs, LocalShard)) else None
    count = torch.zeros(1, dtype=torch.float32, device=dev)
    num = None
    if u_il:
        _, u_lp, u_pred, _ = model_fwd(u_xs, u_il, ys=None, sample=False, label_smoothing=False,
                                       max_dec_timesteps=steps, smooth=smooth, scaling=scaling,
                                       total_length=padded_lengths(u_info["t_max"], n_layers, subsample))
        mask = (u_pred != eos).float()
        count += mask.sum()
    # 4 bytes.  Awaited on the spot (a stream-level wait): an RCCL kernel left resident while the persistent kernels of
    # the judge and the labeled pass are being placed would, with a late rank, hold their workgroups back
    work = global_sum_async(count, group)
    if work is not None:
        work.wait()
    if u_il:
        num = -torch.sum(judge_probs(u_pred) * u_lp * mask)
    sup = sup_local_loss(model_fwd, lab_xs, lab_ilens, lab_ys, 1.0, rank, world_size, n_layers, subsample)
    unsup = num / count[0] if num is not None else None   # 0/0 = nan for an all-<EOS> hypothesis, like the reference
    parts = [p for p in (sup, unsup_weight * unsup if unsup is not None else None) if p is not None]
    loss = sum(parts[1:], parts[0]) if parts else None
    return loss, (unsup, sup)


def judge_local_loss(judge_fwd, masked_sum, ys, rank, world_size):
    """Judge (LM) step (solver.py:288-291): NLL normalised by the GLOBAL sum of (len + 5), known on the host.
    -> (local loss, local avg_prob) or (None, None) for an empty shard.  ys: the global text batch, or this rank's
    LocalShard of it."""
    if isinstance(ys, LocalShard):
        ys_r, total = ys.ys, ys.info["text_norm"]
    else:
        ys_r = [ys[i] for i in shard_indices(len(ys), rank, world_size)]
        total = float(sum(int(y.shape[0]) + 5 for y in ys))
    if not ys_r:
        return None, None
    frac = float(sum(int(y.shape[0]) + 5 for y in ys_r)) / total
    log_probs, probs, _ = judge_fwd(ys_r)
    return -masked_sum(log_probs, ys_r) * frac, masked_sum(probs, ys_r) * frac


def dp_step(make_loss, opt, n_aux, latch, leave_fast_path):
    """One data-parallel optimiser step, resolved at once: DpPipeline.step + resolve - the same code path as the pipelined
    default, with the host read right behind the step (config `pipeline_steps: 0`, and what the tests of the coordinated
    fallback call).  Returns the first n_aux scalars summed over the ranks; raises if the repeat after an abort fails too."""
    pipe = DpPipeline(1, latch, leave_fast_path)
    rec = pipe.step(make_loss, opt, n_aux)
    pipe.resolve(rec)
    return rec["values"]


def _repeat_step(make_loss, opt, n_aux, latch):
    """A step that DpPipeline._recover runs again off the fast path: the host reads the reduced latch BETWEEN the all-reduce
    and the update (the decision is identical on every rank, so the collectives stay matched) and raises if it is still set -
    nothing was applied then."""
    flag_slot = opt.buf.NAUX - 1
    loss, scalars = make_loss()
    opt.zero_grad()
    if loss is not None:
        backward(loss)
    aux = [v if v is not None else 0.0 for v in scalars[:n_aux]] + [0.0] * (flag_slot - n_aux)
    aux.append(latch())
    opt.buf.set_aux(aux)
    opt.reduce()
    values = opt.buf.aux.tolist()
    if values[flag_slot] != 0.0:
        raise RuntimeError("the abort latch is still set on %d rank(s) after a data-parallel step was repeated off the "
                           "persistent kernels; nothing was applied" % int(values[flag_slot]))
    opt.apply()
    return values[:n_aux]


class DpPipeline(object):
    """THE data-parallel optimiser step (Solver._step under data parallelism; no kernel code in here, so the gloo tests run it
    on CPU), with NO host wait inside the step: reading the reduced abort latch on the host between the all-reduce and the
    update would idle the GPU for a host round trip plus the launch of the update, every step.
    make_loss() -> (local loss or None for an empty shard, [scalars]); opt: zero_grad() / buf (FlatBuffers) / reduce() /
    apply(skip_if) / unapply().  The update is enqueued behind the all-reduce at once, PREDICATED ON THE DEVICE on the reduced latch (the
    last aux slot of the flat buffer: opt.apply(skip_if=...); the sum is the same word on every rank, so all ranks skip or
    none does), the reduced aux slots travel to the host asynchronously (stage), and the host looks at step i while step
    i + 1 .. i + depth run.  A rank's latch is sticky until leave_fast_path() clears it, so every step enqueued behind an
    aborted one carries a non-zero sum too and was skipped as well; the first record found set makes EVERY rank (the
    values are identical) take the step counts back, restore the numpy stream that step started with, leave the fast
    path and run the skipped steps again (_repeat_step: host read before the update), in order.  Every rank has to resolve records at the same points
    of its program (the Solver's loops do: they run the same code on all ranks) - the replay is a sequence of collectives.
      latch()              -> this rank's abort latch (0 = clean), float or 0-d tensor
      leave_fast_path(n)   -> switch to the fallback path AND clear the latch (n = ranks that reported an abort)
      stage(aux)           -> (host tensor, wait): start copying the reduced aux slots to the host; wait() blocks until
                              they have landed.  Default: a clone (CPU tensors)."""

    def __init__(self, depth, latch, leave_fast_path, stage=None):
        self.depth, self.latch, self.leave = max(1, int(depth)), latch, leave_fast_path
        self.stage = stage if stage is not None else (lambda aux: (aux.clone(), lambda: None))
        self.pending = []

    def step(self, make_loss, opt, n_aux):
        """Enqueue one step; -> its record (rec["values"]: the first n_aux scalars summed over ranks once resolve(rec) /
        flush() has run, None before)."""
        flag_slot = opt.buf.NAUX - 1
        assert n_aux <= flag_slot
        rec = dict(make_loss=make_loss, opt=opt, n=n_aux, rng=np.random.get_state(), values=None, resolve=self.resolve)
        loss, scalars = make_loss()
        opt.zero_grad()
        if loss is not None:
            backward(loss)
        aux = [v if v is not None else 0.0 for v in scalars[:n_aux]] + [0.0] * (flag_slot - n_aux)
        aux.append(self.latch())
        opt.buf.set_aux(aux)
        opt.reduce()
        rec["host"], rec["wait"] = self.stage(opt.buf.aux)
        opt.apply(skip_if=opt.buf.aux[flag_slot:flag_slot + 1])      # a no-op on the device if any rank's latch was set
        self.pending.append(rec)
        while len(self.pending) > self.depth:
            self.resolve(self.pending[0])
        return rec

    def resolve(self, rec):
        """Read the host records of every outstanding step up to and including `rec` (oldest first)."""
        while self.pending and rec["values"] is None:
            first = self.pending[0]
            first["wait"]()
            vals = first["host"].tolist()
            if vals[-1] != 0.0:
                self._recover(int(vals[-1]))
            else:
                first["values"] = vals[:first["n"]]
                first["make_loss"] = first["opt"] = None
                self.pending.pop(0)

    def flush(self):
        while self.pending:
            self.resolve(self.pending[-1])

    def _recover(self, n_ranks):
        redo, self.pending = self.pending, []
        for r in redo:
            r["opt"].unapply()
        resume = np.random.get_state()
        self.leave(n_ranks)

        for r in redo:
            np.random.set_state(r["rng"])                # every step again from the stream state it started with
            r["values"] = _repeat_step(r["make_loss"], r["opt"], r["n"], self.latch)
            r["make_loss"] = r["opt"] = None
        np.random.set_state(resume)                      # draws per step do not depend on the poisoned values


# ------------------------------------------------------------------------------ flat buffers
class FlatBuffers(object):
    """Re-home every parameter (and its .grad) of a module into two flat fp32 buffers so that the
    gradient exchange is one collective and the optimiser one kernel.  Shared parameters (the
    attention module appears twice in E2E) are stored once.  Offsets are padded to 4
    floats so each view stays 16-byte aligned for the kernels."""

    NAUX = 4
    BUCKET_FLOATS = 4 << 20          # 16 MB of gradients per overlapped all-reduce
    _overlapping = 0                 # buffers with enable_overlap on, process-wide (the side stream is off while any is)
    _side_before = True              # ops._SIDE.enabled when the first of them began to overlap

    def __init__(self, params):
        self.params = []
        seen = set()
        for p in params:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                self.params.append(p)
        self.offsets = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.total = off
        dev = self.params[0].device
        self.flat_p = torch.zeros(off, device=dev, dtype=torch.float32)
        # NAUX spare floats behind the gradients travel in the same all-reduce (per-rank partial losses -> global values)
        self.flat_g = torch.zeros(off + self.NAUX, device=dev, dtype=torch.float32)
        self.aux = self.flat_g[off:]
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.flat_p[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat_p[o:o + n].view_as(p.data)
            p.grad = self.flat_g[o:o + n].view_as(p.data)
        # Overlapped gradient exchange (enable_overlap): the flat buffer is cut into contiguous buckets counted from its END
        # - autograd finishes the decoder's gradients first and encoder layer 0's last, module order is the reverse - and a
        # bucket's all-reduce is issued from a post-accumulate hook as soon as its last gradient exists, while the backward
        # of the layers below is still running.  Buckets are ISSUED IN A FIXED ORDER (0, 1, ...) whatever order they become
        # ready in, and a rank without a backward (empty shard) issues the same sequence in reduce(): the collectives match
        # across ranks by construction.
        self.buckets = []            # (first param index, end param index, lo, hi) in issue order
        hi_i, acc = len(self.params), 0
        for i in range(len(self.params) - 1, -1, -1):
            acc += self.params[i].numel()
            if acc >= self.BUCKET_FLOATS or i == 0:
                lo = self.offsets[i]
                hi = self.offsets[hi_i] if hi_i < len(self.params) else self.total
                self.buckets.append((i, hi_i, lo, hi))
                hi_i, acc = i, 0
        self.bucket_of = [0] * len(self.params)
        for b, (i0, i1, _, _) in enumerate(self.buckets):
            for i in range(i0, i1):
                self.bucket_of[i] = b
        self.overlap = False
        self._group = None
        self._hooks = []
        self._reset_overlap_state()

    # ---- overlapped exchange
    def _reset_overlap_state(self):
        self._pending = [i1 - i0 for (i0, i1, _, _) in self.buckets]
        self._ready = [False] * len(self.buckets)
        self._issued = 0
        self._started = False          # a gradient hook of this step has fired (its backward pass began)
        self._works = []

    def enable_overlap(self, group=None, force=False):
        """Issue each bucket's all-reduce from inside the backward pass (one backward per step; see __init__).  No-op in a
        single process (force: also with a process group of one rank - the RCCL rehearsal a one-GPU box allows)."""
        if self.overlap or not (dist.is_available() and dist.is_initialized()) or (world() <= 1 and not force):
            return
        self.overlap, self._group = True, group
        import ops
        # the hooks below read a gradient the moment autograd has it: no products in flight while ANY buffer overlaps
        if FlatBuffers._overlapping == 0:
            FlatBuffers._side_before = ops._SIDE.enabled
        FlatBuffers._overlapping += 1
        ops._SIDE.enabled = False
        for i, p in enumerate(self.params):
            self._hooks.append(p.register_post_accumulate_grad_hook(lambda q, i=i: self._on_grad(i)))

    def disable_overlap(self):
        """Back to ONE collective after the backward pass (removes the hooks; outstanding collectives are awaited, and a
        step abandoned between two buckets issues the rest of the fixed sequence first, as zero_grad does).  The side
        stream comes back on with the last overlapping buffer (the generator's and the judge's both overlap under
        dp_overlap)."""
        if not self.overlap:
            return
        if self._started and self._issued < len(self.buckets):
            self._issue_ready(force=True)
        for w in self._works:
            w.wait()
        for h in self._hooks:
            h.remove()
        self._hooks, self.overlap = [], False
        self._reset_overlap_state()
        FlatBuffers._overlapping -= 1
        if FlatBuffers._overlapping == 0:
            import ops
            ops._SIDE.enabled = FlatBuffers._side_before

    def _on_grad(self, i):
        b = self.bucket_of[i]
        self._started = True
        self._pending[b] -= 1
        if self._pending[b] < 0:
            raise RuntimeError("FlatBuffers overlap: a second backward pass reached a gradient of this step (one backward "
                               "per zero_grad() with enable_overlap)")
        if self._pending[b] == 0:
            self._ready[b] = True
            self._issue_ready()

    def _issue_ready(self, force=False):
        """Issue buckets in index order as far as they are ready (force: all that are left)."""
        while self._issued < len(self.buckets) and (force or self._ready[self._issued]):
            i0, i1, lo, hi = self.buckets[self._issued]
            dst, src, missing = [], [], False
            for i in range(i0, i1):
                p, v = self.params[i], self._view(i)
                if p.grad is None:
                    missing = True
                elif p.grad.data_ptr() != v.data_ptr():
                    dst.append(v)
                    src.append(p.grad)
            if missing:                                   # a parameter without a gradient this step: its slice is zero
                for i in range(i0, i1):
                    if self.params[i].grad is None:
                        self._view(i).zero_()
            if dst:
                torch._foreach_copy_(dst, src)
            for i in range(i0, i1):
                self.params[i].grad = self._view(i)
            self._works.append(dist.all_reduce(self.flat_g[lo:hi], op=dist.ReduceOp.SUM, group=self._group, async_op=True))
            self._issued += 1

    def zero_grad(self):
        """Detach every .grad: autograd then stores each gradient by reference instead of launching one add kernel per
        parameter into the flat buffer; collect() gathers them with a single multi-tensor copy before the step."""
        if self.overlap:
            # a step that was abandoned after (part of) its backward: ranks may have stopped at different buckets - one
            # of them possibly before its first bucket was complete - so every rank whose backward had BEGUN issues the
            # rest of the fixed sequence before waiting: the collectives stay matched
            if self._started and self._issued < len(self.buckets):
                self._issue_ready(force=True)
            for w in self._works:
                w.wait()
            self._reset_overlap_state()
        for p in self.params:
            p.grad = None

    def _view(self, i):
        """Parameter i's slice of the flat gradient buffer, shaped like the parameter (built once: 100 lookups per step)."""
        views = self.__dict__.get("_views")
        if views is None:
            views = self._views = [self.flat_g[o:o + p.numel()].view_as(p.data) for p, o in zip(self.params, self.offsets)]
        return views[i]

    def collect(self, sumsq=None):
        """Move the gradients autograd produced into the flat buffer and re-attach .grad to its views.
        sumsq (a zeroed 1-element device tensor, one-process steps): the sum of squares of ALL gradients is added to it on the
        way (asr_gather_sumsq_f32: the gather and the norm of clip_grad_norm_ in one pass); returns True if it was - False
        (the caller takes the norm over the flat buffer) when a gradient is already in place or not contiguous, when there is
        nothing to gather, or when the buffers are not on a GPU.  A MISSING gradient does not prevent the fused norm: its slice
        of the flat buffer is zeroed first and adds nothing to the sum."""
        dst, src, offs, missing, in_place = [], [], [], False, False
        for i, p in enumerate(self.params):
            v = self._view(i)
            if p.grad is None:
                missing = True
            elif p.grad.data_ptr() != v.data_ptr():
                dst.append(v)
                src.append(p.grad)
                offs.append(self.offsets[i])
            else:
                in_place = True
        if missing:
            self.flat_g[:self.total].zero_()
        fused = False
        if dst:
            if (self.flat_g.is_cuda and all(g.is_cuda and g.is_contiguous() and g.dtype == torch.float32 for g in src)):
                import hip_backend as hb
                fused = sumsq is not None and not in_place
                hb.gather_sumsq(src, offs, self.flat_g, sumsq if fused else None)
            else:
                torch._foreach_copy_(dst, src)
        for i, p in enumerate(self.params):
            p.grad = self._view(i)
        return fused

    def set_aux(self, values):
        """Scalars (tensors or floats, at most NAUX) that should come out of the step's all-reduce summed over ranks.
        Nothing here moves host memory to the device (a pageable copy would make the host wait for the stream - the wait the
        pipelined data-parallel step exists to avoid): device tensors are copied on the device, host values are kernel
        arguments of a fill."""
        self.aux.zero_()
        on_dev, where = [], []
        for i, v in enumerate(values):
            if torch.is_tensor(v) and v.device == self.aux.device:
                on_dev.append(v.detach().reshape(()).float())
                where.append(i)
            elif float(v) != 0.0:
                self.aux[i].fill_(float(v))
        if on_dev:
            if where == list(range(where[0], where[0] + len(where))):
                self.aux[where[0]:where[0] + len(where)].copy_(torch.stack(on_dev))
            else:
                for i, v in zip(where, on_dev):
                    self.aux[i].copy_(v)

    def allreduce_grads(self, group=None, sumsq=None):
        """The gradient exchange of the step.  Default: ONE SUM all-reduce over the flat gradient buffer (+ aux scalars).
        With enable_overlap(): the buckets not yet issued from the backward pass are issued now (same fixed order on every
        rank), all are awaited, and the aux scalars travel in a 16-byte collective of their own."""
        if self.overlap:
            self._issue_ready(force=True)
            for w in self._works:
                w.wait()
            self._works = []
            dist.all_reduce(self.aux, op=dist.ReduceOp.SUM, group=self._group)
            return False
        exchange = world() > 1 or (FORCE_DP and dist.is_initialized())
        # (one process: the norm the clip needs is the norm of what is being gathered - taken in the same pass)
        fused = self.collect(None if exchange else sumsq)
        if exchange:
            dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=group)
        return fused


# ------------------------------------------------------------------------------ optimiser
class FlatAdam(object):
    """clip_grad_norm_ + Adam(amsgrad, L2 weight decay) (solver.py:152-153,384-385) fused into two
    HIP kernels over the flat buffers (asr_sumsq_f32, asr_adam_clip_f32); no host sync in step().
    state_dict()/load_state_dict() use torch.optim.Adam's schema so `.opt` checkpoints interchange."""

    def __init__(self, module_or_params, lr, weight_decay=0.0, amsgrad=False, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, overlap=None):
        """overlap: issue the gradient all-reduce in buckets from inside the backward pass (FlatBuffers.enable_overlap).
        OPT-IN: None = only when ASR_DP_OVERLAP=1 is set.  The default exchange - of bench.py, the tools and the Solver
        alike - is ONE all-reduce of the flat buffer after the backward pass (north_star), until a multi-GPU run has shown
        that RCCL kernels resident beside the persistent kernels leave the abort latch clear and the overlap gains."""
        params = module_or_params.parameters() if hasattr(module_or_params, "parameters") else module_or_params
        self.buf = FlatBuffers(list(params))
        import os
        if overlap is None:
            overlap = os.environ.get("ASR_DP_OVERLAP", "0") == "1"
        if overlap:
            self.buf.enable_overlap(force=overlap == "force")
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                  params=list(range(len(self.buf.params))))]
        self.max_grad_norm = max_grad_norm
        dev = self.buf.flat_p.device
        self.m = torch.zeros_like(self.buf.flat_p)
        self.v = torch.zeros_like(self.buf.flat_p)
        self.vmax = torch.zeros_like(self.buf.flat_p) if amsgrad else None
        # ||g||^2 of a step: two words used in turn - the update kernel of one step zeroes the word the next step's norm
        # accumulates into (no fill launch per step)
        self.gnorm_pair = torch.zeros(2, device=dev, dtype=torch.float32)
        self.gnorm_sq = self.gnorm_pair[0:1]
        self._applies = 0
        self._norm_taken = False
        self.t = 0

    def zero_grad(self):
        self.buf.zero_grad()

    def reduce(self, group=None):
        """First half of a step: gather the gradients into the flat buffer and (if distributed) all-reduce it together
        with the aux scalars behind it.  A caller that has to look at the reduced aux values before committing to the
        update (Solver._dp_step: the abort flag of the persistent kernels) calls reduce(), reads, then apply()."""
        if self._norm_taken:                         # a reduce() whose apply() never came: its word holds a stale norm and
            self.gnorm_pair.zero_()                  # the other one was not cleared for this step
            self._norm_taken = False
        word = None
        if self.max_grad_norm is not None and self.buf.flat_g.is_cuda:
            word = self._norm_word()
        # one process: ||g||^2 is taken in the pass that gathers the gradients (FlatBuffers.collect)
        self._norm_taken = bool(self.buf.allreduce_grads(group, sumsq=word))
        if word is not None and not self._norm_taken:
            self._applies -= 1                       # (the word was not used: apply() takes it again)

    def _norm_word(self):
        """The accumulator of this step's ||g||^2: the two words of gnorm_pair in turn (apply() has the update kernel clear
        the other one for the next step)."""
        k = self._applies & 1
        self._applies += 1
        self.gnorm_sq = self.gnorm_pair[k:k + 1]
        return self.gnorm_sq

    def apply(self, max_grad_norm=None, skip_if=None):
        """Second half: global grad norm -> clip + Adam on the (reduced) flat buffer.  Returns the device scalar holding
        ||g||^2 (read it with .item() only if you need the number, and before the NEXT apply() has run on the device).  skip_if: a 1-element device tensor (4 bytes); if it is
        not zero when the kernel runs the update is a no-op on the device - the caller that finds it set later takes the
        step count back with unapply()."""
        import hip_backend as hb
        clip = self.max_grad_norm if max_grad_norm is None else max_grad_norm
        g = self.param_groups[0]
        self.t += 1
        # the kernel takes the betas as floats and forms 1 - beta from them: the bias corrections are those of the values it
        # multiplies by (from the decimal beta2 = 0.999, 1 - beta2^t is 1.3e-5 off the kernel's own 1 - float(beta2) at small t,
        # a step scaled by 1 + 6e-6 - tests/test_stream_kernels_gpu.py)
        b1, b2 = (ctypes.c_float(b).value for b in g["betas"])
        lib = hb.load()
        n = self.buf.total
        gptr = nxt = None
        if clip is not None:
            if not self._norm_taken:                 # (else reduce() took the norm with the gather)
                self._norm_word()
                hb.sumsq(self.buf.flat_g[:n], self.gnorm_sq)      # (asr_sumsq_det_f32 in deterministic mode)
            self._norm_taken = False
            k = (self._applies - 1) & 1
            nxt = hb.ptr(self.gnorm_pair[1 - k:2 - k])
            gptr = hb.ptr(self.gnorm_sq)
        hb.check(lib.asr_adam_clip_f32(n, hb.ptr(self.buf.flat_p), hb.ptr(self.buf.flat_g), hb.ptr(self.m),
                                       hb.ptr(self.v), hb.ptr(self.vmax), gptr,
                                       float(clip if clip is not None else 0.0), float(g["lr"]), b1,
                                       b2, float(g["eps"]), float(g["weight_decay"]),
                                       1.0 - b1 ** self.t, 1.0 - b2 ** self.t,
                                       None if skip_if is None else hb.c_p(skip_if.data_ptr()), nxt, hb.stream()),
                 "asr_adam_clip_f32")
        return self.gnorm_sq

    def unapply(self, n=1):
        """n apply() calls were no-ops on the device (skip_if was set): take the step count back."""
        self.t -= int(n)

    def step(self, max_grad_norm=None, group=None):
        """all-reduce (if distributed) -> global grad norm -> clip + Adam; no host sync."""
        self.reduce(group)
        return self.apply(max_grad_norm)

    # ---- torch.optim.Adam-compatible (de)serialisation
    def state_dict(self):
        state = {}
        if self.t > 0:
            for i, (p, o) in enumerate(zip(self.buf.params, self.buf.offsets)):
                n = p.numel()
                ent = dict(step=torch.tensor(float(self.t)), exp_avg=self.m[o:o + n].view_as(p).clone(),
                           exp_avg_sq=self.v[o:o + n].view_as(p).clone())
                if self.vmax is not None:
                    ent["max_exp_avg_sq"] = self.vmax[o:o + n].view_as(p).clone()
                state[i] = ent
        return dict(state=state, param_groups=[dict(self.param_groups[0])])

    def load_state_dict(self, sd):
        grp = sd["param_groups"][0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in grp:
                self.param_groups[0][k] = grp[k]
        for i, ent in sd.get("state", {}).items():
            i = int(i)
            p, o = self.buf.params[i], self.buf.offsets[i]
            n = p.numel()
            self.m[o:o + n].copy_(ent["exp_avg"].reshape(-1))
            self.v[o:o + n].copy_(ent["exp_avg_sq"].reshape(-1))
            if self.vmax is not None and "max_exp_avg_sq" in ent:
                self.vmax[o:o + n].copy_(ent["max_exp_avg_sq"].reshape(-1))
            self.t = int(float(ent["step"]))


# Rehearsal switch (measurement): ASR_FORCE_DP=1 makes a single process take the data-parallel step - process group of one
# rank on RCCL, the flat buffer all-reduced, the update predicated on the reduced latch - so that the step's timeline can be
# looked at on a one-GPU box (tools/profile_step.sh).
import os as _os
FORCE_DP = _os.environ.get("ASR_FORCE_DP", "0") == "1"


def init_distributed():
    """One process per GPU (torch.distributed.run env).  Returns (rank, world, local_rank)."""
    import os
    w = int(os.environ.get("WORLD_SIZE", "1"))
    if w <= 1:
        if FORCE_DP and torch.cuda.is_available() and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group(backend=os.environ.get("ASR_DIST_BACKEND", "nccl"), rank=0, world_size=1)
        return 0, 1, int(os.environ.get("LOCAL_RANK", "0"))
    rank = int(os.environ["RANK"])
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    if torch.cuda.is_available():
        ndev = max(1, torch.cuda.device_count())
        local = local % ndev                                    # rehearsal: several ranks may share one card
        torch.cuda.set_device(local)
        if w > ndev:
            # The persistent kernels need all 256 CUs of a device co-resident (one workgroup per CU).  Two processes
            # sharing a card could each get part of it and starve each other until the bounded spins abort, so a
            # shared-card rehearsal takes the per-step kernels.
            import hip_backend as hb
            hb.disable_persistent(permanent=True)
        backend = os.environ.get("ASR_DIST_BACKEND", "nccl")   # "nccl" is RCCL on ROCm
    else:
        backend = "gloo"
    if not dist.is_initialized():
        dist.init_process_group(backend=backend, rank=rank, world_size=w)
    return rank, w, local
