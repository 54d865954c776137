"""torch.autograd.Function wrappers over the C-ABI kernels (hip_backend).

One Function per *sequence-level* operator so that the sequential chains (encoder
recurrence, decoder loop) never bounce through Python/autograd per time step:

    linear            y = relu?(x W^T + b)                       -> asr_gemm_f32
    lstm_layer        whole (bi)LSTM layer, time-major            -> asr_gemm_f32 + asr_lstm_seq_*
    pyramid_concat    pair-concat (+dropout mask)                 -> asr_pyramid_concat_*
    decoder_sequence  all decoder steps incl. attention           -> asr_dec_* (+ GEMMs)

The Functions here are autograd bookkeeping: which buffers, which gradients, in which order.  The ctypes calls, the choice
"persistent kernel, else the per-step chain" and the path counters are hip_backend's (lstm_seq_fwd / _bwd;
dec_seq_fwd, dec_free_fwd, dec_seq_bwd, dec_smooth_bwd on a hip_backend.DecBuffers).

Workspaces.  Each chain op leases a preallocated, shape-keyed workspace from a pool for the span forward ->
end of backward, so that a train step causes no allocator traffic
(`_Lease`); a second concurrent user of the same shape (e.g. the two model passes of the SSL step) simply gets
another instance.  With autograd disabled (validation / greedy decoding) plain fresh tensors are used.
Outputs that alias a workspace (`y`) are only valid until that op's backward has run — the model consumes
them immediately; double backward / retain_graph through these ops is not supported.

GPU only; see hip_backend for the no-fallback rule.
"""
import ctypes
import os
import weakref

import torch

import hip_backend as hb


def gate_perm(H, device):
    """Row permutation torch (gate-major i,f,g,o) -> gate-interleaved (unit*4+gate)."""
    return torch.arange(4 * H, device=device).view(4, H).t().reshape(-1)


def gate_unperm(H, device):
    return torch.arange(4 * H, device=device).view(H, 4).t().reshape(-1)


# -------------------------------------------------------------------------------------- workspace pool
class _Lease(object):
    """Exclusive use of one workspace (the LSTM's dict of tensors, the decoder's hb.DecBuffers) until release() / garbage
    collection."""

    def __init__(self, free_list, ws):
        self._free, self.ws = free_list, ws

    def release(self):
        if self.ws is not None:
            self._free.append(self.ws)
            self.ws = None

    __del__ = release


class _Pool(object):
    def __init__(self):
        self.free = {}

    def acquire(self, key, factory):
        lst = self.free.setdefault(key, [])
        return _Lease(lst, lst.pop() if lst else factory())


_POOL = _Pool()


# -------------------------------------------------------------------------------------- accumulator arena
class _Arena(object):
    """Every buffer of a train step that has to START FROM ZERO - split-K GEMM outputs (their partial products meet in
    atomics; the outputs of ops.linear among them), bias-gradient sums, the accumulators of the sequence operators' backward
    passes, the loss scalar - cut from ONE buffer that
    ONE fill zeroes at the start of the step (Solver._step opens the scope: `with ops.step_arena(device)`), instead of a
    zero pass or a memset in front of each (39 fills per cfg-2 step, 0.2 ms).  A slice is valid until the next scope opens;
    outside a scope, and for what does not fit yet (the buffer grows to the step's need at the next scope), take() returns
    None and the caller falls back to its own zero fill.

    LIFETIME.  A slice is raw storage of the arena (set_ on the untyped storage: autograd cannot see that slices of
    different steps overlap), so everything a step produced inside its scope - the outputs of ops.linear (the logits and
    log-probs of E2E.forward among them), the weight gradients in .grad - is valid UNTIL THE NEXT SCOPE OPENS and is zeroed
    then.  Solver._step keeps to that: its closures hand back scalars only, which are copied to the step's host record
    inside the scope.  Code that wants to keep a tensor of a step (logging logits, comparing gradients across steps)
    clones it before the next step, or runs the model outside a scope (tests, validation: take() returns None there).

    INVARIANT.  Everything at and behind the cursor is zero: begin() zeroes what the previous scope used, nothing else was
    ever written.  A scope opened inside another one (Solver._recover, from the end of the step that found the abort) relies
    on it; ASR_ARENA_DEBUG=1 checks it at every begin() (a device sync: debugging only)."""

    def __init__(self):
        self.buf, self.cursor, self.want, self.active = None, 0, 0, False

    def begin(self, device):
        device = torch.device(device)
        if self.buf is None or self.buf.device != device or self.buf.numel() < self.want:
            # (first step, or the last step asked for more than there is: a new, larger buffer - zeros already)
            self.buf = torch.zeros(int(self.want * 1.25) + 4096, device=device, dtype=torch.float32) if self.want > 0 else None
        elif self.cursor > 0:
            self.buf[:self.cursor].zero_()               # what the previous step used: ONE fill
        if _ARENA_DEBUG and self.buf is not None:
            assert float(self.buf.abs().max()) == 0.0, "step arena: a value survived behind the cursor"
        self.cursor, self.want, self.active = 0, 0, True

    def end(self):
        self.active = False

    def take(self, shape, device):
        if not self.active:
            return None
        n = 1
        for v in shape:
            n *= int(v)
        n4 = (n + 63) // 64 * 64                         # slices stay 256-byte aligned (GEMM operands live here)
        self.want += n4
        if self.buf is None or self.buf.device != torch.device(device) or self.cursor + n4 > self.buf.numel():
            return None
        # a tensor of its own over the buffer's storage, not a view of the buffer: views share ONE version counter, and an
        # in-place torch op on any slice (index_add_ into an accumulator) would then invalidate every slice that an
        # autograd node saved for its backward (the outputs of ops.linear live here)
        shape = tuple(int(v) for v in shape)
        strides, acc = [], 1
        for v in reversed(shape):
            strides.append(acc)
            acc *= v
        out = torch.empty(0, device=self.buf.device, dtype=torch.float32).set_(
            self.buf.untyped_storage(), self.buf.storage_offset() + self.cursor, shape, tuple(reversed(strides)))
        self.cursor += n4
        return out


_ARENA_DEBUG = os.environ.get("ASR_ARENA_DEBUG", "0") == "1"
_ARENA = _Arena()
_LINEAR_ARENA = os.environ.get("ASR_LINEAR_ARENA", "1") != "0"      # measurement: the outputs of ops.linear from the arena


class step_arena(object):
    """Scope of one train step (forward + backward + optimiser): see _Arena."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        if torch.device(self.device).type == "cuda":
            _ARENA.begin(self.device)
        return _ARENA

    def __exit__(self, *exc):
        _ARENA.end()
        return False


def zeros_acc(shape, device):
    """A zero-initialised accumulator: a slice of the step's arena when there is one, else a fresh zero tensor."""
    t = _ARENA.take(shape, device)
    return t if t is not None else torch.zeros(*shape, device=device, dtype=torch.float32)


# -------------------------------------------------------------------------------------- weight gradients beside the chains
class _SideStream(object):
    """A batch of <= 8 utterances keeps every persistent kernel of the step (LSTM, decoder, judge) on four of the eight XCDs
    (hb.idle_xcd_mask).  The weight-gradient products of the backward pass are off its critical path - dG -> dX -> the
    recurrence of the layer below is - so they go to a SIDE stream, onto the idle XCDs, by workgroups that fit beside a
    persistent one (hb.gemm_side / asr_gemm_side_f32), and run under the recurrence of the layer below.
      defer(dev, launch, keep)   inside a backward function: queue products for the side stream (see there).  The first one
                         of a backward pass registers the join with the autograd engine: when the pass ends, the stream the
                         backward ran on waits for the side stream - code that reads .grad afterwards (the optimiser, a
                         test) finds every gradient complete without knowing about any of this.
      flush()            in front of a recurrence: start what is queued, beside it.
      join_now()         flush + the wait at once (a node that consumes side results inside the pass: _LstmPack.backward).
    Outputs are zeroed on the main stream BEFORE defer() (the side products add into them with atomics).  Off: ASR_SIDE_GEMM=0, the
    fp32-input MFMA arithmetic (no such kernel), deterministic mode (hb.DETERMINISTIC), gradients exchanged from inside the backward pass (dp_overlap: its hooks
    read a gradient as soon as autograd has it).
      count_use(ctx, w) / may_defer(ctx, w)   a weight gradient handed back before its product exists (_Linear): see there."""

    def __init__(self):
        self.enabled = os.environ.get("ASR_SIDE_GEMM", "1") != "0"
        self.streams, self.active, self.mask_hint = {}, None, 0
        self.uses = {}                     # weight data_ptr -> live autograd nodes that use it (count_use)
        self.deferred = []                 # (launch closure, temporaries) waiting for the next recurrence
        self.task = -1                     # the autograd graph task (backward pass) `active` belongs to
        self.launches = 0

    def mask_for(self, nbatch):
        return hb.idle_xcd_mask(nbatch) if self.enabled else 0

    def usable(self, mask=0xff):
        # (deterministic mode: the side products add their K slices with atomics, and a second stream is one more ordering
        # freedom - every weight gradient is formed on the main stream)
        return bool(mask) and self.enabled and not hb.is_deterministic() and (hb.current_arith() & 0xff) != hb.ARITH_F32

    def count_use(self, ctx, weight):
        """A forward use of `weight` that may send it a gradient: counted for as long as its node `ctx` lives - a graph whose
        backward never runs (dropped, or a forward under no_grad) takes its count with it, whichever step comes next."""
        key = weight.data_ptr()
        self.uses[key] = self.uses.get(key, 0) + 1
        weakref.finalize(ctx, self._drop_use, key)

    def _drop_use(self, key):
        n = self.uses.get(key, 0) - 1
        if n > 0:
            self.uses[key] = n
        else:
            self.uses.pop(key, None)

    def may_defer(self, ctx, weight):
        """May the backward of node `ctx` return a zeroed dW of `weight` whose product lands in it after the pass?  Only if
        autograd hands that tensor on unread as the new .grad: a leaf with no .grad yet, no hook that reads its gradient on
        the way, and no other live node using it - any second gradient of the pass (the other model pass of the
        semi-supervised step, whatever its rows or XCD mask) would be ADDED to it on the main stream while it is zeros."""
        return (ctx.side_mask and ctx.needs_input_grad[0] and weight.is_leaf and weight.grad is None
                and not weight._backward_hooks and not getattr(weight, "_post_accumulate_grad_hooks", None)
                and self.uses.get(weight.data_ptr(), 0) == 1 and self.usable(ctx.side_mask))

    def defer(self, dev, launch, keep):
        """Inside a backward function, once the operands are final on the current stream: queue `launch` (a closure that
        enqueues the products on whatever stream is current) for the side stream.  It is NOT started here - right behind a
        recurrence the main stream runs the critical dX products, and side workgroups on half the chip's CUs would starve
        them (measured: a [5 248, 2 048] x [2 048, 512] dX product 394 us instead of 106) - but when the NEXT recurrence is
        about to be enqueued (flush(), called by _LstmLayer.backward in front of its chain kernel), or when the pass ends.
        `keep`: the tensors the products read or write that are temporaries of the caller (kept alive until the launch, then
        handed to record_stream: the allocator must not give their memory to the main stream's next allocation - a fresh,
        ZEROED ticket counter, say - while the side stream still runs)."""
        main = torch.cuda.current_stream(dev)
        st = self.streams.get(dev.index)
        if st is None:
            st = self.streams[dev.index] = torch.cuda.Stream(device=dev)
        task = torch._C._current_graph_task_id()
        if self.active is not None and task != self.task:
            # a pass that never ended (an exception inside backward): its join never ran - what it left is dropped, the
            # side stream is drained, and this pass registers its own join
            self.active[0].wait_stream(self.active[1])
            del self.deferred[:]
            self.active = None
        if self.active is None:
            self.active, self.task = (main, st), task
            torch.autograd.Variable._execution_engine.queue_callback(self.join)
        self.deferred.append((launch, keep))
        self.launches += 1

    def flush(self):
        """Start what has been deferred: the side stream waits for everything enqueued on the main stream so far."""
        if self.active is None or not self.deferred:
            return
        if self.task != torch._C._current_graph_task_id() and torch._C._current_graph_task_id() != -1:
            return                         # (leftovers of a pass that never ended: defer() of THIS pass will drop them)
        main, st = self.active
        ev = torch.cuda.Event()
        ev.record(main)
        st.wait_event(ev)
        with torch.cuda.stream(st):
            for launch, keep in self.deferred:
                launch()
                for t in keep:
                    t.record_stream(st)
        del self.deferred[:]

    def join_now(self):
        if self.active is not None:
            self.flush()
            self.active[0].wait_stream(self.active[1])

    def join(self):
        self.join_now()
        self.active = None


_SIDE = _SideStream()


def _side_product(a, b, out, queue, mask):
    code = hb.current_arith()              # (the arithmetic of the node that queued it, not of whoever flushes)
    return lambda: hb.gemm_side(a, b, out, queue, mask, trans_a=True, arith=code)


def _gemm_acc(A, B, trans_a=False, trans_b=False, shape=None):
    """A product into a fresh output that no epilogue follows (the weight gradients): inside a step's arena the output is a
    pre-zeroed slice and the library accumulates into it - no zero pass in front of a split-K product."""
    out = _ARENA.take(shape, A.device) if shape is not None else None
    if out is None:
        return hb.gemm(A, B, trans_a=trans_a, trans_b=trans_b)
    return hb.gemm(A, B, trans_a=trans_a, trans_b=trans_b, out=out, accumulate=True)


def _colsum_acc(X):
    out = _ARENA.take((X.shape[1],), X.device)
    return hb.colsum(X) if out is None else hb.colsum(X, out=out, accumulate=True)


# --------------------------------------------------------------------------------------
def _with_saved_arith(bwd):
    """The backward of a sequence operator runs under the product arithmetic its FORWARD ran under (ctx.arith), not under
    whatever the host default is when .backward() happens to be called: a forward inside `with hb.arith("f32")` followed by
    a backward outside the block would otherwise mix arithmetics (and the fused-dW_hh decision with them)."""
    import functools

    @functools.wraps(bwd)
    def wrapped(ctx, *grads):
        with hb.arith(ctx.arith):
            return bwd(ctx, *grads)
    return wrapped


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu, drop):
        ctx.arith = hb.current_arith()
        x2 = x.reshape(-1, x.shape[-1])
        seeded = isinstance(drop, hb.SeededMask)
        if seeded:                                   # relu -> dropout in the product's own epilogue pass; the mask is
            assert relu and (x2.shape[0] * weight.shape[0]) % 4 == 0      # regenerated in the backward
        # (inside a train step the output is a pre-zeroed slice of the step's arena: a product the library splits over K
        # then needs no zero pass of its own)
        out = _ARENA.take((x2.shape[0], weight.shape[0]), x2.device) if _LINEAR_ARENA else None
        y = hb.gemm(x2, weight, trans_b=True, bias=bias, relu=relu, drop=drop if seeded else None, out=out,
                    out_zeroed=out is not None)
        ctx.save_for_backward(x2, weight, y if relu else None)
        ctx.side_mask = 0
        if ctx.needs_input_grad[1]:                  # (grad mode is off inside forward: ask the node)
            _SIDE.count_use(ctx, weight)             # EVERY use, whatever its rows or mask (_SideStream.may_defer)
            ctx.side_mask = _SIDE.mask_hint if x2.shape[0] >= 512 else 0
        ctx.relu = relu
        ctx.drop = (drop.seed, drop.p) if seeded else None
        ctx.has_bias = bias is not None
        ctx.in_shape = x.shape
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @_with_saved_arith
    def backward(ctx, dy):
        x2, weight, y = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        if ctx.relu and y.numel() % 4 == 0:
            # one pass: relu gradient (and the dropout mask: y is the dropped-out output, y > 0 <=> kept and active)
            # (its column sums - the bias gradient - from the same pass were tried: the atomics of a column meet in one L2
            # line, 32 us against 8 + 5 for the two launches at the layer-0 projection)
            seed, p = ctx.drop if ctx.drop is not None else (0, 0.0)
            dy2 = hb.relu_dropout_bwd(dy2, y, seed, p)
        elif ctx.relu:
            dy2 = dy2 * (y > 0).to(dy2.dtype)
        dx = hb.gemm(dy2, weight).view(ctx.in_shape) if ctx.needs_input_grad[0] else None
        # the weight gradient beside the recurrence of the layer below (a small batch, >= 512 rows; _SideStream) - unless
        # nothing follows this node in the pass, or autograd would not take dW over unread as the new .grad: a weight with
        # another live use (the other model pass of the semi-supervised step, whatever its rows or mask: autograd would ADD
        # the two on the main stream while this one is still zeros), a .grad to add into, a hook (_SideStream.may_defer)
        if _SIDE.may_defer(ctx, weight):
            dw = zeros_acc((dy2.shape[1], x2.shape[1]), dy2.device)
            queue = zeros_acc((1,), dy2.device)
            # (the closure writes through an ALIAS of dw - a tensor object of its own over the same memory: AccumulateGrad
            # takes a gradient over as .grad only while nobody else holds the tensor object, and CLONES it otherwise - at once,
            # on the main stream, i.e. the zeros)
            _SIDE.defer(dy2.device, _side_product(dy2, x2, dw.detach(), queue, ctx.side_mask), (dy2, x2, queue))
        else:
            dw = _gemm_acc(dy2, x2, trans_a=True, shape=(dy2.shape[1], x2.shape[1]))
        db = _colsum_acc(dy2) if ctx.has_bias else None
        return dx, dw, db, None, None


def linear(x, weight, bias=None, relu=False, drop=None):
    """nn.Linear (+ optional fused ReLU, + optional seeded dropout after it) on the f32 MFMA GEMM (model.py:93-95,144)."""
    return _Linear.apply(x, weight, bias, relu, drop)


# --------------------------------------------------------------------------------------
def _row_capacity(n):
    """Rows a pooled workspace is allocated for: n rounded up to a quarter of its power of two (<= 25 % over), so that the
    row counts of an epoch's batches (every batch has its own sum of lengths) share a handful of workspaces."""
    n = max(int(n), 1)
    q = max(256, 1 << max(n.bit_length() - 3, 0))
    return (n + q - 1) // q * q


def _lstm_workspace(rows, nbatch, H, ndir, dev, with_bwd):
    """Buffers of one LSTM layer for up to `rows` (time, batch) rows and `nbatch` batch rows; _lstm_views cuts the views of a
    call's actual shape out of them."""
    f32 = dict(device=dev, dtype=torch.float32)
    # (zeros, and one row more than asked for: the packed-row dW_hh product reads ONE row behind the matrix on each side -
    # against a zero padding row of the other operand - and that row must hold finite numbers: _LstmLayer.backward zeroes it
    # when a longer batch has used the workspace before)
    alloc = torch.zeros if with_bwd else torch.empty
    ws = dict(gates_buf=alloc(rows + 1, ndir, 4 * H, **f32), y_buf=alloc(rows + 1, ndir * H, **f32),
              c_buf=torch.empty(rows, ndir * H, **f32))
    if with_bwd:
        # the three accumulators the backward starts from zero share one buffer: one fill instead of three
        n1, n2, n3 = nbatch * ndir * H, ndir * 4 * H * H, ndir * 4 * H
        zbuf = torch.empty(n1 + n2 + n3, **f32)
        ws.update(w_hhT=torch.empty(ndir, H, 4 * H, **f32), dy_buf=torch.empty(rows, ndir * H, **f32), zbuf=zbuf,
                  dcarry=zbuf[:n1].view(nbatch, ndir * H), dw_hh=zbuf[n1:n1 + n2].view(ndir, 4 * H, H),
                  db=zbuf[n1 + n2:].view(ndir * 4 * H))
    return ws


def _lstm_views(ws, T, B, H, ndir):
    n = T * B
    ws["gates"] = ws["gates_buf"][:n].view(T, B, ndir, 4 * H)
    ws["y"] = ws["y_buf"][:n].view(T, B, ndir * H)
    ws["c"] = ws["c_buf"][:n].view(T, B, ndir * H)
    if "dy_buf" in ws:
        ws["dy"] = ws["dy_buf"][:n].view(T, B, ndir * H)
    return ws


class _LstmPack(torch.autograd.Function):
    """torch layout of nn.LSTM's parameters (per direction w_ih [4H,I], w_hh [4H,H], b_ih, b_hh; gate-major rows, model.py:
    67-68) -> the kernels' gate-interleaved layout, for ALL layers of a stack in one launch; the backward takes the layers'
    gradients in that layout back in one launch.  Outputs per layer: w_ih_cat [ndir*4H, I], w_hh_il [ndir, 4H, H], bias
    [ndir*4H] (= b_ih + b_hh)."""

    @staticmethod
    def forward(ctx, ndir, nlayers, *params):
        per = 4 * ndir
        layers = [params[per * j:per * (j + 1)] for j in range(nlayers)]
        ctx.ndir, ctx.dims = ndir, [(lp[1].shape[1], lp[0].shape[1]) for lp in layers]
        ctx.set_materialize_grads(False)
        outs = hb.lstm_pack_multi(layers, ndir)
        return tuple(t for out in outs for t in out)

    @staticmethod
    def backward(ctx, *grads):
        _SIDE.join_now()                   # the layers' dW_ih / dW_hh may still be on their way on the side stream
        n = len(ctx.dims)
        per_layer = [grads[3 * j:3 * j + 3] for j in range(n)]
        for j, g in enumerate(per_layer):
            if any(t is None for t in g) and not all(t is None for t in g):     # (never on the product's paths)
                H, I = ctx.dims[j]
                ref = next(t for t in g if t is not None)
                shp = ((ctx.ndir * 4 * H, I), (ctx.ndir, 4 * H, H), (ctx.ndir * 4 * H,))
                per_layer[j] = [t if t is not None else torch.zeros(shp[k], device=ref.device) for k, t in enumerate(g)]
        outs = hb.lstm_unpack_multi(per_layer, ctx.dims, ctx.ndir)
        flat = []
        for j in range(n):
            flat += outs[j] if outs[j] is not None else [None] * (4 * ctx.ndir)
        return (None, None) + tuple(flat)


def lstm_pack(layers, ndir):
    """layers: per layer the flat parameter list of its directions (model._LstmWeights.direction_params) -> per layer
    (w_ih_cat, w_hh_il, bias) for lstm_layer(packed=...)."""
    flat = [p for lp in layers for p in lp]
    out = _LstmPack.apply(ndir, len(layers), *flat)
    return [out[3 * j:3 * j + 3] for j in range(len(layers))]


class _LstmLayer(torch.autograd.Function):
    """One (bi)directional LSTM layer over a padded time-major batch (model.py:79-81).
    w_ih [ndir*4H, I], w_hh [ndir, 4H, H], bias [ndir*4H]: the gate-interleaved parameters (_LstmPack); their gradients
    leave in the same layout.
    rows (hb.LayerRows or None): the packed-row layout - x is then the row matrix [R, 1, I] (every product of this layer is
    a GEMM over the R rows as if it were a time-major batch of one; only the recurrence kernels know about utterances)."""

    @staticmethod
    def forward(ctx, x, lens, ndir, pooled, rows, w_ih, w_hh, bias):
        ctx.arith = hb.current_arith()
        T, B, I = x.shape
        H = w_hh.shape[2]
        dev = x.device
        x2 = x.reshape(T * B, I)
        nbatch = rows.B if rows is not None else B
        if pooled:
            cap = _row_capacity(T * B)
            lease = _POOL.acquire(("lstm", dev.index, cap, nbatch, H, ndir),
                                  lambda: _lstm_workspace(cap, nbatch, H, ndir, dev, True))
            ws = lease.ws
        else:
            lease, ws = None, _lstm_workspace(T * B, nbatch, H, ndir, dev, False)
        _lstm_views(ws, T, B, H, ndir)
        ws["rows_written"] = max(ws.get("rows_written", 0), T * B)      # rows of gates_buf / y_buf that may hold stale values
        ctx.side_mask = _SIDE.mask_hint = _SIDE.mask_for(nbatch) if pooled else 0
        ws["lens"] = lens                      # int32 device tensor, kept for the backward (no copy)
        hb.gemm(x2, w_ih, trans_b=True, bias=bias, out=ws["gates"].view(T * B, ndir * 4 * H))
        hb.lstm_seq_fwd(ws["gates"], w_hh, ws["lens"], ws["y"], ws["c"], rows=rows)
        ctx.save_for_backward(x2, w_ih, w_hh)
        ctx.lease = lease
        ctx.rows = rows
        ctx.dims = (T, B, I, H, ndir)
        return ws["y"].detach()      # fresh tensor object aliasing the workspace (no stale autograd metadata)

    @staticmethod
    @_with_saved_arith
    def backward(ctx, dy):
        x2, w_ih, w_hh = ctx.saved_tensors
        T, B, I, H, ndir = ctx.dims
        lease = ctx.lease
        assert lease is not None and lease.ws is not None, "lstm_layer backward needs the leased workspace " \
            "(autograd was off in forward, or backward ran twice)"
        ws = _lstm_views(lease.ws, T, B, H, ndir)      # (the views of THIS call's shape: the buffers are shared by capacity)
        dev = dy.device
        dyc = dy if dy.is_contiguous() else ws["dy"].copy_(dy)
        zb = _ARENA.take((ws["zbuf"].numel(),), dev)
        if zb is None:
            ws["zbuf"].zero_()                 # dcarry, dw_hh, db
        else:                                  # ... or their places in the step's arena (zeroed with everything else)
            nb_, n2 = ws["dcarry"].numel(), ws["dw_hh"].numel()
            ws = dict(ws, dcarry=zb[:nb_].view_as(ws["dcarry"]), dw_hh=zb[nb_:nb_ + n2].view_as(ws["dw_hh"]),
                      db=zb[nb_ + n2:].view_as(ws["db"]))
        gates, y = ws["gates"], ws["y"]
        _SIDE.flush()                          # weight-gradient products of the layers above: beside THIS layer's recurrence
        # the transposed recurrent weights are only formed if the kernel that reads the forward layout does not apply
        fused_dw, fused_db = hb.lstm_seq_bwd(gates, lambda: ws["w_hhT"].copy_(w_hh.transpose(1, 2)), ws["lens"], dyc,
                                             ws["c"], ws["dcarry"], y=y, dw_hh=ws["dw_hh"], db=ws["db"],
                                             w_hh=w_hh, rows=ctx.rows)                    # gates <- dG in place
        dG = gates.view(T * B, ndir * 4 * H)
        # dW_hh[d] = sum_t dG_t[d]^T h_prev(t), h_prev = y[t-1] (d = 0) or y[t+1] (reverse direction) - unless the persistent
        # kernel has summed it: ONE batched GEMM over the directions, K = (T-1)*B, accumulated into a zeroed output (no zero
        # pass of its own).
        #   d = 0: A = dG[B:, 0:4H],        B = y[:(T-1)B, 0:H]
        #   d = 1: A = dG[:(T-1)B, 4H:8H],  B = y[B:, H:2H]          -> batch strides relative to d = 0 (may be negative)
        # packed rows: K = R instead of R - 1 (a multiple of 4: the GEMM's fast kernels want that).  The one extra pair
        # is (row R of dG, the last row of y) resp. (the last row of dG, row R of y): the last row of the matrix is a
        # padding row - zero in both - and row R exists in the workspace and holds finite numbers (_lstm_workspace)
        with_hh = not fused_dw and T > 1
        ldg, ldy = ndir * 4 * H, ndir * H
        kk = T * B if ctx.rows is not None else (T - 1) * B
        hh_shape = (True, False, 4 * H, H, kk, ldg, ldy, H, ndir, 4 * H - B * ldg, B * ldy + H, 4 * H * H)
        # a small batch: this layer's weight gradients go beside the recurrence of the layer BELOW (_SideStream) - not those of
        # the bottom layer (no input gradient: nothing follows it in the pass, and the main stream's kernels have the whole chip)
        side = bool(ctx.side_mask and ctx.needs_input_grad[0] and _SIDE.usable(ctx.side_mask))
        if side:
            dw_ih = zeros_acc((ndir * 4 * H, I), dev)
            queue = zeros_acc((2,), dev)
            # (without a step arena the accumulators live in the leased workspace and are copied out below, on the main
            # stream: the side product then needs a tensor of its own)
            dw_hh_side = ws["dw_hh"] if zb is not None else torch.zeros_like(ws["dw_hh"])
        if with_hh and ctx.rows is not None and ws.get("rows_written", 0) > T * B:
            # the workspace is shared by capacity: a LONGER batch left its own values in row R - finite ones normally,
            # but NaN when that batch's launch aborted (the kernels poison their outputs), and 0 * NaN is NaN
            ws["gates_buf"][T * B].zero_()
            ws["y_buf"][T * B].zero_()
        dx = hb.gemm(dG, w_ih).view(T, B, I) if ctx.needs_input_grad[0] else None
        if side:
            mask, code = ctx.side_mask, hb.current_arith()

            def launch():
                # (dG and y live in the layer's pooled workspace: no forward pass leases it again before the pass has ended)
                hb.gemm_side(dG, x2, dw_ih, queue[0:1], mask, trans_a=True, arith=code)
                if with_hh:
                    hb.gemm_side_batched(dG, y, dw_hh_side, queue[1:2], mask, *hh_shape, arith=code, a_off=B * ldg)
            _SIDE.defer(dev, launch, (x2, queue))
        else:
            dw_ih = _gemm_acc(dG, x2, trans_a=True, shape=(ndir * 4 * H, I))      # [ndir*4H, I]
        db = ws["db"] if fused_db else _colsum_acc(dG)     # the persistent kernels sum the bias gradient themselves
        if with_hh and not side:
            hb.gemm_batched(dG, y, ws["dw_hh"], *hh_shape, accumulate=True, a_off=B * ldg)
        # the gradients stay gate-interleaved (_LstmPack.backward converts every layer's in one launch); what lives in the
        # leased workspace is copied out of it, slices of the step's arena outlive the lease
        dw_hh, db = (ws["dw_hh"], db) if zb is not None else (ws["dw_hh"].clone(), db.clone() if fused_db else db)
        if side and with_hh:
            dw_hh = dw_hh_side
        lease.release()
        return dx, None, None, None, None, dw_ih, dw_hh, db


def lstm_layer(x, lens, params, ndir, rows=None, packed=None):
    """x [T,B,I] time-major contiguous, lens int32 device [B] -> y [T,B,ndir*H].
    rows (hb.LayerRows): packed rows - x [R, I] -> y [R, ndir*H], lens = rows.lens.
    packed: this layer's (w_ih_cat, w_hh_il, bias) from lstm_pack (a stack converts all its layers in one launch); None:
    converted here from the torch-layout `params`."""
    if packed is None:
        packed = lstm_pack([params], ndir)[0]
    w_ih, w_hh, bias = packed
    pooled = torch.is_grad_enabled() and (x.requires_grad or w_hh.requires_grad)
    if rows is not None:
        return _LstmLayer.apply(x.contiguous().view(rows.R, 1, -1), rows.lens, ndir, pooled, rows, w_ih, w_hh, bias).view(rows.R, -1)
    return _LstmLayer.apply(x.contiguous(), lens, ndir, pooled, None, w_ih, w_hh, bias)


# --------------------------------------------------------------------------------------
class _Pyramid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, rep):
        T, B, C = x.shape
        out = torch.empty((T + 1) // 2, B, 2 * C, device=x.device, dtype=torch.float32)
        hb.pyramid_fwd(x.contiguous(), mask, out)
        if rep is not None:                        # packed rows: the replicate-padded frame of the longest utterances
            out[rep, 0, C:] = out[rep, 0, :C]
        ctx.mask = mask                            # tensor, hb.SeededMask (regenerated in the backward) or None
        ctx.rep = rep
        ctx.shape = (T, B, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        T, B, C = ctx.shape
        din = torch.empty(ctx.shape, device=dout.device, dtype=torch.float32)
        dout = dout.contiguous()
        if ctx.rep is not None:                    # the replica's gradient belongs to the frame it copies; the padding row
            dout = dout.clone()                    # whose place it took gets none
            dout[ctx.rep, 0, :C] += dout[ctx.rep, 0, C:]
            # (not `dout[ctx.rep, 0, C:] = 0.0`: the scalar goes to the device by a blocking copy, and the host, which
            # is to stay a step ahead of the GPU, waits in every backward pass for all that is queued)
            dout[:, 0, C:].index_fill_(0, ctx.rep, 0.0)
        hb.pyramid_bwd(dout, ctx.mask, din)
        return din, None, None


def pyramid_concat(x, mask=None, rep_rows=None):
    """[T,B,C] -> [ceil(T/2),B,2C] (model.py:85-92); `mask` = pre-scaled dropout mask or None.
    Packed rows: x [R, 1, C] (R even) -> [R / 2, 1, 2C]; rep_rows = long tensor of the output rows whose second half is the
    reference's replicate-padded frame (hb.RowLayout.replicated_rows), or None."""
    return _Pyramid.apply(x, mask, rep_rows)


class _RowsUnpack(torch.autograd.Function):
    """Packed encoder output [R, C] -> the padded batch [B, T, C] the decoder reads (model.py:109-112).  The frames behind an
    utterance are what the reference's last projection makes of a zero frame, dropout(relu(bias)): fill [C] * mask."""

    @staticmethod
    def forward(ctx, packed, fill, rows, T, mask, fill_relu):
        ctx.rows, ctx.mask, ctx.C = rows, mask, packed.shape[1]
        ctx.want_fill = fill is not None and fill.requires_grad
        fc = fill.contiguous() if fill is not None else None
        ctx.relu_of = fc if (fill_relu and ctx.want_fill) else None
        return hb.rows_unpack_fwd(packed.contiguous(), rows, T, fc, mask, fill_relu=fill_relu)

    @staticmethod
    def backward(ctx, dout):
        acc = _ARENA.take((ctx.C,), dout.device) if ctx.want_fill else None
        drows, dfill = hb.rows_unpack_bwd(dout.contiguous(), ctx.rows, ctx.C, ctx.mask, ctx.want_fill, relu_of=ctx.relu_of,
                                          dfill=acc)
        return drows, dfill, None, None, None, None


def rows_unpack(packed, rows, T, fill=None, mask=None, fill_relu=False):
    """fill_relu: the padded frames hold relu(fill) * mask - `fill` is the last projection's bias as it is (no relu launch in
    front, none of its backward behind)."""
    return _RowsUnpack.apply(packed, fill, rows, T, mask, fill_relu)


# --------------------------------------------------------------------------------------
def _dec_clear(buf):
    """Zeroed step inputs for a sequence whose inputs are filled in step by step -> fed [L, B] (zeros)."""
    fed = torch.zeros(buf.L, buf.B, dtype=torch.long, device=buf.X.device)   # token whose embedding fed step s (-1: smooth)
    buf.X.zero_()
    if buf.Xd is not None:
        buf.Xd.zero_()
    return fed


def _dec_teacher_forced(buf, emb_w, tokens, w_out, b_out, skip_pred):
    """Every step is fed its teacher token: the inputs are complete before the first step.  -> fed, logits, pred"""
    B, L, D, O, E = (buf.dims[k] for k in "BLDOE")
    X, Xd, xmask = buf.X, buf.Xd, buf.xmask
    if (D + O) % 4 == 0 and E % 4 == 0 and (O + E) % 4 == 0 and tokens.stride(1) == 1:
        # zero fills, embedding gather, input dropout, fed: one launch
        fed = torch.empty(L, B, dtype=torch.long, device=X.device)
        hb.dec_prepare(tokens, emb_w.contiguous(), xmask, X, Xd, fed, L, B, D, O, E)
    else:
        fed = _dec_clear(buf)
        fed.copy_(tokens.t())
        X[:L, :, D + O:] = emb_w[fed]
        if Xd is not None:
            Xd[:L, :, D + O:] = X[:L, :, D + O:] * xmask[:, :, O:]
    hb.dec_seq_fwd(buf)
    logits = hb.gemm(X[1:].view(L * B, buf.KX)[:, :D + O], w_out, trans_b=True, bias=b_out).view(L, B, w_out.shape[0])
    # (skip_pred: the caller takes the argmax from the loss kernel that reads the logits anyway - label_logprob)
    return fed, logits, (None if skip_pred else logits.argmax(-1))


def _dec_free_kernels(buf, emb_w, tokens, tf_flags, smooth, opts, w_out, b_out):
    """Free-running steps on the feedback kernels (hb.dec_free_fwd: persistent, else per step); no sampling, V <= 128.
    -> fed, logits, pred, probs_saved (smooth feedback: a tensor [L-1, B, V]), whether the persistent kernel ran"""
    B, L, D, O = (buf.dims[k] for k in "BLDO")
    X, Xd, dev, V = buf.X, buf.Xd, buf.X.device, w_out.shape[0]
    fed = _dec_clear(buf)
    logits = torch.empty(L, B, V, device=dev, dtype=torch.float32)
    pred = torch.empty(L, B, dtype=torch.long, device=dev)
    emb_c = emb_w.contiguous()
    probs_saved = torch.empty(max(L - 1, 1), B, V, device=dev, dtype=torch.float32) if smooth and tokens is None else []
    tok_c = tokens.contiguous() if tokens is not None else None
    fed[0] = tok_c[:, 0] if tok_c is not None else opts["bos"]
    X[0, :, D + O:] = emb_c[fed[0]]
    if Xd is not None:
        Xd[0, :, D + O:] = X[0, :, D + O:] * buf.xmask[0, :, O:]
    done = hb.dec_free_fwd(buf, w_out, b_out, emb_c, logits, pred, fed, probs_saved, tok_c, tf_flags, smooth,
                           float(opts.get("smooth_scaling", 1.0)), int(opts.get("eos", -1)))
    return fed, logits, pred, probs_saved, done


def _dec_free_torch(buf, emb_w, tokens, tf_flags, smooth, sample, opts, w_out, b_out):
    """Free-running steps with the feedback in torch between the per-step kernels: sampling, V > 128, or the feedback kernels
    switched off.  -> fed, logits, pred, probs_saved (smooth feedback: a list of L-1 tensors [B, V])"""
    B, L, D, O = (buf.dims[k] for k in "BLDO")
    X, Xd, dev, V = buf.X, buf.Xd, buf.X.device, w_out.shape[0]
    fed = _dec_clear(buf)
    fs = buf.fwd_struct()
    logits = torch.empty(L, B, V, device=dev, dtype=torch.float32)
    pred = torch.empty(L, B, dtype=torch.long, device=dev)
    probs_saved = []
    for s in range(L):
        if s == 0:
            tok = tokens[:, 0] if tokens is not None else torch.full((B,), opts["bos"], dtype=torch.long, device=dev)
            fed[0] = tok
            X[0, :, D + O:] = emb_w[tok]
        elif tokens is not None:
            tok = tokens[:, s] if tf_flags[s] else pred[s - 1]
            fed[s] = tok
            X[s, :, D + O:] = emb_w[tok]
        elif not smooth:
            fed[s] = pred[s - 1]
            X[s, :, D + O:] = emb_w[pred[s - 1]]
        else:
            pr = torch.softmax(logits[s - 1] * opts["smooth_scaling"], dim=-1)
            probs_saved.append(pr)
            fed[s] = -1
            hb.gemm(pr, emb_w, out=X[s][:, D + O:])
        if Xd is not None:
            Xd[s, :, D + O:] = X[s, :, D + O:] * buf.xmask[s, :, O:]
        hb.dec_step_fwd(fs, s)
        hb.gemm_skinny(X[s + 1][:, :D + O], w_out, bias=b_out, out=logits[s])
        pred[s] = torch.distributions.Categorical(logits=logits[s]).sample() if sample else logits[s].argmax(-1)
    return fed, logits, pred, probs_saved


def _dec_smooth_bwd_torch(buf, acc, with_dws, w_out, emb_w, probs_saved, k, dw_out, db_out, demb_w):
    """The smooth-feedback backward (hb.dec_smooth_bwd) of a forward that ran on torch glue: the extra gradient is injected
    between the per-step kernels, and the weight gradients that depend on it are added step by step."""
    D, O = buf.dims["D"], buf.dims["O"]
    hb.count_path("dec_bwd", False, "free-running smooth: %s L=%d fused-feedback=False" % (hb.dec_shape(buf), buf.L))
    bs = buf.bwd_struct(acc=acc, with_dws=with_dws)
    G, X = acc["G"], buf.X
    for s in range(buf.L - 1, -1, -1):
        hb.dec_step_bwd(bs, s)
        if s >= 1:
            demb = G[s][:, D + O:]
            pr = probs_saved[s - 1]
            hb.gemm(pr, demb, trans_a=True, out=demb_w, accumulate=True, split_k=1)
            dp = hb.gemm(demb, emb_w, trans_b=True)
            dl = (k * pr * (dp - (pr * dp).sum(-1, keepdim=True))).contiguous()
            hb.gemm(dl, w_out, out=G[s][:, :D + O], accumulate=True, split_k=1)
            hb.gemm(dl, X[s][:, :D + O], trans_a=True, out=dw_out, accumulate=True, split_k=1)
            hb.colsum(dl, out=db_out, accumulate=True)


class _DecoderSeq(torch.autograd.Function):
    """All decoder steps (Decoder.forward loop, model.py:324-351) as one graph node.

    inputs : P [B,Tp,A], Q [B,Tp,O] (= enc_h W_o^T, no bias), emb_w [V,E], w_ih [4D,E+O], w_hh [4D,D],
             b_ih, b_hh, wdec [A,D], convw [C,1,1,2K+1], watt [A,C], gvec [1,A], bo [O], w_out [V,D+O],
             b_out [V], w0 [B,Tp]
    opts   : dict(L, tokens [B,L] long or None, tf_flags list[bool] or None, smooth, smooth_scaling,
                  sample, scaling (attention temperature), xmask [L,B,O+E] or None, pooled)
    returns: logits [L,B,V], ws [L,B,Tp], prediction [L,B] (long)

    The buffers are one hb.DecBuffers (leased from the pool when a backward follows); the launches are hip_backend's.
    forward: teacher-forced (_dec_teacher_forced) | free-running on the feedback kernels (_dec_free_kernels) | free-running on
    torch glue (_dec_free_torch).  backward: the chain backward (hb.dec_seq_bwd) | smooth feedback on the kernels
    (hb.dec_smooth_bwd: persistent, else per step) | smooth feedback on torch glue (_dec_smooth_bwd_torch).
    """

    @staticmethod
    def forward(ctx, P, Q, emb_w, w_ih, w_hh, b_ih, b_hh, wdec, convw, watt, gvec, bo, w_out, b_out, w0, opts):
        ctx.arith = hb.current_arith()
        dev = P.device
        B, Tp, A = P.shape
        O = Q.shape[2]
        D = w_hh.shape[1]
        E = emb_w.shape[1]
        V = w_out.shape[0]
        C = convw.shape[0]
        K = (convw.shape[-1] - 1) // 2
        L = int(opts["L"])
        KX = D + O + E
        xmask_in = opts.get("xmask")
        drop = xmask_in is not None
        pooled = bool(opts.get("pooled", False))
        if pooled:
            lease = _POOL.acquire(("dec", dev.index, B, Tp, A, D, O, E, C, K, L, drop),
                                  lambda: hb.DecBuffers(B, Tp, A, D, O, E, C, K, L, drop, dev, True))
            buf = lease.ws
        else:
            lease, buf = None, hb.DecBuffers(B, Tp, A, D, O, E, C, K, L, drop, dev, False)
        # [4D, KX] gate-interleaved rows + the transposed images the per-step forward (wattT) and the backward (wcatT, wdecT)
        # read, one launch
        hb.dec_pack(w_ih, w_hh, b_ih, b_hh, wdec, watt, D, O, E, A, C, buf.wcat, buf.bcat, buf.wcatT, buf.wdecT, buf.wattT)
        # inputs used as they are (no staging copies); the buffer object keeps them alive until the backward has run
        buf.bind(P, Q, w0, convw, gvec, bo, wdec, watt, xmask_in, opts.get("scaling", 2.0))
        w_out_c = w_out.contiguous()
        tokens = opts.get("tokens")
        tf_flags = opts.get("tf_flags")
        smooth = bool(opts.get("smooth", False))
        sample = bool(opts.get("sample", False))
        all_teacher = tokens is not None and (tf_flags is None or all(tf_flags)) and not sample
        probs_saved, done = [], False
        if all_teacher:
            fed, logits, pred = _dec_teacher_forced(buf, emb_w, tokens, w_out_c, b_out, opts.get("skip_pred"))
        elif hb.USE_FEEDBACK_KERNEL and not sample and V <= 128:
            fed, logits, pred, probs_saved, done = _dec_free_kernels(buf, emb_w, tokens, tf_flags, smooth, opts, w_out_c, b_out)
        else:
            fed, logits, pred, probs_saved = _dec_free_torch(buf, emb_w, tokens, tf_flags, smooth, sample, opts, w_out_c, b_out)
        ctx.lease = lease
        ctx.keep = (fed, probs_saved, w_out_c, emb_w)
        ctx.dims = (B, Tp, A, O, D, E, V, C, K, L, KX)
        ctx.smooth = smooth and tokens is None
        ctx.all_teacher = all_teacher
        # a scheduled-sampling sequence that ran in the persistent kernel takes the persistent backward as well: no gradient
        # flows through an argmax, the backward only needs what the forward saved (X, fed)
        ctx.free_persist = (not all_teacher) and done and not ctx.smooth
        ctx.smooth_scaling = float(opts.get("smooth_scaling", 1.0))
        if pred is not None:
            ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)       # an unused `ws` output arrives as None instead of a zero tensor + copy
        # the attention weights: in a training step a view of the leased workspace (valid until the next forward of the same
        # shape; nothing on the training path keeps them), a copy otherwise
        return logits, (buf.ws.detach() if pooled else buf.ws.clone()), pred

    @staticmethod
    @_with_saved_arith
    def backward(ctx, dlogits, dws, _dpred):
        fed, probs_saved, w_out, emb_w = ctx.keep
        B, Tp, A, O, D, E, V, C, K, L, KX = ctx.dims
        lease = ctx.lease
        assert lease is not None and lease.ws is not None, "decoder_sequence backward needs the leased workspace"
        buf = lease.ws
        X, Xd = buf.X, buf.Xd
        dev = X.device
        if dlogits is None:
            dlogits = torch.zeros(L, B, V, device=dev, dtype=torch.float32)
        dlog2 = dlogits.contiguous().view(L * B, V)
        zb = _ARENA.take((buf.zbuf.numel(),), dev)
        if zb is None:
            buf.zbuf.zero_()                   # G, dwext, dP, dcell, dgvec_part, dwatt_part, dconv_part
            acc = buf.acc
        else:                                  # ... or their places in the step's arena (zeroed with everything else)
            acc = buf.accumulators(zb)
        G = acc["G"]                           # (wcatT, wdecT: written by the forward's dec_pack)
        XO = X[1:].view(L * B, KX)[:, :D + O]
        hb.gemm(dlog2, w_out, out=G[1:].view(L * B, KX)[:, :D + O])
        dw_out = _gemm_acc(dlog2, XO, trans_a=True, shape=(V, D + O))
        db_out = _colsum_acc(dlog2)
        if dws is not None:
            buf.dws.copy_(dws)
        demb_w = zeros_acc(tuple(emb_w.shape), dev)
        if not ctx.smooth:
            hb.dec_seq_bwd(buf, acc, dws is not None, ctx.all_teacher or ctx.free_persist, ctx.all_teacher)
        elif torch.is_tensor(probs_saved):
            # the feedback's gradient reaches the logits inside the kernels; the weight gradients that depend on it are taken
            # once over the whole sequence afterwards
            dtot = hb.dec_smooth_bwd(buf, acc, dws is not None, w_out.contiguous(), emb_w.contiguous(), probs_saved,
                                     ctx.smooth_scaling, dlog2)
            dw_out = hb.gemm(dtot.view(L * B, V), XO, trans_a=True)
            db_out = hb.colsum(dtot.view(L * B, V))
            if L > 1:
                hb.gemm(probs_saved[:L - 1].view((L - 1) * B, V), G[1:L].view((L - 1) * B, KX)[:, D + O:], trans_a=True,
                        out=demb_w, accumulate=True, split_k=1)
        else:
            _dec_smooth_bwd_torch(buf, acc, dws is not None, w_out, emb_w, probs_saved, ctx.smooth_scaling, dw_out, db_out,
                                  demb_w)
        # deferred weight gradients: one GEMM each over the whole sequence
        dg2 = buf.dgates.view(L * B, 4 * D)
        Xin = X[:L] if Xd is None else Xd[:L]
        dwcat = _gemm_acc(dg2, Xin.reshape(L * B, KX), trans_a=True, shape=(4 * D, KX))     # [4D, KX] gate-interleaved rows
        dw_ih, dw_hh, dbias, dbias2 = hb.cell_unpack(dwcat, _colsum_acc(dg2), D, O, E)       # -> torch layout, one launch
        dwdec = _gemm_acc(buf.dD.view(L * B, A), X[1:].view(L * B, KX)[:, :D], trans_a=True, shape=(A, D))
        dgvec, dwatt, dconvw = hb.colsum_parts([acc["dgvec_part"], acc["dwatt_part"], acc["dconv_part"]])   # sums over utterances
        dgvec, dconvw = dgvec.view(1, A), dconvw.view(C, 1, 1, 2 * K + 1)
        # dQ[b] = ws[:, b, :]^T dctx[:, b, :]   (batched over utterances)
        dQ = torch.empty(B, Tp, O, device=dev, dtype=torch.float32)
        dctx_base = G[1:]                               # [L, B, KX], ctx grad at columns D:D+O
        hb.gemm_batched(buf.ws, dctx_base[:, :, D:], dQ, True, False, Tp, O, L, B * Tp, B * KX, O, B, Tp, KX,
                        Tp * O)
        dbo = _colsum_acc(dctx_base.view(L * B, KX)[:, D:D + O])
        # embedding gradient for token-fed steps: one launch over the embedding columns of G as they lie (fed = -1: a step
        # whose input was not a token)
        demb_all = G[:L, :, D + O:]
        nsteps = 1 if torch.is_tensor(probs_saved) else L     # smooth feedback: only step 0 was fed a token (<BOS>)
        if not hb.embedding_grad(fed[:nsteps].reshape(-1), G[:nsteps].view(nsteps * B, KX)[:, D + O:], demb_w):
            if torch.is_tensor(probs_saved):
                demb_w.index_add_(0, fed[0], demb_all[0])
            elif not probs_saved:    # every step was fed a token (decided on the host: no device sync here)
                demb_w.index_add_(0, fed.view(-1), demb_all.reshape(L * B, E))
            else:
                tokfed = fed >= 0
                demb_w.index_add_(0, fed[tokfed], demb_all[tokfed])
        dP = acc["dP"] if zb is not None else acc["dP"].clone()      # (an arena slice outlives the lease)
        lease.release()
        return (dP, dQ, demb_w, dw_ih, dw_hh, dbias, dbias2, dwdec, dconvw, dwatt, dgvec, dbo, dw_out, db_out,
                None, None)


class _LabelLogProb(torch.autograd.Function):
    """(1-ls) log_softmax(logits)[target] + ls sum_v labeldist_v log_softmax(logits)_v  (model.py:354-366) in one
    kernel each way.  logits [..., V] contiguous, index [...] long -> ([...], total, argmax): `total` (with_sum) is
    sum_scale times the sum of all outputs, accumulated by the same kernel - the training loss is that sum times a constant
    (solver.py:377; sum_scale = that constant makes `total` the loss itself), so neither a reduction kernel nor a multiply nor
    their backward follow; a gradient that arrives through `total` alone is one device scalar, broadcast by the backward
    kernel.  argmax (with_argmax): the row's argmax over V, long - the `prediction` output of model.py:346, read off the
    logits the kernel has in its registers anyway."""

    @staticmethod
    def forward(ctx, logits, index, labeldist, ls_weight, with_sum, sum_scale, with_argmax):
        lg = logits.contiguous()
        V = lg.shape[-1]
        rows = lg.numel() // V
        idx = index.contiguous()
        out = torch.empty(lg.shape[:-1], device=lg.device, dtype=torch.float32)
        total = zeros_acc((1,), lg.device).view(()) if with_sum else None
        amax = torch.empty(lg.shape[:-1], device=lg.device, dtype=torch.long) if with_argmax else None
        dist = labeldist.contiguous() if labeldist is not None else None
        det = total is not None and hb.is_deterministic()       # the kernel's own total is one atomic per block: summed behind it
        hb.check(hb.load().asr_label_logprob_fwd(rows, V, hb.ptr(lg), V, ctypes.c_void_p(idx.data_ptr()), hb.ptr(dist),
                                                 float(ls_weight), hb.ptr(out), None if det else hb.ptr(total), float(sum_scale),
                                                 None if amax is None else ctypes.c_void_p(amax.data_ptr()), hb.stream()),
                 "asr_label_logprob_fwd")
        if det:
            hb.sum_det(out, total, sum_scale)
        ctx.save_for_backward(lg, idx, dist)
        ctx.ls, ctx.sum_scale = float(ls_weight), float(sum_scale)
        ctx.set_materialize_grads(False)
        if amax is not None:
            ctx.mark_non_differentiable(amax)
        return out, total, amax

    @staticmethod
    def backward(ctx, g, gt, _gamax):
        lg, idx, dist = ctx.saved_tensors
        V = lg.shape[-1]
        rows = lg.numel() // V
        if g is None and gt is None:
            return (None,) * 7
        if g is None:
            gc, stride, scale = gt.contiguous(), 0, ctx.sum_scale       # d(total) alone: one scalar for every row
        else:
            gc, stride, scale = (g if gt is None else g + gt * ctx.sum_scale).contiguous(), 1, 1.0
        dz = torch.empty_like(lg)
        hb.check(hb.load().asr_label_logprob_bwd(rows, V, hb.ptr(lg), V, ctypes.c_void_p(idx.data_ptr()), hb.ptr(dist),
                                                 ctx.ls, hb.ptr(gc), stride, scale, hb.ptr(dz), V, hb.stream()),
                 "asr_label_logprob_bwd")
        return (dz,) + (None,) * 6


def label_logprob(logits, index, labeldist=None, ls_weight=0.0, with_sum=False, sum_scale=1.0, with_argmax=False):
    """-> out, + total (with_sum), + argmax (with_argmax)."""
    out, total, amax = _LabelLogProb.apply(logits, index, labeldist, ls_weight, with_sum, sum_scale, with_argmax)
    res = (out,) + ((total,) if with_sum else ()) + ((amax,) if with_argmax else ())
    return res if len(res) > 1 else out


class _CtcLoss(torch.autograd.Function):
    """CTC negative log-likelihood per utterance of RAW logits [B, T', V] (blank = 0; the log-softmax is the kernel's) ->
    nll [B]: asr_ctc_loss_fwd / _bwd (csrc/ctc.hip), two launches each way.  The workspace (alpha, the per-frame
    log-sum-exps, the sorted label positions) is leased from the pool from the forward to the end of the backward, like the
    other sequence operators'; without autograd a fresh tensor.  Ordered sums only: nothing here depends on
    hb.is_deterministic().  No host synchronisation: the label lengths are host integers already."""

    @staticmethod
    def forward(ctx, logits, frame_lens, labels, label_lens, zero_infinity):
        B, T, V = logits.shape
        # a [B, T, V] view of a wider row-major buffer goes in as it is (row stride = ld)
        if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1)):
            logits = logits.contiguous()
        ld = logits.stride(1)
        lens = [int(n) for n in label_lens]
        if len(lens) != B:
            raise ValueError("ctc_loss: %d label lengths for %d utterances" % (len(lens), B))
        offsets = [0]
        for n in lens:
            offsets.append(offsets[-1] + n)
        if offsets[-1] != labels.numel():
            raise ValueError("ctc_loss: the label lengths sum to %d, the packed labels hold %d" % (offsets[-1], labels.numel()))
        lmax = max(lens)
        dev = logits.device
        words = (hb.ctc_ws_bytes(B, T, V, lmax) + 3) // 4
        if ctx.needs_input_grad[0]:                  # (grad mode is off inside forward: ask the node)
            cap = _row_capacity(words)
            ctx.lease = _POOL.acquire(("ctc", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
            ws = ctx.lease.ws
        else:
            ctx.lease, ws = None, torch.empty(words, device=dev, dtype=torch.float32)
        offs_dev = hb.to_device_i32(offsets, dev)
        # (a batch of empty transcripts has no label to point at: the library wants a pointer all the same)
        labels = labels.contiguous() if labels.numel() else torch.zeros(1, device=dev, dtype=torch.long)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        hb.ctc_loss_fwd(logits, ld, frame_lens, labels, offs_dev, lmax, zero_infinity, nll, ws)
        ctx.save_for_backward(logits, frame_lens, labels, offs_dev)
        ctx.ld, ctx.lmax, ctx.zero_infinity = ld, lmax, bool(zero_infinity)
        return nll

    @staticmethod
    def backward(ctx, g):
        logits, frame_lens, labels, offs_dev = ctx.saved_tensors
        if ctx.lease is None or ctx.lease.ws is None:
            raise RuntimeError("ctc_loss: the backward runs once, behind a forward that ran with autograd enabled")
        B, T, V = logits.shape
        dz = torch.empty(B, T, V, device=logits.device, dtype=torch.float32)
        hb.ctc_loss_bwd(logits, ctx.ld, frame_lens, labels, offs_dev, ctx.lmax, ctx.zero_infinity, g.contiguous(),
                        ctx.lease.ws, dz, V)
        ctx.lease.release()
        return dz, None, None, None, None


def ctc_loss(logits, frame_lens_dev, labels_packed, label_lens, zero_infinity=True):
    """-> nll [B], the CTC negative log-likelihood of each utterance.  logits [B, T', V] fp32 raw (not log-softmaxed),
    frame_lens_dev int32 [B] on the device (Encoder.last_lens_dev), labels_packed the batch's labels as ONE int64 device
    tensor, label_lens their counts per utterance (host integers).  Blank = 0.  zero_infinity: an utterance without any
    alignment gives loss 0 and a zero gradient (torch.nn.functional.ctc_loss's flag); otherwise +inf."""
    return _CtcLoss.apply(logits, frame_lens_dev, labels_packed, label_lens, zero_infinity)


class _CtcStarLoss(torch.autograd.Function):
    """Star CTC negative log path sum per utterance of RAW logits [B, T', V] -> nll [B]: asr_ctc_star_loss_fwd / _bwd
    (csrc/ctc_star.hip), three launches forward and two backward.  _CtcLoss with one more input, the per-row
    penalty (fp32 [B] on the device; no gradient flows to it): the same pooled workspace lease from the forward to the end of
    the backward, ordered sums only, no host synchronisation."""

    @staticmethod
    def forward(ctx, logits, frame_lens, labels, label_lens, penalty, zero_infinity):
        B, T, V = logits.shape
        if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1)):
            logits = logits.contiguous()
        ld = logits.stride(1)
        lens, offsets, lmax = _label_offsets("ctc_star_loss", label_lens, B, labels.numel())
        dev = logits.device
        words = (hb.ctc_star_ws_bytes(B, T, V, lmax) + 3) // 4
        if ctx.needs_input_grad[0]:
            cap = _row_capacity(words)
            ctx.lease = _POOL.acquire(("ctc_star", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
            ws = ctx.lease.ws
        else:
            ctx.lease, ws = None, torch.empty(words, device=dev, dtype=torch.float32)
        offs_dev = hb.to_device_i32(offsets, dev)
        labels = labels.contiguous() if labels.numel() else torch.zeros(1, device=dev, dtype=torch.long)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        hb.ctc_star_loss_fwd(logits, ld, frame_lens, labels, offs_dev, lmax, penalty, zero_infinity, nll, ws)
        ctx.save_for_backward(logits, frame_lens, labels, offs_dev, penalty)
        ctx.ld, ctx.lmax, ctx.zero_infinity = ld, lmax, bool(zero_infinity)
        return nll

    @staticmethod
    def backward(ctx, g):
        logits, frame_lens, labels, offs_dev, penalty = ctx.saved_tensors
        if ctx.lease is None or ctx.lease.ws is None:
            raise RuntimeError("ctc_star_loss: the backward runs once, behind a forward that ran with autograd enabled")
        B, T, V = logits.shape
        dz = torch.empty(B, T, V, device=logits.device, dtype=torch.float32)
        hb.ctc_star_loss_bwd(logits, ctx.ld, frame_lens, labels, offs_dev, ctx.lmax, penalty, ctx.zero_infinity,
                             g.contiguous(), ctx.lease.ws, dz, V)
        ctx.lease.release()
        return dz, None, None, None, None, None


def ctc_star_loss(logits, frame_lens_dev, labels_packed, label_lens, penalty, zero_infinity=True):
    """-> nll [B]: the star CTC loss of each utterance, for transcripts with missing words (after Star Temporal
    Classification, Pratap et al. 2022).  The arguments are ctc_loss's plus `penalty`: between any two labels, before the
    first and behind the last the lattice may spend frames in a star state that emits "any non-blank token" at
    log p(non-blank) + penalty per frame.  penalty is a Python float for every row or an fp32 [B] tensor, each value <= 0 or
    -inf; ValueError for a positive or NaN value (a tensor on the GPU is read back once for that check: pass a float or a host
    tensor where that matters).  -inf closes the star states of a row - the plain CTC lattice; a float -inf or None calls
    ctc_loss itself.
    The value is the negative log PATH SUM of the star lattice, not a normalised probability: a frame's token may count both
    as a label and as a star, so nll may be negative when the penalty is near 0, and nll <= the CTC nll always.  Infeasible
    rows and zero_infinity as in ctc_loss (a row without frames is infeasible whatever its labels).  No gradient flows to
    penalty."""
    if penalty is None:
        return ctc_loss(logits, frame_lens_dev, labels_packed, label_lens, zero_infinity)
    B = logits.shape[0]
    if torch.is_tensor(penalty):
        host = penalty.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
        if host.numel() != B:
            raise ValueError("ctc_star_loss: %d penalties for %d utterances" % (host.numel(), B))
        if bool((torch.isnan(host) | (host > 0)).any()):
            raise ValueError("ctc_star_loss: every penalty must be <= 0 (or -inf), got %r" % (host.tolist(),))
        pen = penalty.detach().to(device=logits.device, dtype=torch.float32).reshape(B).contiguous()
    else:
        p = float(penalty)
        if p != p or p > 0:
            raise ValueError("ctc_star_loss: the penalty must be <= 0 (or -inf), got %r" % (penalty,))
        if p == float("-inf"):
            return ctc_loss(logits, frame_lens_dev, labels_packed, label_lens, zero_infinity)
        pen = torch.full((B,), p, device=logits.device, dtype=torch.float32)
    return _CtcStarLoss.apply(logits, frame_lens_dev, labels_packed, label_lens, pen, zero_infinity)


class _GtcLoss(torch.autograd.Function):
    """Graph CTC negative log path sum per utterance of RAW logits [B, T', V] -> nll [B]: asr_gtc_loss_fwd / _bwd
    (csrc/gtc.hip), two launches forward and two backward.  _CtcStarLoss with a graph table in place of the
    labels: the same pooled workspace lease from the forward to the end of the backward, ordered sums only, no host
    synchronisation."""

    @staticmethod
    def forward(ctx, logits, frame_lens, table, zero_infinity):
        B, T, V = logits.shape
        if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1)):
            logits = logits.contiguous()
        ld = logits.stride(1)
        dev = logits.device
        words = (hb.gtc_ws_bytes(B, T, V, table.max_nodes) + 3) // 4
        if ctx.needs_input_grad[0]:
            cap = _row_capacity(words)
            ctx.lease = _POOL.acquire(("gtc", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
            ws = ctx.lease.ws
        else:
            ctx.lease, ws = None, torch.empty(words, device=dev, dtype=torch.float32)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        hb.gtc_loss_fwd(logits, ld, frame_lens, table, zero_infinity, nll, ws)
        ctx.save_for_backward(logits, frame_lens)
        ctx.table, ctx.ld, ctx.zero_infinity = table, ld, bool(zero_infinity)
        return nll

    @staticmethod
    def backward(ctx, g):
        logits, frame_lens = ctx.saved_tensors
        if ctx.lease is None or ctx.lease.ws is None:
            raise RuntimeError("gtc_loss: the backward runs once, behind a forward that ran with autograd enabled")
        B, T, V = logits.shape
        dz = torch.empty(B, T, V, device=logits.device, dtype=torch.float32)
        hb.gtc_loss_bwd(logits, ctx.ld, frame_lens, ctx.table, ctx.zero_infinity, g.contiguous(), ctx.lease.ws, dz, V)
        ctx.lease.release()
        return dz, None, None, None


def gtc_loss(logits, frame_lens_dev, graphs, zero_infinity=True):
    """-> nll [B]: the graph CTC loss of each utterance (GTC, Moritz et al. 2021) - the supervision of a row is
    a label graph (gtc.py): the plain CTC lattice (gtc.Graph.ctc), an n-best list with a weight per hypothesis
    (Graph.from_nbest), a confusion network (Graph.from_confusion) or any Graph.  `graphs` is one gtc.Graph for every row or a
    gtc.GraphBatch that names a graph per row; it is compiled and uploaded once per object and device.  The other arguments
    are ctc_loss's: raw logits [B, T', V] (a strided view with a row stride >= V is taken as it is), the frame lengths on the
    device.
    The value is the negative log PATH SUM of the graph, start + emissions + arc weights + final weight summed over all node
    paths of the row's frame count - not a normalised probability: the weights are any log numbers, and two paths may spell
    the same tokens.  A row with no path of finite score, or without frames, counts as 0 with zero_infinity and as +inf
    without; its gradient is zero either way.  No gradient flows to the arc, start or final weights.  UnsupportedShape for a
    graph above hb.GTC_MAX_NODES nodes, ValueError where the graphs do not fit the batch.
    `graphs` may also be the gtc.DeviceGraphTable of gtc_nbest_graphs, one graph per row: whether it fits
    the call is decided from its host-known V and row count, nothing of it is read back."""
    import gtc
    if not isinstance(graphs, (gtc.Graph, gtc.GraphBatch, gtc.DeviceGraphTable)):
        raise ValueError("gtc_loss: graphs must be a gtc.Graph, a gtc.GraphBatch or a gtc.DeviceGraphTable, got %r"
                         % type(graphs).__name__)
    B, _, V = logits.shape
    if graphs.V != V:
        raise ValueError("gtc_loss: the graphs are over %d tokens, the logits over %d" % (graphs.V, V))
    if isinstance(graphs, gtc.GraphBatch) and graphs.graph_of.size != B:
        raise ValueError("gtc_loss: the batch lists a graph for %d utterances, the call has %d" % (graphs.graph_of.size, B))
    if isinstance(graphs, gtc.DeviceGraphTable) and graphs.G != B:
        raise ValueError("gtc_loss: the table holds a graph for %d utterances, the call has %d" % (graphs.G, B))
    return _GtcLoss.apply(logits, frame_lens_dev, graphs.to(logits.device), zero_infinity)


def gtc_nbest_graphs(hyp, hyp_len, score, V, temperature=1.0):
    """-> gtc.DeviceGraphTable: the n-best list of ctc_beam - hyp int32 [B, K, L] padded with -1, hyp_len int32 [B, K] with -1
    in dead slots, score fp32 [B, K] with -inf in dead slots, all on the device - compiled into one prefix-tree graph per row
    on the device (asr_nbest_gtc_f32, csrc/gtc_nbest.hip; two launches, no host synchronisation).  For every row
    the table holds what gtc.Graph.from_nbest and the host compiler make of the same list, element for element, with the
    log-softmax of temperature * score over the row's live slots as weights (gtc.nbest_weights, float64 on the device); a row
    without a live slot gets the empty hypothesis at weight 0.  A tree above 1023 trie nodes cannot raise on the device:
    hypotheses are admitted in rank order while the tree fits, the first that does not and every slot behind it are dropped
    and the weights renormalised over the admitted ones.  The table carries .dropped int32 [B] (live slots lost) and
    .log_weights float64 [B, K] (-inf in dead and dropped slots) as device tensors and goes to gtc_loss / E2E.gtc_nll as it
    is.  The tokens of live hypotheses are trusted to lie in 1 .. V-1, as ctc_beam writes them.  ValueError for a
    temperature that is negative or not finite; UnsupportedShape for K above hb.BEAM_KMAX."""
    import gtc
    t = float(temperature)
    if not (0.0 <= t < float("inf")):
        raise ValueError("gtc_nbest_graphs: the temperature must be finite and >= 0, got %r" % (temperature,))
    if hyp.dim() != 3 or tuple(hyp_len.shape) != tuple(hyp.shape[:2]) or tuple(score.shape) != tuple(hyp.shape[:2]):
        raise ValueError("gtc_nbest_graphs: hyp [B, K, L] with hyp_len and score [B, K], got %s, %s, %s"
                         % (tuple(hyp.shape), tuple(hyp_len.shape), tuple(score.shape)))
    B, K, L = hyp.shape
    dev = hyp.device
    cap_nodes, cap_arcs, ws_bytes = hb.gtc_nbest_bytes(B, K, L, int(V))
    table = gtc.DeviceGraphTable(int(V), B, cap_nodes, cap_arcs, dev)
    table.log_weights = torch.empty(B, K, device=dev, dtype=torch.float64)
    table.dropped = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty((ws_bytes + 3) // 4, device=dev, dtype=torch.int32)
    hb.gtc_nbest(hyp.contiguous(), hyp_len.contiguous(), score.contiguous(), t, table, table.log_weights, table.dropped, ws)
    return table


def _label_offsets(what, label_lens, B, n_labels=None):
    """Host label counts -> (counts, offsets [B + 1], the largest count); ValueError where they do not fit the batch."""
    lens = [int(n) for n in label_lens]
    if len(lens) != B:
        raise ValueError("%s: %d label lengths for %d utterances" % (what, len(lens), B))
    offsets = [0]
    for n in lens:
        if n < 0:
            raise ValueError("%s: a negative label length" % what)
        offsets.append(offsets[-1] + n)
    if n_labels is not None and offsets[-1] != n_labels:
        raise ValueError("%s: the label lengths sum to %d, the packed labels hold %d" % (what, offsets[-1], n_labels))
    return lens, offsets, max(lens)


class _RnntJoint(torch.autograd.Function):
    """The transducer's joint activations Z [B, T, U + 1, J] = tanh(PE [B, T, J] + PP [B, U + 1, J]) on every utterance's
    lattice, exact zeros on padding: asr_rnnt_joint_fwd_f32 / _bwd_f32 (csrc/rnnt.hip), one launch each way.  Z is the memory
    cost of the head - 4 B T (U + 1) J bytes - and is leased from the pool from the forward to the end of the backward like
    the other sequence workspaces (the output aliases it: valid until this node's backward has run); without autograd a
    fresh tensor.  Ordered sums only, no host synchronisation."""

    @staticmethod
    def forward(ctx, pe, pp, frame_lens, label_lens):
        B, T, J = pe.shape
        _, offsets, umax = _label_offsets("rnnt_joint", label_lens, B)
        if tuple(pp.shape) != (B, umax + 1, J):
            raise ValueError("rnnt_joint: pp is %s, the labels need [%d, %d, %d]" % (tuple(pp.shape), B, umax + 1, J))
        hb.rnnt_ws_bytes(B, T, umax, J, 2)           # (UnsupportedShape before anything is leased or written)
        dev = pe.device
        pe, pp = pe.contiguous(), pp.contiguous()
        n = B * T * (umax + 1) * J
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            cap = _row_capacity(n)
            ctx.lease = _POOL.acquire(("rnnt_z", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
            z = ctx.lease.ws[:n].view(B, T, umax + 1, J)
        else:
            ctx.lease, z = None, torch.empty(B, T, umax + 1, J, device=dev, dtype=torch.float32)
        offs_dev = hb.to_device_i32(offsets, dev)
        hb.rnnt_joint_fwd(pe, pp, frame_lens, offs_dev, z)
        ctx.save_for_backward(frame_lens, offs_dev)
        ctx.dims = (B, T, umax, J)
        return z.detach()

    @staticmethod
    def backward(ctx, dz):
        frame_lens, offs_dev = ctx.saved_tensors
        if ctx.lease is None or ctx.lease.ws is None:
            raise RuntimeError("rnnt_joint: the backward runs once, behind a forward that ran with autograd enabled")
        B, T, umax, J = ctx.dims
        z = ctx.lease.ws[:B * T * (umax + 1) * J].view(B, T, umax + 1, J)
        dpe = torch.empty(B, T, J, device=dz.device, dtype=torch.float32)
        dpp = torch.empty(B, umax + 1, J, device=dz.device, dtype=torch.float32)
        hb.rnnt_joint_bwd(dz.contiguous(), z, frame_lens, offs_dev, dpe, dpp)
        ctx.lease.release()
        return dpe, dpp, None, None


def rnnt_joint(pe, pp, frame_lens_dev, label_lens):
    """-> Z [B, T, U + 1, J] = tanh(pe[b, t] + pp[b, u]) for t < T_b, u <= U_b, exact zeros elsewhere.  pe
    [B, T, J] and pp [B, U + 1, J] fp32 (the two projections, from ops.linear), frame_lens_dev int32 [B] on the device
    (Encoder.last_lens_dev), label_lens the label counts per utterance (host integers; U = their maximum).  J a multiple of
    4: hb.UnsupportedShape otherwise."""
    return _RnntJoint.apply(pe, pp, frame_lens_dev, label_lens)


class _RnntLoss(torch.autograd.Function):
    """Transducer negative log-likelihood per utterance of RAW logits [B, T, U + 1, V] (blank = 0; the log-softmax is the
    kernel's) -> nll [B]: asr_rnnt_loss_fwd_f32 / _bwd_f32 (csrc/rnnt.hip), two launches each way.  The workspace (the node
    log-sum-exps, alpha, beta) is leased from the pool from the forward to the end of the backward, like _CtcLoss's; without
    autograd a fresh tensor.  Ordered sums only: nothing here depends on hb.is_deterministic().  No host synchronisation."""

    @staticmethod
    def forward(ctx, logits, frame_lens, labels, label_lens):
        B, T, U1, V = logits.shape
        # a [B, T, U + 1, V] view of a wider row-major buffer goes in as it is (row stride = ld)
        ld = logits.stride(2)
        if not (logits.stride(3) == 1 and ld >= V and logits.stride(1) == U1 * ld and logits.stride(0) == T * U1 * ld):
            logits = logits.contiguous()
            ld = V
        _, offsets, umax = _label_offsets("rnnt_loss", label_lens, B, labels.numel())
        if umax + 1 != U1:
            raise ValueError("rnnt_loss: the logits hold %d label positions, the longest transcript needs %d" % (U1, umax + 1))
        dev = logits.device
        words = (hb.rnnt_ws_bytes(B, T, umax, 4, V) + 3) // 4
        if ctx.needs_input_grad[0]:                  # (grad mode is off inside forward: ask the node)
            cap = _row_capacity(words)
            ctx.lease = _POOL.acquire(("rnnt", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
            ws = ctx.lease.ws
        else:
            ctx.lease, ws = None, torch.empty(words, device=dev, dtype=torch.float32)
        offs_dev = hb.to_device_i32(offsets, dev)
        # (a batch of empty transcripts has no label to point at: the library wants a pointer all the same)
        labels = labels.contiguous() if labels.numel() else torch.zeros(1, device=dev, dtype=torch.long)
        nll = torch.empty(B, device=dev, dtype=torch.float32)
        hb.rnnt_loss_fwd(logits, ld, frame_lens, labels, offs_dev, nll, ws)
        ctx.save_for_backward(logits, frame_lens, labels, offs_dev)
        ctx.ld = ld
        return nll

    @staticmethod
    def backward(ctx, g):
        logits, frame_lens, labels, offs_dev = ctx.saved_tensors
        if ctx.lease is None or ctx.lease.ws is None:
            raise RuntimeError("rnnt_loss: the backward runs once, behind a forward that ran with autograd enabled")
        B, T, U1, V = logits.shape
        dz = torch.empty(B, T, U1, V, device=logits.device, dtype=torch.float32)
        hb.rnnt_loss_bwd(logits, ctx.ld, frame_lens, labels, offs_dev, g.contiguous(), ctx.lease.ws, dz, V)
        ctx.lease.release()
        return dz, None, None, None


def rnnt_loss(logits, frame_lens_dev, labels_packed, label_lens):
    """-> nll [B], the transducer negative log-likelihood of each utterance.  logits [B, T, U + 1, V] fp32 raw
    (not log-softmaxed; a view with row stride >= V is taken as it is), frame_lens_dev int32 [B] on the device
    (Encoder.last_lens_dev; an encoder gives every T_b >= 1), labels_packed the batch's labels as ONE int64 device tensor,
    label_lens their counts per utterance (host integers; U = their maximum).  Blank = 0.  Every utterance with a frame has
    an alignment: there is no zero_infinity case.  A row the kernels cannot score - T_b = 0, or a label outside [1, V) -
    gives nll = +inf and an exact-zero gradient for that row alone (lengths and labels live on the device: no host check,
    no synchronisation); the other rows are not affected."""
    return _RnntLoss.apply(logits, frame_lens_dev, labels_packed, label_lens)


class _MwerLoss(torch.autograd.Function):
    """The expected number of edit errors over the n-best list (csrc/mwer.hip): logits [L, R, V] RAW, time-major, R = B K rows
    -> (loss, seq_logp [R], post [R], risk [B], coef [R]); only `loss` carries a gradient.  Two launches forward, one
    backward; the backward recomputes the rows' softmax from the saved logits and reads the saved coef.  Ordered sums only:
    nothing here depends on hb.is_deterministic().  No host synchronisation."""

    @staticmethod
    def forward(ctx, logits, tokens_lb, npos, err, B, scale):
        L, R, V = logits.shape
        if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == R * logits.stride(1)):
            logits = logits.contiguous()
        dev = logits.device
        tokens_lb, npos, err = tokens_lb.contiguous(), npos.contiguous(), err.contiguous()
        out = torch.empty(3 * R + int(B) + 1, device=dev, dtype=torch.float32)
        seq_logp, post, coef, risk, loss = out[:R], out[R:2 * R], out[2 * R:3 * R], out[3 * R:3 * R + B], out[3 * R + B:]
        ws = torch.empty(L * R, device=dev, dtype=torch.float32)
        hb.mwer_fwd(logits, tokens_lb, npos, err, B, scale, seq_logp, post, coef, risk, loss, ws)
        ctx.save_for_backward(logits, tokens_lb, npos, coef)
        ctx.B, ctx.scale = int(B), float(scale)
        ctx.mark_non_differentiable(seq_logp, post, risk, coef)
        return loss.view(()), seq_logp, post, risk, coef

    @staticmethod
    def backward(ctx, g, *_unused):
        logits, tokens_lb, npos, coef = ctx.saved_tensors
        dz = torch.empty(logits.shape, device=logits.device, dtype=torch.float32)
        hb.mwer_bwd(logits, tokens_lb, npos, coef, ctx.B, g.contiguous(), ctx.scale, dz)
        return dz, None, None, None, None, None


def mwer_loss(logits, tokens_lb, npos, err, scale, n_utts=None):
    """-> (loss, parts): loss = scale * sum_b risk_b, a device scalar with the graph behind it; parts = dict(seq_logp [R],
    post [R], risk [B], coef [R]) without one.  logits [L, R, V] fp32 raw, time-major (ops.decoder_sequence's), rows
    r = b K + k; tokens_lb int64 [L, R] (each hypothesis with its <EOS>, <EOS>-padded); npos int32 [R] (len + 1; <= 0: an
    unused slot); err int32 [R] (edit distances); scale: the caller's 1 / B.  n_utts: B (default round(1 / scale))."""
    B = int(n_utts) if n_utts is not None else int(round(1.0 / float(scale)))
    loss, seq_logp, post, risk, coef = _MwerLoss.apply(logits, tokens_lb, npos, err, B, float(scale))
    return loss, dict(seq_logp=seq_logp, post=post, risk=risk, coef=coef)


class CtcAlignment(object):
    """What ops.ctc_align returns, every field a device tensor: path int32 [B, T'] (the token of each encoder frame, 0 =
    blank, -1 behind the utterance and in every frame of an infeasible one), score fp32 [B] (the best alignment's
    log-probability, -inf: infeasible), and packed like the labels first / last int32 (the inclusive frames of label i, -1:
    infeasible) and token_logp fp32 (the log-probability the path gives label i over its frames); offsets int32 [B + 1]
    (utterance b owns [offsets[b], offsets[b + 1]) of the packed fields) with label_lens, the host's counts."""

    __slots__ = ("path", "score", "first", "last", "token_logp", "offsets", "label_lens")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def ctc_align(logits, frame_lens_dev, labels_packed, label_lens):
    """-> CtcAlignment: the best CTC alignment (Viterbi) of each utterance's labels, asr_ctc_align_f32 (csrc/ctc_align.hip,
    DESIGN 4.16), two launches.  The arguments are ops.ctc_loss's: logits [B, T', V] fp32 raw, frame_lens_dev int32 [B] on
    the device, labels_packed ONE int64 device tensor, label_lens host integers; blank = 0.  Forward only: logits that
    require grad are accepted and nothing is recorded.  No host synchronisation."""
    logits = logits.detach()
    B, T, V = logits.shape
    lens = [int(n) for n in label_lens]
    if len(lens) != B:
        raise ValueError("ctc_align: %d label lengths for %d utterances" % (len(lens), B))
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    if offsets[-1] != labels_packed.numel():
        raise ValueError("ctc_align: the label lengths sum to %d, the packed labels hold %d" % (offsets[-1], labels_packed.numel()))
    lmax, total, dev = max(lens), offsets[-1], logits.device
    ws = torch.empty((hb.ctc_align_ws_bytes(B, T, V, lmax) + 3) // 4, device=dev, dtype=torch.float32)
    offs_dev = hb.to_device_i32(offsets, dev)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    out = CtcAlignment(path=torch.empty(B, T, **i32), score=torch.empty(B, **f32), first=torch.empty(total, **i32),
                       last=torch.empty(total, **i32), token_logp=torch.empty(total, **f32), offsets=offs_dev, label_lens=lens)
    hb.ctc_align(logits, frame_lens_dev, labels_packed.contiguous(), offs_dev, lmax, out.path, out.score, out.first, out.last,
                 out.token_logp, ws)
    return out


class CtcSegmentation(object):
    """What ops.ctc_segment returns, every field a device tensor: path int32 [B, T'] (the token of each encoder frame, 0 =
    blank, -2 outside the text with free ends, -1 behind the recording and in every frame of an infeasible one), score fp32
    [B], first / last int32 and token_logp fp32 packed like the labels, offsets int32 [B + 1] (CtcAlignment's fields, per
    recording); and per utterance, packed [N] in the order of the recordings: utt_begin / utt_end int32 (inclusive encoder
    frames; -1: no labels, or infeasible), utt_logp fp32 (the path's log-probability over begin .. end), utt_conf fp32 (the
    lowest window mean of the path's frame log-probabilities; both 0 without labels, -inf when infeasible); utt_offsets int32
    [N + 1] (utterance u owns [utt_offsets[u], utt_offsets[u + 1]) of the packed label fields) and rec_utts int32 [B + 1]
    (recording b owns the utterances rec_utts[b] .. rec_utts[b + 1] - 1); utt_lens: the host's counts."""

    __slots__ = ("path", "score", "first", "last", "token_logp", "offsets", "utt_begin", "utt_end", "utt_logp", "utt_conf",
                 "utt_offsets", "rec_utts", "utt_lens")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def ctc_segment(logits, frame_lens_dev, labels_packed, utt_lens, *, free_ends=True, window=30):
    """-> CtcSegmentation: CTC segmentation (Kuerzinger et al. 2020) of each recording against its transcript,
    asr_ctc_segment_f32 (csrc/ctc_segment.hip), two launches.  logits [B, T', V] fp32 raw, frame_lens_dev int32
    [B] on the device, labels_packed ONE int64 device tensor (every recording's utterances one after the other), utt_lens a
    list per recording of the label counts of its utterances; blank = 0.  free_ends: the audio before the first and after the
    last label costs nothing (False: ops.ctc_align's alignment, bit for bit, up to hb.CTC_SEG_MAX_LABELS labels); window: the
    frames per block of the confidence.  Forward only: logits that require grad are accepted and nothing is recorded.  No host
    synchronisation."""
    logits = logits.detach()
    B, T, V = logits.shape
    counts = [[int(n) for n in rec] for rec in utt_lens]
    if len(counts) != B:
        raise ValueError("ctc_segment: utterance counts for %d recordings, the logits hold %d" % (len(counts), B))
    if int(window) < 1:
        raise ValueError("ctc_segment: window %d (at least 1 frame)" % int(window))
    offsets, utt_offsets, rec_utts = [0], [0], [0]
    for rec in counts:
        for n in rec:
            if n < 0:
                raise ValueError("ctc_segment: an utterance of %d labels" % n)
            utt_offsets.append(utt_offsets[-1] + n)
        offsets.append(utt_offsets[-1])
        rec_utts.append(len(utt_offsets) - 1)
    if offsets[-1] != labels_packed.numel():
        raise ValueError("ctc_segment: the utterance lengths sum to %d, the packed labels hold %d"
                         % (offsets[-1], labels_packed.numel()))
    lmax = max(offsets[b + 1] - offsets[b] for b in range(B))
    total, N, dev = offsets[-1], len(utt_offsets) - 1, logits.device
    ws = torch.empty((hb.ctc_segment_ws_bytes(B, T, V, lmax) + 3) // 4, device=dev, dtype=torch.float32)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    out = CtcSegmentation(path=torch.empty(B, T, **i32), score=torch.empty(B, **f32), first=torch.empty(total, **i32),
                          last=torch.empty(total, **i32), token_logp=torch.empty(total, **f32),
                          offsets=hb.to_device_i32(offsets, dev), utt_begin=torch.empty(N, **i32), utt_end=torch.empty(N, **i32),
                          utt_logp=torch.empty(N, **f32), utt_conf=torch.empty(N, **f32),
                          utt_offsets=hb.to_device_i32(utt_offsets, dev), rec_utts=hb.to_device_i32(rec_utts, dev), utt_lens=counts)
    hb.ctc_segment(logits, frame_lens_dev, labels_packed.contiguous(), out.offsets, lmax, free_ends, out.utt_offsets,
                   out.rec_utts, int(window), out.path, out.score, out.first, out.last, out.token_logp, out.utt_begin,
                   out.utt_end, out.utt_logp, out.utt_conf, ws)
    return out


class RnntAlignment(object):
    """What ops.rnnt_align returns, every field a device tensor: score fp32 [B] (the best alignment's log-probability, -inf:
    the row cannot be aligned), packed like the labels emit_frame int32 (the encoder frame on which label i is emitted, -1:
    not aligned) and token_logp fp32 (the log-probability of that emission), frame_labels int32 [B, T'] (the labels emitted
    up to and including frame t, -1 behind the utterance) and blank_logp fp32 [B, T'] (the log-probability of the blank that
    leaves frame t, 0 behind the utterance); offsets int32 [B + 1] (utterance b owns [offsets[b], offsets[b + 1]) of the
    packed fields) with label_lens, the host's counts."""

    __slots__ = ("score", "emit_frame", "token_logp", "frame_labels", "blank_logp", "offsets", "label_lens")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def rnnt_align(logits, frame_lens_dev, labels_packed, label_lens):
    """-> RnntAlignment: the best alignment (Viterbi) of each utterance's labels on the transducer lattice,
    asr_transducer_align_f32 (csrc/rnnt_align.hip), two launches.  The arguments are ops.rnnt_loss's: logits
    [B, T', U + 1, V] fp32 raw (a view with row stride >= V is taken as it is), frame_lens_dev int32 [B] on the device,
    labels_packed ONE int64 device tensor, label_lens host integers (U = their maximum); blank = 0, and the blank
    predecessor wins a tie.  Forward only: logits that require grad are accepted and nothing is recorded.  No host
    synchronisation."""
    logits = logits.detach()
    B, T, U1, V = logits.shape
    ld = logits.stride(2)
    if not (logits.stride(3) == 1 and ld >= V and logits.stride(1) == U1 * ld and logits.stride(0) == T * U1 * ld):
        logits, ld = logits.contiguous(), V
    lens, offsets, umax = _label_offsets("rnnt_align", label_lens, B, labels_packed.numel())
    if umax + 1 != U1:
        raise ValueError("rnnt_align: the logits hold %d label positions, the longest transcript needs %d" % (U1, umax + 1))
    total, dev = offsets[-1], logits.device
    ws = torch.empty((hb.rnnt_align_ws_bytes(B, T, umax, V) + 3) // 4, device=dev, dtype=torch.float32)
    offs_dev = hb.to_device_i32(offsets, dev)
    # (a batch of empty transcripts has no label to point at: the library wants a pointer all the same)
    labels = labels_packed.contiguous() if total else torch.zeros(1, device=dev, dtype=torch.long)
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    out = RnntAlignment(score=torch.empty(B, **f32), emit_frame=torch.empty(total, **i32), token_logp=torch.empty(total, **f32),
                        frame_labels=torch.empty(B, T, **i32), blank_logp=torch.empty(B, T, **f32), offsets=offs_dev,
                        label_lens=lens)
    hb.rnnt_align(logits, ld, frame_lens_dev, labels, offs_dev, out.score, out.emit_frame, out.token_logp, out.frame_labels,
                  out.blank_logp, ws)
    return out


def ctc_greedy(logits, frame_lens_dev):
    """-> (ids int32 [B, T'] padded with -1, n int32 [B], frame_tok int32 [B, T']): best-path CTC decoding of raw logits
    [B, T', V] - the argmax of every frame, repeats collapsed, blanks (index 0) dropped: asr_ctc_greedy_f32, one launch.
    Forward only, no host synchronisation."""
    logits = logits.detach()
    B, T, _ = logits.shape
    i32 = dict(device=logits.device, dtype=torch.int32)
    ids, n, frame_tok = torch.empty(B, T, **i32), torch.empty(B, **i32), torch.empty(B, T, **i32)
    hb.ctc_greedy(logits, frame_lens_dev, ids, n, frame_tok)
    return ids, n, frame_tok


def ctc_beam(logits, frame_lens_dev, beam, ngram=None, ngram_weight=0.0, ngram_bonus=0.0, eos_term=True, *, word_lm=None,
             word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False, context=None, ctx_weight=1.0):
    """-> (hyp int32 [B, beam, T'] padded with -1, hyp_len int32 [B, beam] with -1 in unused slots, score fp32 [B, beam]
    descending with -inf in unused slots): the CTC prefix beam search of raw logits [B, T', V] (blank = 0), asr_ctc_beam_f32
    (csrc/ctc_beam.hip), two launches.  Forward only, no host synchronisation.
    With ngram (an ngram.NgramLM, or its table on the device) the LM sits inside the search (asr_ctc_beam_lm_f32, DESIGN
    4.23, two launches): candidates rank by (tot + ngram_weight lm) + ngram_bonus len, eos_term adds the LM's
    end-of-sentence term after the last frame -> (hyp, hyp_len, score: the rank, ctc_score fp32 [B, beam]: tot, lm_score
    fp32 [B, beam]: lm).  Without ngram the call, its launches and its bits are what they were.
    With word_lm (a word_lm.WordLM, or its table on the device) the lexicon and the word-level LM sit inside the search
    (asr_ctc_beam_wlm_f32, DESIGN 4.25, two launches): candidates rank by (tot + word_lm_weight lm) + word_bonus n_words with
    lm the sum over the completed words; lexicon_only keeps only sequences of lexicon words -> (hyp, hyp_len, score,
    ctc_score, lm_score, n_words int32 [B, beam] with -1 in unused slots).  ngram and word_lm together: ValueError.
    With context (a context.ContextGraph for all rows, or a context.ContextBatch with one graph index per row) the phrase
    lists sit inside the search, alone or beside ngram (asr_ctc_beam_ctx_f32, DESIGN 4.32, two launches): a candidate ranks
    by its rank without a context plus ctx_weight bias -> (hyp, hyp_len, score: the rank, ctc_score[, lm_score], ctx_score
    fp32 [B, beam]: the bias, ops.context_score of the hypothesis bit for bit).  context with word_lm: ValueError."""
    if ngram is not None and word_lm is not None:
        raise ValueError("ctc_beam: ngram and word_lm are two LMs for one search: pass one of them")
    if context is not None and word_lm is not None:
        raise ValueError("ctc_beam: a context beside the word LM is not built: pass context with ngram, or alone")
    logits = logits.detach()
    B, T, V = logits.shape
    K, dev = int(beam), logits.device
    ws = torch.empty((hb.ctc_beam_ws_bytes(B, T, V, K) + 3) // 4, device=dev, dtype=torch.float32)
    hyp = torch.empty(B, K, T, device=dev, dtype=torch.int32)
    hyp_len = torch.empty(B, K, device=dev, dtype=torch.int32)
    score = torch.empty(B, K, device=dev, dtype=torch.float32)
    if context is not None:
        ctc_score, ctx_score = torch.empty_like(score), torch.empty_like(score)
        lm_score = torch.empty_like(score) if ngram is not None else None
        hb.ctc_beam_ctx(logits, frame_lens_dev, K, _context_table(context, dev, B), float(ctx_weight),
                        _ngram_table(ngram, dev) if ngram is not None else None, float(ngram_weight), float(ngram_bonus),
                        bool(eos_term), hyp, hyp_len, score, ctc_score, lm_score, ctx_score, ws)
        return (hyp, hyp_len, score, ctc_score) + ((lm_score,) if ngram is not None else ()) + (ctx_score,)
    if ngram is None and word_lm is None:
        hb.ctc_beam(logits, frame_lens_dev, K, hyp, hyp_len, score, ws)
        return hyp, hyp_len, score
    ctc_score, lm_score = torch.empty_like(score), torch.empty_like(score)
    if word_lm is not None:
        n_words = torch.empty_like(hyp_len)
        hb.ctc_beam_wlm(logits, frame_lens_dev, K, word_lm.to(dev), float(word_lm_weight), float(word_bonus), bool(eos_term),
                        bool(lexicon_only), hyp, hyp_len, score, ctc_score, lm_score, n_words, ws)
        return hyp, hyp_len, score, ctc_score, lm_score, n_words
    hb.ctc_beam_lm(logits, frame_lens_dev, K, _ngram_table(ngram, dev), float(ngram_weight), float(ngram_bonus), bool(eos_term),
                   hyp, hyp_len, score, ctc_score, lm_score, ws)
    return hyp, hyp_len, score, ctc_score, lm_score


def rnnt_beam(pe, frame_lens_dev, w_gate, b_gate, w_pred, w_out, b_out, emb, bos, beam, max_len, ngram=None, ngram_weight=0.0,
              ngram_bonus=0.0, eos_term=True, *, word_lm=None, word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
    """Beam search over the transducer head (csrc/rnnt_beam.hip): pe [B, T', J] the projected encoder output,
    w_gate [4 P, E + P] = [w_ih | w_hh] and b_gate = b_ih + b_hh of the prediction cell, w_pred [J, P], w_out [V, J], b_out
    [V], emb [V, E] -> (hyp int32 [B, beam, max_len] padded with -1, hyp_len int32 [B, beam] with -1 in unused slots, score
    fp32 [B, beam] descending with -inf in unused slots): the conventions of ctc_beam.  With ngram (an ngram.NgramLM, or its
    table on the device) candidates rank by (tot + ngram_weight lm) + ngram_bonus u, eos_term adds the LM's end-of-sentence
    term to a final -> (hyp, hyp_len, score: the rank, rnnt_score: tot, lm_score: lm).  A fixed T' + max_len iterations of
    four launches (the step kernel, the gate product, the cell kernel, the projection; the last iteration is the step
    kernel alone), four launches before the loop and the backtrace behind it: 4 (T' + max_len) + 2 in all.  The state and
    the workspace are ONE buffer leased from the pool for the call; nothing in it is read before the call has written it.
    With word_lm (a word_lm.WordLM, or its table on the device) the lexicon and the word-level LM sit inside the search (the
    asr_transducer_wbeam_* entries; the same launches, the extra workspace in the same lease): candidates rank by
    (tot + word_lm_weight lm) + word_bonus n_words with lm the sum over the completed words, a final closes its pending word,
    lexicon_only keeps only sequences of lexicon words -> (hyp, hyp_len, score, rnnt_score, lm_score, n_words int32
    [B, beam] with -1 in unused slots).  ngram and word_lm together: ValueError.
    Forward only, no host synchronisation."""
    if ngram is not None and word_lm is not None:
        raise ValueError("rnnt_beam: ngram and word_lm are two LMs for one search: pass one of them")
    pe = pe.detach().contiguous()
    B, T, J = pe.shape
    K, L, dev = int(beam), int(max_len), pe.device
    if L < 1:
        raise ValueError("rnnt_beam: max_len must be at least 1, got %d" % L)
    V, E, P = w_out.shape[0], emb.shape[1], w_pred.shape[1]
    r64 = lambda n: (n + 63) // 64 * 64                              # noqa: E731
    sizes = [r64((hb.rnnt_beam_ws_bytes(B, T, J, V, K, L, E, P) + 3) // 4)] + \
        [r64(B * K * n) for n in (P, P, E + P, 4 * P, J)]
    if word_lm is not None:
        sizes.append(r64((hb.rnnt_wbeam_ws_bytes(B, K) + 3) // 4))
    cap = _row_capacity(sum(sizes))
    lease = _POOL.acquire(("rnnt_beam", str(dev), cap), lambda: torch.empty(cap, device=dev, dtype=torch.float32))
    try:
        cuts, at = [], 0
        for n in sizes:
            cuts.append(lease.ws[at:at + n])
            at += n
        ws = cuts[0]
        h, c, xh, gates, pp = (t[:B * K * n].view(B * K, n) for t, n in zip(cuts[1:6], (P, P, E + P, 4 * P, J)))
        table = None if ngram is None else _ngram_table(ngram, dev)
        head = (pe, w_out.detach().contiguous(), None if b_out is None else b_out.detach().contiguous(),
                emb.detach().contiguous(), frame_lens_dev, K, L, h, c, xh, pp, ws)
        if word_lm is not None:
            run = hb.RnntWordBeam(*head, word_lm.to(dev), cuts[6], float(word_lm_weight), float(word_bonus), bool(eos_term),
                                  bool(lexicon_only))
        else:
            run = hb.RnntBeam(*head, table, float(ngram_weight), float(ngram_bonus), bool(eos_term))
        w_gate, b_gate, w_pred = w_gate.detach(), b_gate.detach(), w_pred.detach()
        n_it = T + L
        run.init(bos)
        for it in range(n_it + 1):
            if it > 0:
                run.step(it - 1)
                if it == n_it:
                    break
            run.product(xh, w_gate, gates, b_gate)
            run.cell(gates)
            run.product(h, w_pred, pp)
        hyp = torch.empty(B, K, L, device=dev, dtype=torch.int32)
        hyp_len = torch.empty(B, K, device=dev, dtype=torch.int32)
        score = torch.empty(B, K, device=dev, dtype=torch.float32)
        if word_lm is not None:
            rnnt_score, lm_score, n_words = torch.empty_like(score), torch.empty_like(score), torch.empty_like(hyp_len)
            run.backtrace(hyp, hyp_len, score, rnnt_score, lm_score, n_words)
            return hyp, hyp_len, score, rnnt_score, lm_score, n_words
        if table is None:
            run.backtrace(hyp, hyp_len, score)
            return hyp, hyp_len, score
        rnnt_score, lm_score = torch.empty_like(score), torch.empty_like(score)
        run.backtrace(hyp, hyp_len, score, rnnt_score, lm_score)
        return hyp, hyp_len, score, rnnt_score, lm_score
    finally:
        lease.release()


def _ngram_table(ngram, dev):
    """An ngram.NgramLM (compiled and uploaded once per device) or an ngram.NgramTable -> the table on dev."""
    return ngram.to(dev)


def _context_table(context, dev, rows):
    """A context.ContextGraph / ContextBatch (compiled and uploaded once per device) or a context.ContextTable -> the table on
    dev; ValueError when a batch lists its graphs for another number of rows."""
    table = context.to(dev)
    table.rows(rows)
    return table


def context_score(context, ids, lens, graph_of=None, per_token=False):
    """-> score fp32 [N] (and with per_token the deltas fp32 [N, L]): the bias of the padded TOKEN id rows ids [N, L] (int32
    or int64, on the device) with lens int32 [N] (-1: an unused slot, -inf) under their context graphs:
    asr_context_score_f32 (csrc/context.hip), one launch.  graph_of: an int32 tensor [N] on the device naming
    the graph of every row (-1: none, bias 0); None: the context's own list (a ContextBatch over N rows), or its one graph
    for every row (a ContextGraph).  An id outside 1 .. V-1 inside the length gives NaN for that row.  No host
    synchronisation."""
    ids = ids.detach()
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    if ids.dim() != 2:
        raise ValueError("context_score: ids must be [N, L], got %r" % (tuple(ids.shape),))
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    N, L = ids.shape
    dev = ids.device
    table = context.to(dev)
    if graph_of is not None:
        graph_of = graph_of.to(device=dev, dtype=torch.int32).contiguous()
    score = torch.empty(N, device=dev, dtype=torch.float32)
    tok = torch.empty(N, L, device=dev, dtype=torch.float32) if per_token else None
    hb.context_score(table, ids, lens.to(torch.int32).contiguous(), score, tok, graph_of=graph_of)
    return (score, tok) if per_token else score


def ngram_score(ngram, ids, lens, eos_term=True, per_token=False):
    """-> score fp32 [N] (and with per_token the terms fp32 [N, L]): the n-gram LM's log-probability of the padded id
    sequences ids [N, L] (int32 or int64, on the device) with lens int32 [N] (-1: an unused slot, -inf), the tokens in order
    from the context <s>, with the end-of-sentence term when eos_term: asr_ngram_score_f32 (csrc/ngram.hip), one
    launch.  An id outside 0 .. V-1 inside the length gives NaN for that sequence.  No host synchronisation."""
    ids = ids.detach()
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    if ids.dim() != 2:
        raise ValueError("ngram_score: ids must be [N, L], got %r" % (tuple(ids.shape),))
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    N, L = ids.shape
    dev = ids.device
    score = torch.empty(N, device=dev, dtype=torch.float32)
    tok = torch.empty(N, L, device=dev, dtype=torch.float32) if per_token else None
    hb.ngram_score(_ngram_table(ngram, dev), ids, lens.to(torch.int32).contiguous(), score, tok, eos_term=eos_term)
    return (score, tok) if per_token else score


def word_lm_score(word_lm, ids, lens, eos_term=True, per_word=False):
    """-> (score fp32 [N], n_words int32 [N]) (and with per_word the terms fp32 [N, L], word j at column j): the word LM's
    log-probability of the padded TOKEN id rows ids [N, L] (int32 or int64, on the device) with lens int32 [N] (-1: an unused
    slot, -inf) - the row's words (split at <space>, spelled through the lexicon, <unk> outside it) in order from the context
    <s>, with the end-of-sentence term when eos_term: asr_word_lm_score_f32 (csrc/word_lm.hip), one launch.  An
    id outside 0 .. V-1 inside the length gives NaN for that row.  No host synchronisation."""
    ids = ids.detach()
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    if ids.dim() != 2:
        raise ValueError("word_lm_score: ids must be [N, L], got %r" % (tuple(ids.shape),))
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    N, L = ids.shape
    dev = ids.device
    score = torch.empty(N, device=dev, dtype=torch.float32)
    n_words = torch.empty(N, device=dev, dtype=torch.int32)
    terms = torch.empty(N, L, device=dev, dtype=torch.float32) if per_word else None
    hb.word_lm_score(word_lm.to(dev), ids, lens.to(torch.int32).contiguous(), score, n_words, terms, eos_term=eos_term)
    return (score, n_words, terms) if per_word else (score, n_words)


def decoder_sequence(P, Q, emb_w, w_ih, w_hh, b_ih, b_hh, wdec, convw, watt, gvec, bo, w_out, b_out, w0, opts):
    opts = dict(opts)
    opts["pooled"] = torch.is_grad_enabled() and (P.requires_grad or w_hh.requires_grad)
    return _DecoderSeq.apply(P, Q, emb_w, w_ih, w_hh, b_ih, b_hh, wdec, convw, watt, gvec, bo, w_out, b_out, w0, opts)


def attention_step(enc_pad, P, Q, wdec, convw, watt, gvec, bo, dec_z, att_prev, scaling):
    """One stand-alone location-aware attention step (AttLoc.forward, model.py:139-173) on the same kernels as the
    fused loop; forward only (the training path differentiates through decoder_sequence).
    Returns (mlp_o(context) [B,O], w [B,T'])."""
    dev = P.device
    B, Tp, A = P.shape
    O, D, C = Q.shape[2], wdec.shape[1], convw.shape[0]
    K = (convw.shape[-1] - 1) // 2
    E = 16                                                   # dummy embedding width (unused columns of X)
    buf = hb.DecBuffers(B, Tp, A, D, O, E, C, K, 1, False, dev, False)
    with torch.no_grad():
        buf.P.copy_(P); buf.Q.copy_(Q); buf.w0.copy_(att_prev)
        buf.convw.copy_(convw.reshape(C, 2 * K + 1)); buf.gvec.copy_(gvec.reshape(A)); buf.wattT.copy_(watt.t())
        buf.wcat.zero_(); buf.bcat.zero_(); buf.X.zero_()
        buf.X[1, :, :D] = dec_z
        buf.bind(bo=bo, wdec=wdec, watt=watt, scaling=scaling)
        hb.att_step_fwd(buf.fwd_struct(), 0)
        return buf.X[1, :, D:D + O].clone(), buf.ws[0].clone()


BEAM_POLL_STEPS = 8          # the host reads the all-done word of a beam search every this many steps


def beam_search(P, Q, emb_w, w_ih, w_hh, b_ih, b_hh, wdec, convw, watt, gvec, bo, w_out, b_out, w0, beam, L, bos, eos,
                length_penalty=0.0, scaling=2.0, lm=None, lm_weight=0.0, ctc=None, ctc_weight=0.0, ngram=None, ngram_weight=0.0,
                ngram_bonus=0.0, word_lm=None, word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
    """Beam search over the decoder (Decoder.recognize_beams, model.py:369-406; semantics in DESIGN 4.8), eval arithmetic.

    Inputs as decoder_sequence's for B utterances; the search runs B*beam rows (row b*beam + k).  Every step is
    asr_dec_step_fwd at s = 1 -> output-layer GEMM -> beam select -> beam reorder (7 launches, no host sync).  The step
    reads its input slot (X[1], cstate[0], ws[0]) and writes its output slot (X[2], cstate[1], ws[1]); the reorder gathers
    the output slot back into the input slot, so two step slots serve any L.  Step 0 runs at s = 1 as well, from an input
    slot primed with what s = 0 would read (zero z, ctx and cell state, <BOS>, w0).
    lm (with lm_weight != 0): shallow fusion with a language model - dict(emb [V, E'], layers
    [(w_ih, w_hh, b_ih, b_hh)] of the stacked LSTM, w_out [V, H], b_out [V]).  Every beam row carries the LM's state; per
    step the LM consumes the decoder's input token (asr_lm_step_f32 per layer, the output GEMM) and the select ranks
    score + logp + lm_weight * logp_lm; the reorder gathers both states in one launch: 8 + n_layers launches.  Without it
    (or with lm_weight == 0) the search is the plain one, launch for launch.
    ctc (with ctc_weight != 0, a value in [0, 1]): joint CTC-attention decoding - dict(logits [B, T', V] fp32
    raw CTC logits of the encoder frames, frame_lens int32 [B] on the device, optionally lens_host: the host's copy).  Every
    beam row carries its CTC prefix state; per step the prefix score kernel runs before the select, which ranks
    score + (1 - ctc_weight) logp + ctc_weight (psi - psi_prev) (+ lm_weight logp_lm), and the advance kernel beside the
    reorder: 2 launches on top of the plain (9) or the LM search (10 + n_layers), no host synchronisation added.  Without it
    (or with ctc_weight == 0) the search is the plain / LM one, launch for launch and bit for bit.
    ngram (an ngram.NgramLM or its table) or word_lm (a word_lm.WordLM or its table), one of them: the n-gram
    automaton, or the lexicon and the word-level LM, inside the search.  Every beam row carries its LM position beside its score;
    a candidate ranks by (base + ngram_weight lm) + ngram_bonus len - with a word LM (base + word_lm_weight lm) + word_bonus
    n_words - where base is the candidate score of the search without it (the judge's and the CTC term included), lm the LM's
    fp32 sum over the extended sequence (<EOS>: with the end-of-sentence term) and len its tokens without <EOS>; lexicon_only
    keeps only sequences of lexicon words.  One init launch before the loop; the steps are the same launches as without it.
    Returns tokens [B, beam, L] int32 (ranked, <EOS>-padded), scores [B, beam], lengths [B, beam] - and with ngram / word_lm
    behind them att_score [B, beam] (base), lm_score [B, beam] (ops.ngram_score / ops.word_lm_score of the hypothesis, with the
    end term, bit for bit) and n [B, beam] int32 (len, or n_words)."""
    if ngram is not None and word_lm is not None:
        raise ValueError("ngram and word_lm are two LMs for one search: pass one of them")
    dev = P.device
    B, Tp, A = P.shape
    O = Q.shape[2]
    D = w_hh.shape[1]
    E = emb_w.shape[1]
    V = w_out.shape[0]
    C = convw.shape[0]
    Kc = (convw.shape[-1] - 1) // 2
    R = B * beam
    f32 = dict(device=dev, dtype=torch.float32)
    fused = lm is not None and float(lm_weight) != 0.0
    if not 0.0 <= float(ctc_weight) <= 1.0:
        raise ValueError("ctc_weight must lie in [0, 1], got %r" % (ctc_weight,))
    joint = ctc is not None and float(ctc_weight) != 0.0
    if joint and (tuple(ctc["logits"].shape[:2]) != (B, Tp) or ctc["logits"].shape[2] != V):
        raise ValueError("the CTC logits %s are not [%d utterances, %d frames, %d tokens]"
                         % (tuple(ctc["logits"].shape), B, Tp, V))
    if fused and (tuple(lm["w_out"].shape) != (V, lm["layers"][-1][1].shape[1]) or lm["emb"].shape[0] != V):
        raise ValueError("the LM's vocabulary (%d outputs, %d embeddings) is not the decoder's (%d)"
                         % (lm["w_out"].shape[0], lm["emb"].shape[0], V))
    with torch.no_grad():
        search = hb.BeamSearch(B, beam, V, L, eos, dev)
        table_lm = None
        if ngram is not None or word_lm is not None:
            tws = torch.empty(hb.beam_tlm_ws_bytes(B, beam) // 4, device=dev, dtype=torch.int32)
            if ngram is not None:
                table_lm = hb.BeamTableLm(search, tws, ngram=_ngram_table(ngram, dev), weight=ngram_weight, bonus=ngram_bonus)
            else:
                table_lm = hb.BeamTableLm(search, tws, word_lm=word_lm.to(dev), weight=word_lm_weight, bonus=word_bonus,
                                          lexicon_only=lexicon_only)
            table_lm.init()
        if joint:
            prefix = hb.CtcPrefixState(search, ctc["logits"].detach(), ctc["frame_lens"], 0, ctc.get("lens_host"))
        if fused:
            lms = hb.LmStepState(R, lm["emb"], lm["layers"], dev)
            lms.prime(bos)
            lm_w_out, lm_b_out = lm["w_out"].detach().contiguous(), lm["b_out"].detach().contiguous()
            lm_logits = torch.empty(R, V, **f32)
        buf = hb.DecBuffers(R, Tp, A, D, O, E, C, Kc, 2, False, dev, False)      # two step slots (three of X) serve any L
        buf.bind(P.repeat_interleave(beam, 0), Q.repeat_interleave(beam, 0), w0.repeat_interleave(beam, 0), convw, gvec, bo,
                 wdec, watt, None, scaling)
        X, cst, wts = buf.X.zero_(), buf.cstate.zero_(), buf.ws
        hb.dec_pack(w_ih, w_hh, b_ih, b_hh, wdec, watt, D, O, E, A, C, buf.wcat, buf.bcat, None, None, buf.wattT)
        fs = buf.fwd_struct()
        emb_c, w_out_c = emb_w.contiguous(), w_out.contiguous()
        X[1, :, D + O:] = emb_c[bos]
        wts[0].copy_(buf.w0)
        logits = torch.empty(R, V, **f32)
        landing = torch.zeros(1, dtype=torch.int32).pin_memory()
        polled = None
        steps = launches = 0
        for t in range(L):
            hb.dec_step_fwd(fs, 1)
            hb.gemm_skinny(X[2][:, :D + O], w_out_c, bias=b_out, out=logits)
            if fused:
                lms.step()
                hb.gemm_skinny(lms.top(), lm_w_out, bias=lm_b_out, out=lm_logits)
                launches += lms.n + 1                      # the LM's layers and its output GEMM
            if joint:
                prefix.score()
                launches += 1                              # the prefix score
            if table_lm is not None:
                table_lm.select(logits, t, lm_logits if fused else None, lm_weight, prefix if joint else None, ctc_weight)
            elif joint:
                search.select_ctc(logits, prefix, ctc_weight, t, lm_logits if fused else None, lm_weight)
            elif fused:
                search.select_lm(logits, lm_logits, lm_weight, t)
            else:
                search.select(logits, t)
            steps += 1
            launches += 6                                  # 4 decoder-step kernels, the GEMM, the select
            if t == L - 1:
                break
            if fused:
                search.reorder_lm(t, lms, (X[2], X[1], cst[1], cst[0], wts[1], wts[0], emb_c, D, O))
            else:
                search.reorder(t, X[2], X[1], cst[1], cst[0], wts[1], wts[0], emb_c, D, O)
            launches += 1
            if joint:
                prefix.advance(t)
                launches += 1
            if (t + 1) % BEAM_POLL_STEPS == 0:
                # the word copied BEAM_POLL_STEPS steps ago: the host waits for that step at most, never for this one
                if polled is not None:
                    polled.synchronize()
                    if int(landing[0]) == B:
                        break
                landing.copy_(search.ndone, non_blocking=True)
                polled = torch.cuda.Event()
                polled.record()
        kind = "beam_ctc" if joint else ("beam_lm" if fused else "beam")      # (a joint search with an LM counts as beam_ctc)
        hb.LAUNCHES[kind + "_step"] += steps
        hb.LAUNCHES[kind + "_launch"] += launches
        out = search.backtrack(length_penalty) if table_lm is None else table_lm.backtrack(length_penalty)
    return out
