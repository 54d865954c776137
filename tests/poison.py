"""Poisoned buffers: run an operator on memory whose "undefined" contents are chosen by the test.

Every kernel here writes into tensors that come from torch.empty, from the workspace pool (ops._POOL), from the ordered
reductions' scratch (hb._det_ws_cache) or from the pinned upload ring.  In a test process such memory is kind by accident:
fresh zero pages from the driver, or the block the previous, identical case just filled with the right answer.  This module
makes it hostile on purpose, so that a kernel that skips a tile of its output, reads a workspace word it did not write in
this call, or trusts a buffer to be zero that nobody zeroed, computes a visibly different (or non-finite) result.

    with poisoned("nan") as st:         torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty return
        y = hb.gemm(a, b)               memory filled with the pattern; st counts allocations and bytes per dtype
    n = poison_pool("nan", st)          fills what lies in ops._POOL.free, hb._det_ws_cache and the pinned ring

THE RULE.  A buffer is either "contents undefined on entry" - the operator must give the same result whatever it holds -
or "state": its contents ARE the contract between two calls.  Only the first class is poisoned.  State, NOT poisoned:

  * hb._persist_scratch and the abort latch     the persistent kernels' barrier counters and the abort word: zero between
                                                launches is what the kernels rely on and restore themselves
  * the step arena (ops._ARENA)                 "everything at and behind the cursor is zero" is its contract; the tests
                                                CHECK that (arena_is_zero) instead of breaking it
  * hb.BeamSearch counters (score, nfin, ndone, fin_min ...)   torch.zeros / torch.full in the constructor: the state
                                                of the search between its steps (its torch.empty histories ARE poisoned)
  * hb.CtcPrefixState between steps             state / last / psi_prev carry the prefix probabilities from step to step:
                                                poisoned when allocated (the constructor must initialise them), not between
                                                score() and advance()
  * optimiser state (FlatAdam's flat buffers)   the moments are the optimiser's memory
  * tensors a pooled workspace merely REFERS to: the inputs DecBuffers.bind() keeps alive (P, Q, w0, convw, gvec, bo, wdec,
    watt, xmask) and the LSTM workspace's `lens`.  They belong to the caller - model parameters among them - and poisoning
    them would change the inputs of the next call, not its workspace.  (POOL_SKIP)

PATTERNS.  Floating tensors: "nan", "huge" (3e38, the format's largest finite value where that is smaller) and "zero".
Integer and bool tensors only ever receive 0 ("zero") or 1 (the other two): an uninitialised integer may be read as an
index, and it must stay in bounds - these tests must not be able to fault a GPU.  For the same reason a FLOAT workspace
that the C side carves into integer regions is poisoned with nan / huge only after the kernel has been read for a read
before the write (the GPU test module records where each region is written).

After each fill of a device tensor the device is synchronised: some buffers are first written on a side stream (the
upload stream, ops._SideStream), and the fill - enqueued on the current stream - must not land behind such a write.

No GPU is needed to import or use this module (the CPU tests drive it on host tensors).
"""
import contextlib
import sys

import torch

PATTERNS = ("zero", "nan", "huge")
HUGE = 3e38

# attributes of a pooled workspace that are the caller's tensors, not the workspace's own memory (see the docstring)
POOL_SKIP = frozenset(("P", "Q", "w0", "convw", "gvec", "bo", "wdec", "watt", "xmask", "lens"))


class Stats(object):
    """What a scope poisoned: allocations and bytes per dtype (torch.empty & co), tensors found in the pools."""

    def __init__(self):
        self.allocs, self.bytes, self.pool_tensors = {}, {}, 0

    def add(self, t):
        self.allocs[t.dtype] = self.allocs.get(t.dtype, 0) + 1
        self.bytes[t.dtype] = self.bytes.get(t.dtype, 0) + t.numel() * t.element_size()

    @property
    def n_allocs(self):
        return sum(self.allocs.values())

    @property
    def n_bytes(self):
        return sum(self.bytes.values())

    @property
    def total(self):
        """Everything that was poisoned: a case with total == 0 tested nothing."""
        return self.n_allocs + self.pool_tensors

    def merge(self, other):
        for k, v in other.allocs.items():
            self.allocs[k] = self.allocs.get(k, 0) + v
        for k, v in other.bytes.items():
            self.bytes[k] = self.bytes.get(k, 0) + v
        self.pool_tensors += other.pool_tensors
        return self

    def line(self):
        per = ", ".join("%s x%d" % (str(k).replace("torch.", ""), v) for k, v in sorted(self.allocs.items(), key=str))
        return "%d allocations, %d bytes (%s), %d pooled tensors" % (self.n_allocs, self.n_bytes, per or "-", self.pool_tensors)


def fill_value(dtype, pattern):
    """The value `pattern` writes into a tensor of `dtype`: never anything but 0 or 1 for integers and bool."""
    if pattern not in PATTERNS:
        raise ValueError("pattern must be one of %s, got %r" % (PATTERNS, pattern))
    if dtype.is_floating_point or dtype.is_complex:
        if pattern == "zero":
            return 0.0
        if pattern == "nan":
            return float("nan")
        real = dtype if dtype.is_floating_point else torch.empty(0, dtype=dtype).real.dtype
        return min(HUGE, torch.finfo(real).max)
    if dtype == torch.bool:
        return pattern != "zero"
    return 0 if pattern == "zero" else 1


def fill_(t, pattern, stats=None):
    """Fill tensor `t` by the rule (no-op for empty and meta tensors) -> whether anything was written."""
    if not torch.is_tensor(t) or t.numel() == 0 or t.device.type == "meta" or t.is_sparse or t.is_quantized:
        return False
    with torch.no_grad():
        t.detach().fill_(fill_value(t.dtype, pattern))
    if t.is_cuda:
        torch.cuda.synchronize(t.device)
    if stats is not None:
        stats.add(t)
    return True


_TORCH_FUNCS = ("empty", "empty_like", "empty_strided")


@contextlib.contextmanager
def poisoned(pattern, stats=None):
    """Inside the scope torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty - as every module that says
    `torch.empty(...)` sees them: hip_backend, ops, model, frontend, feed, ngram, word_lm - return memory filled with
    `pattern`.  The originals come back on exit, after an exception as well.  -> Stats."""
    fill_value(torch.float32, pattern)                 # (an unknown pattern fails here, before anything is patched)
    st = stats if stats is not None else Stats()
    saved = {name: getattr(torch, name) for name in _TORCH_FUNCS}
    saved_new_empty = torch.Tensor.new_empty

    def wrap(orig):
        def alloc(*args, **kwargs):
            t = orig(*args, **kwargs)
            fill_(t, pattern, st)
            return t
        alloc.__name__ = getattr(orig, "__name__", "alloc")
        alloc.__wrapped__ = orig
        return alloc

    try:
        for name, orig in saved.items():
            setattr(torch, name, wrap(orig))
        torch.Tensor.new_empty = wrap(saved_new_empty)
        yield st
    finally:
        for name, orig in saved.items():
            setattr(torch, name, orig)
        torch.Tensor.new_empty = saved_new_empty


def walk_tensors(obj, skip=POOL_SKIP, _seen=None):
    """Every tensor reachable from `obj` through dicts, lists / tuples and the attributes of plain objects (__dict__ or
    __slots__), except under the names in `skip`; each tensor object once."""
    seen = _seen if _seen is not None else set()
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            if not (isinstance(k, str) and k in skip):
                for t in walk_tensors(v, skip, seen):
                    yield t
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            for t in walk_tensors(v, skip, seen):
                yield t
    elif hasattr(obj, "__dict__") or hasattr(obj, "__slots__"):
        if isinstance(obj, (type, type(sys))) or callable(obj):
            return
        names = list(getattr(obj, "__dict__", {}).keys()) + [n for n in getattr(obj, "__slots__", ()) if hasattr(obj, n)]
        for n in names:
            if n not in skip:
                for t in walk_tensors(getattr(obj, n), skip, seen):
                    yield t


def poison_tree(obj, pattern, stats=None, skip=POOL_SKIP):
    """Fill every tensor walk_tensors finds under `obj` -> the number of tensors filled."""
    n = 0
    for t in walk_tensors(obj, skip):
        n += bool(fill_(t, pattern))
    _mark_rows_stale(obj)
    if stats is not None:
        stats.pool_tensors += n
    return n


def _mark_rows_stale(obj, _depth=0):
    """The pooled LSTM workspace keeps a HOST-side note of how many rows of gates_buf / y_buf may hold stale values
    (`rows_written`; the rows behind it are zeros from the allocation, and the packed-row dW_hh product reads one of them).
    A fill of the whole buffer makes every row stale, and the note has to say so - that number is state, the rows are not."""
    if isinstance(obj, dict):
        if "rows_written" in obj and torch.is_tensor(obj.get("gates_buf")):
            obj["rows_written"] = int(obj["gates_buf"].shape[0])
        for v in obj.values():
            if _depth < 4:
                _mark_rows_stale(v, _depth + 1)
    elif isinstance(obj, (list, tuple)) and _depth < 4:
        for v in obj:
            _mark_rows_stale(v, _depth + 1)


def pool_roots():
    """The three places poison_pool walks, from the modules as they are loaded (none loaded: nothing to walk)."""
    roots = []
    ops = sys.modules.get("ops")
    hb = sys.modules.get("hip_backend")
    if ops is not None and hasattr(ops, "_POOL"):
        roots.append(ops._POOL.free)
    if hb is not None:
        roots.append(getattr(hb, "_det_ws_cache", {}))
        roots.append(getattr(hb, "_pinned_ring", {}))
    return roots


def poison_pool(pattern, stats=None):
    """Fill what lies in ops._POOL.free (dicts of tensors, hb.DecBuffers objects: every tensor attribute they own),
    hb._det_ws_cache and the pinned ring, by the same rule -> the number of tensors filled."""
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()                       # (a pinned buffer may still be the source of a copy in flight)
    return sum(poison_tree(root, pattern, stats) for root in pool_roots())


def empty_pool():
    """Drop every free workspace and the ordered reductions' scratch: the next call allocates (under poisoned(): poison)."""
    ops = sys.modules.get("ops")
    hb = sys.modules.get("hip_backend")
    if ops is not None and hasattr(ops, "_POOL"):
        ops._POOL.free.clear()
    if hb is not None:
        getattr(hb, "_det_ws_cache", {}).clear()
        getattr(hb, "_pinned_ring", {}).clear()


def arena_is_zero():
    """The ASR_ARENA_DEBUG check as a function: the whole step arena holds zeros (True when there is no arena yet).  Call it
    right after a scope has opened."""
    ops = sys.modules.get("ops")
    buf = None if ops is None else ops._ARENA.buf
    return True if buf is None else bool((buf == 0).all())
