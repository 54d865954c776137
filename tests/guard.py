"""Guard bands: run an operator on buffers that lie between two bands of memory the test owns, and look at the bands.

A kernel that stores a few elements outside a buffer it was given damages whatever the caching allocator put next to it:
nothing faults, and the damaged tensor usually belongs to another operator.  A fenced tensor is a view into a private 1-D
byte buffer of BAND + nbytes + BAND bytes; its data starts exactly at the end of the front band and ends exactly where the
back band starts (nbytes is NOT rounded: 33 floats end 132 bytes in and the band begins on the next byte).  A stray store
lands in a band, where check() finds it and names the allocation, the side and the offset.

    ins = guard.Stats()
    z = guard.fence(logits, nan=True, stats=ins)          a fenced copy of an input: same dtype, shape and values
    snap = guard.frozen(z, lens)                           bitwise snapshots of the inputs the operator declares const
    with guard.guarded("one") as st:                       torch.empty, empty_like, empty_strided, zeros, zeros_like, full,
        y = hb.gemm(a, b)                                  full_like, ones, Tensor.new_empty, new_zeros and new_full - as
    guard.check(st, ins)                                   hip_backend, ops, model, frontend, feed, ngram, word_lm, gtc and
    guard.assert_frozen(snap)                              context see them - return fenced memory

BAND = 8192 bytes: a multiple of 256, so the 16-byte alignment asr_aligned16 demands and the 256-byte alignment torch gives
survive, and twice the widest store footprint of one workgroup here (256 lanes x 16 bytes).

BAND CONTENTS.  poison.py's rule holds: these tests must not be able to fault a GPU.  A band turns an out-of-bounds access
into an access to owned memory, but a band word that a kernel READS as an index must stay small:
  * integer and bool tensors: filled through the tensor's own dtype with 1 (int_pattern "one") or 0 ("zero");
  * float tensors the library allocates (they may be carved into integer regions on the C side): 32-bit words of integer
    value 1 or 0;
  * float tensors the TEST fences itself with nan=True - pure float data: logits, waveforms, weights, dense float outputs -
    32-bit words 0x7fc5a5a5, the quiet NaN of gemm_terms_ref.SENTINEL: an out-of-bounds read that reaches the result shows
    up as NaN in the existing parity checks.
Every GPU case runs under both integer patterns: a stray store of 1 is invisible under "one" and visible under "zero".

NOT FENCED.  Pinned host memory; non-contiguous allocations (empty_strided with other strides, *_like of a non-contiguous
tensor) - passed through and listed in Stats.unfenced with their call sites; tensors on other devices than `devices`
(device tensors only by default); and the INTERIOR of the step arena (ops._ARENA): it sub-allocates from one buffer, the
buffer as a whole is fenced, a store from one slice into the next is not seen - operator cases run outside a step_arena
scope.  The pools (ops._POOL, hb._det_ws_cache, the pinned ring) are emptied with poison.empty_pool() before a scope opens
and after it closes, so pooled workspaces are allocated - fenced - inside it.

The registry (Stats.records) holds a strong reference to every buffer until the Stats object goes: the band of a tensor the
operator has already dropped must still be checked.  The bands are never freed by the tests and no buffer is placed against
the end of a real allocation.  An out-of-bounds READ that does not reach the result is not detectable this way.

No GPU is needed to import or use this module (the CPU tests drive it on host tensors with devices=("cpu",)).
"""
import contextlib
import os
import sys

import torch

BAND = 8192
NAN_WORD = 0x7fc5a5a5                                  # gemm_terms_ref.SENTINEL (pinned by tests/test_guard_cpu.py)
INT_PATTERNS = ("one", "zero")

TORCH_FUNCS = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like", "full", "full_like", "ones")
TENSOR_METHODS = ("new_empty", "new_zeros", "new_full")
PRODUCT_MODULES = ("hip_backend", "ops", "model", "frontend", "feed", "ngram", "word_lm", "gtc", "context")

_EMPTY = torch.empty                                   # the originals, whatever scope is open when fence() runs
_THIS = os.path.abspath(__file__).rsplit(".", 1)[0]


class GuardError(AssertionError):
    """check() found damaged bands: .damage lists them."""

    def __init__(self, damage):
        self.damage = damage
        AssertionError.__init__(self, "%d damaged guard band(s):\n  %s" % (len(damage), "\n  ".join(d.line() for d in damage)))


class Damage(object):
    """One damaged band: record (the allocation), side ("front" / "back"), offset (of the first damaged byte relative to
    the first byte of the data: -1 is the byte in front of it, record.nbytes the byte behind it), nbytes (damaged bytes in
    this band), words (the first damaged 32-bit words of the band, from the one that holds `offset`)."""

    def __init__(self, record, side, offset, nbytes, words):
        self.record, self.side, self.offset, self.nbytes, self.words = record, side, offset, nbytes, words

    def line(self):
        r = self.record
        return "%s %s allocated at %s: %s band, first damaged byte at data%+d, %d byte(s) damaged, words %s" % (
            str(r.dtype).replace("torch.", ""), list(r.shape), r.site, self.side, self.offset, self.nbytes,
            " ".join("%08x" % w for w in self.words))


class Record(object):
    """One fenced allocation: base (the uint8 buffer, kept alive), shape, dtype, nbytes, site, pattern (the bytes both bands
    repeat)."""
    __slots__ = ("base", "shape", "dtype", "nbytes", "site", "pattern")

    def __init__(self, base, shape, dtype, nbytes, site, pattern):
        self.base, self.shape, self.dtype, self.nbytes, self.site, self.pattern = base, tuple(shape), dtype, nbytes, site, pattern

    def bands(self):
        return self.base[:BAND], self.base[BAND + self.nbytes:]


class Stats(object):
    """What a scope fenced: allocations and bytes per dtype, the records check() walks, and `unfenced`: (what, call site) of
    every allocation on a guarded device that had to be passed through."""

    def __init__(self):
        self.allocs, self.bytes, self.records, self.unfenced = {}, {}, [], []

    def add(self, rec):
        self.allocs[rec.dtype] = self.allocs.get(rec.dtype, 0) + 1
        self.bytes[rec.dtype] = self.bytes.get(rec.dtype, 0) + rec.nbytes
        self.records.append(rec)

    @property
    def n_allocs(self):
        return sum(self.allocs.values())

    @property
    def n_bytes(self):
        return sum(self.bytes.values())

    @property
    def n_bands(self):
        return 2 * len(self.records)

    def merge(self, other):
        for k, v in other.allocs.items():
            self.allocs[k] = self.allocs.get(k, 0) + v
        for k, v in other.bytes.items():
            self.bytes[k] = self.bytes.get(k, 0) + v
        self.records += other.records
        self.unfenced += other.unfenced
        return self

    def line(self):
        per = ", ".join("%s x%d %dB" % (str(k).replace("torch.", ""), v, self.bytes[k]) for k, v in sorted(self.allocs.items(), key=str))
        return "%d fenced, %d bytes (%s), %d unfenced" % (self.n_allocs, self.n_bytes, per or "-", len(self.unfenced))


def call_site():
    """file:line of the first frame outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename).rsplit(".", 1)[0] == _THIS:
        f = f.f_back
    while f is not None and f.f_code.co_filename.endswith("contextlib.py"):
        f = f.f_back
    return "?" if f is None else "%s:%d" % (os.path.basename(f.f_code.co_filename), f.f_lineno)


def band_pattern(dtype, int_pattern="one", nan=False):
    """The bytes a band of a tensor of `dtype` repeats (little endian): see BAND CONTENTS."""
    if int_pattern not in INT_PATTERNS:
        raise ValueError("int_pattern must be one of %s, got %r" % (INT_PATTERNS, int_pattern))
    v = 1 if int_pattern == "one" else 0
    if dtype.is_floating_point or dtype.is_complex:
        return (NAN_WORD if nan else v).to_bytes(4, "little")
    if nan:
        raise ValueError("nan=True is for float tensors, got %s" % dtype)
    return v.to_bytes(1 if dtype == torch.bool else _EMPTY(0, dtype=dtype).element_size(), "little")


def _fill_band(band, dtype, pattern):
    if dtype.is_floating_point or dtype.is_complex:
        # 32-bit words, written bytewise: a band of 33 half floats starts 66 bytes in, on no word boundary of the base
        band.view(-1, len(pattern)).copy_(torch.tensor(list(pattern), dtype=torch.uint8).to(band.device))
    else:
        band.view(dtype).fill_(int.from_bytes(pattern, "little"))      # through the tensor's own dtype


def fenced_empty(shape, dtype=None, device=None, nan=False, int_pattern="one", stats=None):
    """-> a contiguous tensor of `shape` whose memory lies between two bands; its contents are undefined."""
    dtype = torch.get_default_dtype() if dtype is None else dtype
    device = torch.device("cpu" if device is None else device)
    shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
    pattern = band_pattern(dtype, int_pattern, nan)
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * _EMPTY(0, dtype=dtype).element_size()
    base = _EMPTY(BAND + nbytes + BAND, dtype=torch.uint8, device=device)
    rec = Record(base, shape, dtype, nbytes, call_site(), pattern)
    for band in rec.bands():
        _fill_band(band, dtype, pattern)
    if base.is_cuda:
        torch.cuda.synchronize(base.device)            # (poison.py: a first write on a side stream must not pass the fill)
    if stats is not None:
        stats.add(rec)
    return base[BAND:BAND + nbytes].view(dtype).view(shape)


def fence(t, nan=False, int_pattern="one", stats=None):
    """-> a fenced copy of `t`: same dtype, shape, values, device and requires_grad.  Contiguous tensors only."""
    if not torch.is_tensor(t) or not t.is_contiguous():
        raise ValueError("fence() takes a contiguous tensor")
    with torch.no_grad():
        out = fenced_empty(t.shape, t.dtype, t.device, nan, int_pattern, stats)
        out.copy_(t.detach())
    if t.requires_grad:
        out.requires_grad_(True)
    return out


def _fenceable(t, devices):
    """None: not this scope's business; "" : fence it; a reason: pass it through and list it."""
    if not torch.is_tensor(t) or t.device.type not in devices or t.layout != torch.strided or t.is_quantized:
        return None
    if t.device.type == "cpu" and t.is_pinned():
        return None
    if not t.is_contiguous():
        return "non-contiguous strides %s" % (tuple(t.stride()),)
    return ""


@contextlib.contextmanager
def guarded(int_pattern="one", stats=None, devices=("cuda",)):
    """Inside the scope the allocation functions of TORCH_FUNCS and TENSOR_METHODS return fenced memory with the values the
    original gives (zeros, the fill value; `empty` stays undefined).  The originals come back on exit, after an exception
    as well.  -> Stats."""
    band_pattern(torch.float32, int_pattern)           # (an unknown pattern fails here, before anything is patched)
    st = stats if stats is not None else Stats()
    saved = {name: getattr(torch, name) for name in TORCH_FUNCS}
    saved_methods = {name: getattr(torch.Tensor, name) for name in TENSOR_METHODS}

    def wrap(orig, name):
        def alloc(*args, **kwargs):
            t = orig(*args, **kwargs)
            why = _fenceable(t, devices)
            if why is None:
                return t
            if why:
                st.unfenced.append(("%s %s %s: %s" % (name, str(t.dtype).replace("torch.", ""), list(t.shape), why), call_site()))
                return t
            return fence(t, False, int_pattern, st)
        alloc.__name__ = name
        alloc.__wrapped__ = orig
        return alloc

    try:
        for name, orig in saved.items():
            setattr(torch, name, wrap(orig, name))
        for name, orig in saved_methods.items():
            setattr(torch.Tensor, name, wrap(orig, name))
        yield st
    finally:
        for name, orig in saved.items():
            setattr(torch, name, orig)
        for name, orig in saved_methods.items():
            setattr(torch.Tensor, name, orig)


def damage(*stats):
    """-> [Damage] of every registered buffer of the Stats objects, the device synchronised first."""
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
    found = []
    for st in stats:
        for rec in st.records:
            p = len(rec.pattern)
            want = torch.tensor(list(rec.pattern), dtype=torch.uint8)
            for side, band in zip(("front", "back"), rec.bands()):
                got = band.cpu()
                bad = (got.view(-1, p) != want).any(1)
                if not bool(bad.any()):
                    continue
                diff = (got != want.repeat(BAND // p)).nonzero().flatten()
                first = int(diff[0])
                w0 = first // 4 * 4
                words = [int.from_bytes(bytes(got[i:i + 4].tolist()), "little") for i in range(w0, min(w0 + 16, BAND), 4)]
                found.append(Damage(rec, side, first - BAND if side == "front" else rec.nbytes + first, int(diff.numel()), words))
    return found


def check(*stats):
    """Every band of every registered buffer still holds what was written there, or GuardError names each damaged one."""
    found = damage(*stats)
    if found:
        raise GuardError(found)
    return sum(st.n_bands for st in stats)


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def frozen(*tensors):
    """-> a bitwise snapshot of the tensors (None entries are kept as None)."""
    return [(t, None if t is None else _bits(t).clone()) for t in tensors]


def assert_frozen(snapshot, what=""):
    """Every tensor of the snapshot holds the bits it held: compared through an integer view, so NaN equals itself."""
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
    for i, (t, was) in enumerate(snapshot):
        if t is None:
            continue
        now = _bits(t)
        if not torch.equal(now, was):
            first = int((now != was).nonzero()[0])
            raise AssertionError("%s: const input %d (%s %s) was written: %d byte(s) changed, the first at byte %d" % (
                what, i, str(t.dtype).replace("torch.", ""), list(t.shape), int((now != was).sum()), first))
