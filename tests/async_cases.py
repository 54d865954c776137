"""A GPU that lags behind the host, on purpose (tests/test_async_gpu.py, tests/test_async_cpu.py).

Every other test enqueues one operation, synchronises and reads.  The product does not run that way: the host enqueues the
next step while the GPU is still in this one, small host arrays travel through a ring of pinned buffers
(hip_backend._to_device), workspaces come back from pools and free lists.  A lifetime or ordering mistake in that host layer
hands wrong lengths or a reused buffer to a correct kernel - and shows only while the GPU is BEHIND.

    stalled(stream)        a delay kernel on `stream` and an event right behind it -> Stall; Stall.proved() is
                           `not event.query()`: the GPU had not yet got past the delay, so NOTHING enqueued behind it had run
    run_case(...)          one case: the scripted host phase once without a stall (the base outputs, and the host time), a
                           stall of 20 x that time (50 ms ... 2 s), the whole host phase again behind the stall, proved()
                           BEFORE anything synchronises, then the comparison, bit for bit

The host phase of a case is what the next step of a real program does while this one is still queued:
    (a) the call under test, its own uploads included            (c) the same operator on other inputs of the same shapes
    (b) >= 16 further to_device_* uploads of the same sizes      (d) everything of (a) but its outputs dropped, gc.collect(),
        with other (valid) values                                    fresh allocations of the same sizes filled with NaN
A case whose stall had ended before the host phase did has proven nothing: it FAILS (no skip, no second try).

No GPU is needed to import this module; the CPU tests drive run_case with a fake stall."""
import gc
import time

import numpy as np
import torch

FACTOR, MIN_MS, MAX_MS = 20.0, 50.0, 2000.0
SCRIBBLES = 16
_CYCLES_PER_MS = {}


class NotProven(AssertionError):
    """The stall had ended before the host phase did."""


def cycles_per_ms():
    """torch.cuda._sleep counts device clock cycles: their rate is measured once per process, two events around a short
    sleep and around one five times as long - the DIFFERENCE of the two times is the cycles' own (what a launch and the
    events cost is in both, and is not small beside a short sleep).  No clock rate is assumed; a
    pair that turns out shorter than 1 ms is measured once more, ten times as long."""
    dev = torch.cuda.current_device()
    if dev not in _CYCLES_PER_MS:
        def timed(cycles):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        rate = None
        for cycles in (1000000, 10000000):
            timed(cycles)                                   # (the first launch of the kernel is not measured)
            ms = timed(5 * cycles) - timed(cycles)
            rate = 4 * cycles / max(ms, 1e-3)
            if ms >= 1.0:
                break
        _CYCLES_PER_MS[dev] = rate
    return _CYCLES_PER_MS[dev]


class Stall(object):
    def __init__(self, event, ms):
        self.event, self.ms = event, ms

    def proved(self):
        """The delay was still running (or waiting): nothing enqueued behind it on its stream has run."""
        return not self.event.query()


def stalled(stream=None, ms=MIN_MS):
    """A delay kernel of ~`ms` milliseconds on `stream` (None: the current one) and an event right behind it."""
    stream = torch.cuda.current_stream() if stream is None else stream
    cycles = int(cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        event = torch.cuda.Event()
        event.record(stream)
    return Stall(event, ms)


def stall_ms(host_ms):
    return min(MAX_MS, max(MIN_MS, FACTOR * host_ms))


def words(t):
    """A tensor or array of a 4- or 8-byte type -> its words as int32 (the comparison of test_batch_invariance_gpu)."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.int32)
    assert a.dtype in (np.float32, np.int32, np.int64, np.float64), a.dtype
    return a.reshape(-1).view(np.int32)


def differing(got, want):
    """Two dicts of outputs -> (words compared, words differing); the keys and the shapes must agree."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    n = bad = 0
    for k in got:
        x, y = words(got[k]), words(want[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        n, bad = n + x.size, bad + int((x != y).sum())
    return n, bad


class Tracker(object):
    """What call (a) put on the device, by size: refilled with NaN in (d).  Host arrays go up through pinned staging
    buffers and asynchronous copies (a copy from pageable memory would make the host wait for the stalled stream); the
    staging buffers are made in the run without a stall and taken again, in the same order, behind the stall - the host
    phase is the same program both times - so that nothing is allocated while the GPU is held up."""

    def __init__(self, stage=None):
        self.nbytes, self.stage = [], stage if stage is not None else dict(bufs=[], i=0)

    def dev(self, array, device="cuda"):
        a = np.ascontiguousarray(array)
        if torch.device(device).type != "cuda":
            t = torch.from_numpy(a.copy())
        else:
            st = self.stage
            if st["i"] == len(st["bufs"]):
                st["bufs"].append(torch.from_numpy(a.copy()).pin_memory())
            host = st["bufs"][st["i"]]
            st["i"] += 1
            assert host.shape == a.shape and host.dtype == torch.from_numpy(a).dtype, "the host phase is not the same program"
            host.copy_(torch.from_numpy(a))
            t = host.to(device, non_blocking=True)
        self.nbytes.append(t.numel() * t.element_size())
        return t

    def refill(self, device):
        """Fresh allocations of every noted size on the current stream, filled with NaN (the caching allocator hands a
        freed block of the same size class out again at once)."""
        return [torch.full((max(1, n // 4),), float("nan"), dtype=torch.float32, device=device) for n in self.nbytes]


def scribble(hb, device, specs, n=SCRIBBLES):
    """(b): n further uploads per spec, specs = [(kind, values)] with kind in i32 / i64 / f32 and `values` a list of VALID
    alternatives (every length <= T, every offset inside the packed extent); they cycle.  -> the tensors (kept alive)."""
    up = dict(i32=hb.to_device_i32, i64=hb.to_device_i64, f32=hb.to_device_f32)
    kept = []
    for kind, alternatives in specs:
        for i in range(n):
            kept.append(up[kind](alternatives[i % len(alternatives)], device))
    return kept


def run_case(name, call_a, call_c, scribbles=(), hb=None, device="cuda", stream=None, stall=stalled, sync=None, out=print):
    """call_a(tracker) / call_c(tracker) -> dict of output tensors: they build their inputs from host arrays (tracker.dev,
    the library's own uploads) and keep nothing else.  scribbles: the specs of scribble().  stream: the stream the stall goes
    on (None: the current one).  -> the record line; raises NotProven / AssertionError."""
    sync = sync or torch.cuda.synchronize

    stage = dict(bufs=[], i=0)

    def host_phase():
        stage["i"] = 0                                               # (every staging buffer again: the GPU is idle here)
        tr = Tracker(stage)
        a = call_a(tr)                                               # (a): its inputs die with the call
        kept = scribble(hb, device, scribbles) if scribbles else []  # (b)
        c = call_c(Tracker(stage))                                   # (c)
        gc.collect()                                                 # (d)
        nan = tr.refill(device)
        return a, c, (kept, nan)

    sync()
    t0 = time.perf_counter()
    base_a, base_c, keep = host_phase()
    host_ms = (time.perf_counter() - t0) * 1e3
    sync()
    base_a = {k: words(v).copy() for k, v in base_a.items()}
    base_c = {k: words(v).copy() for k, v in base_c.items()}
    del keep
    ms = stall_ms(host_ms)
    st = stall(stream, ms)
    got_a, got_c, keep = host_phase()
    proved = st.proved()                                             # before anything synchronises
    sync()
    if not proved:
        out("async-invariance %s host %.2f stall %.0f proved 0" % (name, host_ms, ms))
        raise NotProven("%s: the %.0f ms stall had ended before the host phase (%.2f ms without a stall) did: nothing is "
                        "proven" % (name, ms, host_ms))
    na, bad_a = differing(got_a, base_a)
    nc, bad_c = differing(got_c, base_c)
    line = "async-invariance %s host %.2f stall %.0f proved 1 words %d/%d" % (name, host_ms, ms, na + nc, bad_a + bad_c)
    out(line)
    assert na > 0 and nc > 0, "%s compared nothing" % name
    assert bad_a == 0 and bad_c == 0, ("%s: behind a stalled GPU %d of %d words of the call and %d of %d words of the call "
                                      "behind it differ from the synchronous run" % (name, bad_a, na, bad_c, nc))
    return line
