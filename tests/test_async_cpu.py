"""The host side of the asynchronous uploads and of the stall harness, without a GPU (tests/async_cases.py).
1. A tensor returned by hip_backend.to_device_* on the CPU owns its values: 20 uploads of one size, all kept, all intact.
2. The ring's discipline on a simulated GPU (copies read their pinned source when they RUN; the event type and the buffer
   type of the ring replaced by recorders): no buffer is rewritten before the copy that reads it has run, the host never
   blocks, a buffer whose copy is outstanding is kept until it has run; rings of different keys share nothing.
3. The harness: proved() is false once the event has fired, and a case whose stall ended early FAILS."""
import numpy as np
import pytest
import torch

import async_cases as A


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry._ensure_paths()
    import hip_backend
    return hip_backend


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind,dtype", [("i32", torch.int32), ("i64", torch.int64), ("f32", torch.float32)])
def test_cpu_uploads_own_their_values(hb, kind, dtype):
    up = dict(i32=hb.to_device_i32, i64=hb.to_device_i64, f32=hb.to_device_f32)[kind]
    values = [np.arange(4) + 10 * i for i in range(20)]
    kept = [up(v.astype(np.float32) if kind == "f32" else [int(x) for x in v], "cpu") for v in values]
    for i, (t, v) in enumerate(zip(kept, values)):
        assert t.dtype == dtype and t.shape == (4,)
        assert t.tolist() == v.tolist(), "upload %d holds %s after %d later uploads, not %s" % (i, t.tolist(), 19 - i, v.tolist())
    assert len(set(t.data_ptr() for t in kept)) == 20, "two uploads share their memory"


def test_cpu_upload_keeps_the_shape_and_is_detached_from_its_source(hb):
    src = np.arange(6, dtype=np.int32).reshape(2, 3)
    t = hb.to_device_i32(src, "cpu")
    src[:] = -1
    assert t.shape == (2, 3) and t.tolist() == [[0, 1, 2], [3, 4, 5]]


# ------------------------------------------------------------------------------------------------------------ 2
class _Gpu(object):
    """A GPU the test drives by hand: per stream a queue of copies and events that run, in order, when the test says so.  A
    copy reads its (pinned) source WHEN IT RUNS - that is what makes an early rewrite of the source a wrong result."""

    def __init__(self):
        self.queues, self.events, self.buffers, self.waits = {}, [], [], 0

    def copy(self, stream, buf):
        result = dict(value=None)
        self.queues.setdefault(stream, []).append(("copy", buf, result))
        return result

    def run(self, stream, n=None):
        q = self.queues.get(stream, [])
        for _ in range(len(q) if n is None else min(n, len(q))):
            kind, obj, result = q.pop(0)
            if kind == "copy":
                result["value"] = obj.value.tolist()
            else:
                obj.fired = True


def _fakes(gpu):
    class Event(object):
        def __init__(self):
            self.fired, self.queries = True, 0
            gpu.events.append(self)

        def record(self, stream=None):
            self.fired = False
            gpu.queues.setdefault(stream, []).append(("event", self, None))

        def query(self):
            self.queries += 1
            return self.fired

        def synchronize(self):
            gpu.waits += 1
            assert self.fired, "the host would block on a copy that has not run"

    class Buffer(object):
        def __init__(self, size, dtype):
            self.value = None
            gpu.buffers.append(self)

        def copy_(self, flat):
            self.value = flat.clone()
            return self
    return Event, Buffer


@pytest.fixture
def gpu(hb, monkeypatch):
    g = _Gpu()
    event, buffer = _fakes(g)
    monkeypatch.setattr(hb, "_ring_event", event)
    monkeypatch.setattr(hb, "_ring_buffer", buffer)
    return g


def _upload(hb, gpu, ring, values, stream):
    """What _to_device does with a ring: stage, enqueue the copy on `stream`, tell the ring."""
    k = hb._ring_stage(ring, torch.tensor(values, dtype=torch.int32))
    result = gpu.copy(stream, ring["bufs"][k])
    hb._ring_sent(ring, k, stream)
    return result


def test_the_simulated_gpu_shows_a_ring_without_events_to_be_wrong(gpu):
    """The parent commit's discipline - eight buffers, rewritten in turn without a look - on the simulated GPU: the first
    upload arrives with the ninth's values.  (The check below has teeth.)"""
    bufs = [_fakes(gpu)[1](4, torch.int32) for _ in range(8)]
    results = []
    for i in range(9):
        bufs[i % 8].copy_(torch.tensor([i] * 4, dtype=torch.int32))
        results.append(gpu.copy("s", bufs[i % 8]))
    gpu.run("s")
    assert results[0]["value"] == [8] * 4


def test_steady_state_takes_eight_buffers_and_one_look_per_lap(hb, gpu):
    ring = hb._ring_new(4, torch.int32)
    assert hb.RING_SLOTS == 8 and len(gpu.buffers) == 8
    results = []
    for i in range(40):
        results.append(_upload(hb, gpu, ring, [i] * 4, "s"))
        gpu.run("s")                                        # the GPU keeps up
    assert [r["value"] for r in results] == [[i] * 4 for i in range(40)]
    assert len(gpu.buffers) == 8 and not ring["retired"] and gpu.waits == 0
    assert len(gpu.events) == 5 and sum(e.queries for e in gpu.events) == 4, "one event and one look per lap"


def test_a_slot_is_never_rewritten_before_its_copy_has_run(hb, gpu):
    """25 uploads with no copy running at all (a GPU stalled for all of them), then the GPU catches up: every upload
    arrives with its own values, the host never waited, and no outstanding source was dropped."""
    ring = hb._ring_new(4, torch.int32)
    results = [_upload(hb, gpu, ring, [i] * 4, "s") for i in range(25)]
    assert gpu.waits == 0 and len(gpu.buffers) == 25, "a source was rewritten or the host waited"
    alive = [b for b, _ in ring["retired"]] + ring["bufs"]
    assert all(any(b is a for a in alive) for b in gpu.buffers), "an outstanding source was dropped"
    gpu.run("s")
    assert [r["value"] for r in results] == [[i] * 4 for i in range(25)]
    # once the copies have run the ring stops growing and lets the retired buffers go
    for i in range(25, 41):
        results.append(_upload(hb, gpu, ring, [i] * 4, "s"))
        gpu.run("s")
    assert len(gpu.buffers) == 25 and not ring["retired"]
    assert [r["value"] for r in results[25:]] == [[i] * 4 for i in range(25, 41)]


@pytest.mark.parametrize("seed", range(6))
def test_any_interleaving_of_uploads_streams_and_gpu_progress(hb, gpu, seed):
    """300 uploads on two streams that change at random (the upload stream switched on and off in the middle of a lap),
    the GPU advancing by random amounts on either: every upload arrives intact, the host never waits."""
    rs = np.random.RandomState(seed)
    ring = hb._ring_new(4, torch.int32)
    results, stream = [], "main"
    for i in range(300):
        if rs.rand() < 0.15:
            stream = "side" if stream == "main" else "main"
        results.append(_upload(hb, gpu, ring, [i] * 4, stream))
        if rs.rand() < 0.5:
            gpu.run(str(rs.choice(["main", "side"])), int(rs.randint(0, 12)))
    gpu.run("main")
    gpu.run("side")
    assert [r["value"] for r in results] == [[i] * 4 for i in range(300)]
    assert gpu.waits == 0


def test_rings_of_different_keys_do_not_interact(hb, gpu):
    """Ring a's stream is stalled, ring b's keeps up: b's progress frees nothing of a, a's backlog costs b nothing."""
    ra, rb = hb._ring_new(4, torch.int32), hb._ring_new(5, torch.int32)
    made = len(gpu.buffers)
    res_a, res_b = [], []
    for i in range(20):
        res_a.append(_upload(hb, gpu, ra, [i] * 4, "a"))
        res_b.append(_upload(hb, gpu, rb, [100 + i] * 5, "b"))
        gpu.run("b")
    assert not set(id(x) for x in ra["bufs"]) & set(id(x) for x in rb["bufs"])
    assert not rb["retired"] and len(ra["retired"]) == 12 and len(gpu.buffers) == made + 12
    assert ra["i"] == rb["i"] == 20
    gpu.run("a")
    assert [r["value"] for r in res_a] == [[i] * 4 for i in range(20)]
    assert [r["value"] for r in res_b] == [[100 + i] * 5 for i in range(20)]


# ------------------------------------------------------------------------------------------------------------ 3
class _Fired(object):
    def __init__(self, fired):
        self.fired = fired

    def query(self):
        return self.fired


def test_proved_is_false_once_the_event_has_fired():
    assert A.Stall(_Fired(False), 50.0).proved()
    assert not A.Stall(_Fired(True), 50.0).proved()


def test_stall_length_is_twenty_host_times_within_its_bounds():
    assert A.stall_ms(0.1) == 50.0 and A.stall_ms(10.0) == 200.0 and A.stall_ms(500.0) == 2000.0


def _cpu_case(fired, lines, wrong=False):
    calls = []

    def call(tr):
        calls.append(1)
        x = tr.dev(np.arange(8, dtype=np.float32), "cpu")
        return dict(y=x * 2 + (1 if wrong and len(calls) > 2 else 0))
    return A.run_case("fake", call, call, device="cpu", stall=lambda stream, ms: A.Stall(_Fired(fired), ms),
                      sync=lambda: None, out=lines.append)


def test_a_case_whose_stall_ended_early_fails():
    lines = []
    with pytest.raises(A.NotProven):
        _cpu_case(True, lines)
    assert len(lines) == 1 and " proved 0" in lines[0]


def test_a_proven_case_passes_and_a_differing_one_fails():
    lines = []
    line = _cpu_case(False, lines)
    assert lines == [line] and line.startswith("async-invariance fake host ") and line.endswith(" proved 1 words 16/0")
    with pytest.raises(AssertionError) as e:
        _cpu_case(False, lines, wrong=True)
    assert not isinstance(e.value, A.NotProven) and lines[-1].endswith("words 16/16")
