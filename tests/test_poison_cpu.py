"""tests/poison.py itself, on host tensors: the patterns per dtype, restoration, the counters, the pool walk, and the rule
that an integer tensor never receives anything but 0 or 1.  No GPU."""
import math

import pytest
import torch

import poison

FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
INTS = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
H32 = float(torch.tensor(3e38, dtype=torch.float32))         # 3e38 as float32 holds it
ORIGINALS = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)


def _originals_back():
    return (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == ORIGINALS


@pytest.mark.parametrize("dtype", FLOATS)
def test_float_patterns(dtype):
    with poison.poisoned("nan"):
        t = torch.empty(3, 5, dtype=dtype)
    assert bool(torch.isnan(t).all())
    with poison.poisoned("huge"):
        t = torch.empty(3, 5, dtype=dtype)
    want = min(3e38, torch.finfo(dtype).max)
    assert bool(torch.isfinite(t).all())                     # huge is a finite number in every format
    assert bool((t.double() == torch.tensor(want, dtype=dtype).double()).all())
    assert float(t.double().min()) >= 6e4                    # (float16's largest; 3e38 itself in the wider formats)
    with poison.poisoned("zero"):
        t = torch.empty(3, 5, dtype=dtype)
    assert bool((t == 0).all())


def test_complex_pattern():
    with poison.poisoned("nan"):
        t = torch.empty(4, dtype=torch.complex64)
    assert bool(torch.isnan(t.real).all())
    with poison.poisoned("huge"):
        t = torch.empty(4, dtype=torch.complex64)
    assert bool((t.real == torch.tensor(3e38, dtype=torch.float32)).all())


@pytest.mark.parametrize("dtype", INTS + (torch.bool,))
@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_integer_tensors_only_ever_hold_0_or_1(dtype, pattern):
    want = 0 if pattern == "zero" else 1
    assert int(poison.fill_value(dtype, pattern)) == want
    with poison.poisoned(pattern):
        made = [torch.empty(7, 3, dtype=dtype), torch.empty_like(torch.full((5,), 99).to(dtype) if dtype != torch.bool
                                                                 else torch.ones(5, dtype=dtype)),
                torch.empty_strided((4, 3), (1, 4), dtype=dtype), torch.zeros(2, dtype=torch.float32).new_empty((6,), dtype=dtype)]
    for t in made:
        assert t.dtype == dtype
        assert bool((t.to(torch.int64) == want).all())
    # the pool walk obeys the same rule
    tree = dict(a=torch.full((9,), 1).to(dtype) if dtype == torch.bool else torch.full((9,), 77).to(dtype))
    assert poison.poison_tree(tree, pattern) == 1
    assert bool((tree["a"].to(torch.int64) == want).all())


def test_every_entry_point_is_patched_and_keeps_its_semantics():
    base = torch.zeros(2, 3, dtype=torch.float64)
    with poison.poisoned("nan") as st:
        a = torch.empty(2, 3)
        b = torch.empty((4,), dtype=torch.float64)
        c = torch.empty_like(base)
        d = torch.empty_strided((3, 2), (1, 3))
        e = base.new_empty((5,))
        f = base.new_empty(2, 2, dtype=torch.float32)
        z = torch.empty(0)                                   # (nothing to fill: not counted)
        m = torch.empty((2, 2), device="meta")               # (no memory behind it: not counted)
    assert a.shape == (2, 3) and b.dtype == torch.float64 and c.shape == base.shape and c.dtype == torch.float64
    assert d.stride() == (1, 3) and e.dtype == torch.float64 and f.dtype == torch.float32
    assert z.numel() == 0 and m.device.type == "meta"
    for t in (a, b, c, d, e, f):
        assert bool(torch.isnan(t).all())
    assert st.n_allocs == 6
    assert st.allocs == {torch.float32: 3, torch.float64: 3}
    assert st.bytes == {torch.float32: (6 + 6 + 4) * 4, torch.float64: (4 + 6 + 5) * 8}
    assert st.n_bytes == 64 + 120 and st.total == 6 and st.pool_tensors == 0
    assert "6 allocations" in st.line()


def test_a_tensor_that_requires_grad_is_filled_too():
    with poison.poisoned("huge"):
        t = torch.empty(3, requires_grad=True)
    assert t.requires_grad and t.is_leaf and bool((t.detach() == 3e38).all())


def test_restored_after_exit():
    with poison.poisoned("nan"):
        assert torch.empty is not ORIGINALS[0] and torch.Tensor.new_empty is not ORIGINALS[3]
    assert _originals_back()


def test_restored_after_an_exception():
    with pytest.raises(RuntimeError, match="boom"):
        with poison.poisoned("huge"):
            torch.empty(2)
            raise RuntimeError("boom")
    assert _originals_back()


def test_nested_scopes_restore_in_order():
    with poison.poisoned("zero") as outer:
        with poison.poisoned("nan") as inner:
            t = torch.empty(2)
        u = torch.empty(2)
    assert math.isnan(float(t[0])) and float(u[0]) == 0.0
    assert inner.n_allocs == 1 and outer.n_allocs == 2       # (the outer scope sees the inner one's allocation as well)
    assert _originals_back()


def test_unknown_pattern_patches_nothing():
    with pytest.raises(ValueError):
        with poison.poisoned("garbage"):
            pass
    assert _originals_back()
    with pytest.raises(ValueError):
        poison.fill_value(torch.int32, "big")


def test_shared_stats_accumulate():
    st = poison.Stats()
    with poison.poisoned("nan", st):
        torch.empty(2)
    with poison.poisoned("zero", st):
        torch.empty(3, dtype=torch.int32)
    assert st.allocs == {torch.float32: 1, torch.int32: 1} and st.n_bytes == 8 + 12
    other = poison.Stats()
    other.pool_tensors = 2
    assert st.merge(other).total == 4


class _Buffers(object):
    """Stands for hb.DecBuffers: tensors as attributes, some of them the caller's (bind())."""

    def __init__(self):
        self.X = torch.ones(2, 3)
        self.fed = torch.full((4,), 1000, dtype=torch.int64)
        self.none = None
        self.dims = dict(B=2)
        self.acc = dict(G=torch.ones(3), parts=[torch.ones(2), (torch.ones(1), torch.ones(1))])
        self.wdec = torch.ones(2, 2)                         # a model parameter kept alive by bind(): not the workspace's
        self.name = "x"


class _Slotted(object):
    __slots__ = ("path", "score", "unset")

    def __init__(self):
        self.path, self.score = torch.full((3,), 50, dtype=torch.int32), torch.ones(3)


def test_pool_walk_over_dicts_lists_and_objects():
    lens = torch.tensor([9, 7, 4], dtype=torch.int32)
    buf = _Buffers()
    shared = torch.ones(5)
    free = {("lstm", 0, 256): [dict(gates_buf=torch.ones(4, 2), y=shared, y_again=shared, lens=lens, rows_written=12)],
            ("dec", 0): [buf, _Slotted()],
            ("ctc", "cpu", 256): [torch.ones(8), torch.ones(0)],
            "empty": []}
    st = poison.Stats()
    n = poison.poison_tree(free, "nan", st)
    # gates_buf, y (once: y_again is the same tensor object), X, fed, G, 1 + 2 parts, path, score, the ctc buffer
    assert n == 11 and st.pool_tensors == 11
    assert free[("lstm", 0, 256)][0]["rows_written"] == 4     # every row of gates_buf is stale now, and the note says so
    assert bool(torch.isnan(free[("lstm", 0, 256)][0]["gates_buf"]).all()) and bool(torch.isnan(shared).all())
    assert bool(torch.isnan(buf.X).all()) and bool(torch.isnan(buf.acc["G"]).all())
    assert all(bool(torch.isnan(t).all()) for t in (buf.acc["parts"][0],) + buf.acc["parts"][1])
    assert bool((buf.fed == 1).all())                        # an integer: 1, never NaN's bit pattern or a large value
    sl = free[("dec", 0)][1]
    assert bool((sl.path == 1).all()) and bool(torch.isnan(sl.score).all())
    # what the workspace only refers to stays as it was
    assert lens.tolist() == [9, 7, 4] and bool((buf.wdec == 1).all())
    assert poison.POOL_SKIP >= {"lens", "wdec", "watt", "P", "Q"}
    # the same walk with nothing skipped reaches them
    assert poison.poison_tree(dict(lens=lens), "zero", skip=()) == 1 and lens.tolist() == [0, 0, 0]


def test_walk_survives_cycles():
    a = dict(t=torch.ones(2))
    a["self"] = a
    assert poison.poison_tree(a, "huge") == 1 and float(a["t"][0]) == H32


def test_poison_pool_walks_the_three_places(monkeypatch):
    import types
    import sys
    fake_ops = types.SimpleNamespace(_POOL=types.SimpleNamespace(free={"k": [dict(a=torch.ones(3))]}),
                                     _ARENA=types.SimpleNamespace(buf=torch.zeros(4)))
    fake_hb = types.SimpleNamespace(_det_ws_cache={("d", 0): torch.ones(6)},
                                    _pinned_ring={("cpu", "i32", 4): dict(bufs=[torch.full((4,), 9, dtype=torch.int32)], i=3)})
    monkeypatch.setitem(sys.modules, "ops", fake_ops)
    monkeypatch.setitem(sys.modules, "hip_backend", fake_hb)
    st = poison.Stats()
    assert poison.poison_pool("huge", st) == 3 and st.pool_tensors == 3 and st.total == 3
    assert float(fake_ops._POOL.free["k"][0]["a"][0]) == H32
    assert float(fake_hb._det_ws_cache[("d", 0)][5]) == H32
    ring = fake_hb._pinned_ring[("cpu", "i32", 4)]
    assert ring["bufs"][0].tolist() == [1, 1, 1, 1] and ring["i"] == 3
    assert poison.arena_is_zero()
    fake_ops._ARENA.buf[2] = 1e-30
    assert not poison.arena_is_zero()
    poison.empty_pool()
    assert not fake_ops._POOL.free and not fake_hb._det_ws_cache and not fake_hb._pinned_ring
