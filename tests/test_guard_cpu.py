"""tests/guard.py itself, on host tensors: the geometry of a fenced tensor, the positive controls (a byte in front of the
data, a byte behind it, a stray 1 in an integer band), the scope, the completeness of the wrapped allocation functions
against the product modules' source, and the bitwise snapshots.  No GPU."""
import os
import re

import pytest
import torch

import guard

CPU = ("cpu",)
ORIGINALS = tuple(getattr(torch, n) for n in guard.TORCH_FUNCS) + tuple(getattr(torch.Tensor, n) for n in guard.TENSOR_METHODS)
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semi-supervised-asr_amd")


def _originals_back():
    return tuple(getattr(torch, n) for n in guard.TORCH_FUNCS) + tuple(getattr(torch.Tensor, n) for n in guard.TENSOR_METHODS) == ORIGINALS


def _values(n, dtype):
    if dtype == torch.bool:
        return torch.arange(n) % 3 == 0
    return (torch.arange(n) * 7 - 5).to(dtype)


def _at(t, k, n=1):
    """n elements from element k of the 1-D fenced tensor t - k < 0 and k >= len(t) lie in the bands - through as_strided."""
    return t.as_strided((n,), (1,), t.storage_offset() + k)


def _bytes_view(rec):
    """The whole private buffer of a record as plain bytes, through as_strided on the base."""
    return rec.base.as_strided((rec.base.numel(),), (1,), 0)


def test_band_is_what_the_issue_says_and_the_nan_word_is_the_gemm_sentinel():
    import gemm_terms_ref
    assert guard.BAND == 8192 and guard.BAND % 256 == 0 and guard.BAND == 2 * 256 * 16
    assert guard.NAN_WORD == gemm_terms_ref.SENTINEL == 0x7fc5a5a5
    assert guard.band_pattern(torch.float32, "one", nan=True) == bytes([0xa5, 0xa5, 0xc5, 0x7f])
    assert guard.band_pattern(torch.float32, "one") == bytes([1, 0, 0, 0]) == guard.band_pattern(torch.float64, "one")
    assert guard.band_pattern(torch.float16, "zero") == bytes(4)
    assert guard.band_pattern(torch.int64, "one") == bytes([1, 0, 0, 0, 0, 0, 0, 0])
    assert guard.band_pattern(torch.bool, "one") == bytes([1]) and guard.band_pattern(torch.int32, "zero") == bytes(4)
    with pytest.raises(ValueError):
        guard.band_pattern(torch.int32, "one", nan=True)      # an integer band never holds anything but 0 or 1
    with pytest.raises(ValueError):
        guard.band_pattern(torch.int32, "two")


@pytest.mark.parametrize("pattern", guard.INT_PATTERNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64, torch.bool])
@pytest.mark.parametrize("n", [1, 3, 33, 257])
def test_geometry(n, dtype, pattern):
    src = _values(n, dtype)
    st = guard.Stats()
    t = guard.fence(src, int_pattern=pattern, stats=st)
    es = src.element_size()
    assert t.dtype == dtype and t.shape == src.shape and t.is_contiguous() and torch.equal(t, src)
    assert t.data_ptr() != src.data_ptr()
    rec, = st.records
    assert rec.nbytes == n * es and rec.base.dtype == torch.uint8 and rec.base.dim() == 1
    assert rec.base.numel() == guard.BAND + n * es + guard.BAND             # nbytes is not rounded
    # the data starts exactly at the end of the front band and ends exactly where the back band starts
    assert t.data_ptr() - rec.base.data_ptr() == guard.BAND and t.data_ptr() % 16 == 0
    front, back = rec.bands()
    assert front.numel() == back.numel() == guard.BAND
    assert front.data_ptr() + guard.BAND == t.data_ptr() and back.data_ptr() == t.data_ptr() + n * es
    # contents: the tensor's own dtype holds 1 / 0 (integers, bool), 32-bit words of integer value 1 / 0 (floats)
    want = 1 if pattern == "one" else 0
    for band in (front, back):
        if dtype.is_floating_point:
            words = torch.frombuffer(bytearray(bytes(band.tolist())), dtype=torch.int32)
        else:
            words = band.view(dtype).to(torch.int64)
        assert bool((words == want).all())
    assert st.allocs == {dtype: 1} and st.bytes == {dtype: n * es} and st.n_allocs == 1 and st.n_bytes == n * es
    assert st.n_bands == 2 and st.unfenced == []
    assert guard.check(st) == 2


def test_nan_band_of_a_float_tensor_the_test_fences():
    st = guard.Stats()
    t = guard.fence(torch.arange(33, dtype=torch.float32), nan=True, stats=st)
    for band in st.records[0].bands():
        words = torch.frombuffer(bytearray(bytes(band.tolist())), dtype=torch.int32)
        assert bool((words == guard.NAN_WORD).all())
        assert bool(torch.isnan(torch.frombuffer(bytearray(bytes(band.tolist())), dtype=torch.float32)).all())
    assert t[32] == 32 and guard.check(st) == 2


def test_half_floats_at_an_odd_count_end_on_no_word_boundary():
    st = guard.Stats()
    t = guard.fence(torch.arange(33, dtype=torch.float16), stats=st)
    rec, = st.records
    assert rec.nbytes == 66 and rec.base.numel() == 2 * guard.BAND + 66 and float(t[32]) == 32.0
    assert bytes(rec.bands()[1][:8].tolist()) == bytes([1, 0, 0, 0, 1, 0, 0, 0])
    assert guard.check(st) == 2


def test_shapes_scalars_and_empty_tensors():
    st = guard.Stats()
    a = guard.fenced_empty((3, 5), torch.float32, "cpu", stats=st)
    b = guard.fence(torch.tensor(2.5), stats=st)
    c = guard.fenced_empty((0, 4), torch.int32, "cpu", stats=st)
    d = guard.fence(torch.ones(3, requires_grad=True), stats=st)
    assert a.shape == (3, 5) and a.stride() == (5, 1) and b.shape == () and float(b) == 2.5 and c.shape == (0, 4)
    assert d.requires_grad and d.is_leaf
    assert [r.nbytes for r in st.records] == [60, 4, 0, 12] and st.records[2].base.numel() == 2 * guard.BAND
    assert guard.check(st) == 8
    with pytest.raises(ValueError):
        guard.fence(torch.zeros(4, 4).t())


# ------------------------------------------------------------------------------------------------- positive controls
def _stray_byte(rec, at, value=0xee):
    """A plain torch write through an as_strided view of the base buffer, `at` bytes from the start of the data."""
    _bytes_view(rec).as_strided((1,), (1,), guard.BAND + at).fill_(value)


@pytest.mark.parametrize("dtype,n", [(torch.float32, 33), (torch.int32, 3), (torch.int64, 1), (torch.bool, 257)])
def test_one_byte_before_and_one_byte_after_the_data_are_reported(dtype, n):
    here = "test_guard_cpu.py:"
    for side, at in (("front", -1), ("back", None)):
        st = guard.Stats()
        t = guard.fence(_values(n, dtype), stats=st)
        rec, = st.records
        at = rec.nbytes if at is None else at
        assert guard.check(st) == 2                              # an intact buffer passes
        _stray_byte(rec, at)
        with pytest.raises(guard.GuardError) as e:
            guard.check(st)
        d, = e.value.damage
        assert (d.side, d.offset, d.nbytes) == (side, at, 1) and d.record is rec
        assert rec.site.startswith(here) and rec.site in str(e.value)
        assert side in str(e.value) and "data%+d" % at in str(e.value) and str(list(t.shape)) in str(e.value)
        assert str(dtype).replace("torch.", "") in str(e.value)
        assert any(w != int.from_bytes((rec.pattern * 4)[:4], "little") for w in d.words)
        assert torch.equal(t, _values(n, dtype))                 # (the data itself was not touched)


def test_the_call_site_is_the_line_of_the_allocation():
    import inspect
    st = guard.Stats()
    line = inspect.currentframe().f_lineno + 1
    guard.fenced_empty((4,), torch.float32, "cpu", stats=st)
    with guard.guarded("one", st, devices=CPU):
        line2 = inspect.currentframe().f_lineno + 1
        torch.zeros(3)
    assert [r.site for r in st.records] == ["test_guard_cpu.py:%d" % line, "test_guard_cpu.py:%d" % line2]


def test_a_write_of_1_into_an_integer_band_is_missed_under_one_and_caught_under_zero():
    """Why both patterns run: a kernel that stores the VALUE 1 one element too far."""
    seen = {}
    for pattern in guard.INT_PATTERNS:
        st = guard.Stats()
        t = guard.fence(torch.arange(33, dtype=torch.int32), int_pattern=pattern, stats=st)
        _at(t, 33).fill_(1)                    # element [33] of a tensor of 33: the first word of the band
        seen[pattern] = guard.damage(st)
    assert seen["one"] == []
    d, = seen["zero"]
    assert (d.side, d.offset, d.nbytes, d.words[0]) == ("back", 132, 1, 1)
    # and the other way round for a stray 0
    for pattern, n_found in (("one", 1), ("zero", 0)):
        st = guard.Stats()
        t = guard.fence(torch.arange(33, dtype=torch.int32), int_pattern=pattern, stats=st)
        _at(t, -1).fill_(0)
        assert len(guard.damage(st)) == n_found
    # the float workspaces of the library follow the same rule: 32-bit words
    for pattern, n_found in (("one", 0), ("zero", 1)):
        with guard.guarded(pattern, devices=CPU) as st:
            ws = torch.empty(33)
        _at(ws.view(torch.int32), 33).fill_(1)
        assert len(guard.damage(st)) == n_found


def test_several_damaged_allocations_are_all_named():
    st = guard.Stats()
    a = guard.fence(torch.zeros(5), stats=st)
    guard.fence(torch.zeros(6), stats=st)
    c = guard.fence(torch.zeros(7, dtype=torch.int64), stats=st)
    _at(a, 5, 3).fill_(9.0)
    _at(c, -2).fill_(-1)
    with pytest.raises(guard.GuardError) as e:
        guard.check(st)
    got = [(d.record.shape, d.side, d.offset, d.nbytes) for d in e.value.damage]
    assert got == [((5,), "back", 20, 3 * 3), ((7,), "front", -16, 8)]       # (9.0f = 0x41100000: 3 of its 4 bytes differ
    assert e.value.damage[0].words[:3] == [0x41100000] * 3                       # from the band's 01 00 00 00, one is 00)
    assert e.value.damage[1].words[:2] == [0xffffffff, 0xffffffff]


# ------------------------------------------------------------------------------------------------- the scope
def test_every_wrapped_function_fences_and_keeps_its_semantics():
    base = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    with guard.guarded("zero", devices=CPU) as st:
        made = dict(empty=torch.empty(2, 3), empty_kw=torch.empty((4,), dtype=torch.int32), empty_like=torch.empty_like(base),
                    empty_strided=torch.empty_strided((3, 2), (2, 1)), zeros=torch.zeros(3, 2, dtype=torch.int64),
                    zeros_like=torch.zeros_like(base), full=torch.full((5,), 7), full_f=torch.full((2, 2), -1.5),
                    full_like=torch.full_like(base, 3.0), ones=torch.ones(4, dtype=torch.bool), new_empty=base.new_empty((5,)),
                    new_zeros=base.new_zeros(2, 2, dtype=torch.float32), new_full=base.new_full((3,), 2.0),
                    grad=torch.zeros(3, requires_grad=True))
        meta = torch.empty((2, 2), device="meta")
    assert meta.device.type == "meta"
    assert made["empty"].shape == (2, 3) and made["empty_kw"].dtype == torch.int32 and made["empty_like"].dtype == torch.float64
    assert made["empty_strided"].stride() == (2, 1) and made["new_empty"].dtype == torch.float64
    assert made["zeros"].dtype == torch.int64 and not made["zeros"].any() and not made["zeros_like"].any()
    assert made["full"].dtype == torch.int64 and made["full"].tolist() == [7] * 5 and bool((made["full_f"] == -1.5).all())
    assert bool((made["full_like"] == 3.0).all()) and made["full_like"].shape == (2, 3) and made["ones"].all()
    assert made["new_zeros"].dtype == torch.float32 and not made["new_zeros"].any() and made["new_full"].tolist() == [2.0] * 3
    assert made["grad"].requires_grad and made["grad"].is_leaf
    assert st.n_allocs == len(made) == 14 and st.unfenced == []
    ptrs = {r.base.data_ptr() + guard.BAND for r in st.records}
    assert all(t.data_ptr() in ptrs for t in made.values())
    assert st.allocs[torch.float64] == 5 and st.bytes[torch.int64] == 6 * 8 + 5 * 8
    assert "14 fenced" in st.line() and guard.check(st) == 28
    assert _originals_back()


def test_only_the_named_devices_are_fenced_and_pinned_memory_is_left_alone():
    with guard.guarded("one") as st:                             # the default: device tensors only
        t = torch.empty(5)
        z = torch.zeros(3, dtype=torch.int32)
    assert st.n_allocs == 0 and st.unfenced == [] and t.shape == (5,) and not z.any()
    assert guard._fenceable(torch.empty(3), CPU) == "" and guard._fenceable(torch.empty(3), ("cuda",)) is None


def test_restored_after_an_exception():
    with pytest.raises(RuntimeError, match="boom"):
        with guard.guarded("one", devices=CPU):
            assert torch.empty is not ORIGINALS[0] and torch.Tensor.new_zeros is not ORIGINALS[-2]
            torch.empty(2)
            raise RuntimeError("boom")
    assert _originals_back()
    with pytest.raises(ValueError):
        with guard.guarded("two"):
            pass
    assert _originals_back()


def test_a_non_contiguous_empty_strided_is_passed_through_and_listed():
    import inspect
    proto = torch.zeros(3, 4).t()
    with guard.guarded("one", devices=CPU) as st:
        line = inspect.currentframe().f_lineno + 1
        t = torch.empty_strided((4, 3), (1, 4))
        u = torch.empty_like(proto)
        ok = torch.empty_strided((4, 3), (3, 1))
    assert t.stride() == (1, 4) and u.stride() == (1, 4) and st.n_allocs == 1 and ok.is_contiguous()
    assert len(st.unfenced) == 2
    what, site = st.unfenced[0]
    assert "empty_strided" in what and "[4, 3]" in what and "(1, 4)" in what and site == "test_guard_cpu.py:%d" % line
    assert st.unfenced[1][0].startswith("empty_like")


def test_stats_merge():
    a, b = guard.Stats(), guard.Stats()
    guard.fence(torch.zeros(3), stats=a)
    guard.fence(torch.zeros(2, dtype=torch.int32), stats=b)
    b.unfenced.append(("x", "y"))
    a.merge(b)
    assert a.allocs == {torch.float32: 1, torch.int32: 1} and a.n_bytes == 20 and a.n_bands == 4 and a.unfenced == [("x", "y")]


# ------------------------------------------------------------------------------------------------- completeness
# every torch function that creates a new tensor from a size, a prototype or host data
CREATORS = frozenset("""empty empty_like empty_strided empty_permuted zeros zeros_like ones ones_like full full_like rand rand_like
randn randn_like randint randint_like randperm normal arange range linspace logspace eye tensor as_tensor asarray from_numpy
frombuffer scalar_tensor tril_indices triu_indices hann_window hamming_window blackman_window bartlett_window kaiser_window
sparse_coo_tensor complex polar""".split())
# the ones the product modules call that need no fence, each with the reason
ALLOWED = {
    "tensor": "input construction from host values (lengths, offsets, tables): uploaded, never a kernel's output",
    "from_numpy": "input construction: wraps host memory of the caller",
    "arange": "input construction (index vectors), written by torch itself",
    "randint": "a host draw of torch's own sampler (the seed of hb.SeededMask), read back with .item()",
    "new_tensor": "input construction from host values, like torch.tensor",
}


def test_every_allocation_call_of_the_product_modules_is_wrapped():
    called, methods = {}, {}
    for mod in guard.PRODUCT_MODULES:
        src = open(os.path.join(PKG, mod + ".py")).read()
        for m in re.finditer(r"\btorch\.([A-Za-z_0-9]+)\(", src):
            called.setdefault(m.group(1), set()).add(mod)
        for m in re.finditer(r"\.(new_[A-Za-z_0-9]+)\(", src):
            methods.setdefault(m.group(1), set()).add(mod)
    assert "empty" in called and "zeros" in called and "new_zeros" in methods, "the scan found nothing: did the modules move?"
    wrapped = set(guard.TORCH_FUNCS) | set(guard.TENSOR_METHODS)
    missing = {n: sorted(mods) for n, mods in called.items() if n in CREATORS and n not in wrapped and n not in ALLOWED}
    missing.update({n: sorted(mods) for n, mods in methods.items() if n not in wrapped and n not in ALLOWED})
    assert not missing, "allocation calls guard.guarded() does not wrap (wrap them, or allow them with a reason): %r" % missing
    for name in ALLOWED:
        assert name not in wrapped and (name in called or name in methods), "%s is allowed but no longer called" % name
    for name in guard.TORCH_FUNCS:
        assert name in CREATORS and callable(getattr(torch, name))
    # the randint of the allow-list is a host draw: if it moves to the device it becomes a kernel output
    for mod in called["randint"]:
        for line in open(os.path.join(PKG, mod + ".py")):
            if "torch.randint(" in line:
                assert "device=" not in line, line


# ------------------------------------------------------------------------------------------------- snapshots
def test_frozen_and_assert_frozen_on_tensors_holding_nan():
    a = torch.tensor([1.0, float("nan"), -0.0, float("inf")])
    b = torch.tensor([3, -1], dtype=torch.int64)
    c = torch.tensor([True, False])
    d = torch.full((2, 3), float("nan")).t()                    # (a non-contiguous input is snapshotted by value)
    snap = guard.frozen(a, None, b, c, d)
    guard.assert_frozen(snap)                                    # NaN compares equal to itself
    a[2] = 0.0                                                   # -0.0 -> +0.0: equal as floats, not as bits
    with pytest.raises(AssertionError, match="const input 0 .*1 byte"):
        guard.assert_frozen(snap, "case")
    a[2] = -0.0
    guard.assert_frozen(snap)
    a[1] = torch.tensor([0x7fc5a5a5], dtype=torch.int32).view(torch.float32)[0]     # another NaN
    with pytest.raises(AssertionError, match="const input 0"):
        guard.assert_frozen(snap)
    snap = guard.frozen(a, b, c)
    c[1] = True
    with pytest.raises(AssertionError, match="const input 2 .bool"):
        guard.assert_frozen(snap)
