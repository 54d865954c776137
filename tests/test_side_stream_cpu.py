"""The bookkeeping that decides whether a weight gradient may leave for the side stream (ops._SideStream.count_use /
may_defer) and which flat buffers keep the side stream off (parallel.FlatBuffers.enable_overlap), on CPU:
the decision is host logic; tests/test_side_stream_gpu.py holds the gradients themselves."""
import socket

import pytest
import torch
import torch.distributed as dist


class _Use(torch.autograd.Function):
    """A stand-in for ops._Linear's bookkeeping: counts its use of w, records the decision its backward would take."""
    log = []

    @staticmethod
    def forward(ctx, x, w):
        import ops
        ctx.side_mask = 0
        if ctx.needs_input_grad[1]:
            ops._SIDE.count_use(ctx, w)
            ctx.side_mask = 0xF0
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        import ops
        x, w = ctx.saved_tensors
        _Use.log.append(bool(ops._SIDE.may_defer(ctx, w)))
        return dy @ w, dy.t() @ x


@pytest.fixture
def side():
    import ops
    s = ops._SIDE
    saved = s.enabled
    s.enabled = True
    del _Use.log[:]
    yield s
    s.enabled = saved


def test_a_use_counts_while_its_graph_lives(side):
    w = torch.randn(3, 4, requires_grad=True)
    x = torch.randn(5, 4, requires_grad=True)
    key = w.data_ptr()
    y = _Use.apply(x, w).sum()
    assert side.uses.get(key) == 1
    del y                                              # a forward whose backward never runs
    assert key not in side.uses
    with torch.no_grad():
        _Use.apply(x, w)
    assert key not in side.uses
    _Use.apply(x, w).sum().backward()
    assert _Use.log == [True]                          # the single use defers ...
    _Use.apply(x, w.detach()).sum()                    # (no gradient wanted: not a use)
    assert key not in side.uses


def test_no_deferral_with_a_second_use_a_grad_or_a_hook(side):
    w = torch.randn(3, 4, requires_grad=True)
    x = torch.randn(5, 4, requires_grad=True)
    (_Use.apply(x, w).sum() + _Use.apply(x[:2], w).sum()).backward()
    assert _Use.log == [False, False]                  # two uses in one graph, whatever their shapes
    del _Use.log[:]
    w.grad = None
    keep = _Use.apply(x, w).sum()                      # a live graph of another use ...
    _Use.apply(x, w).sum().backward()
    assert _Use.log == [False]
    del keep
    del _Use.log[:]
    w.grad = None
    _Use.apply(x, w).sum().backward()                  # ... gone: defers
    assert _Use.log == [True]
    del _Use.log[:]
    _Use.apply(x, w).sum().backward()                  # .grad holds the previous gradient: autograd adds in place
    assert _Use.log == [False]
    w.grad = None
    h = w.register_post_accumulate_grad_hook(lambda p: None)
    _Use.apply(x, w).sum().backward()
    h.remove()
    w.grad = None
    h = w.register_hook(lambda g: g)
    _Use.apply(x, w).sum().backward()
    h.remove()
    w.grad = None
    _Use.apply(x, w).sum().backward()                  # hooks removed: defers again
    assert _Use.log == [False, False, False, True]
    w2 = w * 2.0                                       # not a leaf: its gradient goes on to another node
    _Use.apply(x, w2).sum().backward()
    assert _Use.log[-1] is False


def test_overlapping_buffers_keep_the_side_stream_off(side, monkeypatch):
    """Two buffers overlap (the generator's and the judge's under dp_overlap); disabling one leaves the side stream off,
    disabling the last restores what it was; a buffer that never overlapped changes nothing."""
    import parallel
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        a = parallel.FlatBuffers([torch.randn(8, requires_grad=True)])
        b = parallel.FlatBuffers([torch.randn(8, requires_grad=True)])
        c = parallel.FlatBuffers([torch.randn(8, requires_grad=True)])
        a.enable_overlap(force=True)
        b.enable_overlap(force=True)
        assert a.overlap and b.overlap and not side.enabled
        b.disable_overlap()
        assert not side.enabled, "the side stream came back on while a's hooks are live"
        c.disable_overlap()
        b.disable_overlap()
        assert not side.enabled
        a.disable_overlap()
        assert side.enabled
        side.enabled = False                           # ... and what it was, not the environment's default
        a.enable_overlap(force=True)
        a.disable_overlap()
        assert not side.enabled
    finally:
        dist.destroy_process_group()
