"""CPU: held streams of the graphed hops — the hilc_state_slots_hold entry point (additive under ABI 16) and its argument
checks, its custom op and fake kernel, and the host-side hold / stop bookkeeping of SessionQueue.  (No kernel is launched here.)"""
import ctypes

import pytest
import torch

from tests.hops import assert_entry_points, bare_model


def test_hold_symbol_exported_and_declared():
    assert_entry_points(["hilc_state_slots_hold"])


def test_hold_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_state_slots_hold
    # (src, dst, slice_off, slice_len, nslices, streams, hold, wav, wav_len, indices, n_max, frames, packets, stride, nbytes, stream)
    outs = (p, 320, p, 8, 1, p, 100, p)
    none = (None, 0, None, 0, 0, None, 0, None)
    for k in range(5):                                    # src, dst, slice_off, slice_len, hold
        args = [p, p, p, p, 52, 4, p]
        args[k if k < 4 else 6] = None
        assert f(*args, *outs, None) == -2, k
    assert f(p, p, p, p, 0, 4, p, *outs, None) == -1
    assert f(p, p, p, p, 52, 0, p, *outs, None) == -1
    assert f(p, p, p, p, 52, -3, p, *outs, None) == -1
    assert f(p, p, p, p, 129, 4, p, *outs, None) == -4    # the slice table is staged in LDS
    # null outputs pass the pointer checks (the call fails on the shape instead: nothing is launched)
    assert f(p, p, p, p, 0, 4, p, *none, None) == -1
    assert f(p, p, p, p, 129, 4, p, *none, None) == -4
    # a given output needs its length
    assert f(p, p, p, p, 52, 4, p, p, 0, None, 0, 0, None, 0, None, None) == -1
    assert f(p, p, p, p, 52, 4, p, None, 0, p, 0, 1, None, 0, None, None) == -1
    assert f(p, p, p, p, 52, 4, p, None, 0, p, 8, 0, None, 0, None, None) == -1
    assert f(p, p, p, p, 52, 4, p, None, 0, None, 0, 0, p, 0, None, None) == -1


def test_hold_op_registered_with_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hilcodec_amd import graph_step as G
    layout = G.state_layout(bare_model(), 5)
    assert hasattr(torch.ops.hilcodec, "state_slots_hold")
    schema = str(torch.ops.hilcodec.state_slots_hold.default._schema)
    for arg in ("Tensor(a!) dst", "Tensor(b!)? wav", "Tensor(c!)? indices", "Tensor(d!)? packets", "Tensor(e!)? nbytes"):
        assert arg in schema, arg
    with FakeTensorMode():
        src, dst = torch.empty(layout.total), torch.empty(layout.total)
        off, lens = torch.empty(52, dtype=torch.int64), torch.empty(52, dtype=torch.int32)
        hold = torch.empty(5, dtype=torch.int32)
        assert torch.ops.hilcodec.state_slots_hold(src, dst, off, lens, hold, torch.empty(5, 1, 320),
                                                   torch.empty(8, 5, 1, dtype=torch.int64), torch.empty(5, 10, dtype=torch.uint8),
                                                   torch.empty(5, dtype=torch.int32)) is None
        assert torch.ops.hilcodec.state_slots_hold(src, dst, off, lens, hold, None, None, None, None) is None
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.state_slots_hold(torch.zeros(layout.total), torch.zeros(layout.total), torch.zeros(52, dtype=torch.int64),
                                            torch.zeros(52, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), None, None, None, None)


def test_session_queue_hold_and_stop():
    from hilcodec_amd import graph_step as G
    q = G.SessionQueue(6, 8, 2, G.state_layout(bare_model(), 6))
    assert q.held == frozenset() and q.stopped == ()
    for bad in (-1, 6, 100):
        with pytest.raises(IndexError):
            q.hold([1, bad])
        with pytest.raises(IndexError):
            q.stop(bad)
    assert q.held == frozenset()                          # a refused hold takes no slot
    with pytest.raises(ValueError):
        q.hold(torch.zeros(2, dtype=torch.int32, device="meta"))     # not a host tensor
    assert G.SessionQueue.host_slots(None) == [] and G.SessionQueue.host_slots(()) == []
    q.hold(torch.tensor([4, 1]))
    q.hold(range(1, 3))
    assert q.held == {1, 2, 4} and not q.pending          # holds alone queue no action
    q.clear()
    assert q.held == frozenset()                          # a hold lasts one hop
    q.stop(3)
    q.stop(0)
    q.hold([5])
    assert q.stopped == (0, 3) and q.held == {0, 3, 5}
    q.clear()
    assert q.stopped == (0, 3) and q.held == {0, 3}       # a stop lasts
    q.set_bitrate(3, 2)                                   # a stopped slot keeps its bitrate changes
    assert q.n == {3: 2} and q.stopped == (0, 3)
    q.start(3)                                            # start ends the stop; it takes effect at the next hop
    assert q.stopped == (0,) and q.starts == {3: None} and q.held == {0}
    q.start(1)
    q.hold([1])                                           # start and hold in one hop: both queued
    assert q.starts == {3: None, 1: None} and q.held == {0, 1}
    q.clear()
    q.stop(4)
    q.reset()
    assert q.stopped == () and q.held == frozenset() and not q.pending
