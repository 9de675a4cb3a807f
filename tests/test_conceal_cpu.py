"""CPU: loss concealment of the graphed receiver — the hilc_conceal_prepare / hilc_conceal_gain entry points (additive under
ABI 16) and their argument checks, their custom ops and fake kernels, the wire helpers that define substitute packets and fade
tables, and the host-side checks of step(lost=...).  (No kernel is launched here.)"""
import ctypes

import pytest
import torch

from hilcodec_amd import wire
from tests.hops import assert_entry_points, bare_model

NEW = ("hilc_conceal_prepare", "hilc_conceal_gain")


def test_conceal_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)


def test_conceal_prepare_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_conceal_prepare
    # (state, action, hold, lost, n_per_stream, packets, ramp, B, T, n_max, fade_hops, stream)
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert f(*args, 4, 1, 8, 4, None) == -2, k
    assert f(*[p] * 7, 0, 1, 8, 4, None) == -1
    assert f(*[p] * 7, -2, 1, 8, 4, None) == -1
    assert f(*[p] * 7, 4, 0, 8, 4, None) == -1
    assert f(*[p] * 7, 4, 1, 0, 4, None) == -5
    assert f(*[p] * 7, 4, 1, 8, 0, None) == -5           # fade_hops >= 1
    assert f(*[p] * 7, 4, 1, 8, -1, None) == -5
    assert f(*[p] * 7, 4, 1, 33, 4, None) == -4          # n_max <= 32, as hilc_rvq_decode_packed


def test_conceal_gain_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_conceal_gain
    # (wav, ramp, gains, weights, B, samples, fade_hops, stream)
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert f(*args, 4, 320, 4, None) == -2, k
    assert f(p, p, p, p, 0, 320, 4, None) == -1
    assert f(p, p, p, p, 4, 0, 4, None) == -1
    assert f(p, p, p, p, 4, 320, 0, None) == -5


def test_conceal_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("conceal_prepare", "conceal_gain"):
        assert hasattr(torch.ops.hilcodec, name), name
    schema = str(torch.ops.hilcodec.conceal_prepare.default._schema)
    for arg in ("Tensor(a!) state", "Tensor(b!) hold", "Tensor(c!) n_slot", "Tensor(d!) packets"):
        assert arg in schema, arg
    assert "Tensor(a!) wav" in str(torch.ops.hilcodec.conceal_gain.default._schema)
    B, n, T = 5, 8, 2
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        ramp = torch.ops.hilcodec.conceal_prepare(i32(B, n + 3), i32(B), i32(B), i32(B), i32(B),
                                                  torch.empty(B, wire.packet_bytes(n, T), dtype=torch.uint8), T, 4)
        assert tuple(ramp.shape) == (B,) and ramp.dtype == torch.int32
        assert torch.ops.hilcodec.conceal_gain(torch.empty(B, 1, 320 * T), i32(B), torch.empty(5), torch.empty(320 * T)) is None
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.conceal_gain(torch.zeros(B, 1, 320), torch.zeros(B, dtype=torch.int32), torch.zeros(5), torch.zeros(320))
    with pytest.raises(RuntimeError):
        z = torch.zeros(B, dtype=torch.int32)
        torch.ops.hilcodec.conceal_prepare(torch.zeros(B, n + 3, dtype=torch.int32), z, z, z, z,
                                           torch.zeros(B, wire.packet_bytes(n, 1), dtype=torch.uint8), 1, 4)


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 8, 12])
def test_conceal_packet_round_trip(n, T):
    gen = torch.Generator().manual_seed(31 * n + T)
    codes = torch.randint(0, 1024, (n, T), generator=gen)
    src = wire.pack_stream_packet(codes)
    sub = wire.conceal_packet(src, n, T)
    assert len(sub) == wire.packet_bytes(n, T)
    got = wire.unpack_stream_packet(sub, n, T)
    for t in range(T):
        assert torch.equal(got[:, t], codes[:, -1]), t
    assert wire.conceal_packet(src + b"\x00\x07", n, T) == sub      # bytes past the packet are not read


@pytest.mark.parametrize("F", [1, 3, 4, 7])
@pytest.mark.parametrize("S", [320, 1280])
def test_conceal_tables(F, S):
    G, W = wire.conceal_tables(F, S)
    assert G.dtype == torch.float32 and W.dtype == torch.float32
    assert tuple(G.shape) == (F + 1,) and tuple(W.shape) == (S,)
    assert float(G[0]) == 1.0 and float(G[F]) == 0.0 and float(W[S - 1]) == 1.0
    for k in range(F + 1):                                # float64 quotient, rounded once
        assert float(G[k]) == float(torch.tensor((F - k) / F, dtype=torch.float64).float())
    for s in (0, 1, S // 3, S - 2):
        assert float(W[s]) == float(torch.tensor((s + 1) / S, dtype=torch.float64).float())
    assert bool((G[1:] < G[:-1]).all()) and bool((W[1:] > W[:-1]).all())
    for bad in ((0, S), (F, 0)):
        with pytest.raises(ValueError):
            wire.conceal_tables(*bad)


def test_session_queue_lost_checks():
    from hilcodec_amd import graph_step as G
    q = G.SessionQueue(6, 8, 2, G.state_layout(bare_model(), 6, "dec"), one_sided=True)
    assert q.lost_slots(None) == [] and q.lost_slots(()) == []
    assert q.lost_slots([4, 1, 4], hold=[0, 2]) == [1, 4]
    assert q.lost_slots(torch.tensor([3])) == [3]
    for bad in (-1, 6):
        with pytest.raises(IndexError):
            q.lost_slots([1, bad])
    with pytest.raises(ValueError):
        q.lost_slots([1, 2], hold=[2])                    # lost and held on the same hop
    with pytest.raises(ValueError):
        q.lost_slots(torch.zeros(1, dtype=torch.int32, device="meta"))   # not a host tensor
    q.stop(5)
    with pytest.raises(ValueError):
        q.lost_slots([5])                                 # a stopped slot has no stream to conceal
    assert q.lost_slots([0, 3]) == [0, 3]
    q.start(5)                                            # a start ends the stop: lost on its start hop is fine
    assert q.lost_slots([5]) == [5]
