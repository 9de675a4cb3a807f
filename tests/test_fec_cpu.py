"""CPU: in-band forward error correction of the graphed sender / receiver — the hilc_pack_codes_10bit_fec / hilc_fec_select entry
points (additive under ABI 16) and their argument checks, their custom ops and fake kernels, the wire helpers that define the FEC
packet format, and the host-side checks of step(fec=...).  (No kernel is launched here.)"""
import ctypes

import pytest
import torch

from hilcodec_amd import wire
from tests.hops import assert_entry_points, bare_model

NEW = ("hilc_pack_codes_10bit_fec", "hilc_fec_select")


def test_fec_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)


def test_pack_codes_10bit_fec_argument_checks():
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)
    f = lib.hilc_pack_codes_10bit_fec
    # (indices, n_per_stream, prev_in, prev_out, action, hold, packets, nbytes, B, T, n_max, m, stream)
    ok = [p, None, p, q, None, None, p, p]
    for k in (0, 2, 3, 6, 7):                             # required pointers
        args = list(ok)
        args[k] = None
        assert f(*args, 4, 1, 8, 2, None) == -2, k
    assert f(*ok, 0, 1, 8, 2, None) == -1
    assert f(*ok, -1, 1, 8, 2, None) == -1
    assert f(*ok, 4, 0, 8, 2, None) == -1
    assert f(p, None, p, p, None, None, p, p, 4, 1, 8, 2, None) == -1     # prev_in == prev_out
    assert f(*ok, 4, 1, 0, 1, None) == -5                # n_max >= 1
    assert f(*ok, 4, 1, 8, 0, None) == -5                # m >= 1
    assert f(*ok, 4, 1, 8, -1, None) == -5
    assert f(*ok, 4, 1, 8, 9, None) == -5                # m <= n_max
    assert f(*ok, 4, 1, 24, 9, None) == -4               # n_max + m <= 32
    assert f(*ok, 4, 1, 16, 17, None) == -5


def test_fec_select_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_fec_select
    # (packets, fec, n_per_stream, out, B, T, n_max, m, stream)
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert f(*args, 4, 1, 8, 2, None) == -2, k
    assert f(*[p] * 4, 0, 1, 8, 2, None) == -1
    assert f(*[p] * 4, 4, 0, 8, 2, None) == -1
    assert f(*[p] * 4, 4, -3, 8, 2, None) == -1
    assert f(*[p] * 4, 4, 1, 0, 1, None) == -5
    assert f(*[p] * 4, 4, 1, 8, 0, None) == -5
    assert f(*[p] * 4, 4, 1, 8, 9, None) == -5
    assert f(*[p] * 4, 4, 1, 30, 3, None) == -4


def test_fec_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("pack_codes_10bit_fec", "fec_select"):
        assert hasattr(torch.ops.hilcodec, name), name
    assert "Tensor(a!) prev_out" in str(torch.ops.hilcodec.pack_codes_10bit_fec.default._schema)
    assert "Tensor(a!) n_slot" in str(torch.ops.hilcodec.fec_select.default._schema)
    B, n, m = 5, 8, 2
    for T in (1, 3):
        with FakeTensorMode():
            i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
            idx = torch.empty(n, B, T, dtype=torch.int64)
            pk, nb = torch.ops.hilcodec.pack_codes_10bit_fec(idx, i32(B), i32(B, 1 + m * T), i32(B, 1 + m * T), i32(B), i32(B), m)
            assert tuple(pk.shape) == (B, wire.fec_packet_bytes(n, m, T)) and pk.dtype == torch.uint8
            assert tuple(nb.shape) == (B,) and nb.dtype == torch.int32
            out = torch.ops.hilcodec.fec_select(torch.empty(B, wire.fec_packet_bytes(n, m, T), dtype=torch.uint8), i32(B), i32(B),
                                                n, m, T)
            assert tuple(out.shape) == (B, wire.packet_bytes(n, T)) and out.dtype == torch.uint8
    z = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.fec_select(torch.zeros(B, wire.fec_packet_bytes(n, m, 1), dtype=torch.uint8), z, z, n, m, 1)
    with pytest.raises(RuntimeError):
        rows = torch.zeros(B, 1 + m, dtype=torch.int32)
        torch.ops.hilcodec.pack_codes_10bit_fec(torch.zeros(n, B, 1, dtype=torch.int64), None, rows, rows.clone(), None, None, m)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_fec_wire_round_trip(T):
    gen = torch.Generator().manual_seed(T)
    for n in range(1, 13):
        for m in range(1, n + 1):
            cur = torch.randint(0, 1024, (n, T), generator=gen)
            prev = torch.randint(0, 1024, (m, T), generator=gen)
            pk = wire.pack_fec_packet(cur, prev)
            assert pk == wire.pack_stream_packet(torch.cat([cur, prev]))
            assert len(pk) == wire.fec_packet_bytes(n, m, T) == wire.packet_bytes(n + m, T)
            assert wire.fec_primary(pk, n, T) == wire.pack_stream_packet(cur)             # the sender without FEC, byte for byte
            assert torch.equal(wire.unpack_stream_packet(pk, n, T), cur)                  # a receiver without FEC reads it as it is
            red = wire.fec_redundant(pk, n, m, T)
            assert red == wire.pack_stream_packet(prev) and len(red) == wire.packet_bytes(m, T)
            assert wire.fec_present(len(pk), n, m, T) is True
            plain = wire.pack_fec_packet(cur, None)
            assert plain == wire.pack_stream_packet(cur)
            assert wire.fec_present(len(plain), n, m, T) is False
            assert wire.fec_primary(plain, n, T) == plain
            assert len(pk) - len(plain) >= 1
            for stray in {0, len(plain) - 1, len(plain) + 1, len(pk) + 1} - {len(plain), len(pk)}:
                with pytest.raises(ValueError):
                    wire.fec_present(stray, n, m, T)


def test_fec_primary_zeroes_trailing_bits():
    # n = 1, T = 1: 10 primary bits, the second byte's top 2 bits are primary and the rest belong to the redundant codes
    pk = wire.pack_fec_packet(torch.tensor([[0x3FF]]), torch.tensor([[0x3FF]]))
    assert pk == bytes([0xFF, 0xFF, 0xF0])
    assert wire.fec_primary(pk, 1, 1) == bytes([0xFF, 0xC0])
    assert wire.fec_redundant(pk, 1, 1, 1) == bytes([0xFF, 0xC0])
    with pytest.raises(ValueError):
        wire.fec_present(2, 1, 0, 1)


def test_session_queue_fec_checks():
    from hilcodec_amd import graph_step as G
    q = G.SessionQueue(6, 8, 2, G.state_layout(bare_model(), 6, "dec"), one_sided=True)
    assert q.fec_slots(None) == [] and q.fec_slots(()) == []
    assert q.fec_slots([4, 1, 4], hold=[0], lost=[2]) == [1, 4]
    assert q.fec_slots(torch.tensor([3])) == [3]
    for bad in (-1, 6):
        with pytest.raises(IndexError):
            q.fec_slots([1, bad])
    with pytest.raises(ValueError):
        q.fec_slots([1, 2], hold=[2])                     # fec and held on the same hop
    with pytest.raises(ValueError):
        q.fec_slots([1, 2], lost=[1])                     # fec and lost on the same hop
    with pytest.raises(ValueError):
        q.fec_slots(torch.zeros(1, dtype=torch.int32, device="meta"))    # not a host tensor
    q.stop(5)
    with pytest.raises(ValueError):
        q.fec_slots([5])                                  # a stopped slot has no stream
    q.start(5)
    assert q.fec_slots([5]) == [5]                        # a start ends the stop


def test_session_queue_n_min():
    from hilcodec_amd import graph_step as G
    q = G.SessionQueue(4, 8, 2, G.state_layout(bare_model(), 4, "enc"), one_sided=True)
    q.start(0, n=1)
    q.n_min = 3                                           # what GraphedEncodeHop(fec_stages=3) sets
    for bad in (1, 2, 9):
        with pytest.raises(ValueError):
            q.start(1, n=bad)
        with pytest.raises(ValueError):
            q.set_bitrate(1, bad)
    q.start(1, n=3)
    q.set_bitrate(2, 8)
    assert q.n == {0: 1, 1: 3, 2: 8}


def test_fec_stages_checks():
    from hilcodec_amd import graph_step as G
    assert G._fec_stages(0, 8) == 0 and G._fec_stages(2, 8) == 2 and G._fec_stages(8, 8) == 8
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError):
            G._fec_stages(bad, 8)
    with pytest.raises(ValueError):
        G._fec_stages(9, 24)                              # n + m > 32
