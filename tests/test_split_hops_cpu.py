"""CPU: the sender / receiver split of the graphed hop — the per-stream packet format (pinned to the body of
wire.pack_indices_10bit), the two packet entry points of the C ABI and their argument checks, the fake kernels of their ops, the
one-sided state layout and the one-sided session checks.  (No kernel is launched here.)"""
import ctypes

import pytest
import torch

from hilcodec_amd import wire
from tests.hops import assert_entry_points, bare_model

NEW = ("hilc_pack_codes_10bit", "hilc_rvq_decode_packed")


def test_stream_packet_is_the_10bit_body():
    g = torch.Generator().manual_seed(21)
    for n in range(1, 13):
        for T in range(1, 6):
            for codes in (torch.randint(0, 1024, (n, T), generator=g), torch.zeros(n, T, dtype=torch.int64),
                          torch.full((n, T), 1023), torch.randint(0, 2, (n, T), generator=g) * 1023):
                blob = wire.pack_stream_packet(codes)
                assert blob == wire.pack_indices_10bit(codes.view(n, 1, T))[12:]
                assert len(blob) == wire.packet_bytes(n, T) == -(-10 * n * T // 8)
                assert torch.equal(wire.unpack_stream_packet(blob, n, T), codes)
                assert torch.equal(wire.unpack_stream_packet(blob + b"\0" * 3, n, T), codes)   # a row of a [B, stride] batch
                assert wire.packet_n(len(blob), T) == n
    # the batch form: stream b's packet is the body of the whole [n, B, T] packing cut to one stream
    idx = torch.randint(0, 1024, (8, 5, 2), generator=g)
    for b in range(5):
        assert wire.pack_stream_packet(idx[:, b]) == wire.pack_indices_10bit(idx[:, b:b + 1])[12:]


def test_packet_n_rejects_other_lengths():
    for T in range(1, 6):
        valid = {wire.packet_bytes(n, T) for n in range(1, 40)}
        for nbytes in range(0, max(valid) + 1):
            if nbytes not in valid:
                with pytest.raises(ValueError):
                    wire.packet_n(nbytes, T)
    with pytest.raises(ValueError):
        wire.pack_stream_packet(torch.tensor([[1024]]))
    with pytest.raises(ValueError):
        wire.pack_stream_packet(torch.zeros(2, 2, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        wire.unpack_stream_packet(b"\0" * 9, 8, 1)


def test_packet_symbols_exported_and_declared():
    assert_entry_points(NEW)


def test_packet_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    # pack(indices, n_per_stream, packets, nbytes, B, T, n_max, stream)
    assert lib.hilc_pack_codes_10bit(None, p, p, p, 4, 1, 8, None) == -2
    assert lib.hilc_pack_codes_10bit(p, p, None, p, 4, 1, 8, None) == -2
    assert lib.hilc_pack_codes_10bit(p, p, p, None, 4, 1, 8, None) == -2
    assert lib.hilc_pack_codes_10bit(p, p, p, p, 0, 1, 8, None) == -1
    assert lib.hilc_pack_codes_10bit(p, p, p, p, 4, 0, 8, None) == -1
    assert lib.hilc_pack_codes_10bit(p, p, p, p, 4, 1, 0, None) == -5
    # decode(packets, n_per_stream, codebooks, q, B, C, T, K, Nq, n_max, stream)
    assert lib.hilc_rvq_decode_packed(None, p, p, p, 4, 128, 1, 1024, 16, 8, None) == -2
    assert lib.hilc_rvq_decode_packed(p, p, None, p, 4, 128, 1, 1024, 16, 8, None) == -2
    assert lib.hilc_rvq_decode_packed(p, p, p, None, 4, 128, 1, 1024, 16, 8, None) == -2
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 0, 128, 1, 1024, 16, 8, None) == -1
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 0, 1, 1024, 16, 8, None) == -1
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 0, 1024, 16, 8, None) == -1
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 1, 1024, 0, 8, None) == -1
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 1, 1024, 16, 0, None) == -5
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 1, 1024, 16, 17, None) == -5
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 1, 512, 16, 8, None) == -4     # 10-bit codes need K = 1024
    assert lib.hilc_rvq_decode_packed(p, p, p, p, 4, 128, 1, 1024, 40, 33, None) == -4   # stages staged in LDS


def test_packet_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hilcodec_amd import ops
    for name in ("pack_codes_10bit", "rvq_decode_packed"):
        assert hasattr(torch.ops.hilcodec, name)
    with FakeTensorMode():
        for n, B, T in ((8, 37, 1), (12, 5, 2), (3, 1, 5)):
            idx = torch.empty(n, B, T, dtype=torch.int64)
            packets, nbytes = ops.pack_codes_10bit(idx, torch.empty(B, dtype=torch.int32))
            assert packets.shape == (B, wire.packet_bytes(n, T)) and packets.dtype == torch.uint8
            assert nbytes.shape == (B,) and nbytes.dtype == torch.int32
            q = ops.rvq_decode_packed(packets, torch.empty(16, 1024, 128), n, T, n_clip=torch.empty(B, dtype=torch.int32))
            assert q.shape == (B, T, 128) and q.dtype == torch.float32
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.pack_codes_10bit(torch.zeros(8, 2, 1, dtype=torch.int64), None)


@pytest.mark.parametrize("side", ["enc", "dec"])
def test_one_sided_layout(side):
    from hilcodec_amd import graph_step as G
    model = bare_model()
    B = 3
    both = G.state_layout(model, B)
    assert (both.n_enc, len(both.shapes)) == (22, 52)                      # the default is today's layout
    layout = G.state_layout(model, B, side)
    k = 22 if side == "enc" else 30
    assert len(layout.shapes) == k and layout.n_enc == (22 if side == "enc" else 0)
    part = both.shapes[:22] if side == "enc" else both.shapes[22:]
    assert layout.shapes == part and layout.record_len == sum(s[1] * s[2] for s in part)
    blk = G.StateBlock(model, B, torch.device("cpu"), side)
    views = blk.enc if side == "enc" else blk.dec
    assert (blk.dec if side == "enc" else blk.enc) == []
    assert blk.layout.off == layout.off and blk.buffer.numel() == layout.total
    base = blk.buffer.data_ptr()
    for v, s, o, n in zip(views, layout.shapes, layout.off, layout.lens):
        assert tuple(v.shape) == s and n == s[1] * s[2] and o % 4 == 0
        for b in range(B):
            assert v[b].data_ptr() == base + 4 * (o + b * n)
    blk.buffer.copy_(torch.arange(blk.buffer.numel(), dtype=torch.float32))
    one = [c[2:3] for c in views]
    rec = layout.record(one, []) if side == "enc" else layout.record([], one)
    assert rec.shape == (layout.record_len,)
    e2, d2 = layout.split(rec)
    back = e2 if side == "enc" else d2
    assert (d2 if side == "enc" else e2) == [] and all(torch.equal(a, b) for a, b in zip(back, one))
    with pytest.raises(ValueError):
        G.state_layout(model, B, "neither")


@pytest.mark.parametrize("side", ["enc", "dec"])
def test_one_sided_session_queue_checks(side):
    from hilcodec_amd import graph_step as G
    model = bare_model()
    layout = G.state_layout(model, 6, side)
    q = G.SessionQueue(6, 8, 2, layout, one_sided=True)
    ce, cd = model.initialize_cache(torch.zeros(1, 1, 1))
    mine, other = (ce, cd) if side == "enc" else (cd, ce)

    def start(slot, caches=None, n=None):
        return q.start(slot, caches, None, n) if side == "enc" else q.start(slot, None, caches, n)

    for bad in (-1, 6):
        with pytest.raises(IndexError):
            start(bad)
        with pytest.raises(IndexError):
            q.set_bitrate(bad, 2)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            start(1, n=bad)
        with pytest.raises(ValueError):
            q.set_bitrate(1, bad)
    start(0, mine)
    start(0, mine, n=3)                                   # the same slot again: replaces
    start(1, mine)
    assert q.loads == 2 and q.starts[0].shape == (layout.record_len,)
    with pytest.raises(RuntimeError):
        start(2, mine)                                    # a third load in one hop
    start(2)
    assert q.starts[2] is None and q.loads == 2
    with pytest.raises(ValueError):
        start(3, mine[:-1])                               # a cache missing
    with pytest.raises(ValueError):
        start(3, other)                                   # the other side's caches
    with pytest.raises(ValueError):
        q.start(3, ce, cd)                                # both sides into a one-sided block
    bad = list(mine)
    bad[4] = torch.zeros(1, bad[4].shape[1], bad[4].shape[2] + 1)
    with pytest.raises(ValueError):
        start(3, bad)
    with pytest.raises(ValueError):
        start(3, [c.expand(2, -1, -1) for c in mine])     # B = 2 caches: one stream only
    # the two-sided queue keeps its check
    q2 = G.SessionQueue(6, 8, 2, G.state_layout(model, 6))
    with pytest.raises(ValueError):
        q2.start(0, ce, None)
