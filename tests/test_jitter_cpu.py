"""CPU: transport header and jitter buffer — the hilc_packet_header / hilc_jitter_step entry points (additive under ABI 16) and their
argument checks, their custom ops and fake kernels, JitterConfig, the header helpers of wire.py and the receiver's rules
(jitter.JitterModel) on hand-built arrival traces.  (No kernel is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd import jitter, wire
from hilcodec_amd.jitter import JitterConfig, JitterModel
from tests.hops import assert_entry_points

NEW = ("hilc_packet_header", "hilc_jitter_step")


def test_jitter_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)


def test_packet_header_argument_checks():
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)
    f = lib.hilc_packet_header
    # (packets, nbytes, n_per_stream, kind, action, hold, counter_in, counter_out, out, out_nbytes, B, T, n_max, m, stream)
    ok = [p, p, None, None, None, None, p, q, p, p]
    for k in (0, 1, 6, 7, 8, 9):
        args = list(ok)
        args[k] = None
        assert f(*args, 4, 1, 8, 0, None) == -2, k
    assert f(*ok, 0, 1, 8, 0, None) == -1
    assert f(*ok, 4, 0, 8, 0, None) == -1
    args = list(ok)
    args[7] = p                                           # counter_in == counter_out
    assert f(*args, 4, 1, 8, 0, None) == -1
    assert f(*ok, 4, 1, 0, 0, None) == -5
    assert f(*ok, 4, 1, 8, -1, None) == -5
    assert f(*ok, 4, 1, 8, 9, None) == -5                  # m > n_max
    assert f(*ok, 4, 1, 32, 0, None) == -4                 # n does not fit 5 bits
    assert f(*ok, 4, 1, 24, 9, None) == -4                 # n_max + m > 32


def test_jitter_step_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_jitter_step
    # (arrivals, offsets, max_arrivals, action, hold, n, lost, fec, packets, state, meta, ring, B, T, n_max, m, order, conceal, D, C, s)
    head = lambda *a: [a[0], a[1], 8, None, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]]
    ok = [p, p, p, p, None, None, p, p, p, p]
    for k in range(10):
        if k in (4, 5):
            continue
        args = list(ok)
        args[k] = None
        assert f(*head(*args), 4, 1, 8, 0, -1, 0, 2, 8, None) == -2, k
    assert f(*head(*ok), 4, 1, 8, 0, -1, 1, 2, 8, None) == -2          # conceal without lost
    assert f(*head(*ok), 4, 1, 8, 2, -1, 0, 2, 8, None) == -2          # FEC without fec
    args = head(*ok)
    args[2] = -1
    assert f(*args, 4, 1, 8, 0, -1, 0, 2, 8, None) == -1
    assert f(*head(*ok), 0, 1, 8, 0, -1, 0, 2, 8, None) == -1
    assert f(*head(*ok), 4, 0, 8, 0, -1, 0, 2, 8, None) == -1
    assert f(*head(*ok), 4, 1, 0, 0, -1, 0, 2, 8, None) == -5
    assert f(*head(*ok), 4, 1, 8, 0, 17, 0, 2, 8, None) == -5          # order
    assert f(*head(*ok), 4, 1, 8, 0, -2, 0, 2, 8, None) == -5
    for D, C in ((2, 6), (0, 1), (0, 64), (7, 8), (-1, 8)):
        assert f(*head(*ok), 4, 1, 8, 0, -1, 0, D, C, None) == -5, (D, C)
    assert f(*head(*ok), 4, 1, 32, 0, -1, 0, 2, 8, None) == -4
    assert f(*head(*ok), 4, 1, 1, 0, 8, 0, 2, 8, None) == -1           # a SID of 9 bytes in a 2-byte row


def test_jitter_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hilcodec_amd.ops  # noqa: F401  (registers the ops)
    for name in ("packet_header", "jitter_step"):
        assert hasattr(torch.ops.hilcodec, name), name
    sch = str(torch.ops.hilcodec.packet_header.default._schema)
    assert "Tensor(a!) ctr_out" in sch
    sch = str(torch.ops.hilcodec.jitter_step.default._schema)
    assert "Tensor(a!) hold" in sch and "Tensor(e!) packets" in sch and "Tensor(f!) state" in sch and "Tensor(h!) ring" in sch
    B, n, m, T = 5, 8, 2, 1
    stride = wire.packet_bytes(n + m, T)
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        out, cnt = torch.ops.hilcodec.packet_header(torch.empty(B, stride, dtype=torch.uint8), i32(B), None, None, None, None, i32(B),
                                                    i32(B), n, m, T)
        assert out.shape == (B, wire.transport_bytes(n, m, T)) and out.dtype == torch.uint8
        assert cnt.shape == (B,) and cnt.dtype == torch.int32
        torch.ops.hilcodec.jitter_step(i32(10, 1 + (3 + stride + 3) // 4), i32(B + 1), None, i32(B), i32(B), None, i32(B),
                                       torch.empty(B, stride, dtype=torch.uint8), i32(B, 14), i32(B, 8), i32(B, 8, (stride + 3) // 4),
                                       n, m, T, -1, 2)


def test_jitter_config():
    c = JitterConfig()
    assert (c.depth, c.capacity) == (2, 8)
    for C in (2, 4, 8, 16, 32):
        JitterConfig(depth=C - 2, capacity=C)
        JitterConfig(depth=0, capacity=C)
    for kw in (dict(capacity=1), dict(capacity=3, depth=0), dict(capacity=64), dict(capacity=6, depth=0), dict(capacity=0, depth=0),
               dict(depth=-1), dict(depth=7, capacity=8), dict(depth=1.5), dict(depth=True), dict(capacity="8")):
        with pytest.raises(ValueError):
            JitterConfig(**kw)
    assert jitter.ST_WORDS == 14 and len(jitter.STAT_NAMES) == jitter.ST_WORDS - jitter.STAT_ACCEPTED


# ---------------------------------------------------------------- the header
def test_transport_round_trip():
    T, n_max, m, K = 1, 8, 2, 8
    assert wire.TRANSPORT_HEADER == 3
    assert wire.transport_bytes(8, 0, 1) == 13 and wire.transport_bytes(8, 2, 1) == 16 and wire.transport_bytes(8, 2, 2) == 28
    rng = np.random.default_rng(1)
    for hop in (0, 1, 255, 256, 65535, 65536 + 7):
        for n in (2, 5, 8):
            for fec in (False, True):
                body = rng.integers(0, 256, (wire.fec_packet_bytes(n, m, T) if fec else wire.packet_bytes(n, T))).astype(np.uint8)
                pkt = wire.pack_transport(hop, body.tobytes(), n, fec=fec)
                assert pkt[:2] == bytes([(hop >> 8) & 0xFF, hop & 0xFF]) and pkt[2] == (0x40 if fec else 0) | n
                assert wire.parse_transport(pkt, len(pkt), T, n_max, m, K) == (hop & 0xFFFF, False, fec, n, body.tobytes())
        sid = bytes(range(1, 1 + 1 + K))
        pkt = wire.pack_transport(hop, sid, 0, sid=True)
        assert pkt[2] == 0x80 and len(pkt) == 3 + 1 + K
        assert wire.parse_transport(pkt + b"\0\0", len(pkt), T, n_max, m, K) == (hop & 0xFFFF, True, False, 0, sid)
    for bad in (dict(n=0), dict(n=32), dict(n=1, sid=True), dict(n=0, sid=True, fec=True)):
        with pytest.raises(ValueError):
            wire.pack_transport(0, b"", **bad)


def test_parse_transport_malformed():
    T, n_max, m, K = 1, 8, 2, 8
    good = wire.pack_transport(9, bytes(wire.packet_bytes(4, T)), 4)
    parse = lambda pkt, nb=None, **kw: wire.parse_transport(pkt, len(pkt) if nb is None else nb, kw.get("T", T), kw.get("n_max", n_max),
                                                             kw.get("m", m), kw.get("K", K))
    assert parse(good)[3] == 4
    cases = [
        (good, 2, {}),                                                            # shorter than the header
        (good, -1, {}),
        (good, len(good) + 1, {}),                                                 # longer than the buffer
        (bytes([0, 9, 0x20 | 4]) + good[3:], None, {}),                            # bit 5
        (good[:-1], None, {}),                                                     # length does not match
        (good + b"\0", None, {}),
        (bytes([0, 9, 0]) + good[3:], None, {}),                                   # n = 0
        (wire.pack_transport(9, bytes(wire.packet_bytes(9, T)), 9), None, {}),     # n > n_max
        (wire.pack_transport(9, bytes(1 + K), 0, sid=True), None, dict(K=None)),  # SID without cng_order
        (wire.pack_transport(9, bytes(K), 0, sid=True), None, {}),                # SID of the wrong length
        (bytes([0, 9, 0x80 | 1]) + bytes(1 + K), None, {}),                        # SID with n != 0
        (bytes([0, 9, 0xC0]) + bytes(1 + K), None, {}),                            # SID with the FEC flag
        (wire.pack_transport(9, bytes(wire.fec_packet_bytes(4, m, T)), 4, fec=True), None, dict(m=0)),   # FEC without fec_stages
        (wire.pack_transport(9, bytes(wire.fec_packet_bytes(1, m, T)), 1, fec=True), None, {}),          # n < m
        (wire.pack_transport(9, bytes(wire.fec_packet_bytes(4, m, T)), 4), None, {}),                    # FEC length, no flag
        (wire.pack_transport(9, bytes(wire.packet_bytes(4, T)), 4, fec=True), None, {}),                 # flag, plain length
    ]
    for i, (pkt, nb, kw) in enumerate(cases):
        with pytest.raises(ValueError):
            parse(pkt, nb, **kw)
            pytest.fail(f"case {i}")


# ---------------------------------------------------------------- the receiver's rules
T = 1


def codes(h, n=8, fec=False, m=2):
    """a headed codes packet whose body starts with h mod 256 (to tell played packets apart)"""
    body = bytearray(wire.fec_packet_bytes(n, m, T) if fec else wire.packet_bytes(n, T))
    body[0], body[1] = h & 0xFF, 0x5A
    return wire.pack_transport(h, bytes(body), n, fec=fec)


def sid(h, K=8):
    body = bytearray(1 + K)
    body[0] = h & 0x7F
    return wire.pack_transport(h, bytes(body), 0, sid=True)


class Trace:
    """one slot (B = 1) of JitterModel, driven hop by hop; `hop()` returns that hop's decision: 'H' held, ('P', b0) played (b0 = the
    packet row's first byte), ('S', b0) SID, 'Q' silent, 'L' lost (concealed), ('F', b0) FEC, ('h', v) a host hold v"""

    def __init__(self, D=0, C=8, m=0, K=8, conceal=True, n=8, B=1):
        self.model = JitterModel(B, JitterConfig(depth=D, capacity=C), n, m, T, K, conceal)

    def hop(self, pkts=(), hold=0, start=0, slots=None, nbytes=None):
        tb = self.model.tbytes
        A = len(pkts)
        arr = np.zeros((A, tb), dtype=np.uint8)
        for a, p in enumerate(pkts):
            arr[a, :min(len(p), tb)] = np.frombuffer(p[:tb], dtype=np.uint8)
        nb = [len(p) for p in pkts] if nbytes is None else nbytes
        sl = [0] * A if slots is None else slots
        B = self.model.B
        rows = self.model.step(np.full(B, start), np.full(B, hold), sl, arr, nb)
        self.rows = rows
        return self.decide(rows, 0, hold)

    @staticmethod
    def decide(rows, b, hold=0):
        if hold:
            assert rows["hold"][b] == hold and not rows["packets"][b].any()
            return ("h", hold)
        hv, b0 = rows["hold"][b], int(rows["packets"][b][0])
        if hv == 1:
            assert not rows["packets"][b].any() and rows["n"][b] == 8
            return "H"
        if hv == 2:
            return ("S", b0)
        if hv == 3:
            return "Q"
        if rows["lost"][b]:
            return "L"
        if rows["fec"][b]:
            return ("F", b0)
        return ("P", b0)

    def stat(self, name):
        return int(self.model.state[0, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index(name)])


def test_model_in_order():
    t = Trace(D=0)
    assert [t.hop([codes(h)]) for h in range(5)] == [("P", h) for h in range(5)]
    assert t.stat("decoded") == 5 and t.stat("accepted") == 5
    t = Trace(D=3)
    out = [t.hop([codes(h)]) for h in range(7)]
    assert out == ["H"] * 3 + [("P", h) for h in range(4)]
    assert int(t.model.state[0, jitter.ST_NEXT]) == 4 and int(t.model.state[0, jitter.ST_WAIT]) == 0
    assert bin(int(t.model.state[0, jitter.ST_MASK]) & 0xFF).count("1") == 3        # 4, 5, 6 are buffered


def test_model_reorder_within_window():
    t = Trace(D=2)
    arrivals = [[0], [2], [1], [3, 5], [4], [], [], []]
    out = [t.hop([codes(h) for h in a]) for a in arrivals]
    assert out == ["H", "H", ("P", 0), ("P", 1), ("P", 2), ("P", 3), ("P", 4), ("P", 5)]
    assert t.stat("late") == 0 and t.stat("accepted") == 6


def test_model_duplicates_late_early_malformed():
    t = Trace(D=1, C=4)
    t.hop([codes(10)])
    assert t.hop([codes(11), codes(11), codes(10)]) == ("P", 10)   # the copy of 11 is a duplicate; 10 is still in the ring
    assert t.stat("duplicate") == 2
    assert t.hop([codes(10), codes(15), codes(14), codes(16)]) == ("P", 11)   # 10 late; window [11, 15): 14 kept, 15 and 16 early
    assert (t.stat("late"), t.stat("early")) == (1, 2)
    bad = [codes(12)[:5], bytes([0, 12, 0x20 | 8]) + codes(12)[3:], b"\0\x0c", codes(12, fec=True)]   # m = 0: FEC is malformed
    assert t.hop(bad) == "L"
    assert t.stat("malformed") == 4 and t.stat("lost") == 1
    assert t.hop([], hold=0, nbytes=[]) == "L"                     # 13
    assert t.hop() == ("P", 14) and t.hop() == "L"
    assert t.stat("accepted") == 3 and t.stat("lost") == 3


def test_model_sid_and_dtx_gap():
    t = Trace(D=0)
    arrivals = [[codes(0)], [sid(1)], [], [], [], [codes(5)], []]
    out = [t.hop(a) for a in arrivals]
    assert out == [("P", 0), ("S", 1), "Q", "Q", "Q", ("P", 5), "L"]
    assert t.stat("noise") == 4 and int(t.model.state[0, jitter.ST_IN_DTX]) == 0
    assert t.rows["n"][0] == 8


def test_model_lost_first_sid():
    t = Trace(D=0)
    arrivals = [[codes(0)], [], [], [], [sid(4)], [], [codes(6)]]
    out = [t.hop(a) for a in arrivals]
    assert out == [("P", 0), "L", "L", "L", ("S", 4), "Q", ("P", 6)]
    t = Trace(D=0, conceal=False)
    assert [t.hop(a) for a in arrivals] == [("P", 0), "H", "H", "H", ("S", 4), "Q", ("P", 6)]


def test_model_fec_only_with_a_redundant_section():
    t = Trace(D=1, m=2)
    out = [t.hop(a) for a in ([codes(0)], [codes(2, fec=True)], [codes(3, fec=True)], [], [], [])]
    assert out == ["H", ("P", 0), ("F", 2), ("P", 2), ("P", 3), "L"]
    assert t.stat("fec") == 1 and t.stat("lost") == 1
    # n of a FEC slot is the next packet's primary n; the packet row its whole body
    t = Trace(D=1, m=2)
    t.hop([codes(0)])
    t.hop([codes(2, n=5, fec=True)])
    assert t.hop() == ("F", 2) and t.rows["n"][0] == 5 and t.rows["fec"][0] == 1
    body = np.frombuffer(codes(2, n=5, fec=True)[3:], dtype=np.uint8)
    assert np.array_equal(t.rows["packets"][0, :len(body)], body) and not t.rows["packets"][0, len(body):].any()
    # h + 1 without a redundant section, or a SID: lost
    t = Trace(D=1, m=2)
    assert [t.hop(a) for a in ([codes(0)], [codes(2)], [], [])] == ["H", ("P", 0), "L", ("P", 2)]
    t = Trace(D=1, m=2)
    assert [t.hop(a) for a in ([codes(0)], [sid(2)], [], [])] == ["H", ("P", 0), "L", ("S", 2)]


def test_model_host_hold_pauses_playout():
    t = Trace(D=0)
    assert t.hop([codes(0)]) == ("P", 0)
    assert t.hop([codes(1)], hold=1) == ("h", 1)
    assert t.hop([codes(2)], hold=1) == ("h", 1)
    assert t.hop([codes(3)]) == ("P", 1)
    assert [t.hop() for _ in range(3)] == [("P", 2), ("P", 3), "L"]
    # a hold during priming does not count down
    t = Trace(D=2)
    assert [t.hop([codes(0)]), t.hop(hold=1), t.hop(), t.hop(), t.hop()] == ["H", ("h", 1), "H", ("P", 0), "L"]


def test_model_start_on_the_same_hop_as_arrivals():
    t = Trace(D=0)
    for h in range(100, 104):
        t.hop([codes(h)])
    assert t.hop([codes(0)]) == "L" and t.stat("late") == 1       # a sender restart without a receiver start: late
    assert t.hop([codes(1)], start=1) == ("P", 1)                 # the start clears the state first, then 1 anchors
    assert t.stat("late") == 0 and t.stat("accepted") == 1
    assert not t.model.meta[0].any()


def test_model_wrap():
    t = Trace(D=1, C=4)
    hs = [65534, 65535, 0, 1, 2]
    out = [t.hop([codes(h)]) for h in hs] + [t.hop()]
    assert out == ["H"] + [("P", h & 0xFF) for h in hs]
    assert int(t.model.state[0, jitter.ST_NEXT]) == 3
    assert t.stat("late") == 0 and t.stat("early") == 0


def test_model_slots_are_independent():
    t = Trace(D=0, B=3)
    rows = t.model.step(np.zeros(3), np.array([0, 0, 1]), [2, 0, 2, 1], np.zeros((4, t.model.tbytes), dtype=np.uint8), [0, 0, 0, 0])
    assert list(rows["hold"]) == [1, 1, 1] and t.model.state[:, jitter.STAT_MALFORMED].tolist() == [1, 1, 2]
    pk = [codes(5), codes(7), sid(9)]
    arr = np.zeros((3, t.model.tbytes), dtype=np.uint8)
    for a, p in enumerate(pk):
        arr[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    rows = t.model.step(np.zeros(3), np.array([0, 0, 1]), [1, 0, 2], arr, [len(p) for p in pk])
    assert [Trace.decide(rows, b) for b in (0, 1)] == [("P", 7), ("P", 5)] and rows["hold"][2] == 1
    assert t.model.state[2, jitter.ST_ANCHORED] == 1 and t.model.state[2, jitter.ST_NEXT] == 9
