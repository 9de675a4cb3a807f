"""CPU: NACK and retransmission (hilcodec_amd/rtx.py, the definition of hilc_nack_build and hilc_rtx_step): the wire format of a
NACK, both models on scripted rings and histories, the closed loop on the models (jitter.JitterModel as the receiver, a stand-in
sender with an RtxModel, tests/rtx_loop.py) and the entry points.  Everything is integer: every comparison is exact."""
import os
import re

import numpy as np
import pytest

from hilcodec_amd import jitter, rtx, wire
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.rtx import NackConfig, NackModel, RtxConfig, RtxModel, nack_words
from tests.hops import HEADER, assert_entry_points
from tests.rtx_loop import HOPS, bursts_of_two, lost, run_models, singles_and_pairs


# ---------------------------------------------------------------- wire
def test_nack_round_trip_and_errors():
    assert wire.NACK_BYTES == 4
    for base, bitmap in ((0, 0), (1, 0x8001), (65535, 0xFFFF), (0x1234, 0x00F0)):
        blob = wire.pack_nack(base, bitmap)
        assert isinstance(blob, bytes) and blob == bytes([base >> 8, base & 255, bitmap >> 8, bitmap & 255])
        assert wire.parse_nack(blob) == (base, bitmap)
    assert wire.parse_nack(np.array([1, 2, 3, 4], dtype=np.uint8)) == (0x0102, 0x0304)
    for bad in ((-1, 0), (65536, 0), (0, -1), (0, 65536), (1.0, 0), (True, 0)):
        with pytest.raises(ValueError):
            wire.pack_nack(*bad)
    for bad in (b"", b"abc", b"abcde"):
        with pytest.raises(ValueError):
            wire.parse_nack(bad)
    assert wire.nack_hops(7, 0) == [7] and wire.nack_hops(7, 0b101) == [7, 8, 10]
    assert wire.nack_hops(100, 0xFFFF) == list(range(100, 117))
    # the bitmap crosses the 16-bit wrap
    assert wire.nack_hops(65535, 0b1001) == [65535, 0, 3] and wire.nack_hops(65530, 1 << 15) == [65530, 10]
    with pytest.raises(ValueError):
        wire.nack_hops(65536, 0)
    assert nack_words(65535, 0b1001) == (rtx.NACK_PRESENT | 65535, 0b1001)


def test_configs_check_their_ranges():
    assert NackConfig() == NackConfig(2, 3, 2, False) and RtxConfig() == RtxConfig(16, 2)
    NackConfig(1, 1, 1, True), NackConfig(30, 255, 255), RtxConfig(2, 1), RtxConfig(64, 4)
    for kw in (dict(rtt_hops=0), dict(rtt_hops=31), dict(retry_hops=0), dict(retry_hops=256), dict(max_requests=0),
               dict(max_requests=256), dict(rtt_hops=2.0), dict(retry_hops=True), dict(skip_fecable=1)):
        with pytest.raises(ValueError):
            NackConfig(**kw)
    for kw in (dict(history=1), dict(history=3), dict(history=128), dict(history=24), dict(per_hop=0), dict(per_hop=5),
               dict(history=16.0), dict(per_hop=True)):
        with pytest.raises(ValueError):
            RtxConfig(**kw)
    assert rtx.NK_WORDS == rtx.NK_RING + 32 and len(rtx.NK_NAMES) == rtx.NK_RING
    assert rtx.RX_WORDS == rtx.RX_DROPPED + 1 == len(rtx.RX_NAMES)
    for bad in (3, 64, 1):
        with pytest.raises(ValueError):
            NackModel(1, NackConfig(), bad)


def test_layouts_match_header():
    """rtx.<NAME> is `#define HILC_RTX_<NAME>`, value for value, in both directions"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_RTX_"):
            header[name[len("HILC_RTX_"):]] = env[name]
    python = {k: v for k, v in vars(rtx).items() if k.isupper() and not k.startswith("_") and isinstance(v, int) and not isinstance(v, bool)
              and k not in vars(jitter)}
    assert len(header) >= 16 and header == python
    assert env["HILC_WIRE_NACK_BYTES"] == wire.NACK_BYTES
    assert rtx.NK_RING_WORDS == 32 and sorted(v for k, v in header.items() if k.startswith("RX_") and k != "RX_WORDS") == list(range(5))


def test_entry_points_are_declared_exported_and_bound():
    assert_entry_points(("hilc_nack_build", "hilc_rtx_step"), in_abi16_line=True)
    assert os.path.isfile(os.path.join(os.path.dirname(rtx.__file__), "csrc", "rtx.hip"))


# ---------------------------------------------------------------- NackModel on scripted rings
class Ring:
    """one slot's jitter rows, scripted: `next`, the occupied hops with their kind ("c" codes, "f" codes with the FEC flag, "s" SID)"""

    def __init__(self, cfg, C=8, m=0, B=1):
        self.C, self.model = C, NackModel(B, cfg, C, m)
        self.js = np.zeros((B, jitter.ST_WORDS), dtype=np.int32)
        self.meta = np.zeros((B, C), dtype=np.int32)

    def set(self, nxt, present, b=0, in_dtx=False, anchored=True):
        js, C = self.js[b], self.C
        js[:] = 0
        self.meta[b] = 0
        js[jitter.ST_ANCHORED], js[jitter.ST_NEXT], js[jitter.ST_IN_DTX] = int(anchored), nxt & 0xFFFF, int(in_dtx)
        mask = 0
        for h, kind in dict(present).items():
            assert 0 <= ((h - nxt + 0x8000) & 0xFFFF) - 0x8000 < C
            i = h & (C - 1)
            mask |= 1 << i
            word = jitter.meta_word(h, kind == "s", kind == "f", 0 if kind == "s" else 4)
            self.meta[b, i] = word - (1 << 32) if word >= 1 << 31 else word
        js[jitter.ST_MASK] = mask - (1 << 32) if mask >= 1 << 31 else mask

    def step(self, action=None):
        B = len(self.js)
        out = self.model.step(self.js, self.meta, np.zeros(B, dtype=np.int32) if action is None else action)
        return [(wire.nack_hops(*wire.parse_nack(out["nacks"][b])) if out["due"][b] else None) for b in range(B)]

    def word(self, h, b=0):
        w = int(self.model.state[b, rtx.NK_RING + (h & (self.C - 1))]) & 0xFFFFFFFF
        return w & 0xFFFF, (w >> 16) & 255, w >> 24

    def counters(self, b=0):
        return tuple(int(v) for v in self.model.state[b, :rtx.NK_RING])


def test_nack_model_asks_retries_and_gives_up():
    r = Ring(NackConfig(rtt_hops=2, retry_hops=3, max_requests=2), C=16)
    codes = lambda *hops: {h: "c" for h in hops}
    # next = 100, hop 102 missing below 103: d = 2
    r.set(100, codes(100, 101, 103))
    assert r.step() == [[102]] and r.word(102) == (102, 1, 0) and r.counters() == (1, 1, 0, 0)
    before = r.model.nacks.copy()
    # not before retry_hops: three hops age it (the clock stands: a held slot still asks), the NACK bytes stay
    for age in (1, 2, 3):
        assert r.step() == [None] and r.word(102) == (102, 1, age) and np.array_equal(r.model.nacks, before)
    assert r.step() == [[102]] and r.word(102) == (102, 2, 0) and r.counters() == (2, 2, 0, 0)
    # at most max_requests: it ages for ever (saturating at 255) and is never asked again
    for _ in range(300):
        assert r.step() == [None]
    assert r.word(102) == (102, 2, 255) and r.counters() == (2, 2, 0, 0)
    # the clock passes it: EXPIRED, the word is free
    r.set(103, codes(103, 104))
    assert r.step() == [None] and r.word(102) == (0, 0, 0) and r.counters() == (2, 2, 0, 1)
    # a hole that arrives: RECOVERED
    r.set(103, codes(103, 106))
    assert r.step() == [[104, 105]] and r.counters() == (3, 4, 0, 1)
    r.set(104, codes(104, 106))
    assert r.step() == [None] and r.word(104) == (0, 0, 0) and r.word(105) == (105, 1, 1) and r.counters() == (3, 4, 1, 1)
    # a word whose hop left the window while another hop sits in its ring entry is EXPIRED, not RECOVERED
    r.set(110, codes(110, 105 + 16))
    assert r.step()[0] == list(range(111, 121)) and r.counters()[2:] == (1, 2)


def test_nack_model_skips_what_cannot_or_need_not_come():
    # d + 1 < rtt_hops is never asked: with rtt_hops = 3 the holes at d = 0 and 1 wait for nothing
    r = Ring(NackConfig(rtt_hops=3, retry_hops=1, max_requests=5))
    r.set(50, {53: "c"})
    assert r.step() == [[52]] and r.word(50) == r.word(51) == (0, 0, 0)
    r.set(51, {53: "c"})
    assert r.step() == [None] and r.counters() == (1, 1, 0, 0) and r.word(52) == (52, 1, 1)      # d = 1 now: it only ages
    # holes behind a SID are DTX silence; holes behind codes are not
    r = Ring(NackConfig(rtt_hops=1))
    r.set(10, {10: "c", 12: "s", 15: "c"})
    assert r.step() == [[11]]
    r = Ring(NackConfig(rtt_hops=1))
    r.set(10, {10: "s", 12: "c", 15: "c"})
    assert r.step() == [[13, 14]]
    # nothing below and ST_IN_DTX set: silence up to the first packet; without it they are asked
    r = Ring(NackConfig(rtt_hops=1))
    r.set(10, {12: "c", 14: "c"}, in_dtx=True)
    assert r.step() == [[13]]
    r = Ring(NackConfig(rtt_hops=1))
    r.set(10, {12: "c", 14: "c"})
    assert r.step() == [[10, 11, 13]]
    # a tail loss shows nothing, an empty ring nothing, a slot that is not anchored nothing
    r = Ring(NackConfig(rtt_hops=1))
    r.set(10, {10: "c"})
    assert r.step() == [None]
    r.set(10, {})
    assert r.step() == [None]
    r.set(10, {12: "c"}, anchored=False)
    assert r.step() == [None] and r.counters() == (0, 0, 0, 0)


def test_nack_model_skip_fecable():
    present = {20: "c", 22: "f", 24: "c", 26: "s"}
    for skip, m, want in ((True, 1, [23, 25]), (False, 1, [21, 23, 25]), (True, 0, [21, 23, 25])):
        r = Ring(NackConfig(rtt_hops=1, skip_fecable=skip), m=m)
        r.set(20, present)
        assert r.step() == [want], (skip, m)


def test_nack_model_far_holes_wait():
    """a hole 17 or more above base waits for a later hop and is not marked"""
    r = Ring(NackConfig(rtt_hops=1, retry_hops=2, max_requests=3), C=32)
    r.set(65530, {(65530 + 31) & 0xFFFF: "c"})
    want = [(65530 + k) & 0xFFFF for k in range(17)]
    assert r.step() == [want] and wire.parse_nack(r.model.nacks[0]) == (65530, 0xFFFF)
    assert r.word(want[-1]) == (want[-1], 1, 0) and r.word((65530 + 17) & 0xFFFF) == (0, 0, 0) and r.counters() == (1, 17, 0, 0)
    # next hop: the 14 further ones (free words) are asked, across the wrap; the first 17 age
    rest = [(65530 + k) & 0xFFFF for k in range(17, 31)]
    assert r.step() == [rest] and r.word(want[0]) == (want[0], 1, 1) and r.counters() == (2, 31, 0, 0)
    assert r.step() == [None]
    assert r.step() == [want]                                 # age 2 = retry_hops: the first 17 again, the rest at age 1


def test_nack_model_start_and_independent_slots():
    r = Ring(NackConfig(rtt_hops=1), B=3)
    r.set(5, {5: "c", 7: "c"}, b=0)
    r.set(900, {903: "c"}, b=2)
    assert r.step() == [[6], None, [900, 901, 902]]
    row1, row2 = r.model.state[1].copy(), r.model.state[2].copy()
    assert not row1.any() and r.counters(2) == (1, 3, 0, 0)
    # a start on slot 0 clears its row, bytes and flag; the jitter step has cleared its ring on the same hop; slot 2 only ages
    r.set(0, {}, b=0, anchored=False)
    assert r.step(np.array([-1, 0, 0]))[0] is None and not r.model.state[0].any() and not r.model.nacks[0].any()
    assert not r.model.state[1].any() and r.word(901, 2) == (901, 1, 1) and np.array_equal(r.model.state[2, :rtx.NK_RING], row2[:rtx.NK_RING])
    # a start on a hop that already anchored again: cleared first, then the rule
    r.set(40, {40: "c", 42: "c"}, b=0)
    assert r.step(np.array([-1, 0, 0]))[0] == [41] and r.counters(0) == (1, 1, 0, 0)


# ---------------------------------------------------------------- RtxModel
TB = wire.transport_bytes(4, 1, 1)                           # 3 + 7 = 10 bytes: no multiple of 4


def headed(h, seed=0, body=5, fec=False):
    rng = np.random.default_rng(1000 * seed + h)
    return wire.pack_transport(h, rng.integers(0, 256, size=body, dtype=np.uint8).tobytes(), 4, fec=fec)


def rows_of(blobs):
    out = np.zeros((len(blobs), TB), dtype=np.uint8)
    for b, p in enumerate(blobs):
        out[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return out, [len(p) for p in blobs]


def sent_of(out, b):
    return [out["packets"][b, q, :out["nbytes"][b, q]].tobytes() for q in range(out["nbytes"].shape[1]) if out["nbytes"][b, q]]


def test_rtx_model_store_fetch_miss_and_budget():
    m = RtxModel(1, RtxConfig(history=4, per_hop=2), TB)
    packets = {h: headed(h, body=7 if h % 2 else 5, fec=bool(h % 2)) for h in range(10)}
    for h in range(6):
        out = m.step(*rows_of([packets[h]]))
        assert not out["nbytes"].any() and not out["packets"].any()
    assert m.state[0].tolist() == [6, 0, 0, 0, 0]
    # byte-exact, zero past the length, in request order; hop 6 is stored on this hop and fetched on it
    out = m.step(*rows_of([packets[6]]), nacks=[nack_words(4, 0b10)])
    assert sent_of(out, 0) == [packets[4], packets[6]] and not out["packets"][0, 0, len(packets[4]):].any()
    assert m.state[0].tolist() == [7, 1, 2, 0, 0]
    # older than R hops: hop 2's entry holds hop 6, the tag does not match -> MISS, never a stale packet; hop 9 was never sent
    out = m.step(*rows_of([b""]), nacks=[nack_words(2, 1 << 6)])
    assert sent_of(out, 0) == [] and m.state[0].tolist() == [7, 2, 2, 2, 0]
    # the budget in request order: 3, 4, 5, 6 are all there, two are sent, two dropped
    out = m.step(*rows_of([b""]), nacks=[nack_words(3, 0b111)])
    assert sent_of(out, 0) == [packets[3], packets[4]] and m.state[0].tolist() == [7, 3, 4, 2, 2]
    # no NACK: the rows are zero again
    out = m.step(*rows_of([b""]))
    assert not out["nbytes"].any() and not out["packets"].any() and m.state[0].tolist() == [7, 3, 4, 2, 2]


def test_rtx_model_start_held_and_wrap():
    m = RtxModel(2, RtxConfig(history=8, per_hop=4), TB)
    h0 = 65533
    sent = {}
    for k in range(6):                                       # hops 65533 .. 2: across the wrap, both slots
        h = (h0 + k) & 0xFFFF
        sent[h] = [headed(h, seed=b) for b in range(2)]
        m.step(*rows_of(sent[h]))
    out = m.step(*rows_of([b"", b""]), nacks=[nack_words(65534, 0b1101), (0, 0)])     # a held hop stores nothing but answers
    assert sent_of(out, 0) == [sent[h][0] for h in (65534, 65535, 1, 2)] and sent_of(out, 1) == []
    assert m.state.tolist() == [[6, 1, 4, 0, 0], [6, 0, 0, 0, 0]]
    # a start on slot 0 empties its history, the counters stay; its neighbour's is intact
    out = m.step(*rows_of([b"", b""]), nacks=[nack_words(0, 0), nack_words(0, 0b1)], action=[-1, 0])
    assert sent_of(out, 0) == [] and sent_of(out, 1) == [sent[0][1], sent[1][1]]
    assert m.state.tolist() == [[6, 2, 4, 1, 0], [6, 1, 2, 0, 0]] and not m.tags[0].any()
    # a start on a hop that sends: cleared first, then stored (h = 0 again: the tag carries the byte count, so it is not "empty")
    p = headed(0, seed=9)
    out = m.step(*rows_of([p, b""]), nacks=[nack_words(0, 0), (0, 0)], action=[-1, 0])
    assert sent_of(out, 0) == [p] and m.tags[0, 0] == len(p) << 16


# ---------------------------------------------------------------- the closed loop on the models
@pytest.mark.parametrize("h0", [0, 65400])
@pytest.mark.parametrize("pattern", [singles_and_pairs, bursts_of_two])
def test_closed_loop_recovers_every_loss(pattern, h0):
    """depth 4 >= rtt_hops 2 + longest burst 2, capacity 8, 400 hops: with NACK and retransmission nothing is lost and every played
    body is the sent one; the same trace without them loses exactly what was dropped.  Slot 1 is an undisturbed neighbour."""
    drops = pattern()
    assert len(drops) == (40 if pattern is singles_and_pairs else 44) and max(drops) < HOPS - 8
    jm, nm, rm, wrong = run_models({0: drops}, h0=h0)
    assert lost(jm) == 0 and wrong == {0: [], 1: []}
    assert nm.state[0, rtx.NK_ASKED] == len(drops) == rm.state[0, rtx.RX_SENT] and rm.state[0, rtx.RX_MISS] == 0
    assert nm.state[0, rtx.NK_RECOVERED] + nm.state[0, rtx.NK_EXPIRED] == len(drops)
    jm0, nm0, rm0, wrong0 = run_models({0: drops}, h0=h0, nack=False)
    assert lost(jm0) == len(drops) and sorted(wrong0[0]) == sorted(drops) and wrong0[1] == []
    # the neighbour shows the same rows as in a run where nobody loses anything
    jq, nq, rq, _ = run_models({}, h0=h0)
    assert np.array_equal(jm.state[1], jq.state[1]) and np.array_equal(nm.state[1], nq.state[1]) and not nm.state[1, :rtx.NK_RING].any()
    assert np.array_equal(rm.state[1], rq.state[1]) and np.array_equal(rm.tags[1], rq.tags[1]) and lost(jm, 1) == 0


def test_closed_loop_needs_the_depth():
    """depth 2 < rtt_hops + 1: a single loss shows when the next packet arrives, at d = 0, too late to ask: every loss stays"""
    drops = singles_and_pairs()
    jm, nm, _, _ = run_models({0: drops}, jcfg=JitterConfig(2, 8))
    assert lost(jm) == len(drops) and nm.state[0, rtx.NK_ASKED] == 0


def test_closed_loop_second_request():
    """depth 6, hop 50 and its first retransmission dropped: the second request recovers it, one request alone loses exactly it"""
    jm, nm, rm, wrong = run_models({0: {50}}, jcfg=JitterConfig(6, 8), ncfg=NackConfig(2, 2, 2), drop_rtx=[(0, 50)])
    assert lost(jm) == 0 and wrong == {0: [], 1: []} and nm.state[0, rtx.NK_ASKED] == 2 == rm.state[0, rtx.RX_SENT]
    jm, nm, rm, wrong = run_models({0: {50}}, jcfg=JitterConfig(6, 8), ncfg=NackConfig(2, 2, 1), drop_rtx=[(0, 50)])
    assert lost(jm) == 1 and wrong == {0: [50], 1: []} and nm.state[0, rtx.NK_ASKED] == 1 == rm.state[0, rtx.RX_SENT]
