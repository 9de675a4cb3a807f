"""CPU: the delay-based bandwidth estimate (hilcodec_amd/bwe.py, the definition of hilc_rx_bwe and hilc_rate_cap): the row layouts
against the C header, the configurations' bounds, the cap's wire format, BweModel and CapModel on scripted traces, the custom ops' fake
kernels, the library's argument checks, and the closed loop on the models over a drop-tail bottleneck (tests/bwe_loop.py).  Everything
is integer: every comparison is exact.

The closed loop's figures, hops [1000, 3000) of 3 000 (rate= alone -> with bwe= and cap=; profiles/bwe_loop.txt): bottleneck 60: loss
0.031 -> 0.000, mean one-way delay 60.2 -> 27.5 ms, 55.9 bits per hop sent (0.93 of the bottleneck); 80: loss 0.057 -> 0.000, delay
59.0 -> 27.9 ms, 74.8 bits (0.93); 200: byte-equal packets, no decrease."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from hilcodec_amd import bwe, dtx, jitter, rate, report, wire
from hilcodec_amd.bwe import BweConfig, BweModel, CapConfig, CapModel, cap_word
from hilcodec_amd.rate import RateConfig, RateModel
from tests.bwe_loop import LOOP_BWE, run_models
from tests.hops import HEADER, assert_entry_points, bare_model
from tests.rate_loop import N

DEV_CPU = torch.device("cpu")


# ---------------------------------------------------------------- layout and entry points
def test_layouts_match_header():
    """bwe.<NAME> is `#define HILC_BWE_<NAME>`, value for value, in both directions; both rows are dense"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_BWE_"):
            header[name[len("HILC_BWE_"):]] = env[name]
    borrowed = set(vars(report)) | set(vars(rate)) | set(vars(wire))
    python = {k: v for k, v in vars(bwe).items() if k.isupper() and not k.startswith("_") and isinstance(v, int)
              and not isinstance(v, bool) and k not in borrowed}
    assert len(header) >= 60 and header == python
    scalars = sorted(v for k, v in header.items() if k.startswith("BW_") and k not in ("BW_WORDS", "BW_TREND", "BW_RING"))
    assert scalars == list(range(bwe.BW_TREND)) and bwe.BW_RING == bwe.BW_TREND + 2 * bwe.MAX_WINDOW
    assert bwe.BW_WORDS == bwe.BW_RING + 2 * bwe.MAX_WINDOW == 156
    assert [getattr(bwe, "BW_" + n.upper()) for n in bwe.BW_NAMES] == list(range(bwe.BW_SAMPLES, bwe.BW_TREND))
    assert sorted(v for k, v in header.items() if k.startswith("CP_") and k != "CP_WORDS") == list(range(bwe.CP_WORDS))
    assert [getattr(bwe, "CP_" + n.upper()) for n in bwe.CP_NAMES] == list(range(bwe.CP_CAPS, bwe.CP_WORDS))
    assert env["HILC_WIRE_CAP_BYTES"] == wire.CAP_BYTES == 3 and bwe.HOP_TICKS == 320
    # the constants the rule names: 12.5, 6 and 600 in Q16; 0.0087 / 24 and 0.039 / 24 in Q24; 10 ms and 100 ms in ticks
    assert (bwe.THR_START, bwe.THR_MIN, bwe.THR_MAX) == (int(12.5 * 65536), 6 << 16, 600 << 16)
    assert (bwe.K_UP, bwe.K_DOWN) == (round(0.0087 / 24 * (1 << 24)), round(0.039 / 24 * (1 << 24)))
    assert (bwe.OVER_TICKS, bwe.ADAPT_TICKS) == (240, 2400)
    assert "cap" in __import__("hilcodec_amd.sessions", fromlist=["x"]).ONE_HOP_ROWS


def test_entry_points_are_declared_exported_and_bound():
    assert_entry_points(("hilc_rx_bwe", "hilc_rate_cap"), in_abi16_line=True)
    assert os.path.isfile(os.path.join(os.path.dirname(bwe.__file__), "csrc", "bwe.hip"))


# ---------------------------------------------------------------- configuration and the wire
def test_config_checks_its_ranges():
    c = BweConfig(2.625, 9.0)
    assert c == BweConfig(2.625, 9.0, 20, 16, 26, 218, None, 8, 72000) and c.increase(1) == 70 and c.increase(3) == 210
    assert BweConfig(3, 9, increase_q16=5).increase(3) == 5 and BweConfig(3, 3).increase(2000) == 65535
    BweConfig(1, 2, window=2, rate_window=4, alpha_q8=256, beta_q8=1, increase_q16=0, interval=1024, reset_ticks=1 << 17)
    for kw in (dict(min_kbps=0), dict(min_kbps=-1.0), dict(max_kbps=float("inf")), dict(max_kbps=float("nan")), dict(min_kbps=True),
               dict(min_kbps="3"), dict(min_kbps=10.0), dict(window=1), dict(window=33), dict(window=20.0), dict(rate_window=3),
               dict(rate_window=33), dict(alpha_q8=0), dict(alpha_q8=257), dict(beta_q8=0), dict(beta_q8=256), dict(increase_q16=-1),
               dict(increase_q16=65536), dict(increase_q16=True), dict(interval=0), dict(interval=1025), dict(reset_ticks=0),
               dict(reset_ticks=(1 << 17) + 1)):
        with pytest.raises(ValueError):
            BweConfig(**{**dict(min_kbps=2.625, max_kbps=9.0), **kw})
    assert CapConfig() == CapConfig(0) and CapConfig(40).timeout_hops == 40
    for bad in (-1, 1.5, True, 1 << 30):
        with pytest.raises(ValueError):
            CapConfig(bad)


def test_bits_converts_and_checks_the_uint16_cap():
    assert bwe.bits(LOOP_BWE, 1) == (35, 120) == rate.bucket(RateConfig(2.625, 9.0), 1, 0, True)[1:3]
    assert bwe.bits(BweConfig(2.625, 9.0), 3) == (105, 360)
    top = 65535 * 24000 / 320 / 1000                                                 # kbps of 65535 bits per hop
    assert bwe.bits(BweConfig(3.0, top), 1).max_bits == 65535
    for cfg, T in ((BweConfig(3.0, top + 0.1), 1), (BweConfig(3.0, 9.0), 547), (BweConfig(0.07, 9.0), 1), (LOOP_BWE, 0),
                   (LOOP_BWE, bwe.MAX_FRAMES + 1), (RateConfig(3.0, 9.0), 1)):
        with pytest.raises(ValueError):
            bwe.bits(cfg, T)
    with pytest.raises(ValueError):
        BweModel(1, BweConfig(3.0, 4000.0), 31, 1, bwe.MAX_FRAMES)                   # a headed packet of more than 2^15 bytes
    for lo, hi in ((0, 5), (6, 5), (1, (1 << 22) + 1)):
        with pytest.raises(ValueError):
            CapModel(1, CapConfig(), lo, hi)
    assert bwe.kbps(BweModel(2, LOOP_BWE, N).state, 1).tolist() == [9.0, 9.0]


def test_cap_round_trip_and_refusals():
    for seq, cap in ((0, 0), (255, 65535), (7, 300), (200, 0x1234)):
        blob = wire.pack_cap(seq, cap)
        assert len(blob) == wire.CAP_BYTES and wire.parse_cap(blob) == (seq, cap) and blob[1:] == cap.to_bytes(2, "big")
        assert cap_word(seq, cap) == bwe.CAP_PRESENT | seq << 16 | cap
        assert wire.parse_cap(np.frombuffer(blob, dtype=np.uint8)) == (seq, cap)
    for seq, cap in ((-1, 0), (256, 0), (0, -1), (0, 65536), (True, 0), (0, 1.0), ("1", 0)):
        with pytest.raises(ValueError):
            wire.pack_cap(seq, cap)
    for blob in (b"", b"ab", b"abcd"):
        with pytest.raises(ValueError):
            wire.parse_cap(blob)


# ---------------------------------------------------------------- BweModel on scripted traces
TB = wire.transport_bytes(N, 0, 1)                           # 13


def packet(h, n=N, sid_order=None):
    if sid_order is not None:
        return wire.pack_transport(h, bytes(1 + sid_order), 0, sid=True)
    return wire.pack_transport(h, bytes(wire.packet_bytes(n, 1)), n)


def feed(m, h, t, b=0, **kw):
    """one hop with one arrival (h, t) for slot b -> the step's output"""
    p = packet(h, **kw)
    row = np.zeros((1, m.tbytes), dtype=np.uint8)
    row[0, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return m.step(None, [b], row, [len(p)], [t])


def row(m, b=0):
    names = ("rate_q8", "thr", "seen", "last_h", "last_t", "acc", "sm", "count", "prev_m", "over_ticks", "over_count", "signal", "state",
             "phase", "seq", "n", "head", "rn", "rhead") + bwe.BW_NAMES
    return {k: int(m.state[b, getattr(bwe, "BW_" + k.upper())]) for k in names}


def test_model_fresh_rows_first_arrival_and_emission():
    m = BweModel(2, LOOP_BWE, N)
    assert m.state[:, bwe.BW_RATE_Q8].tolist() == [120 * 256] * 2 and m.state[:, bwe.BW_THR].tolist() == [bwe.THR_START] * 2
    assert not m.state[:, bwe.BW_SEEN:].any() and not m.caps.any()
    # hops without arrivals: the phase runs, nothing is emitted for a slot that has seen nothing
    for _ in range(10):
        o = m.step(None, [], np.zeros((0, TB), dtype=np.uint8), [], [])
        assert not o["due"].any()
    assert row(m)["phase"] == 10 and row(m)["caps"] == 0
    # the first arrival is only remembered; the cap is due at once (the phase is past the interval)
    o = feed(m, 7, 1000)
    r = row(m)
    assert (r["seen"], r["last_h"], r["last_t"], r["samples"], r["rn"], r["n"]) == (1, 7, 1000, 0, 1, 0)
    assert o["due"].tolist() == [1, 0] and wire.parse_cap(o["caps"][0]) == (1, 120) and (r["phase"], r["seq"], r["caps"]) == (0, 1, 1)
    # then every `interval` hops; the bytes stay between caps
    for k in range(1, 17):
        o = feed(m, 7 + k, 1000 + 320 * k)
        assert o["due"][0] == (k % 8 == 0) and wire.parse_cap(o["caps"][0]) == (1 + k // 8, 120)
    r = row(m)
    assert r["samples"] == 16 and r["acc"] == 0 and r["sm"] == 0 and r["signal"] == bwe.SIGNAL_NORMAL and r["state"] == bwe.STATE_INCREASE
    assert r["increased"] == 16 and r["rate_q8"] == 120 * 256                      # saturated at max_bits
    # an action clears the row and the cap bytes, counters included
    o = m.step([1, 0], [], np.zeros((0, TB), dtype=np.uint8), [], [])
    assert row(m) == {**{k: 0 for k in row(m)}, "rate_q8": 120 * 256, "thr": bwe.THR_START, "phase": 1} and not o["caps"].any()
    assert not m.state[0, bwe.BW_TREND:].any()


def test_model_growing_delay_signals_overuse_and_falls_to_beta_r():
    """packets sent one hop apart arrive 352 ticks apart: the queue grows by a tenth of a hop per hop"""
    m = BweModel(1, LOOP_BWE, N)
    first = None
    for k in range(40):
        o = feed(m, k, 352 * k)
        assert (row(m)["thr"] >= bwe.THR_MIN) and row(m)["thr"] <= bwe.THR_MAX
        if row(m)["decreased"] and first is None:
            first = k
            R_q8 = (15 * 104 * 256 * 320) // (15 * 352)                             # 16 packets of 104 bits, 15 gaps of 352 ticks
            assert row(m)["rate_q8"] == (R_q8 * 218) >> 8 == m.incoming_q8(m.state[0]) * 218 >> 8
            assert o["due"][0] == 1 and wire.parse_cap(o["caps"][0])[1] == row(m)["rate_q8"] >> 8 == 80
            assert row(m)["state"] == bwe.STATE_HOLD and row(m)["signal"] == bwe.SIGNAL_OVERUSE and row(m)["phase"] == 0
    # not before the window of 20 samples is full (sample k is the k-th), and soon after
    assert first is not None and 20 <= first <= 24 and row(m)["overuse"] >= 1 and row(m)["acc"] == 32 * 39
    # while the delay keeps growing, the estimate stays down: only a lower value replaces it
    assert row(m)["rate_q8"] <= 80 * 256 + 255


@pytest.mark.parametrize("delay", [0, 5000, 1 << 20, (1 << 32) - 7])
def test_model_constant_delay_of_any_size_never_decreases(delay):
    m = BweModel(1, LOOP_BWE, N)
    for k in range(300):
        feed(m, 65500 + k, delay + 320 * k)                  # the hop index wraps 2^16 on the way, the tick 2^32 for the last delay
    r = row(m)
    assert (r["samples"], r["overuse"], r["underuse"], r["decreased"], r["old"], r["reset"]) == (299, 0, 0, 0, 0, 0)
    assert r["acc"] == 0 and r["rate_q8"] == 120 * 256 and r["thr"] == bwe.THR_MIN


def test_model_draining_queue_signals_underuse_and_holds():
    m = BweModel(1, BweConfig(2.625, 9.0, increase_q16=0), N)
    m.state[0, bwe.BW_RATE_Q8] = 60 * 256
    t = 0
    for k in range(60):
        t += 320 if k < 30 else 280                          # arrivals closer together than they were sent: the queue drains
        feed(m, k, t)
    r = row(m)
    assert r["underuse"] == 1 and r["signal"] == bwe.SIGNAL_UNDERUSE and r["state"] == bwe.STATE_HOLD and r["acc"] < 0
    assert r["rate_q8"] > 60 * 256 and r["decreased"] == 0                          # it rose (by one per calm sample) until the under-use


def test_model_old_hop_indices_are_ignored():
    m = BweModel(1, LOOP_BWE, N)
    for k in range(30):
        feed(m, 100 + k, 320 * k)
    before = row(m)
    for h, t in ((129, 320 * 29), (120, 320 * 31), (129 - 32768 + 65536, 320 * 32)):          # a duplicate, a retransmission, dh = -32768
        feed(m, h & 0xFFFF, t)
    after = row(m)
    assert after["old"] == 3
    assert {k: v for k, v in after.items() if k not in ("old", "phase", "seq", "caps")} == \
        {k: v for k, v in before.items() if k not in ("old", "phase", "seq", "caps")}
    feed(m, 130, 320 * 33)                                   # the next new packet is measured against the last sampled one
    assert row(m)["samples"] == before["samples"] + 1 and row(m)["acc"] == 320 * 33 - 320 * 29 - 320


def test_model_gap_above_reset_ticks_and_backward_time_restart():
    m = BweModel(1, LOOP_BWE, N)
    for k in range(30):
        feed(m, k, 350 * k)
    assert row(m)["count"] == 29 and row(m)["n"] == 20 and row(m)["rn"] == 16
    feed(m, 40, 350 * 29 + 72000)                            # exactly reset_ticks: still a sample
    assert row(m)["reset"] == 0 and row(m)["count"] == 30
    rate_before = row(m)["rate_q8"]
    feed(m, 41, 350 * 29 + 72000 + 72001)
    r = row(m)
    assert (r["reset"], r["count"], r["n"], r["head"], r["acc"], r["sm"], r["rn"], r["thr"]) == (1, 0, 0, 0, 0, 0, 1, bwe.THR_START)
    assert (r["last_h"], r["rate_q8"], r["seen"]) == (41, rate_before, 1)
    feed(m, 42, 350 * 29 + 72000 + 72001 - 5)                # time runs backwards: da < 0
    assert row(m)["reset"] == 2 and row(m)["samples"] == 30


def test_model_sid_and_malformed_arrivals():
    K = 5
    m = BweModel(1, LOOP_BWE, N, 0, 1, K)
    for k in range(10):
        feed(m, k, 320 * k)
    assert row(m)["rn"] == 10
    feed(m, 10, 3200, sid_order=K)                           # a SID is sampled for its delay, and empties the rate ring
    assert row(m)["rn"] == 0 and row(m)["samples"] == 10 and row(m)["malformed"] == 0
    for k in range(11, 14):
        feed(m, k, 320 * k)
    assert row(m)["rn"] == 3 and m.incoming_q8(m.state[0]) is None                  # fewer than 4 entries: no valid rate
    feed(m, 14, 320 * 14)
    assert m.incoming_q8(m.state[0]) == 3 * 104 * 256 * 320 // (3 * 320)
    before = row(m)
    bad = np.zeros((3, m.tbytes), dtype=np.uint8)
    bad[0, :3] = (0, 15, 0x20 | 8)                           # the reserved bit
    bad[1, :3] = (0, 15, 9)                                  # n = 9 > n_max
    m.step(None, [0, 0, 0], bad, [13, 13, 2], [5000, 5000, 5000])
    after = row(m)
    assert after["malformed"] == 3 and {k: v for k, v in after.items() if k not in ("malformed", "phase", "seq", "caps")} == \
        {k: v for k, v in before.items() if k not in ("malformed", "phase", "seq", "caps")}
    plain = BweModel(1, LOOP_BWE, N)                         # without comfort noise a SID is malformed
    feed(plain, 0, 0, sid_order=K)
    assert row(plain)["malformed"] == 1 and row(plain)["seen"] == 0


def test_model_threshold_stays_in_bounds_and_the_int64_bounds_hold_at_the_extremes():
    """the model asserts every 64-bit bound itself (bwe._fits and the asserts beside the regression): these traces take it to them"""
    rng = np.random.default_rng(5)
    wide = BweConfig(2.625, 9.0, window=32, rate_window=32, alpha_q8=256, reset_ticks=1 << 17)
    m = BweModel(1, wide, N)
    t = 0
    for k in range(80):                                      # the largest gap every time: acc at its clamp, the longest window
        t += 1 << 17
        feed(m, k, t)
        assert bwe.THR_MIN <= row(m)["thr"] <= bwe.THR_MAX
    assert row(m)["acc"] == bwe.ACC_MAX and row(m)["sm"] == bwe.ACC_MAX << 8 and row(m)["reset"] == 0
    h = 79
    for k in range(80):                                      # the largest hop step with no time passing: acc at the other clamp
        h += 32767
        t += k & 1
        feed(m, h & 0xFFFF, t)
        assert bwe.THR_MIN <= row(m)["thr"] <= bwe.THR_MAX and abs(row(m)["prev_m"]) <= bwe.SLOPE_MAX * 240
    assert row(m)["acc"] == -bwe.ACC_MAX and row(m)["old"] == 0
    m = BweModel(1, BweConfig(0.075, 9.83, window=32, rate_window=32, alpha_q8=256, increase_q16=65535), 31, 1, 500)
    assert m.bits == (499, 65533) and m.tbytes == 20003
    big = np.zeros((1, m.tbytes), dtype=np.uint8)
    t = 0
    for k in range(200):                                     # the widest packets one tick apart: the largest incoming rate
        p = wire.pack_transport(k, bytes(wire.packet_bytes(32, 500)), 31, fec=True)
        big[0, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        t += int(rng.integers(1, 3))
        m.step(None, [0], big, [len(p)], [t])
        assert bwe.THR_MIN <= row(m)["thr"] <= bwe.THR_MAX
    assert row(m)["samples"] == 199 and m.incoming_q8(m.state[0]) > 1 << 40


def test_model_random_jitter_keeps_the_threshold_in_bounds():
    rng = np.random.default_rng(11)
    m = BweModel(1, LOOP_BWE, N)
    t = 0
    for k in range(600):
        t += int(rng.integers(0, 2000)) if k % 100 < 50 else int(rng.integers(0, 200))      # the queue fills, then drains
        feed(m, k, t)
        assert bwe.THR_MIN <= row(m)["thr"] <= bwe.THR_MAX
    assert row(m)["overuse"] > 0 and row(m)["underuse"] > 0


@pytest.mark.parametrize("trace", ["noise", "fast", "slow"])
def test_model_never_decreases_on_an_uncongested_link(trace):
    """6 000 hops of a sender that is not congested: uniform 0 - 5 ms of arrival noise, or a sender clock 200 ppm off either way"""
    rng = np.random.default_rng(2)
    m = BweModel(1, LOOP_BWE, N)
    for k in range(6000):
        t = 320 * k + int(rng.integers(0, 121)) if trace == "noise" else (320 * k * (1000000 + (200 if trace == "slow" else -200))) // 1000000
        feed(m, k & 0xFFFF, t)
    r = row(m)
    assert r["decreased"] == 0 and r["overuse"] == 0 and r["rate_q8"] == 120 * 256 and r["samples"] == 5999


# ---------------------------------------------------------------- CapModel
def cap_row(m, b=0):
    return {k: int(m.state[b, getattr(bwe, "CP_" + k.upper())]) for k in ("cap_q8", "seen", "last", "age") + bwe.CP_NAMES}


def test_cap_model_sequence_clamp_timeout_hold_and_action():
    rm = RateModel(2, RateConfig(2.625, 9.0), N, 1, 0, True)
    cm = CapModel(2, CapConfig(timeout_hops=4), 35, 120)
    cm.step(rm.state)
    assert not cm.state[:, :bwe.CP_AGE].any() and cm.state[:, bwe.CP_AGE].tolist() == [1, 1] and rm.state[:, rate.RC_RATE_Q8].tolist() == [120 * 256] * 2
    cm.step(rm.state, [cap_word(5, 80), cap_word(9, 20)])                            # below min_bits: clamped to 35
    assert cap_row(cm) == dict(cap_q8=80 * 256, seen=1, last=5, age=1, caps=1, stale=0, timeout=0, clamped=1)
    assert cap_row(cm, 1)["cap_q8"] == 35 * 256 and rm.state[:, rate.RC_RATE_Q8].tolist() == [80 * 256, 35 * 256]
    # stale: the same seq, an older one, d = 128; a fresh one above max_bits: clamped to 120, which lowers nothing
    for seq in (5, 4, 133):
        cm.step(rm.state, [cap_word(seq, 40), 0], hold=[0, 1])
    assert cap_row(cm)["stale"] == 3 and cap_row(cm)["cap_q8"] == 80 * 256 and cap_row(cm)["timeout"] == 1 and cap_row(cm)["seen"] == 0
    assert cap_row(cm, 1)["age"] == 1 and cap_row(cm, 1)["seen"] == 1              # held: no ageing, so no timeout
    cm.step(rm.state, [cap_word(4, 500), 0])                                         # forgotten: any seq is the first again
    assert cap_row(cm)["cap_q8"] == 120 * 256 and cap_row(cm)["caps"] == 2 and cap_row(cm)["clamped"] == 1
    assert rm.state[0, rate.RC_RATE_Q8] == 80 * 256                                  # the cap never raises the rate
    # the rate rule's own increase is cut back on the next hop
    cm.step(rm.state, [cap_word(5, 60), 0])
    rm.ceiling([report.report_word(1, 0, 0), 0])
    assert rm.state[0, rate.RC_RATE_Q8] > 60 * 256
    cm.step(rm.state)
    assert rm.state[0, rate.RC_RATE_Q8] == 60 * 256 and cap_row(cm)["clamped"] == 3
    # a held slot takes its cap too; an action clears the row first
    cm.step(rm.state, [0, cap_word(200, 50)], action=[1, 0], hold=[0, 1])
    assert cap_row(cm) == dict(cap_q8=0, seen=0, last=0, age=1, caps=0, stale=0, timeout=0, clamped=0)
    assert cap_row(cm, 1)["last"] == 200 and cap_row(cm, 1)["cap_q8"] == 50 * 256 and cap_row(cm, 1)["age"] == 0
    never = CapModel(1, CapConfig(), 35, 120)
    one = RateModel(1, RateConfig(2.625, 9.0), N, 1, 0, True)
    never.step(one.state, [cap_word(1, 70)])
    for _ in range(50):
        never.step(one.state)
    assert cap_row(never)["age"] == 51 and cap_row(never)["timeout"] == 0 and cap_row(never)["seen"] == 1


# ---------------------------------------------------------------- custom ops, the library's checks, the hops' options
def test_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hilcodec_amd import ops
    with FakeTensorMode():
        B, A = 5, 10
        ints = dict(dtype=torch.int32, device="cuda")
        arrivals, offsets, times = torch.zeros(A, 1 + (TB + 3) // 4, **ints), torch.zeros(B + 1, **ints), torch.zeros(A, **ints)
        rows, due = torch.zeros(B, bwe.BW_WORDS, **ints), torch.zeros(B, **ints)
        caps = torch.zeros(B, 3, dtype=torch.uint8, device="cuda")
        assert ops.rx_bwe(arrivals, offsets, times, rows, caps, due, LOOP_BWE, N, 1, 0, None, torch.zeros(B, **ints)) is None
        cp, rc = torch.zeros(B, bwe.CP_WORDS, **ints), torch.zeros(B, rate.RC_WORDS, **ints)
        assert ops.rate_cap(cp, rc, CapConfig(), 35, 120, torch.zeros(B, **ints)) is None
    # the wrapper checks the configuration against the hop before anything is dispatched
    with pytest.raises(ValueError, match="bits per hop"):
        ops.rx_bwe(None, None, None, None, None, None, BweConfig(3.0, 9.0), N, 547)
    assert torch.ops.hilcodec.rx_bwe.default._schema.is_mutable and torch.ops.hilcodec.rate_cap.default._schema.is_mutable


def test_library_argument_checks():
    """null pointers and bad shapes are refused before any launch (no GPU is touched: every call returns from its checks)"""
    from hilcodec_amd._lib import lib
    OK_NULL, OK_SHAPE = -2, -1
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=4, T=1, n_max=8, m=0, order=-1, min_bits=35, max_bits=120, window=20, rate_window=16, alpha_q8=26, beta_q8=218,
                increase_q16=70, interval=8, reset_ticks=72000)

    def rx(arrivals=p, offsets=p, times=p, max_arrivals=8, rows=p, caps=p, due=p, **kw):
        a = {**good, **kw}
        return lib.hilc_rx_bwe(arrivals, offsets, times, max_arrivals, None, rows, caps, due, *[a[k] for k in good], None)

    for name in ("arrivals", "offsets", "times", "rows", "caps", "due"):
        assert rx(**{name: None}) == OK_NULL, name
    for kw in (dict(B=0), dict(max_arrivals=-1), dict(T=0), dict(T=1025), dict(n_max=0), dict(n_max=32), dict(m=-1), dict(m=9),
               dict(n_max=31, m=2), dict(order=-2), dict(order=dtx.MAX_ORDER + 1), dict(n_max=31, m=1, T=1024), dict(min_bits=0),
               dict(min_bits=121), dict(max_bits=65536), dict(window=1), dict(window=33), dict(rate_window=3), dict(rate_window=33),
               dict(alpha_q8=0), dict(alpha_q8=257), dict(beta_q8=0), dict(beta_q8=256), dict(increase_q16=-1), dict(increase_q16=65536),
               dict(interval=0), dict(interval=1025), dict(reset_ticks=0), dict(reset_ticks=(1 << 17) + 1)):
        assert rx(**kw) == OK_SHAPE, kw

    def cap(rows=p, rate_rows=p, B=4, min_bits=35, max_bits=120, timeout_hops=0):
        return lib.hilc_rate_cap(None, None, None, rows, rate_rows, B, min_bits, max_bits, timeout_hops, None)

    assert cap(rows=None) == OK_NULL and cap(rate_rows=None) == OK_NULL
    for kw in (dict(B=0), dict(min_bits=0), dict(min_bits=121), dict(max_bits=(1 << 22) + 1), dict(timeout_hops=-1)):
        assert cap(**kw) == OK_SHAPE, kw


def test_hop_options_are_checked_before_anything_is_allocated():
    """the constructors refuse a bwe= without jitter=, a cap= without rate= and wrong types before they touch a device"""
    import inspect
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    model = bare_model()
    with pytest.raises(ValueError, match="jitter"):
        GraphedDecodeHop(model, 2, 1, N, DEV_CPU, sessions=True, bwe=LOOP_BWE)
    with pytest.raises(ValueError, match="BweConfig"):
        GraphedDecodeHop(model, 2, 1, N, DEV_CPU, sessions=True, jitter=jitter.JitterConfig(2, 8), bwe=CapConfig())
    with pytest.raises(ValueError, match="bits per hop"):
        GraphedDecodeHop(model, 2, 600, N, DEV_CPU, sessions=True, jitter=jitter.JitterConfig(2, 8), bwe=LOOP_BWE)
    with pytest.raises(ValueError, match="rate"):
        GraphedEncodeHop(model, 2, 320, N, DEV_CPU, sessions=True, header=True, cap=CapConfig())
    with pytest.raises(ValueError, match="CapConfig"):
        GraphedEncodeHop(model, 2, 320, N, DEV_CPU, sessions=True, header=True, rate=RateConfig(2.625, 9.0), cap=LOOP_BWE)
    assert inspect.signature(GraphedDecodeHop.__init__).parameters["bwe"].default is None
    assert inspect.signature(GraphedDecodeHop.play).parameters["times"].default is None
    assert inspect.signature(GraphedEncodeHop.__init__).parameters["cap"].default is None
    assert inspect.signature(GraphedEncodeHop.step).parameters["caps"].default is None


# ---------------------------------------------------------------- the closed loop on the models
STEP = ((0, 200), (1000, 60), (2000, 200))


@pytest.fixture(scope="module")
def loops():
    """each loop once: {(caps, estimate): Loop}"""
    return {(caps, est): run_models(list(caps) if isinstance(caps, tuple) else caps, estimate=est)
            for caps in (60, 80, 200, STEP) for est in (True, False)}


@pytest.mark.parametrize("cap", [60, 80])
def test_closed_loop_lowers_loss_and_delay_at_a_bottleneck_without_starving_it(loops, cap):
    with_, without = loops[cap, True], loops[cap, False]
    lo, hi = 1000, 3000
    loss, loss0 = with_.trace.loss(lo, hi), without.trace.loss(lo, hi)
    delay, delay0 = with_.mean_delay_ms(lo, hi), without.mean_delay_ms(lo, hi)
    bits = with_.trace.mean_bits(lo, hi)
    print(f"bottleneck {cap}: loss {loss0:.4f} -> {loss:.4f}, mean delay {delay0:.1f} -> {delay:.1f} ms, {bits:.1f} bits per hop sent "
          f"({bits / cap:.3f} of the bottleneck); estimate row {with_.bm.state[0, :bwe.BW_TREND].tolist()}")
    assert loss0 > 0 and loss < loss0
    assert delay < delay0
    assert bits >= 0.8 * cap
    # the loop is closed: the receiver saw the queue grow, its caps arrived in order and held the sender's rate down
    st, cp = with_.bm.state[0], with_.cm.state[0]
    assert st[bwe.BW_DECREASED] > 0 and st[bwe.BW_OVERUSE] > 0 and st[bwe.BW_OLD] == 0 and st[bwe.BW_MALFORMED] == 0
    assert cp[bwe.CP_CAPS] >= 3000 // 8 - 2 and cp[bwe.CP_STALE] == 0 and cp[bwe.CP_CLAMPED] > 0
    assert not without.bm.state[0, bwe.BW_SEEN:].any()                              # the run without never fed its estimator


def test_closed_loop_leaves_a_wide_link_alone(loops):
    with_, without = loops[200, True], loops[200, False]
    assert with_.packets == without.packets and len(with_.packets) == 3000          # byte-equal, hop for hop
    st = with_.bm.state[0]
    assert st[bwe.BW_DECREASED] == 0 and st[bwe.BW_OVERUSE] == 0 and st[bwe.BW_RATE_Q8] == 120 * 256
    assert with_.cm.state[0, bwe.CP_CLAMPED] == 0 and np.array_equal(with_.rate_rows, without.rate_rows)


def test_closed_loop_follows_a_step_down_and_recovers(loops):
    with_, without = loops[STEP, True], loops[STEP, False]
    assert with_.trace.loss(1000, 2000) < without.trace.loss(1000, 2000)
    assert with_.mean_delay_ms(1200, 2000) < without.mean_delay_ms(1200, 2000)
    assert (with_.trace.n[:1000] == N).all() and (with_.trace.n[1100:2000] < N).any()
    assert (with_.trace.n[2800:] == N).all() and not with_.trace.dropped[2200:].any()
