"""CPU: report-driven rate control (hilcodec_amd/rate.py, the definition of hilc_rate_ceiling and hilc_rate_charge): the row layout
against the C header, the configuration's bounds, RateModel on scripted hops, the custom ops' fake kernels, the library's argument
checks, and the closed loop on the models over a drop-tail bottleneck (tests/rate_loop.py).  Everything is integer: every comparison
is exact.

The closed loop's figures, last 1 000 of 3 000 hops (loss without -> with control; bits sent per hop): bottleneck 60: 0.423 -> 0.031,
62.0; 80: 0.230 -> 0.056, 85.0; 200: no loss, n = 8 throughout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from hilcodec_amd import rate, report, vbr, wire
from hilcodec_amd.rate import RateConfig, RateModel
from hilcodec_amd.report import report_word
from tests.hops import HEADER, assert_entry_points
from tests.rate_loop import FULL_BITS, LOOP_RATE, N, run_models

# ---------------------------------------------------------------- layout and entry points
def test_layouts_match_header():
    """rate.<NAME> is `#define HILC_RATE_<NAME>`, value for value, in both directions; the row is dense"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    env, header = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        if name.startswith("HILC_RATE_"):
            header[name[len("HILC_RATE_"):]] = env[name]
    borrowed = set(vars(report)) | set(vars(vbr)) | set(vars(wire))
    python = {k: v for k, v in vars(rate).items() if k.isupper() and not k.startswith("_") and isinstance(v, int)
              and not isinstance(v, bool) and k not in borrowed}
    assert len(header) >= 14 and header == python
    words = sorted(v for k, v in header.items() if k.startswith("RC_") and k != "RC_WORDS")
    assert words == list(range(rate.RC_WORDS)) and rate.RC_WORDS == 12
    assert [getattr(rate, "RC_" + n.upper()) for n in rate.RC_NAMES] == list(range(rate.RC_REPORTS, rate.RC_WORDS))
    assert (rate.RC_RATE_Q8, rate.RC_CREDIT, rate.RC_SEEN, rate.RC_LAST, rate.RC_AGE, rate.RC_LOSS) == tuple(range(6))
    assert env["HILC_REPORT_REPORT_PRESENT"] == report.REPORT_PRESENT and env["HILC_WIRE_TRANSPORT_HEADER"] == wire.TRANSPORT_HEADER


def test_entry_points_are_declared_exported_and_bound():
    assert_entry_points(("hilc_rate_ceiling", "hilc_rate_charge"), in_abi16_line=True)
    assert os.path.isfile(os.path.join(os.path.dirname(rate.__file__), "csrc", "rate.hip"))


# ---------------------------------------------------------------- configuration
def test_config_checks_its_ranges():
    c = RateConfig(2.625, 9.0)
    assert c == RateConfig(2.625, 9.0, None, 26, 5, 13, 8, 0) and c.start == 9.0
    RateConfig(3, 9, 3), RateConfig(3, 9, 9), RateConfig(3, 3), RateConfig(1, 2, high_q8=255, low_q8=254), RateConfig(1, 2, high_q8=1, low_q8=0)
    for kw in (dict(min_kbps=0), dict(min_kbps=-1.0), dict(max_kbps=float("inf")), dict(max_kbps=float("nan")), dict(min_kbps=True),
               dict(min_kbps="3"), dict(start_kbps=0), dict(min_kbps=10.0), dict(start_kbps=2.0), dict(start_kbps=9.5),
               dict(high_q8=256), dict(high_q8=0), dict(low_q8=-1), dict(low_q8=26), dict(low_q8=30), dict(high_q8=5), dict(high_q8=26.0),
               dict(increase_q8=-1), dict(increase_q8=65536), dict(increase_q8=True), dict(burst_hops=0), dict(burst_hops=1 << 30),
               dict(timeout_hops=-1), dict(timeout_hops=1.5)):
        with pytest.raises(ValueError):
            RateConfig(**{**dict(min_kbps=2.625, max_kbps=9.0), **kw})


def test_bucket_converts_and_checks_the_floor_and_the_int32_bounds():
    b = rate.bucket(LOOP_RATE, 1, 0, True)
    assert b == (10, 35, 120, 120, 24) and b.min_bits == 35 and b.start_bits == 120
    assert rate.bucket(RateConfig(2.625, 9.0, 6.0), 3, 0, False) == (30, 105, 360, 240, 0)
    # floor(Fraction(kbps) 1000 T 320 / 24000), as vbr.bucket_bits
    assert rate.bucket(RateConfig(2.69, 9.05), 1)[1:4] == (35, 120, 120) == (vbr.bucket_bits(vbr.VbrConfig(6.0, cap_kbps=2.69), 1)[1],) + (120, 120)
    # the floor: 8 TRANSPORT_HEADER header + 10 T (max(m, 1) + m)
    assert [rate.floor_bits(T, m, h) for T, m, h in ((1, 0, False), (1, 0, True), (1, 2, True), (3, 2, False))] == [10, 34, 64, 120]
    rate.bucket(RateConfig(0.75, 9.0), 1, 0, False)                                  # 10 bits pay for one stage
    rate.bucket(RateConfig(4.875, 9.0), 1, 2, True)                                    # 65 bits >= 64: header, 2 + 2 stages
    for cfg, T, m, h in ((RateConfig(0.74, 9.0), 1, 0, False), (RateConfig(2.5, 9.0), 1, 0, True), (RateConfig(4.75, 9.0), 1, 2, True),
                         (RateConfig(3.5, 24.0), 3, 2, True)):
        with pytest.raises(ValueError, match="floor"):
            rate.bucket(cfg, T, m, h)
    # max_bits burst_hops <= vbr.MAX_BURST_BITS, max_bits <= MAX_RATE_BITS
    top = rate.MAX_RATE_BITS * 24000 / 320 / 1000                                    # kbps of 2^22 bits per hop
    rate.bucket(RateConfig(3.0, top), 1)
    for cfg in (RateConfig(3.0, top + 1), RateConfig(3.0, top, burst_hops=257), RateConfig(3.0, 9.0, burst_hops=(1 << 30) // 120 + 1)):
        with pytest.raises(ValueError, match="bits per hop"):
            rate.bucket(cfg, 1)
    assert rate.MAX_RATE_BITS * 8 < vbr.MAX_BURST_BITS and rate.MAX_RATE_BITS * 512 <= 1 << 31
    for bad in (dict(frames=0), dict(fec_stages=-1)):
        with pytest.raises(ValueError):
            rate.bucket(LOOP_RATE, **{**dict(frames=1, fec_stages=0), **bad})
    with pytest.raises(ValueError):
        rate.bucket(vbr.VbrConfig(6.0), 1)
    with pytest.raises(ValueError):
        RateModel(1, LOOP_RATE, 33)


def test_kbps_is_the_inverse():
    m = RateModel(3, RateConfig(2.625, 9.0, 6.0), N, 1, 0, True)
    assert rate.kbps(m.state[0], 1) == 6.0 and rate.kbps(m.state, 1).tolist() == [6.0, 6.0, 6.0]
    assert rate.kbps(torch.from_numpy(RateModel(1, LOOP_RATE, N, 3, 0, True).state), 3).tolist() == [9.0]


# ---------------------------------------------------------------- RateModel on scripted hops
def model(B=1, m=0, T=1, header=True, **kw):
    return RateModel(B, RateConfig(**{**dict(min_kbps=4.875, max_kbps=9.0), **kw}), N, T, m, header)     # 65 .. 120 bits


def row(m, b=0):
    return {k: int(m.state[b, getattr(rate, "RC_" + k.upper())]) for k in ("rate_q8", "credit", "seen", "last", "age", "loss") + rate.RC_NAMES}


def test_model_fresh_rows_and_a_hop_without_reports():
    m = model(2)
    assert m.state[:, rate.RC_RATE_Q8].tolist() == [120 * 256] * 2 and m.state[:, rate.RC_CREDIT].tolist() == [960] * 2
    assert not m.state[:, rate.RC_SEEN:].any()
    # full bucket: n_ceil = n; the hop's 13 bytes are charged; the next fill is capped at burst_hops rate
    assert m.ceiling().tolist() == [N, N] and row(m)["credit"] == 960 and row(m)["age"] == 1 and row(m)["limited"] == 0
    m.charge([13, 0])
    assert m.state[:, rate.RC_CREDIT].tolist() == [856, 960]
    assert m.ceiling().tolist() == [N, N] and m.state[:, rate.RC_CREDIT].tolist() == [960, 960]


def test_model_report_branches_stale_and_wrap():
    m = model()
    # high loss: rate (512 - loss) >> 9, a 64-bit product; loss is loss_q8, the residual is ignored
    m.ceiling([report_word(1, 128, 0)])
    assert row(m)["rate_q8"] == (120 * 256 * 384) >> 9 == 23040 and row(m)["decreased"] == 1 and row(m)["loss"] == 128
    assert (row(m)["seen"], row(m)["last"], row(m)["age"], row(m)["reports"]) == (1, 1, 1, 1)
    m.ceiling([report_word(2, 26, 255)])                        # exactly high_q8
    assert row(m)["rate_q8"] == (23040 * 486) >> 9 == 21870 and row(m)["decreased"] == 2
    # in between: kept
    for seq, loss in ((3, 25), (4, 6)):
        m.ceiling([report_word(seq, loss, 0)])
        assert row(m)["rate_q8"] == 21870 and row(m)["loss"] == loss
    assert (row(m)["reports"], row(m)["decreased"], row(m)["increased"]) == (4, 2, 0)
    # low loss: rate + max(256, rate increase_q8 >> 8)
    m.ceiling([report_word(5, 5, 200)])
    assert row(m)["rate_q8"] == 21870 + ((21870 * 13) >> 8) == 22980 and row(m)["increased"] == 1
    # stale: the same seq, an older one, d = 128; none of them touches anything but the counter (and the hop's age)
    before = row(m)
    for seq in (5, 4, 5 + 128, 5 - 127 + 256):
        m.ceiling([report_word(seq & 255, 255, 0)])
    after = row(m)
    assert after["stale"] == 4 and after["age"] == before["age"] + 4 and after["last"] == 5
    assert {k: v for k, v in after.items() if k not in ("stale", "age", "credit")} == {k: v for k, v in before.items() if k not in ("stale", "age", "credit")}
    # d = 127 is the farthest accepted; then across the wrap: last = 132 -> 250 -> 3 (d = 9)
    m.ceiling([report_word(132, 10, 0)])
    assert row(m)["last"] == 132 and row(m)["age"] == 1
    m.ceiling([report_word(250, 10, 0)])
    m.ceiling([report_word(3, 10, 0)])
    assert row(m)["last"] == 3 and row(m)["reports"] == 8 and row(m)["stale"] == 4
    m.ceiling([report_word(250, 10, 0)])                        # d = 247: stale
    assert row(m)["last"] == 3 and row(m)["stale"] == 5


def test_model_saturates_at_min_and_max():
    m = model(increase_q8=0)
    for k in range(1, 12):
        m.ceiling([report_word(k, 255, 0)])
    assert row(m)["rate_q8"] == 65 * 256 and row(m)["decreased"] == 11
    m.ceiling([report_word(12, 0, 0)])
    assert row(m)["rate_q8"] == 65 * 256 + 256                 # never less than one bit per hop
    m = model(increase_q8=65535)
    m.ceiling([report_word(1, 200, 0)])
    m.ceiling([report_word(2, 0, 0)])
    assert row(m)["rate_q8"] == 120 * 256 and row(m)["increased"] == 1
    m.ceiling([report_word(3, 0, 0)])
    assert row(m)["rate_q8"] == 120 * 256 and row(m)["increased"] == 2
    # the 64-bit product: the largest rate the rows hold
    big = RateModel(1, RateConfig(3.0, rate.MAX_RATE_BITS * 0.075, increase_q8=65535), N, 1, 0, False)
    top = big.bits.max_bits
    assert rate.MAX_RATE_BITS - 1 <= top <= rate.MAX_RATE_BITS
    big.ceiling([report_word(1, 26, 0)])
    assert big.state[0, rate.RC_RATE_Q8] == ((top << 8) * 486) >> 9 > 1 << 29
    big.ceiling([report_word(2, 0, 0)])
    assert big.state[0, rate.RC_RATE_Q8] == top << 8 and big.state[0, rate.RC_CREDIT] == 8 * top


def test_model_timeout():
    m = model(start_kbps=6.0, timeout_hops=3)
    m.ceiling([report_word(9, 255, 0)])
    assert row(m)["rate_q8"] == max(65 * 256, (80 * 256 * 257) >> 9) and row(m)["age"] == 1 and row(m)["seen"] == 1
    m.ceiling()
    assert row(m)["age"] == 2 and row(m)["timeout"] == 0
    m.ceiling()                                                 # AGE reaches 3: back to start, the sequence number is forgotten
    assert row(m)["rate_q8"] == 80 * 256 and (row(m)["seen"], row(m)["age"], row(m)["timeout"], row(m)["last"]) == (0, 0, 1, 9)
    m.ceiling([report_word(9, 0, 0)])                           # with SEEN = 0 any seq is accepted
    assert row(m)["reports"] == 2 and row(m)["increased"] == 1 and row(m)["stale"] == 0
    never = model(timeout_hops=0)
    for _ in range(50):
        never.ceiling()
    assert row(never)["age"] == 50 and row(never)["timeout"] == 0


def test_model_held_slots_keep_credit_and_age_but_take_reports():
    m = model(2)
    m.ceiling()
    m.charge([13, 13])
    before = row(m, 1)
    out = m.ceiling([0, report_word(1, 128, 0)], hold=[0, 1], n_slot=[N, 5])
    assert out.tolist() == [N, 5]                               # a held slot reports its own n
    after = row(m, 1)
    assert after["credit"] == before["credit"] == 856 and after["age"] == 0 and after["limited"] == 0
    assert after["rate_q8"] == 23040 and after["reports"] == 1 and after["decreased"] == 1 and after["seen"] == 1
    out = m.ceiling(hold=[0, 1])
    assert row(m, 1)["age"] == 0 and row(m, 1)["credit"] == 856 and row(m, 0)["age"] == 3
    # released: it ages and fills at the new rate (burst_hops 90 = 720 caps the 856)
    m.ceiling()
    assert row(m, 1)["age"] == 1 and row(m, 1)["credit"] == 720
    # a held slot's answered NACKs are still charged
    m.ceiling(hold=[0, 1])
    m.charge([13, 0], [[0, 0], [13, 10]])
    assert row(m, 1)["credit"] == 720 - 8 * 23 and row(m, 0)["credit"] == 960 - 104


def test_model_action_resets_rate_credit_memory_and_counters():
    m = model(2, start_kbps=6.0, timeout_hops=40)
    for k in range(1, 4):
        m.ceiling([report_word(k, 255, 0)] * 2)
        m.charge([13, 13])
    m.ceiling([report_word(3, 0, 0)] * 2)
    assert row(m)["stale"] == 1 and row(m)["decreased"] == 3 and row(m)["rate_q8"] < 80 * 256
    keep = row(m, 1)
    out = m.ceiling([report_word(7, 0, 0), 0], action=[-1, 0])
    # cleared first (counters too), then the hop's report is taken by the fresh row
    assert row(m) == dict(rate_q8=80 * 256 + ((80 * 256 * 13) >> 8), credit=8 * 84, seen=1, last=7, age=1, loss=0, reports=1, stale=0,
                          decreased=0, increased=1, timeout=0, limited=0) and out[0] == N
    assert {k: v for k, v in row(m, 1).items() if k not in ("age", "credit")} == {k: v for k, v in keep.items() if k not in ("age", "credit")}
    # a held slot with an action: reset, and the refilled credit stays as it is
    m.charge([13, 13])
    m.ceiling(action=[0, 3], hold=[0, 1])
    assert row(m, 1) == dict(rate_q8=80 * 256, credit=640, seen=0, last=0, age=0, loss=0, reports=0, stale=0, decreased=0, increased=0,
                             timeout=0, limited=0)


def test_model_debt_floor_and_the_ceiling_under_debt():
    m = model()
    for k in range(1, 12):
        m.ceiling([report_word(k, 255, 0)])                    # down to 65 bits per hop
    m.state[0, rate.RC_CREDIT] = 30
    m.charge([13], [[40, 40]])                                  # 744 bits: the debt stops at -burst_hops (rate >> 8)
    assert row(m)["credit"] == -8 * 65
    limited = row(m)["limited"]
    assert m.ceiling().tolist() == [1] and row(m)["credit"] == -520 + 65 and row(m)["limited"] == limited + 1      # max(0, credit - overhead)
    m.charge([5])
    assert row(m)["credit"] == -455 - 40
    for _ in range(7):
        assert m.ceiling().tolist() == [1]
    assert row(m)["credit"] == -495 + 7 * 65 == -40
    assert m.ceiling().tolist() == [1] and row(m)["credit"] == 25               # 25 - 24 pays for no stage: still the floor
    assert m.ceiling().tolist() == [6] and row(m)["credit"] == 90               # (90 - 24) // 10
    # the credit never exceeds burst_hops (rate >> 8), at the new, lower rate at once
    m = model()
    m.ceiling([report_word(1, 255, 0)])
    assert row(m)["credit"] == 8 * (row(m)["rate_q8"] >> 8) < 960


def test_model_overhead_with_and_without_a_live_redundant_section():
    for header, hdr in ((True, 24), (False, 0)):
        m = model(4, m=2, T=3, header=header, min_kbps=11.0, max_kbps=24.0)   # 146 bits >= 24 + 30 (2 + 2)
        prev = np.zeros((4, 1 + 2 * 3), dtype=np.int32)
        prev[0, 0], prev[1, 0], prev[3, 0] = 1, 0, 1
        m.state[:, rate.RC_CREDIT] = 200 - (m.state[:, rate.RC_RATE_Q8] >> 8)
        out = m.ceiling(prev=prev, action=[0, 0, 0, 1])
        # slot 0: live section; 1: switched off (word 0 is 0); 3: an action on this hop sends no section and refills the bucket
        assert out.tolist()[:3] == [(200 - hdr - 60) // 30, (200 - hdr) // 30, (200 - hdr) // 30] and out[3] == N
        # the words 0 alone do as well, and None means no live section
        m.state[:, rate.RC_CREDIT] = 200 - (m.state[:, rate.RC_RATE_Q8] >> 8)
        assert m.ceiling(prev=prev[:, 0]).tolist()[:2] == out.tolist()[:2]
        m.state[:, rate.RC_CREDIT] = 200 - (m.state[:, rate.RC_RATE_Q8] >> 8)
        assert m.ceiling().tolist()[:2] == [(200 - hdr) // 30] * 2
        # the floor: min(n_slot, max(m, 1)) stages even when the credit pays for fewer; the ceiling: n_slot
        m.state[:, rate.RC_CREDIT] = -100 - 960
        assert m.ceiling(prev=prev, n_slot=[8, 1, 3, 0]).tolist() == [2, 1, 2, 1]
        m.state[:, rate.RC_CREDIT] = 900
        assert m.ceiling(prev=prev, n_slot=[8, 1, 3, 99]).tolist() == [8, 1, 3, 8]
    plain = model(1, m=0)
    plain.state[0, rate.RC_CREDIT] = -500
    assert plain.ceiling().tolist() == [1]


# ---------------------------------------------------------------- custom ops and the library's checks
def test_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hilcodec_amd import ops
    with FakeTensorMode():
        B = 5
        ints = dict(dtype=torch.int32, device="cuda")
        rows, n_ceil, nbytes = torch.zeros(B, rate.RC_WORDS, **ints), torch.zeros(B, **ints), torch.zeros(B, **ints)
        assert ops.rate_ceiling(rows, n_ceil, N, 1, 2, True, RateConfig(4.875, 9.0), torch.zeros(B, **ints), None, None, None,
                                torch.zeros(B, 3, **ints)) is None
        assert ops.rate_charge(nbytes, rows, LOOP_RATE, torch.zeros(B, 2, **ints)) is None
        assert ops.rate_charge(nbytes, rows, LOOP_RATE) is None
    # the wrapper checks the configuration against the sender before anything is dispatched
    with pytest.raises(ValueError, match="floor"):
        ops.rate_ceiling(None, None, N, 1, 2, True, LOOP_RATE)
    assert torch.ops.hilcodec.rate_ceiling.default._schema.is_mutable and torch.ops.hilcodec.rate_charge.default._schema.is_mutable


def test_library_argument_checks():
    """null pointers and bad shapes are refused before any launch (no GPU is touched: every call returns from its checks)"""
    from hilcodec_amd._lib import lib
    OK_NULL, OK_SHAPE = -2, -1
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=4, T=1, n_max=8, m=0, header=1, min_bits=35, max_bits=120, start_bits=120, high_q8=26, low_q8=5, increase_q8=13,
                burst_hops=8, timeout_hops=0)

    def ceiling(rows=p, n_ceil=p, **kw):
        a = {**good, **kw}
        return lib.hilc_rate_ceiling(None, None, None, None, None, rows, n_ceil, *[a[k] for k in good], None)

    assert ceiling(rows=None) == OK_NULL and ceiling(n_ceil=None) == OK_NULL
    for kw in (dict(B=0), dict(T=0), dict(n_max=0), dict(n_max=33), dict(m=-1), dict(m=9), dict(low_q8=-1), dict(low_q8=26), dict(high_q8=256),
               dict(increase_q8=-1), dict(increase_q8=65536), dict(burst_hops=0), dict(timeout_hops=-1), dict(min_bits=33),
               dict(header=0, min_bits=9, start_bits=9), dict(m=2, min_bits=63), dict(T=3, min_bits=53), dict(start_bits=34),
               dict(start_bits=121), dict(max_bits=(1 << 22) + 1, start_bits=120), dict(max_bits=1 << 22, burst_hops=257),
               dict(min_bits=121), dict(n_max=32, T=1 << 20)):
        assert ceiling(**kw) == OK_SHAPE, kw

    def charge(nbytes=p, rtx=p, rows=p, B=4, per_hop=2, burst_hops=8):
        return lib.hilc_rate_charge(nbytes, rtx, rows, B, per_hop, burst_hops, None)

    assert charge(nbytes=None) == OK_NULL and charge(rows=None) == OK_NULL and charge(rtx=None) == OK_NULL
    for kw in (dict(B=0), dict(per_hop=-1), dict(per_hop=5), dict(burst_hops=0)):
        assert charge(**kw) == OK_SHAPE, kw


# ---------------------------------------------------------------- the closed loop on the models
@pytest.fixture(scope="module")
def loops():
    """each loop once: {(caps, control): (trace, model, rows, n_ceil)}"""
    runs = {}
    for caps in (60, 80, 200, ((0, 60), (1000, 200))):
        for control in (True, False):
            if control or isinstance(caps, int):
                runs[caps, control] = run_models(list(caps) if isinstance(caps, tuple) else caps, control=control)
    return runs


@pytest.mark.parametrize("cap", [60, 80])
def test_closed_loop_halves_the_loss_at_a_bottleneck(loops, cap):
    tr, rm, rows, _ = loops[cap, True]
    tr0 = loops[cap, False][0]
    loss, loss0, bits = tr.loss(2000, 3000), tr0.loss(2000, 3000), tr.mean_bits(2000, 3000)
    print(f"bottleneck {cap}: loss {loss0:.3f} -> {loss:.3f}, {bits:.1f} bits per hop sent; rate row {rm.state[0].tolist()}")
    assert tr0.mean_bits(2000, 3000) == FULL_BITS and abs(loss0 - (1 - cap / FULL_BITS)) < 0.01       # the sender without control
    assert loss <= 0.5 * loss0
    assert bits <= 1.1 * cap
    assert rm.state[0, rate.RC_DECREASED] > 0 and rm.state[0, rate.RC_STALE] == 0 and rm.state[0, rate.RC_REPORTS] >= 3000 // 16 - 2
    # every bit sent went through the bucket: the debt never reaches its floor here, so each hop is charged in full, and over the
    # window what was sent is what the rate paid (less the fills lost at the cap of the bucket) minus what the credit gained
    paid = int((rows[2000:3000, 0, rate.RC_RATE_Q8] >> 8).sum())
    assert int(tr.bits[2000:3000, 0].sum()) <= paid + int(rows[1999, 0, rate.RC_CREDIT]) - int(rows[2999, 0, rate.RC_CREDIT])
    assert (rows[:, 0, rate.RC_CREDIT] > -8 * (rows[:, 0, rate.RC_RATE_Q8] >> 8)).all()


def test_closed_loop_leaves_a_wide_link_alone(loops):
    tr, rm, rows, ceil = loops[200, True]
    assert rm.state[0, rate.RC_DECREASED] == 0 and (ceil == N).all() and (tr.n == N).all() and not tr.dropped.any()
    assert rm.state[0, rate.RC_LIMITED] == 0 and rm.state[0, rate.RC_RATE_Q8] == 120 * 256


def test_closed_loop_recovers_after_the_bottleneck_widens(loops):
    tr, rm, rows, ceil = loops[((0, 60), (1000, 200)), True]
    assert tr.loss(0, 1000) > 0 and (tr.n[:1000] < N).any()
    assert (tr.n[2500:] == N).all() and (ceil[2500:] == N).all() and not tr.dropped[2500:].any()
