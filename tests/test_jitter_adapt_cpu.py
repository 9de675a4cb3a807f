"""CPU: adaptive playout of the jitter buffer — the hilc_jitter_adapt_step entry point (additive under ABI 16) and its argument checks,
its custom op and fake kernel, AdaptConfig / JitterConfig(adapt=), and the rules (jitter.JitterModel with cfg.adapt): off means off, a
healthy stream is left alone, the drift / restart / burst traces the fixed buffer fails on, and hand-built traces for each rule.
(No kernel is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd import jitter, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel
from tests.hops import assert_entry_points

NAME = "hilc_jitter_adapt_step"
T = 1


# ---------------------------------------------------------------- the entry point, the op, the configs
def test_adapt_symbol_exported_and_declared():
    from hilcodec_amd import _lib
    assert_entry_points([NAME], in_abi16_line=True)
    assert _lib.SIGNATURES[NAME][:20] == _lib.SIGNATURES["hilc_jitter_step"][:20]
    assert jitter.ST_WORDS == 14 and jitter.AD_WORDS == 12 and len(jitter.STAT_NAMES) == 9


def test_adapt_step_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_jitter_adapt_step
    # (arrivals, offsets, max_arrivals, action, hold, n, lost, fec, packets, state, meta, ring, B, T, n_max, m, order, conceal, D, C,
    #  adapt, headroom, max_late, window, resync, force_windows, stream)
    head = lambda *a: [a[0], a[1], 8, None, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]]
    ok = [p, p, p, p, None, None, p, p, p, p]
    good = (p, 1, 6, 50, 4, 4, None)
    assert f(*head(*ok), 4, 1, 8, 0, -1, 0, 2, 8, None, 1, 6, 50, 4, 4, None) == -2            # adapt
    for bad in ((-1, 6, 50, 4, 4), (7, 6, 50, 4, 4), (1, 0, 50, 4, 4), (1, 7, 50, 4, 4), (1, 6, 0, 4, 4), (1, 6, 50, 1, 4),
                (1, 6, 50, 4, -1)):
        assert f(*head(*ok), 4, 1, 8, 0, -1, 0, 2, 8, p, *bad, None) == -5, bad
    assert f(*head(*ok), 4, 1, 8, 0, -1, 0, 0, 2, p, 0, 1, 50, 4, 4, None) == -5                # capacity 2 leaves no max_late
    assert f(*head(*ok), 4, 1, 8, 0, -1, 0, 1, 4, p, 3, 2, 50, 4, 4, None) == -5                # headroom > C - 2
    # the checks of hilc_jitter_step
    for k in range(10):
        if k in (4, 5):
            continue
        args = list(ok)
        args[k] = None
        assert f(*head(*args), 4, 1, 8, 0, -1, 0, 2, 8, *good) == -2, k
    assert f(*head(*ok), 4, 1, 8, 0, -1, 1, 2, 8, *good) == -2          # conceal without lost
    assert f(*head(*ok), 4, 1, 8, 2, -1, 0, 2, 8, *good) == -2          # FEC without fec
    args = head(*ok)
    args[2] = -1
    assert f(*args, 4, 1, 8, 0, -1, 0, 2, 8, *good) == -1
    assert f(*head(*ok), 0, 1, 8, 0, -1, 0, 2, 8, *good) == -1
    assert f(*head(*ok), 4, 0, 8, 0, -1, 0, 2, 8, *good) == -1
    assert f(*head(*ok), 4, 1, 0, 0, -1, 0, 2, 8, *good) == -5
    assert f(*head(*ok), 4, 1, 8, 0, 17, 0, 2, 8, *good) == -5          # order
    assert f(*head(*ok), 4, 1, 8, 0, -2, 0, 2, 8, *good) == -5
    for D, C in ((2, 6), (0, 1), (0, 64), (7, 8), (-1, 8)):
        assert f(*head(*ok), 4, 1, 8, 0, -1, 0, D, C, p, 0, 1, 50, 4, 4, None) == -5, (D, C)
    assert f(*head(*ok), 4, 1, 32, 0, -1, 0, 2, 8, *good) == -4
    assert f(*head(*ok), 4, 1, 1, 0, 8, 0, 2, 8, *good) == -1           # a SID of 9 bytes in a 2-byte row


def test_adapt_op_registered_with_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hilcodec_amd.ops  # noqa: F401  (registers the ops)
    assert hasattr(torch.ops.hilcodec, "jitter_adapt_step")
    sch = str(torch.ops.hilcodec.jitter_adapt_step.default._schema)
    for part in ("Tensor(a!) hold", "Tensor(e!) packets", "Tensor(f!) state", "Tensor(g!) meta", "Tensor(h!) ring", "Tensor(i!) adapt"):
        assert part in sch, part
    B, n, m = 5, 8, 2
    stride = wire.packet_bytes(n + m, T)
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        out = torch.ops.hilcodec.jitter_adapt_step(i32(10, 1 + (3 + stride + 3) // 4), i32(B + 1), None, i32(B), i32(B), None, i32(B),
                                                   torch.empty(B, stride, dtype=torch.uint8), i32(B, 14), i32(B, 8),
                                                   i32(B, 8, (stride + 3) // 4), i32(B, 12), n, m, T, -1, 2, 1, 6, 50, 4, 4)
        assert out is None


def test_adapt_config():
    a = AdaptConfig()
    assert (a.headroom, a.max_late, a.window, a.resync, a.force_windows) == (1, None, 50, 4, 4)
    AdaptConfig(headroom=0, max_late=1, window=1, resync=2, force_windows=0)
    for kw in (dict(headroom=-1), dict(max_late=0), dict(window=0), dict(resync=1), dict(force_windows=-1), dict(headroom=True),
               dict(window=2.0), dict(resync="4"), dict(max_late=1.5), dict(force_windows=False), dict(headroom=None)):
        with pytest.raises(ValueError):
            AdaptConfig(**kw)
    with pytest.raises(Exception):
        a.window = 3                                            # frozen
    c = JitterConfig()
    assert (c.depth, c.capacity, c.adapt) == (2, 8, None)
    c = JitterConfig(2, 8, adapt=a)
    assert c.adapt is a and a.max_late_for(8) == 6 and AdaptConfig(max_late=3).max_late_for(8) == 3
    JitterConfig(2, 4, adapt=AdaptConfig(headroom=2, max_late=2))
    JitterConfig(0, 32, adapt=AdaptConfig(headroom=30, max_late=30))
    for C, kw in ((8, dict(headroom=7)), (8, dict(max_late=7)), (4, dict(headroom=3)), (4, dict(max_late=3)), (2, dict(headroom=0))):
        with pytest.raises(ValueError):
            JitterConfig(0, C, adapt=AdaptConfig(**kw))
    for bad in ((1, 6), "adapt", True, 1):
        with pytest.raises(ValueError):
            JitterConfig(2, 8, adapt=bad)


# ---------------------------------------------------------------- traffic
def codes(h, n=8, fec=False, m=2):
    """a headed codes packet whose body starts with h mod 256 (to tell played packets apart)"""
    body = bytearray(wire.fec_packet_bytes(n, m, T) if fec else wire.packet_bytes(n, T))
    body[0], body[1] = h & 0xFF, 0x5A
    return wire.pack_transport(h & 0xFFFF, bytes(body), n, fec=fec)


def sid(h, K=8):
    body = bytearray(1 + K)
    body[0] = h & 0x7F
    return wire.pack_transport(h & 0xFFFF, bytes(body), 0, sid=True)


def rows_of(pkts, tbytes):
    arr = np.zeros((len(pkts), tbytes), dtype=np.uint8)
    for a, p in enumerate(pkts):
        arr[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return arr, [len(p) for p in pkts]


def seeded_traffic(B, hops, seed, D, m=2, K=8, healthy=False):
    """[(action, hold, slots, packets, nbytes)] per hop.  Loss, reordering, duplicates, SIDs and DTX silence, restarts of sender and
    receiver together; not `healthy`: delays up to D + 3 and host holds too.  `healthy`: no delay exceeds D, a copy travels with
    its original and a stream's first packet is neither lost nor delayed — nothing is ever late or early."""
    rng = np.random.default_rng(seed)
    tb = wire.transport_bytes(8, m, T)
    h = rng.integers(0, 65536, B)
    first, quiet = np.ones(B, dtype=bool), np.zeros(B, dtype=int)
    flight, out = [], []
    for k in range(hops):
        action = (rng.random(B) < 0.01).astype(np.int32) if k else np.ones(B, dtype=np.int32)
        hold = np.zeros(B, dtype=np.int32) if healthy else (rng.random(B) < 0.03).astype(np.int32)
        for b in np.nonzero(action)[0]:
            h[b], first[b], quiet[b] = 0, True, 0
            flight = [f for f in flight if f[1] != b]
        for b in range(B):
            if hold[b]:
                continue
            hb = int(h[b])
            h[b] = (hb + 1) & 0xFFFF
            if quiet[b] == 0 and not first[b] and rng.random() < 0.05:
                quiet[b] = int(rng.integers(3, 12))
            if quiet[b]:
                quiet[b] -= 1
                if quiet[b] % 4 != 2:
                    continue                                 # silent: nothing sent
                p = sid(hb)
            else:
                fec = bool(rng.random() < 0.7)
                p = codes(hb, n=int(rng.integers(m, 9)), fec=fec, m=m)
            if not first[b] and rng.random() < 0.06:
                continue
            due = k + (0 if first[b] else int(rng.integers(0, D + (1 if healthy else 4))))
            first[b] = False
            for _ in range(2 if rng.random() < 0.03 else 1):
                flight.append((due if healthy else k + int(rng.integers(0, D + 4)), b, p))
        now = [f for f in flight if f[0] <= k]
        flight = [f for f in flight if f[0] > k]
        now = [now[i] for i in rng.permutation(len(now))]
        arr, nb = rows_of([f[2] for f in now], tb)
        out.append((action, hold, [f[1] for f in now], arr, nb))
    return out


def same_hop(a, b, ra, rb, k):
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), (key, k)
    assert np.array_equal(a.state, b.state) and np.array_equal(a.meta, b.meta) and np.array_equal(a.body, b.body), k


def test_off_means_off():
    B, D, C = 12, 2, 8
    today = JitterModel(B, JitterConfig(D, C), 8, 2, T, 8, True)
    off = JitterModel(B, JitterConfig(depth=D, capacity=C, adapt=None), 8, 2, T, 8, True)
    assert not hasattr(off, "adapt")
    for k, hop in enumerate(seeded_traffic(B, 300, 3, D)):
        same_hop(today, off, today.step(*hop), off.step(*hop), k)
    st = today.state
    for name in ("duplicate", "late", "fec", "lost", "noise"):
        assert st[:, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index(name)].sum() > 0, name


@pytest.mark.parametrize("D,C,conceal", [(2, 8, True), (1, 4, False), (5, 16, True)])
def test_adaptation_leaves_a_healthy_stream_alone(D, C, conceal):
    B, hops = 12, 300
    fixed = JitterModel(B, JitterConfig(D, C), 8, 2, T, 8, conceal)
    adaptive = JitterModel(B, JitterConfig(D, C, adapt=AdaptConfig(window=10 * hops)), 8, 2, T, 8, conceal)
    for k, hop in enumerate(seeded_traffic(B, hops, 5, D, healthy=True)):
        same_hop(fixed, adaptive, fixed.step(*hop), adaptive.step(*hop), k)
        assert not adaptive.adapt[:, jitter.AD_GROWN:].any() and not adaptive.adapt[:, jitter.AD_DEBT].any(), k
    st = fixed.state
    assert st[:, jitter.STAT_LATE].sum() == 0 and st[:, jitter.STAT_EARLY].sum() == 0
    for name in ("duplicate", "fec", "lost", "noise"):
        assert st[:, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index(name)].sum() > 0, name


# ---------------------------------------------------------------- the four traces (depth 2, capacity 8, one slot)
def run_schedule(cfg, schedule):
    """one slot; schedule[k] = the hop indices of the packets that arrive on hop k"""
    model = JitterModel(1, cfg, 8, 0, T, 8, True)
    for k, hs in enumerate(schedule):
        arr, nb = rows_of([codes(h) for h in hs], model.tbytes)
        model.step([int(k == 0)], [0], [0] * len(hs), arr, nb)
    return model


def stat(model, name):
    if name in jitter.AD_NAMES:
        return int(model.adapt[0, jitter.AD_GROWN + jitter.AD_NAMES.index(name)])
    return int(model.state[0, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index(name)])


def drifting(hops, every, per_tick, h0=0):
    """the sender emits `per_tick` packets (0: a slow clock, 2: a fast one) on every `every`-th receiver hop, else one"""
    out, h = [], h0
    for k in range(hops):
        c = per_tick if k % every == every - 1 else 1
        out.append([h + i for i in range(c)])
        h += c
    return out


def delayed(hops, delay_of, h0=0):
    """packet h0 + k is sent on hop k and arrives delay_of(k) hops later; the trace ends with the sender"""
    out = [[] for _ in range(hops + 8)]
    for k in range(hops):
        out[k + delay_of(k)].append(h0 + k)
    return out[:hops]


FIXED, ADAPTIVE = JitterConfig(2, 8), JitterConfig(2, 8, adapt=AdaptConfig())


def test_trace_slow_sender():
    sched = drifting(2000, 100, 0)
    fixed, ad = run_schedule(FIXED, sched), run_schedule(ADAPTIVE, sched)
    assert stat(fixed, "late") >= 1500                       # once late, late for ever
    assert stat(ad, "late") + stat(ad, "lost") <= 20 and stat(ad, "forced") == 0
    assert stat(ad, "decoded") >= 1980 - 20 - 3 and stat(ad, "grown") >= 17 and stat(ad, "shrunk") == 0


def test_trace_fast_sender():
    sched = drifting(2000, 100, 2)
    fixed, ad = run_schedule(FIXED, sched), run_schedule(ADAPTIVE, sched)
    assert stat(fixed, "early") >= 1000
    assert stat(ad, "early") + stat(ad, "lost") <= 20
    assert stat(ad, "shrunk") >= 17 and stat(ad, "grown") == 0


def test_trace_sender_restart():
    sched = [[k if k < 500 else k - 500] for k in range(1000)]
    fixed, ad = run_schedule(FIXED, sched), run_schedule(ADAPTIVE, sched)
    assert stat(fixed, "late") == 500 and stat(fixed, "decoded") == 500
    assert stat(ad, "resync") == 1 and stat(ad, "late") <= ADAPTIVE.adapt.resync
    assert stat(ad, "decoded") >= 1000 - ADAPTIVE.adapt.resync - 8


def test_trace_jitter_burst():
    rng = np.random.default_rng(1)
    sched = delayed(1400, lambda k: int(rng.integers(0, 5)) if 400 <= k < 1000 else 0)
    fixed, ad = run_schedule(FIXED, sched), run_schedule(ADAPTIVE, sched)
    assert stat(fixed, "late") >= 150
    assert stat(ad, "late") <= 10 and stat(ad, "grown") >= 1 and stat(ad, "shrunk") >= 1 and stat(ad, "resync") == 0


@pytest.mark.parametrize("h0,hops", [(65300, 1000), (0, 5000)])
def test_trace_steady_jitter_is_left_alone(h0, hops):
    """0..3 hops of jitter at depth 4: the smallest margin of every window is the headroom of 1, so nothing is wanted"""
    rng = np.random.default_rng(2)
    sched = delayed(hops, lambda k: int(rng.integers(0, 4)) if k else 0, h0)
    ad = run_schedule(JitterConfig(4, 8, adapt=AdaptConfig()), sched)
    assert [stat(ad, name) for name in jitter.AD_NAMES] == [0, 0, 0, 0]
    assert stat(ad, "late") == 0 and stat(ad, "lost") == 0 and stat(ad, "decoded") >= hops - 5


# ---------------------------------------------------------------- each rule on a hand-built trace
class Trace:
    """one slot of an adaptive JitterModel, driven hop by hop; `hop()` returns that hop's decision: 'H' held, ('P', b0) played (b0 =
    the packet row's first byte), ('S', b0) SID, 'Q' silent, 'L' lost (concealed), ('F', b0) FEC"""

    def __init__(self, D=0, C=8, m=0, K=8, conceal=True, **adapt):
        self.model = JitterModel(1, JitterConfig(D, C, adapt=AdaptConfig(**adapt)), 8, m, T, K, conceal)

    def hop(self, pkts=(), hold=0, start=0):
        arr, nb = rows_of(list(pkts), self.model.tbytes)
        rows = self.rows = self.model.step([start], [hold], [0] * len(nb), arr, nb)
        hv, b0 = rows["hold"][0], int(rows["packets"][0][0])
        if hv == 1:
            assert not rows["packets"][0].any()
            return "H"
        if hv == 2:
            return ("S", b0)
        if hv == 3:
            return "Q"
        if rows["lost"][0]:
            return "L"
        return ("F", b0) if rows["fec"][0] else ("P", b0)

    def ad(self, word):
        return int(self.model.adapt[0, word])

    def st(self, word):
        return int(self.model.state[0, word])


def test_rule_grow_waits_for_a_free_hop():
    t = Trace(D=0, window=4, force_windows=2)
    assert [t.hop([codes(h)]) for h in range(4)] == [("P", h) for h in range(4)]
    assert (t.ad(jitter.AD_PENDING), t.ad(jitter.AD_MARGIN), t.ad(jitter.AD_STALE)) == (1, 0, 0)      # want = headroom 1 - margin 0
    assert t.hop([codes(4)]) == ("P", 4) and t.ad(jitter.AD_GROWN) == 0                              # speech: it waits
    assert t.hop() == "L"                                                                            # packet 5 is missing: free
    assert (t.ad(jitter.AD_GROWN), t.ad(jitter.AD_FORCED), t.ad(jitter.AD_PENDING)) == (1, 0, 0)
    assert t.st(jitter.ST_NEXT) == 5 and t.st(jitter.STAT_LOST) == 0                                 # inserted: the clock stands
    assert t.hop([codes(6)]) == "L" and t.st(jitter.STAT_LOST) == 1                                  # now 5 is played: lost
    assert t.hop([codes(7)]) == ("P", 6) and t.ad(jitter.AD_MIN) == 1                                # one hop of margin from here


def test_rule_grow_is_forced_after_force_windows():
    t = Trace(D=0, window=4, force_windows=2)
    out = [t.hop([codes(h)]) for h in range(12)]
    assert out == [("P", h) for h in range(12)]
    assert (t.ad(jitter.AD_PENDING), t.ad(jitter.AD_STALE), t.ad(jitter.AD_GROWN)) == (1, 2, 0)
    assert t.hop([codes(12)]) == "L"                         # packet 12 is there, and the hop is padded all the same
    assert (t.ad(jitter.AD_GROWN), t.ad(jitter.AD_FORCED), t.ad(jitter.AD_PENDING), t.ad(jitter.AD_STALE)) == (1, 1, 0, 0)
    assert t.st(jitter.ST_NEXT) == 12 and t.st(jitter.STAT_LOST) == 0
    assert [t.hop([codes(h)]) for h in range(13, 21)] == [("P", h - 1) for h in range(13, 21)]
    assert (t.ad(jitter.AD_MARGIN), t.ad(jitter.AD_PENDING), t.ad(jitter.AD_GROWN)) == (1, 0, 1)     # at the headroom: it rests
    # force_windows = 0: never forced
    t = Trace(D=0, window=4, force_windows=0)
    assert [t.hop([codes(h)]) for h in range(40)] == [("P", h) for h in range(40)]
    assert t.ad(jitter.AD_PENDING) == 1 and t.ad(jitter.AD_GROWN) == 0 and t.ad(jitter.AD_STALE) == 9


def test_rule_shrink_discards_a_present_entry():
    # through the windowed estimate: depth 3 against a headroom of 1 is two hops too deep
    t = Trace(D=3, window=4, force_windows=1)
    out = [t.hop([codes(h)]) for h in range(11)]
    assert out == ["H"] * 3 + [("P", h) for h in range(8)]
    assert (t.ad(jitter.AD_PENDING), t.ad(jitter.AD_STALE)) == (-2, 1)
    assert t.hop([codes(11)]) == ("P", 9)                    # entry 8 is skipped
    assert (t.ad(jitter.AD_SHRUNK), t.ad(jitter.AD_FORCED), t.ad(jitter.AD_PENDING)) == (1, 1, -1)
    assert t.st(jitter.ST_NEXT) == 10 and t.st(jitter.STAT_DECODED) == 9 and t.st(jitter.ST_MASK) == 0b1100
    assert t.model.meta[0, 0] == 0
    # through an early arrival: one past the window is an urgent debt of one hop
    t = Trace(D=0)
    assert [t.hop([codes(h)]) for h in range(4)] == [("P", h) for h in range(4)]
    assert t.hop([codes(4), codes(12)]) == "L"               # 12: d = 8 = C, early by 1; entry 4 is skipped, 5 is not there
    assert (t.st(jitter.STAT_EARLY), t.ad(jitter.AD_SHRUNK), t.ad(jitter.AD_DEBT)) == (1, 1, 0)
    assert t.st(jitter.ST_NEXT) == 6 and t.st(jitter.ST_MASK) == 0 and not t.model.meta[0].any()
    assert t.st(jitter.STAT_DECODED) == 4 and t.st(jitter.STAT_LOST) == 1


@pytest.mark.parametrize("conceal,dtx_on,want", [(True, False, "L"), (False, False, "H"), (True, True, "Q"), (False, True, "Q")])
def test_rule_inserted_hop_row(conceal, dtx_on, want):
    t = Trace(D=0, conceal=conceal)
    t.hop([codes(0)])
    assert t.hop([sid(1)] if dtx_on else [codes(1)]) == (("S", 1) if dtx_on else ("P", 1))
    gap = t.hop()                                            # 2 is missing
    before = t.model.state[0].copy()
    assert t.hop([codes(2)]) == want                         # 2 comes one hop late: a debt of 1, paid at once
    assert (t.ad(jitter.AD_GROWN), t.ad(jitter.AD_DEBT), t.st(jitter.ST_NEXT)) == (1, 0, 3)
    assert t.rows["n"][0] == 8 and not t.rows["packets"][0].any() and t.rows["fec"][0] == 0
    assert t.rows["lost"][0] == int(want == "L") and t.rows["hold"][0] == {"L": 0, "H": 1, "Q": 3}[want]
    after = t.model.state[0].copy()
    after[jitter.STAT_LATE] -= 1
    assert np.array_equal(before, after)                     # no STAT_* counter moves but the late arrival's
    assert gap == ("Q" if dtx_on else "L" if conceal else "H")
    assert t.hop([codes(3), codes(4)]) == ("P", 3) and t.hop([codes(5)]) == ("P", 4)


def test_rule_debt_beyond_max_late_is_ignored():
    for late, debt in ((2, 2), (3, 0)):
        t = Trace(D=0, max_late=2)
        for h in range(6):
            t.hop([codes(h)])
        t.hop([codes(6 - late)], hold=1)                     # a copy of a played packet; held, so that the debt can be read
        assert (t.st(jitter.STAT_LATE), t.ad(jitter.AD_DEBT)) == (1, debt)
    for early, debt in ((2, -2), (3, 0)):
        t = Trace(D=0, max_late=2)
        for h in range(6):
            t.hop([codes(h)])
        t.hop([codes(6 + 7 + early)], hold=1)                # the window is [6, 14)
        assert (t.st(jitter.STAT_EARLY), t.ad(jitter.AD_DEBT)) == (1, debt)
    # the larger debt stays
    t = Trace(D=0)
    for h in range(6):
        t.hop([codes(h)])
    t.hop([codes(3), codes(5), codes(4)], hold=1)
    assert t.ad(jitter.AD_DEBT) == 3 and t.ad(jitter.AD_RUN) == 3
    # no debt while priming
    t = Trace(D=2)
    t.hop([codes(10)])
    t.hop([codes(9)])
    assert t.st(jitter.STAT_LATE) == 1 and t.ad(jitter.AD_DEBT) == 0


def test_rule_resync_needs_a_run_of_outliers():
    t = Trace(D=1, resync=3)
    for h in range(6):
        t.hop([codes(h)])
    assert t.st(jitter.ST_NEXT) == 5
    t.hop([codes(1000)])
    t.hop([codes(1001)])
    assert (t.ad(jitter.AD_RUN), t.ad(jitter.AD_LAST), t.st(jitter.STAT_EARLY)) == (2, 1001, 2)
    t.hop([codes(8)])                                        # a good packet ends the run
    assert t.ad(jitter.AD_RUN) == 0
    t.hop([codes(1002)])
    t.hop([codes(1003), codes(9), codes(9)])                 # so does a duplicate
    assert t.ad(jitter.AD_RUN) == 0 and t.ad(jitter.AD_RESYNC) == 0 and t.st(jitter.ST_ANCHORED) == 1
    t.hop([codes(1004), b"\0\1"])                            # a malformed packet does not
    assert t.ad(jitter.AD_RUN) == 1 and t.st(jitter.STAT_MALFORMED) == 1
    t.hop([codes(1005)])
    accepted = t.st(jitter.STAT_ACCEPTED)
    assert t.hop([codes(1006)]) == "H"                       # the third in a row: the slot anchors on it and primes again
    assert (t.ad(jitter.AD_RESYNC), t.ad(jitter.AD_RUN), t.ad(jitter.AD_MIN), t.ad(jitter.AD_MARGIN)) == (1, 0, 8, 1)
    assert (t.st(jitter.ST_NEXT), t.st(jitter.ST_WAIT), t.st(jitter.ST_MASK)) == (1006, 0, 1 << (1006 & 7))
    assert t.st(jitter.STAT_ACCEPTED) == accepted + 1 and t.st(jitter.STAT_EARLY) == 7
    assert [t.hop([codes(1007)]), t.hop([codes(1008)])] == [("P", 1006 & 0xFF), ("P", 1007 & 0xFF)]


def test_rule_resync_needs_outliers_that_agree():
    t = Trace(D=0, resync=3)
    for h in range(4):
        t.hop([codes(h)])
    for h in (1000, 1020, 1040, 1060, 1052, 1059):           # 8 = C apart is too far, 7 is not
        t.hop([codes(h)])
    assert (t.ad(jitter.AD_RUN), t.ad(jitter.AD_RESYNC)) == (2, 0)
    t.hop([codes(1055)])
    assert t.ad(jitter.AD_RESYNC) == 1 and t.st(jitter.ST_NEXT) == 1056


def test_rule_wrap():
    # the slow sender across the 16-bit wrap: the same counters as from 0
    at0 = run_schedule(ADAPTIVE, drifting(600, 50, 0))
    wrap = run_schedule(ADAPTIVE, drifting(600, 50, 0, h0=65300))
    assert wrap.state[0, jitter.ST_NEXT] == (at0.state[0, jitter.ST_NEXT] + 65300) & 0xFFFF
    assert np.array_equal(wrap.state[0, jitter.STAT_ACCEPTED:], at0.state[0, jitter.STAT_ACCEPTED:])
    assert np.array_equal(np.delete(wrap.adapt[0], jitter.AD_LAST), np.delete(at0.adapt[0], jitter.AD_LAST))
    # the first D + 1 skips are absorbed by the depth; a window as long as the gap between two skips follows them through the urgent
    # debt, so a skip costs at most one late packet and one lost hop
    assert stat(wrap, "grown") >= 600 // 50 - 3 and stat(wrap, "late") <= 600 // 50 and stat(wrap, "lost") <= 600 // 50
    # a late debt, an early debt and a run of outliers whose h straddle the wrap
    t = Trace(D=0, resync=3)
    for h in range(65530, 65536):
        t.hop([codes(h)])
    t.hop([codes(65534), codes(7)], hold=1)                  # next = 0: late by 2, then d = 7 is stored
    assert (t.st(jitter.STAT_LATE), t.ad(jitter.AD_DEBT), t.ad(jitter.AD_RUN), t.st(jitter.ST_MASK)) == (1, 2, 0, 1 << 7)
    t.hop([codes(9)], hold=1)                                # early by 2: the smaller debt wins
    assert (t.st(jitter.STAT_EARLY), t.ad(jitter.AD_DEBT), t.ad(jitter.AD_RUN)) == (1, -2, 1)
    t = Trace(D=0, resync=3)
    for h in range(100, 104):
        t.hop([codes(h)])
    t.hop([codes(65533), codes(65535), codes(2)])
    assert t.ad(jitter.AD_RESYNC) == 1 and t.st(jitter.ST_NEXT) == 3


def test_rule_start_clears_the_adapt_row():
    t = Trace(D=0)
    for h in range(6):
        t.hop([codes(h)])
    t.hop([codes(4)])
    assert t.ad(jitter.AD_GROWN) == 1
    t.hop(start=1)
    assert not t.model.adapt[0].any() and not t.model.state[0].any()
    t.hop([codes(50)])
    assert (t.ad(jitter.AD_MIN), t.ad(jitter.AD_MARGIN), t.ad(jitter.AD_GROWN)) == (8, 0, 0)


class Counting(JitterModel):
    """counts, per slot, the hops past priming that were not held"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.playing = np.zeros(self.B, dtype=np.int64)

    def _play(self, b, rows):
        st = self.state[b]
        self.playing[b] += int(rows["hold"][b] == 0 and st[jitter.ST_ANCHORED] != 0 and st[jitter.ST_WAIT] == 0)
        super()._play(b, rows)


@pytest.mark.parametrize("conceal", [True, False])
def test_played_hops_identity(conceal):
    B, D = 12, 2
    model = Counting(B, JitterConfig(D, 8, adapt=AdaptConfig(window=8, resync=3, force_windows=2)), 8, 2, T, 8, conceal)
    for action, hold, slots, arr, nb in seeded_traffic(B, 400, 7, D):
        model.playing[action != 0] = 0
        model.step(action, hold, slots, arr, nb)
        st = model.state
        played = st[:, jitter.STAT_DECODED] + st[:, jitter.STAT_FEC] + st[:, jitter.STAT_LOST] + st[:, jitter.STAT_NOISE]
        assert np.array_equal(played + model.adapt[:, jitter.AD_GROWN], model.playing)
    assert model.adapt[:, jitter.AD_GROWN].sum() > 0 and model.adapt[:, jitter.AD_SHRUNK].sum() > 0
