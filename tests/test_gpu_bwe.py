"""GPU: the delay-based bandwidth estimate of the graphed hops (GraphedDecodeHop(bwe=BweConfig(...)), GraphedEncodeHop(cap=CapConfig(...))).
hilc_rx_bwe against bwe.BweModel on scripted arrival traces that reach every branch; hilc_rate_cap in front of hilc_rate_ceiling against
bwe.CapModel and rate.RateModel; the receiver with `bwe` against the receiver without; the sender with `cap` and no caps against the
sender with `rate` alone, and with scripted caps against the models; the closed loop of tests/bwe_loop.py with the real sender and
receiver — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import bwe, dtx, rate, rtx, synth, wire
from hilcodec_amd.bwe import BweConfig, BweModel, CapConfig, CapModel, cap_word
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.rate import RateConfig, RateModel
from hilcodec_amd.report import ReportConfig, report_word
from tests.bwe_loop import LOOP_BWE, LOOP_CAP, TimedLink, run_models
from tests.hops import Network, arrival_arrays, arrival_records, caches_equal
from tests.rate_loop import LOOP_JITTER, LOOP_RATE, LOOP_REPORT, ReportLine, Trace

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
N = 8
B_KERNEL = 70                                                # a last workgroup with idle waves


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def dev_times(slots, times, max_a):
    """the arrival ticks as play() stages them: mod 2^32 as int32, in the records' slot-grouped (stable) order, padded to max_a"""
    out = np.zeros(max_a, dtype=np.int32)
    order = np.argsort(np.asarray(slots, dtype=np.int64), kind="stable")
    out[:len(order)] = np.array([int(t) & 0xFFFFFFFF for t in times], dtype=np.uint32).view(np.int32)[order] if len(order) else 0
    return torch.from_numpy(out).to(DEV)


# ---------------------------------------------------------------- hilc_rx_bwe against BweModel
class ArrivalScript:
    """seeded arrivals of B slots for hilc_rx_bwe, 0 - 3 per slot and hop: packets in hop order whose queueing delay stays, grows and
    drains in stretches of 20 hops (shifted per slot), hop steps of 1 - 3, duplicates and older hop indices, malformed records, SIDs,
    gaps above reset_ticks, time running backwards; the first slots start just below the wrap of the tick (2^32) and of the hop index
    (2^16).  A script, not a network: several packets of a slot may arrive on one hop."""

    def __init__(self, B, n, m, K, T, seed, reset_ticks):
        self.B, self.n, self.m, self.K, self.T, self.reset_ticks = B, n, m, K, T, reset_ticks
        self.rng = r = np.random.default_rng(seed)
        self.tbytes = wire.transport_bytes(n, m, T)
        self.h = r.integers(0, 65536, B).astype(np.int64)
        self.h[:8] = 65536 - r.integers(1, 30, 8)
        self.base = [int(v) for v in r.integers(0, 1 << 32, B)]          # the send time of the slot's last packet, ticks
        for b in range(4, 12):
            self.base[b] = (1 << 32) - int(r.integers(1, 20000))
        self.extra = np.zeros(B, dtype=np.int64)                         # the slot's queueing delay, ticks
        self.last_t = list(self.base)

    def _codes(self, h):
        r = self.rng
        nb = int(r.integers(max(self.m, 1), self.n + 1))
        fec = self.m >= 1 and r.random() < 0.6
        body = r.integers(0, 256, wire.packet_bytes(nb + (self.m if fec else 0), self.T)).astype(np.uint8).tobytes()
        return wire.pack_transport(h, body, nb, fec=fec)

    def hop(self, k):
        """-> (slots, packets uint8 [A, tbytes], nbytes, times) of hop k, in push order"""
        r, T = self.rng, self.T
        out = []
        for b in range(self.B):
            phase = ((k + 7 * b) % 60) // 20                             # 0 steady, 1 growing, 2 draining
            for _ in range(int(r.choice([0, 1, 1, 1, 2, 3]))):
                u = r.random()
                if u < 0.07:                                             # a duplicate or an older hop index, at any time
                    h = (int(self.h[b]) - int(r.integers(0, 6))) & 0xFFFF
                    out.append((b, self._codes(h), None, self.last_t[b] + int(r.integers(-500, 500))))
                    continue
                if u < 0.11:                                             # malformed: the reserved bit, a short count, a cut body
                    p, how = bytearray(self._codes(int(self.h[b]) + 1)), int(r.integers(0, 3))
                    nb = len(p) - (how == 1) if how else len(p)
                    if how == 0:
                        p[2] |= 0x20
                    out.append((b, bytes(p), 2 if how == 2 else nb, self.last_t[b] + 5))
                    continue
                dh = int(r.choice([1, 1, 1, 2, 3]))
                self.h[b] = (self.h[b] + dh) & 0xFFFF
                self.base[b] += bwe.HOP_TICKS * T * dh
                if u < 0.14:                                             # a gap above reset_ticks
                    self.base[b] += self.reset_ticks + int(r.integers(1, 1000))
                if phase == 1:
                    self.extra[b] += T * int(r.integers(40, 120))
                elif phase == 2:
                    self.extra[b] = max(0, self.extra[b] - T * int(r.integers(40, 100)))
                t = self.base[b] + int(self.extra[b]) + int(r.integers(0, 20))
                if 0.14 <= u < 0.16:                                     # time runs backwards
                    t = self.last_t[b] - int(r.integers(1, 1000))
                    self.base[b] = t
                    self.extra[b] = 0
                self.last_t[b] = t
                sid = self.K is not None and 0.16 <= u < 0.20
                p = wire.pack_transport(int(self.h[b]), bytes(dtx.sid_bytes(self.K)), 0, sid=True) if sid else self._codes(int(self.h[b]))
                out.append((b, p, None, t))
        # the slots interleaved at random, each slot's own order kept: the records are grouped by slot again on the way to the kernel
        queues = {}
        for e in out:
            queues.setdefault(e[0], []).append(e)
        out = [queues[out[i][0]].pop(0) for i in r.permutation(len(out))]
        packets = np.zeros((len(out), self.tbytes), dtype=np.uint8)
        for a, e in enumerate(out):
            packets[a, :len(e[1])] = np.frombuffer(e[1], dtype=np.uint8)
        return [e[0] for e in out], packets, [len(e[1]) if e[2] is None else e[2] for e in out], [e[3] for e in out]


KERNEL_BWE = dict(window=8, rate_window=6, interval=5)


def kernel_cfg(T):
    return BweConfig(2.625, 9.0, reset_ticks=4000 * T, **KERNEL_BWE)


@pytest.mark.parametrize("T,m", [(1, 0), (3, 0), (1, 2), (3, 2)])
def test_rx_bwe_kernel(T, m):
    from hilcodec_amd import ops
    B, hops, K = B_KERNEL, 60, 5
    cfg = kernel_cfg(T)
    model = BweModel(B, cfg, N, m, T, K)
    script = ArrivalScript(B, N, m, K, T, 10 * T + m, cfg.reset_ticks)
    rng = np.random.default_rng(T + m)
    max_a = 3 * B
    rows = torch.from_numpy(model.state.copy()).to(DEV)
    caps = torch.zeros(B, wire.CAP_BYTES, dtype=torch.uint8, device=DEV)
    due = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    for k in range(hops):
        slots, packets, nbytes, times = script.hop(k)
        action = (rng.random(B) < 0.01).astype(np.int32) * rng.choice([-1, 1, 2], B).astype(np.int32)
        want = model.step(action, slots, packets, nbytes, times)
        rec, offs = arrival_records(slots, packets, nbytes, script.tbytes, B, max_a)
        ops.rx_bwe(rec, offs, dev_times(slots, times, max_a), rows, caps, due, cfg, N, T, m, K, dev(action))
        assert np.array_equal(rows.cpu().numpy(), model.state), k
        assert np.array_equal(caps.cpu().numpy(), want["caps"]) and np.array_equal(due.cpu().numpy(), want["due"]), k
    moved = {name: int(model.state[:, bwe.BW_SAMPLES + i].sum()) for i, name in enumerate(bwe.BW_NAMES)}
    assert all(v > 0 for v in moved.values()), moved                     # the trace reached every branch
    assert (model.state[:, bwe.BW_SIGNAL] == bwe.SIGNAL_UNDERUSE).any() or moved["underuse"] > 0
    # no action row, no arrivals: every slot's phase runs
    want = model.step(None, [], np.zeros((0, script.tbytes), dtype=np.uint8), [], [])
    rec, offs = arrival_records([], np.zeros((0, script.tbytes), dtype=np.uint8), [], script.tbytes, B, max_a)
    ops.rx_bwe(rec, offs, dev_times([], [], max_a), rows, caps, due, cfg, N, T, m, K)
    assert np.array_equal(rows.cpu().numpy(), model.state) and np.array_equal(due.cpu().numpy(), want["due"])


# ---------------------------------------------------------------- hilc_rate_cap and hilc_rate_ceiling against CapModel and RateModel
def test_rate_cap_kernel_in_front_of_the_ceiling():
    from hilcodec_amd import ops
    B, hops = B_KERNEL, 40
    rcfg, ccfg = RateConfig(4.875, 24.0, 9.0, timeout_hops=9, burst_hops=3), CapConfig(timeout_hops=6)
    rm = RateModel(B, rcfg, N, 1, 0, True)
    cm = CapModel(B, ccfg, rm.bits.min_bits, rm.bits.max_bits)                        # 65 .. 320 bits
    rng = np.random.default_rng(41)
    rows, cp = torch.from_numpy(rm.state.copy()).to(DEV), torch.from_numpy(cm.state.copy()).to(DEV)
    n_ceil = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    seq, rseq = rng.integers(0, 256, B), rng.integers(0, 256, B)
    for k in range(hops):
        words, reports = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        for b in np.nonzero(rng.random(B) < 0.3)[0]:
            how = rng.random()
            if how < 0.7:
                seq[b] = (seq[b] + int(rng.integers(1, 4))) & 255                # fresh
            elif how >= 0.85:
                seq[b] = (seq[b] - int(rng.integers(1, 100))) & 255              # older; in between: repeated
            words[b] = cap_word(int(seq[b]), int(rng.choice([0, 30, 64, 65, 66, 100, 200, 319, 320, 321, 5000, 65535])))
        for b in np.nonzero(rng.random(B) < 0.2)[0]:
            rseq[b] = (rseq[b] + 1) & 255
            reports[b] = report_word(int(rseq[b]), int(rng.choice([0, 3, 20, 26, 100])), 0)
        action = (rng.random(B) < 0.03).astype(np.int32) * rng.choice([-1, 1, 2], B).astype(np.int32)
        hold = (rng.random(B) < 0.2).astype(np.int32) * rng.choice([1, 2, 3], B).astype(np.int32)
        cm.step(rm.state, words, action, hold)
        ops.rate_cap(cp, rows, ccfg, rm.bits.min_bits, rm.bits.max_bits, dev(words), dev(action), dev(hold))
        assert np.array_equal(cp.cpu().numpy(), cm.state) and np.array_equal(rows.cpu().numpy(), rm.state), k
        want = rm.ceiling(reports, action, hold)
        ops.rate_ceiling(rows, n_ceil, N, 1, 0, True, rcfg, report=dev(reports), action=dev(action), hold=dev(hold))
        assert np.array_equal(rows.cpu().numpy(), rm.state) and np.array_equal(n_ceil.cpu().numpy(), want), k
        nbytes = np.where(hold != 0, 0, rng.integers(0, 14, B)).astype(np.int32)
        rm.charge(nbytes)
        ops.rate_charge(dev(nbytes), rows, rcfg)
    assert all(cm.state[:, bwe.CP_CAPS + i].sum() > 0 for i in range(len(bwe.CP_NAMES)))
    assert (cm.state[:, bwe.CP_CAP_Q8] == 65 * 256).any() and (cm.state[:, bwe.CP_CAP_Q8] == 320 * 256).any()
    # no cap, action or hold rows: every slot ages
    age = cm.state[:, bwe.CP_AGE].copy()
    cm.step(rm.state)
    ops.rate_cap(cp, rows, ccfg, rm.bits.min_bits, rm.bits.max_bits)
    assert np.array_equal(cp.cpu().numpy(), cm.state) and np.array_equal(rows.cpu().numpy(), rm.state) and (cm.state[:, bwe.CP_AGE] != age).any()


def test_kernels_refuse_bad_configs():
    """the library's error code reaches the caller and nothing is launched: the rows keep their sentinel"""
    z = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device=DEV)
    B, A = 2, 4
    tb = wire.transport_bytes(N, 0, 1)
    rows, due = z(B, bwe.BW_WORDS, v=-9), z(B, v=-9)
    caps = torch.full((B, 3), 7, dtype=torch.uint8, device=DEV)
    arrivals, offsets, times = z(A, 1 + (tb + 3) // 4), z(B + 1), z(A)
    good = dict(n=N, m=0, frames=1, order=-1, min_bits=35, max_bits=120, window=20, rate_window=16, alpha_q8=26, beta_q8=218,
                increase_q16=70, interval=8, reset_ticks=72000)
    for kw in (dict(min_bits=0), dict(min_bits=121), dict(max_bits=65536), dict(window=1), dict(window=33), dict(rate_window=3),
               dict(alpha_q8=0), dict(alpha_q8=257), dict(beta_q8=256), dict(increase_q16=65536), dict(interval=0), dict(reset_ticks=0),
               dict(reset_ticks=(1 << 17) + 1), dict(order=17)):
        with pytest.raises(RuntimeError, match=r"hilc_rx_bwe.*code -1"):
            torch.ops.hilcodec.rx_bwe(arrivals, offsets, times, None, rows, caps, due, *{**good, **kw}.values())
    for bad in (dict(arrivals=z(A, 3)), dict(offsets=z(B)), dict(times=z(A + 1)), dict(rows=z(B, bwe.BW_WORDS - 1)),
                dict(caps=torch.zeros(B, 4, dtype=torch.uint8, device=DEV)), dict(action=z(B + 1))):
        a = {**dict(arrivals=arrivals, offsets=offsets, times=times, action=None, rows=rows, caps=caps, due=due), **bad}
        with pytest.raises(RuntimeError):
            torch.ops.hilcodec.rx_bwe(*a.values(), *good.values())
    cp, rc = z(B, bwe.CP_WORDS, v=-9), z(B, rate.RC_WORDS, v=-9)
    for args in ((0, 120, 0), (121, 120, 0), (35, (1 << 22) + 1, 0), (35, 120, -1)):
        with pytest.raises(RuntimeError, match=r"hilc_rate_cap.*code -1"):
            torch.ops.hilcodec.rate_cap(None, None, None, cp, rc, *args)
    for bad in ((z(3), None, None, cp, rc), (None, None, None, z(B, bwe.CP_WORDS + 1), rc), (None, None, None, cp, z(B, 3))):
        with pytest.raises(RuntimeError):
            torch.ops.hilcodec.rate_cap(*bad, 35, 120, 0)
    torch.cuda.synchronize()
    assert bool((rows == -9).all()) and bool((due == -9).all()) and bool((caps == 7).all())
    assert bool((cp == -9).all()) and bool((rc == -9).all())


# ---------------------------------------------------------------- the receiver graph
def test_estimating_receiver_only_observes(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, n, m, K, hops = 4, 8, 2, 8, 40
    jc, cfg = JitterConfig(2, 8), BweConfig(2.625, 9.0, reset_ticks=3000, **KERNEL_BWE)
    kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=jc, report=ReportConfig(8, 4), nack=rtx.NackConfig())
    rx = GraphedDecodeHop(speech, B, 1, n, DEV, bwe=cfg, **kw)
    ref = GraphedDecodeHop(speech, B, 1, n, DEV, **kw)
    # without bwe= the stage is today's: no word for the times
    assert rx.stage.dev.numel() == ref.stage.dev.numel() + rx.max_arrivals and ref.stage.times is None
    bm = BweModel(B, cfg, n, m, 1, K)
    net = Network(B, n, m, K, 1, seed=6, loss=0.05, delay=0, dup=0.03, bad=0.03, sid=0.05, every=10, mild=False)
    rng = np.random.default_rng(8)
    queue = np.zeros(B, dtype=np.int64)
    for k in range(hops):
        slots, packets, nbytes, action, hold = net.hop()
        if k == 25:
            assert bm.state[1, bwe.BW_SAMPLES] > 0
            action[1] = 1                                    # a start in the middle clears that slot's row only
        for b in np.nonzero(action)[0]:
            rx.start(int(b))
            ref.start(int(b))
        queue = np.where((k // 10) % 2 == 0, queue + 60, np.maximum(0, queue - 80))   # the link's queue fills for 10 hops, then drains
        times = [(1 << 32) - 3000 + HOP * k + int(queue[s]) + int(rng.integers(0, 30)) for s in slots]      # the tick wraps on hop 9
        before = bm.state.copy()
        want = bm.step(action, slots, packets, nbytes, times)
        if k == 25:
            assert bm.state[1, bwe.BW_SAMPLES] <= 3 and (before[[0, 2, 3], bwe.BW_SAMPLES] <= bm.state[[0, 2, 3], bwe.BW_SAMPLES]).all()
            assert (bm.state[[0, 2, 3], bwe.BW_SAMPLES] > 3).all()
        a = rx.play(slots, torch.from_numpy(packets), nbytes, times=times).clone()
        b = ref.play(slots, torch.from_numpy(packets), nbytes).clone()
        assert torch.equal(a, b), k
        assert caches_equal(rx.cache_dec, ref.cache_dec), k
        for name in ("jitter_state", "concealed", "cng_state", "reports", "report_due", "report_state", "nacks", "nack_due", "nack_state"):
            assert torch.equal(getattr(rx, name), getattr(ref, name)), (name, k)
        assert np.array_equal(rx.bwe_state.cpu().numpy(), bm.state), k
        assert np.array_equal(rx.caps.cpu().numpy(), want["caps"]) and np.array_equal(rx.cap_due.cpu().numpy(), want["due"]), k
    assert (bm.state[:, bwe.BW_CAPS] > 0).all() and bm.state[:, bwe.BW_OVERUSE].sum() > 0 and bm.state[:, bwe.BW_OLD].sum() > 0
    assert bwe.kbps(rx.bwe_state, 1).shape == (B,)
    # times as a host tensor or an array, in another push order, are the same ticks
    slots, packets, nbytes, action, hold = net.hop()
    times = [HOP * hops + 7 * i for i in range(len(slots))]
    want = bm.step(None, slots, packets, nbytes, times)
    rx.play(slots, torch.from_numpy(packets), nbytes, times=torch.tensor(times, dtype=torch.int64))
    assert np.array_equal(rx.bwe_state.cpu().numpy(), bm.state) and np.array_equal(rx.cap_due.cpu().numpy(), want["due"])
    # a start of every slot with no arrival on that hop restores the cleared rows (the receiver's reset: it has no other); the
    # rows were allocated as cleared, which is what the fresh model holds
    fresh = BweModel(B, cfg, n, m, 1, K)
    rx.play(slots, torch.from_numpy(packets), nbytes, times=np.asarray(times) + HOP)
    assert rx.bwe_state[:, bwe.BW_SEEN].any() and rx.caps.any()
    for b in range(B):
        rx.start(b)
    rx.play([], torch.zeros(0, rx.tstride, dtype=torch.uint8), [])
    fresh.state[:, bwe.BW_PHASE] = 1
    assert np.array_equal(rx.bwe_state.cpu().numpy(), fresh.state) and not rx.caps.any() and not rx.cap_due.any()


# ---------------------------------------------------------------- the sender graph
def test_sender_with_cap_and_no_caps_is_the_sender_with_rate_alone(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 4, 14
    cfg = RateConfig(2.625, 9.0, burst_hops=2)
    kw = dict(sessions=True, header=True, rate=cfg)
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, cap=CapConfig(timeout_hops=5), **kw)
    ref = GraphedEncodeHop(speech, B, HOP, N, DEV, **kw)
    assert tx.stage.dev.numel() == ref.stage.dev.numel() + B and "cap" not in ref.stage.row       # one more one-hop row, appended
    x = synth.synth_clips(B, HOP * hops, seed=31).to(DEV)
    for k in range(hops):
        if k == 5:
            tx.start(2)
            ref.start(2)
        holds = [0] if k in (6, 7) else []
        reports = ([1, 3], [wire.pack_report(k, 128 if k < 8 else 0, 0)] * 2) if k % 3 == 1 else None
        xk = x[:, :, HOP * k:HOP * (k + 1)].contiguous()
        (pk, nb), (pk1, nb1) = tx.step(xk, hold=holds, reports=reports), ref.step(xk, hold=holds, reports=reports)
        assert torch.equal(pk, pk1) and torch.equal(nb, nb1) and torch.equal(tx.indices, ref.indices), k
        assert torch.equal(tx.rate_state, ref.rate_state) and torch.equal(tx.n_ceil, ref.n_ceil), k
        assert caches_equal(tx.cache_enc, ref.cache_enc), k
    st = tx.cap_state.cpu().numpy()
    assert not st[:, :bwe.CP_AGE].any() and not st[:, [bwe.CP_CAPS, bwe.CP_STALE, bwe.CP_CLAMPED]].any()
    assert (st[:, bwe.CP_TIMEOUT] >= 1).all()                                        # the row ran: it aged, with nothing to forget
    assert int(tx.rate_state[1, rate.RC_DECREASED]) > 0                              # the reports did move the rate, in both


def test_scripted_caps_against_the_models(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 4, 30
    rcfg, ccfg = RateConfig(2.625, 9.0, burst_hops=2), CapConfig(timeout_hops=7)
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, sessions=True, header=True, rate=rcfg, cap=ccfg)
    rm = RateModel(B, rcfg, N, 1, 0, True)
    cm = CapModel(B, ccfg, rm.bits.min_bits, rm.bits.max_bits)
    x = synth.synth_clips(B, HOP * hops, seed=37).to(DEV)
    script = {2: [(0, 2, 60), (1, 9, 20)], 3: [(0, 2, 100), (2, 250, 5000)], 4: [(0, 1, 40), (2, 3, 90), (2, 4, 70)], 9: [(1, 10, 50)],
              12: [(3, 0, 45)], 13: [(3, 130, 80)], 20: [(0, 5, 110), (3, 131, 64)]}
    seen = []
    for k in range(hops):
        caps = script.get(k, [])
        words, reports, action, hold = (np.zeros(B, dtype=np.int64) for _ in range(4))
        for s, seq, bits in caps:
            words[s] = cap_word(seq, bits)                   # a slot named twice keeps its last
        given = dict(caps=([s for s, _, _ in caps], [wire.pack_cap(seq, bits) for _, seq, bits in caps])) if caps else {}
        if k % 5 == 0:
            reports[:] = report_word(k, 0, 0)                # calm reports: the loss rule keeps probing upward
            given["reports"] = (list(range(B)), [wire.pack_report(k, 0, 0)] * B)
        if k == 15:
            tx.start(1)
            action[1] = -1
        if k in (10, 11, 12):
            hold[3] = 1                                      # a held slot takes its cap, and does not age
        cm.step(rm.state, words, action, hold)
        want = rm.ceiling(reports, action, hold)
        pk, nb = tx.step(x[:, :, HOP * k:HOP * (k + 1)].contiguous(), hold=np.nonzero(hold)[0].tolist(), **given)
        rm.charge(nb.cpu().numpy())
        assert np.array_equal(tx.cap_state.cpu().numpy(), cm.state), k
        assert np.array_equal(tx.rate_state.cpu().numpy(), rm.state) and np.array_equal(tx.n_ceil.cpu().numpy(), want), k
        for b in range(B):
            assert int(nb[b]) == (0 if hold[b] else wire.TRANSPORT_HEADER + wire.packet_bytes(int(want[b]), 1)), (k, b)
        seen.append(want.copy())
    assert all(cm.state[:, bwe.CP_CAPS + i].sum() > 0 for i in range(len(bwe.CP_NAMES)))
    assert min(s[0] for s in seen) <= 3 and min(s[1] for s in seen[:15]) <= 1 and seen[-1][1] == N
    tx.reset()
    assert not tx.cap_state.any()


# ---------------------------------------------------------------- end to end
def test_closed_loop_with_the_real_hops(speech):
    """GraphedEncodeHop(rate, cap, header, sessions) -> a timed bottleneck of 60 bits per hop -> GraphedDecodeHop(jitter, report, bwe) ->
    reports and caps back, 400 hops: what was sent and dropped, the rate rows, the ceilings, the estimate rows and the cap rows are the
    model loop's on every hop"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B, hops, cap = 2, 400, 60
    tx = GraphedEncodeHop(speech, B, HOP, N, DEV, sessions=True, header=True, rate=LOOP_RATE, cap=LOOP_CAP)
    rx = GraphedDecodeHop(speech, B, 1, N, DEV, sessions=True, jitter=LOOP_JITTER, report=LOOP_REPORT, conceal=True, bwe=LOOP_BWE)
    x = (torch.randn(B, 1, hops * HOP, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    links, line, cap_line, trace = [TimedLink(cap) for _ in range(B)], ReportLine(), ReportLine(), Trace(hops, B)
    want = run_models(cap, hops=hops, B=B)
    for t in range(hops):
        slots, blobs = line.reports_for(t)
        cslots, cblobs = cap_line.reports_for(t)
        pk, nb = tx.step(x[:, :, HOP * t:HOP * (t + 1)].contiguous(), reports=(slots, blobs) if slots else None,
                         caps=(cslots, cblobs) if cslots else None)
        pk, nb = pk.cpu().numpy(), nb.cpu().numpy()
        assert np.array_equal(tx.rate_state.cpu().numpy(), want.rate_rows[t]) and np.array_equal(tx.n_ceil.cpu().numpy(), want.ceil[t]), t
        assert np.array_equal(tx.cap_state.cpu().numpy(), want.cap_rows[t]), t
        arrived, ticks = [], []
        for b in range(B):
            sent = pk[b, :nb[b]].tobytes()
            dropped, got = links[b].hop(sent, t)
            trace.n[t, b], trace.bits[t, b], trace.dropped[t, b] = sent[2] & wire.N_MASK, 8 * len(sent), dropped
            arrived += [(b, p) for p, _ in got]
            ticks += [tick for _, tick in got]
        sl, packets, nbytes = arrival_arrays(arrived, rx.tstride)
        wav = rx.play(sl, torch.from_numpy(packets), nbytes, times=ticks)
        assert bool(torch.isfinite(wav).all()), t
        assert np.array_equal(rx.bwe_state.cpu().numpy(), want.bwe_rows[t]), t
        due, rep = rx.report_due.cpu().numpy(), rx.reports.cpu().numpy()
        line.push(t, [(b, rep[b].tobytes()) for b in range(B) if due[b]])
        due, caps = rx.cap_due.cpu().numpy(), rx.caps.cpu().numpy()
        cap_line.push(t, [(b, caps[b].tobytes()) for b in range(B) if due[b]])
    m = want.trace
    assert np.array_equal(trace.n, m.n) and np.array_equal(trace.bits, m.bits) and np.array_equal(trace.dropped, m.dropped)
    assert [l.delays for l in links] == [l.delays for l in want.links]
    assert want.bwe_rows[-1, :, bwe.BW_DECREASED].min() >= 1 and want.cap_rows[-1, :, bwe.CP_CLAMPED].min() >= 1


# ---------------------------------------------------------------- accessors and argument errors
def test_accessors_and_argument_errors(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    jc = JitterConfig(2, 8)
    plain = GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, jitter=jc)
    for name in ("caps", "cap_due", "bwe_state"):
        with pytest.raises(RuntimeError):
            getattr(plain, name)
    none = torch.zeros(0, plain.tstride, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        plain.play([], none, [], times=[])                   # without bwe=, times must be None
    rx = GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, jitter=jc, bwe=LOOP_BWE)
    assert rx.caps.shape == (2, 3) and rx.caps.dtype == torch.uint8 and rx.cap_due.shape == (2,) and rx.cap_due.dtype == torch.int32
    assert rx.bwe_state.shape == (2, bwe.BW_WORDS) and rx.bwe_state.is_cuda and bwe.kbps(rx.bwe_state, 1).tolist() == [9.0, 9.0]
    assert np.array_equal(rx.bwe_state.cpu().numpy(), BweModel(2, LOOP_BWE, N).state)       # allocated as cleared
    one = torch.zeros(1, rx.tstride, dtype=torch.uint8)
    p = wire.pack_transport(0, bytes(wire.packet_bytes(N, 1)), N)
    one[0, :len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8)
    for bad in (None, [], [1, 2], torch.zeros(1, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError):
            rx.play([0], one, [len(p)], times=bad)
    assert not rx.bwe_state[:, bwe.BW_PHASE].any()           # nothing was launched
    rx.play([], none, [])                                    # no arrivals: no times needed
    rx.play([0], one, [len(p)], times=[(1 << 40) + 5])       # any int: taken mod 2^32
    assert rx.bwe_state[0, bwe.BW_LAST_T] == 5 and rx.bwe_state[:, bwe.BW_SEEN].tolist() == [1, 0]
    x = torch.zeros(2, 1, HOP, device=DEV)
    rated = GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True, header=True, rate=LOOP_RATE)
    with pytest.raises(RuntimeError):
        rated.cap_state
    with pytest.raises(RuntimeError):
        rated.step(x, caps=([0], [b"\x01\x00\x40"]))
    tx = GraphedEncodeHop(speech, 2, HOP, N, DEV, sessions=True, header=True, rate=LOOP_RATE, cap=CapConfig())
    assert tx.cap_state.shape == (2, bwe.CP_WORDS) and tx.cap_state.dtype == torch.int32 and not tx.cap_state.any()
    for bad in (([2], [b"abc"]), ([0], [b"ab"]), ([0, 1], [b"abc"]), ([0], torch.zeros(1, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            tx.step(x, caps=bad)
    assert tx.cap_state[:, bwe.CP_AGE].tolist() == [0, 0]                            # nothing was launched
    # a slot named twice keeps its last cap; a cap applies to exactly one hop; a uint8 tensor does as well as bytes
    tx.step(x, caps=([1, 1], [wire.pack_cap(5, 40), wire.pack_cap(9, 50)]))
    st = tx.cap_state.cpu().numpy()
    assert st[1, bwe.CP_LAST] == 9 and st[1, bwe.CP_CAPS] == 1 and st[1, bwe.CP_CAP_Q8] == 50 * 256 and st[0, bwe.CP_SEEN] == 0
    tx.step(x, caps=([0], torch.tensor([[3, 0, 70]], dtype=torch.uint8)))
    st = tx.cap_state.cpu().numpy()
    assert st[1, bwe.CP_CAPS] == 1 and st[1, bwe.CP_STALE] == 0 and st[:, bwe.CP_AGE].tolist() == [1, 2] and st[0, bwe.CP_CAP_Q8] == 70 * 256
    assert tx.rate_state[:, rate.RC_RATE_Q8].tolist() == [70 * 256, 50 * 256]
