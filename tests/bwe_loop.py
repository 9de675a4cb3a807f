"""What the CPU and the GPU tests of the delay-based bandwidth estimate share: the drop-tail bottleneck of tests/rate_loop.py with every
delivery timed inside its hop, and the closed loop on the models alone, reports and caps returning through delay lines.  A plain
module, imported as `from tests.bwe_loop import ...`."""
import numpy as np

from hilcodec_amd import bwe, rate, report, wire
from hilcodec_amd.bwe import BweConfig, BweModel, CapConfig, CapModel
from hilcodec_amd.jitter import JitterModel
from hilcodec_amd.rate import RateModel
from hilcodec_amd.report import ReportModel
from tests.hops import arrival_arrays
from tests.rate_loop import LOOP_JITTER, LOOP_RATE, LOOP_REPORT, N, T, Link, ReportLine, Trace, cap_at

LOOP_BWE = BweConfig(min_kbps=2.625, max_kbps=9.0)           # the bounds of LOOP_RATE: 35 and 120 bits per hop
LOOP_CAP = CapConfig()
HOP_TICKS = bwe.HOP_TICKS * T


class TimedLink(Link):
    """tests.rate_loop.Link with every delivery timed: the packet whose last bit leaves after `used` of hop t's `cap` bits arrives at
    tick 320 t + used 320 // cap.  `delays`: per delivered packet (the hop it was sent on, arrival tick - 320 x that hop)."""

    def __init__(self, cap):
        super().__init__(cap)
        self.delays = []

    def hop(self, packet, t):
        """drain, then offer hop t's packet: -> (dropped, [(packet, arrival tick) delivered on this hop])"""
        budget, out = self.cap, []
        while self.queue and budget > 0:
            take = min(budget, self.queue[0][1])
            self.queue[0][1] -= take
            self.backlog -= take
            budget -= take
            if self.queue[0][1] == 0:
                p, _, sent_on = self.queue.pop(0)
                tick = HOP_TICKS * t + (self.cap - budget) * HOP_TICKS // self.cap
                out.append((p, tick))
                self.delays.append((sent_on, tick - HOP_TICKS * sent_on))
        dropped = False
        bits = 8 * len(packet)
        if bits:
            self.sent += 1
            if self.backlog + bits > 4 * self.cap:
                dropped = True
                self.dropped += 1
            else:
                self.queue.append([packet, bits, t])
                self.backlog += bits
        return dropped, out

    def delay_ticks(self, lo, hi):
        """the one-way delays (ticks) of the delivered packets that were sent on hops [lo, hi)"""
        return np.array([d for s, d in self.delays if lo <= s < hi], dtype=np.int64)


class Loop:
    """what a closed loop returns: the Trace, the links, the models, and per hop the rate rows after the charge, n_ceil, the estimate
    rows and the cap rows"""

    def __init__(self, hops, B):
        self.trace = Trace(hops, B)
        self.rate_rows = np.zeros((hops, B, rate.RC_WORDS), dtype=np.int32)
        self.ceil = np.zeros((hops, B), dtype=np.int32)
        self.bwe_rows = np.zeros((hops, B, bwe.BW_WORDS), dtype=np.int32)
        self.cap_rows = np.zeros((hops, B, bwe.CP_WORDS), dtype=np.int32)
        self.packets = []                                     # per hop, the packets as sent
        self.links = self.rm = self.bm = self.cm = None

    def mean_delay_ms(self, lo, hi, b=0):
        return float(self.links[b].delay_ticks(lo, hi).mean()) / 24.0

    def p95_delay_ms(self, lo, hi, b=0):
        return float(np.percentile(self.links[b].delay_ticks(lo, hi), 95)) / 24.0


def stand_in_packets(rng, t, n_sent):
    """the stand-in sender's headed packets of hop t: n_sent[b] stages of random bodies"""
    return [wire.pack_transport(t, rng.integers(0, 256, size=wire.packet_bytes(int(n), T), dtype=np.uint8).tobytes(), int(n)) for n in n_sent]


def feedback_words(line, t, B, word):
    """the one-hop row of hop t from a ReportLine: word(blob) per slot, 0 elsewhere"""
    words = np.zeros(B, dtype=np.int64)
    for s, blob in zip(*line.reports_for(t)):
        words[s] = word(blob)
    return words


def run_models(caps, hops=3000, estimate=True, cfg=LOOP_RATE, bwe_cfg=LOOP_BWE, B=1, seed=3):
    """the closed loop on the models alone: tests.rate_loop.run_models with timed links and, with `estimate`, a BweModel beside the
    receiver's ReportModel whose caps return through a ReportLine of their own to a CapModel in front of the sender's RateModel"""
    rng = np.random.default_rng(seed)
    tb = wire.transport_bytes(N, 0, T)
    rm = RateModel(B, cfg, N, T, 0, True)
    cm = CapModel(B, LOOP_CAP, rm.bits.min_bits, rm.bits.max_bits)
    jm = JitterModel(B, LOOP_JITTER, N, 0, T, None, conceal=True)
    pm = ReportModel(B, LOOP_REPORT)
    bm = BweModel(B, bwe_cfg, N, 0, T, None)
    out = Loop(hops, B)
    out.links, out.rm, out.bm, out.cm = [TimedLink(cap_at(caps, 0)) for _ in range(B)], rm, bm, cm
    line, cap_line = ReportLine(), ReportLine()
    zeros = np.zeros(B, dtype=np.int32)
    for t in range(hops):
        words = feedback_words(line, t, B, lambda blob: report.report_word(*wire.parse_report(blob)))
        cap_words = feedback_words(cap_line, t, B, lambda blob: bwe.cap_word(*wire.parse_cap(blob)))
        if estimate:
            cm.step(rm.state, cap_words)
        n_ceil = rm.ceiling(words)
        sent = stand_in_packets(rng, t, n_ceil)
        rm.charge([len(p) for p in sent])
        out.rate_rows[t], out.ceil[t], out.cap_rows[t] = rm.state, n_ceil, cm.state
        out.packets.append(sent)
        arrived, ticks = [], []
        for b in range(B):
            out.links[b].cap = cap_at(caps, t)
            dropped, got = out.links[b].hop(sent[b], t)
            out.trace.n[t, b], out.trace.bits[t, b], out.trace.dropped[t, b] = n_ceil[b], 8 * len(sent[b]), dropped
            arrived += [(b, p) for p, _ in got]
            ticks += [tick for _, tick in got]
        slots, packets, nbytes = arrival_arrays(arrived, tb)
        jm.step(zeros, zeros, slots, packets, nbytes)
        o = pm.step(jm.state, zeros)
        line.push(t, [(b, o["reports"][b].tobytes()) for b in range(B) if o["due"][b]])
        if estimate:
            e = bm.step(None, slots, packets, nbytes, ticks)
            cap_line.push(t, [(b, e["caps"][b].tobytes()) for b in range(B) if e["due"][b]])
        out.bwe_rows[t] = bm.state
    return out
