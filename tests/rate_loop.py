"""What the CPU and the GPU tests of rate control share: a drop-tail bottleneck link, the delay line that carries receiver reports
back to the sender, and the closed loop on the models alone.  A plain module, imported as `from tests.rate_loop import ...`."""
import numpy as np

from hilcodec_amd import rate, report, wire
from hilcodec_amd.jitter import JitterConfig, JitterModel
from hilcodec_amd.rate import RateConfig, RateModel
from hilcodec_amd.report import ReportConfig, ReportModel
from tests.hops import arrival_arrays

N, T = 8, 1                                                  # stages and frames of the loop's sender; its packets carry the header
LOOP_RATE = RateConfig(min_kbps=2.625, max_kbps=9.0)         # binary-exact: 35 and 120 bits per hop
LOOP_REPORT = ReportConfig(window=64, interval=16)
LOOP_JITTER = JitterConfig(depth=4, capacity=8)              # the link's delay varies by at most 3 hops: nothing arrives late
REPORT_DELAY = 4
FULL_BITS = 8 * wire.transport_bytes(N, 0, T)                # 104: what a sender without rate control sends per hop


class Link:
    """one slot's drop-tail bottleneck, store and forward: each hop first drains `cap` bits of what is queued (a packet is delivered on
    the hop its last bit drains; what a hop does not use of its `cap` is gone), then takes the hop's packet behind them, unless that
    would queue more than 4 cap bits: a packet that does not fit is dropped.  A packet is therefore 1 to 4 hops under way."""

    def __init__(self, cap):
        self.cap, self.queue, self.backlog = int(cap), [], 0
        self.sent = self.dropped = 0

    def hop(self, packet):
        """drain, then offer this hop's packet (bytes; b"": nothing sent): -> (dropped, [packets delivered on this hop])"""
        budget, out = self.cap, []
        while self.queue and budget > 0:
            take = min(budget, self.queue[0][1])
            self.queue[0][1] -= take
            self.backlog -= take
            budget -= take
            if self.queue[0][1] == 0:
                out.append(self.queue.pop(0)[0])
        dropped = False
        bits = 8 * len(packet)
        if bits:
            self.sent += 1
            if self.backlog + bits > 4 * self.cap:
                dropped = True
                self.dropped += 1
            else:
                self.queue.append([packet, bits])
                self.backlog += bits
        return dropped, out


class ReportLine:
    """a report emitted on iteration t reaches the sender's step t + REPORT_DELAY"""

    def __init__(self, delay=REPORT_DELAY):
        self.delay, self.line = int(delay), {}

    def push(self, t, reports):
        """reports: [(slot, 3-byte blob)] emitted by the receiver on iteration t"""
        if reports:
            self.line[t + self.delay] = list(reports)

    def reports_for(self, t):
        slots_blobs = self.line.pop(t, [])
        return [s for s, _ in slots_blobs], [b for _, b in slots_blobs]


def cap_at(caps, t):
    """caps: an int, or [(first hop, cap)] ascending -> the bottleneck at hop t"""
    if isinstance(caps, int):
        return caps
    return [c for t0, c in caps if t0 <= t][-1]


class Trace:
    """per hop and slot of a closed loop: n sent, bits sent, dropped by the link"""

    def __init__(self, hops, B):
        self.n = np.zeros((hops, B), dtype=np.int64)
        self.bits = np.zeros((hops, B), dtype=np.int64)
        self.dropped = np.zeros((hops, B), dtype=bool)

    def loss(self, lo, hi, b=0):
        """the packets of hops [lo, hi) the link dropped, as a fraction of those sent"""
        return float(self.dropped[lo:hi, b].sum()) / max(1, int((self.bits[lo:hi, b] > 0).sum()))

    def mean_bits(self, lo, hi, b=0):
        return float(self.bits[lo:hi, b].mean())


def run_models(caps, hops=3000, control=True, cfg=LOOP_RATE, B=1, seed=3):
    """the closed loop on the models alone: a stand-in sender of headed packets (N stages at most, one frame, random bodies) whose n
    is a RateModel's n_ceil (control=False: always N), one Link per slot, a JitterModel with a ReportModel, reports back through a
    ReportLine.  Returns (Trace, RateModel, per hop the rate rows after the charge [hops, B, RC_WORDS], per hop n_ceil [hops, B])"""
    rng = np.random.default_rng(seed)
    tb = wire.transport_bytes(N, 0, T)
    rm = RateModel(B, cfg, N, T, 0, True)
    jm = JitterModel(B, LOOP_JITTER, N, 0, T, None, conceal=True)
    pm = ReportModel(B, LOOP_REPORT)
    links = [Link(cap_at(caps, 0)) for _ in range(B)]
    line = ReportLine()
    trace = Trace(hops, B)
    rows = np.zeros((hops, B, rate.RC_WORDS), dtype=np.int32)
    ceil = np.zeros((hops, B), dtype=np.int32)
    zeros = np.zeros(B, dtype=np.int32)
    for t in range(hops):
        words = np.zeros(B, dtype=np.int64)
        for s, blob in zip(*line.reports_for(t)):
            words[s] = report.report_word(*wire.parse_report(blob))
        n_ceil = rm.ceiling(words)
        ceil[t] = n_ceil
        n_sent = n_ceil if control else np.full(B, N)
        sent = [wire.pack_transport(t, rng.integers(0, 256, size=wire.packet_bytes(int(n_sent[b]), T), dtype=np.uint8).tobytes(),
                                    int(n_sent[b])) for b in range(B)]
        rm.charge([len(p) for p in sent])
        rows[t] = rm.state
        arrived = []
        for b in range(B):
            links[b].cap = cap_at(caps, t)
            dropped, out = links[b].hop(sent[b])
            trace.n[t, b], trace.bits[t, b], trace.dropped[t, b] = n_sent[b], 8 * len(sent[b]), dropped
            arrived += [(b, p) for p in out]
        jm.step(zeros, zeros, *arrival_arrays(arrived, tb))
        o = pm.step(jm.state, zeros)
        line.push(t, [(b, o["reports"][b].tobytes()) for b in range(B) if o["due"][b]])
    return trace, rm, rows, ceil
