"""What the CPU and the GPU tests of NACK / retransmission share: the seeded loss patterns, the channel between a sender and a
receiver (first transmissions dropped by hop, NACKs delayed by rtt_hops, requests and retransmissions not lost unless a test says
so) and the closed loop on the models alone.  A plain module, imported as `from tests.rtx_loop import ...`."""
import numpy as np

from hilcodec_amd import jitter, rtx, wire
from hilcodec_amd.jitter import JitterConfig, JitterModel
from hilcodec_amd.rtx import NackConfig, NackModel, RtxConfig, RtxModel
from tests.hops import arrival_arrays

HOPS = 400
LOOP_JITTER = JitterConfig(depth=4, capacity=8)
LOOP_NACK = NackConfig(rtt_hops=2, retry_hops=3, max_requests=2)
LOOP_RTX = RtxConfig(history=16, per_hop=2)


def singles_and_pairs(seed=11, count=40, lo=8, hi=HOPS - 16):
    """`count` dropped hops in [lo, hi): random singles and adjacent pairs, never three in a row (the loop's condition is depth >=
    rtt_hops + longest burst, and the longest burst here is 2)"""
    rng = np.random.default_rng(seed)
    drops = set()
    while len(drops) < count:
        t = int(rng.integers(lo, hi))
        trial = drops | {t}
        if not any({u, u + 1, u + 2} <= trial for u in (t - 2, t - 1, t)):
            drops = trial
    assert any(t + 1 in drops for t in drops) and any(t - 1 not in drops and t + 1 not in drops for t in drops)
    return drops


def bursts_of_two(seed=12, count=22, lo=8, hi=HOPS - 16):
    """`count` bursts of two dropped hops in [lo, hi) that do not touch each other"""
    rng = np.random.default_rng(seed)
    starts = set()
    while len(starts) < count:
        t = int(rng.integers(lo, hi))
        if all(abs(t - u) >= 3 for u in starts):
            starts.add(t)
    return {t + k for t in starts for k in (0, 1)}


class Channel:
    """drops[b]: the loop iterations whose first transmission of slot b is lost; drop_rtx: (slot, hop index) pairs whose FIRST
    retransmission is lost; a NACK emitted on iteration t reaches the sender on iteration t + rtt_hops, whose retransmissions arrive
    with that iteration's packets, behind them"""

    def __init__(self, drops, rtt_hops, drop_rtx=()):
        self.drops, self.rtt, self.drop_rtx = drops, int(rtt_hops), set(drop_rtx)
        self.line = {}

    def push_nacks(self, t, nacks):
        """nacks: [(slot, 4-byte blob)] emitted by the receiver on iteration t"""
        self.line[t + self.rtt] = list(nacks)

    def nacks_for(self, t):
        slots_blobs = self.line.pop(t, [])
        return [s for s, _ in slots_blobs], [b for _, b in slots_blobs]

    def arrivals(self, t, first, again):
        """first / again: [(slot, headed packet bytes)] of iteration t -> the ones that arrive, in push order"""
        out = [(s, p) for s, p in first if t not in self.drops.get(s, ())]
        for s, p in again:
            key = (s, (p[0] << 8) | p[1])
            if key in self.drop_rtx:
                self.drop_rtx.discard(key)
            else:
                out.append((s, p))
        return out


def run_models(drops, jcfg=LOOP_JITTER, ncfg=LOOP_NACK, rcfg=LOOP_RTX, hops=HOPS, h0=0, nack=True, drop_rtx=(), B=2, n=4, seed=5):
    """the closed loop on the models alone: a stand-in sender of synthetic headed packets (n stages, one frame, random bodies, hop
    index from h0) with an RtxModel, the channel, a JitterModel (fixed clock, conceal) with a NackModel.  Returns the models, and per
    slot the iterations whose played body is not the one sent for that hop"""
    rng = np.random.default_rng(seed)
    tb = wire.transport_bytes(n, 0, 1)
    jm = JitterModel(B, jcfg, n, 0, 1, None, conceal=True)
    nm = NackModel(B, ncfg, jcfg.capacity, 0)
    rm = RtxModel(B, rcfg, tb)
    ch = Channel(drops, ncfg.rtt_hops, drop_rtx)
    bodies = rng.integers(0, 256, size=(hops, B, tb - wire.TRANSPORT_HEADER), dtype=np.uint8)
    zeros = np.zeros(B, dtype=np.int32)
    wrong = {b: [] for b in range(B)}
    for t in range(hops):
        sent = [wire.pack_transport(h0 + t, bodies[t, b].tobytes(), n) for b in range(B)]
        words = np.zeros((B, 2), dtype=np.int64)
        for s, blob in zip(*ch.nacks_for(t)):
            words[s] = rtx.nack_words(*wire.parse_nack(blob))
        out = rm.step(np.stack([np.frombuffer(p, dtype=np.uint8) for p in sent]), [tb] * B, words)
        again = [(b, out["packets"][b, q, :out["nbytes"][b, q]].tobytes()) for b in range(B) for q in range(rcfg.per_hop)
                 if out["nbytes"][b, q] > 0]
        rows = jm.step(zeros, zeros, *arrival_arrays(ch.arrivals(t, list(enumerate(sent)), again), tb))
        if nack:
            o = nm.step(jm.state, jm.meta, zeros)
            ch.push_nacks(t, [(b, o["nacks"][b].tobytes()) for b in range(B) if o["due"][b]])
        if t >= jcfg.depth:                                  # play call t plays hop t - depth
            for b in range(B):
                good = rows["hold"][b] == 0 and rows["lost"][b] == 0 and np.array_equal(rows["packets"][b], bodies[t - jcfg.depth, b])
                if not good:
                    wrong[b].append(t - jcfg.depth)
    return jm, nm, rm, wrong


def lost(jm, b=0):
    return int(jm.state[b, jitter.STAT_LOST])
