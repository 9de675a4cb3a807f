"""What the CPU and the GPU tests of the protected forwarding hop (GraphedForwardHop(srtp=)) share: keys by name, a seeded call whose
senders protect what they send (srtp.SenderModel), and the listeners' clients (srtp.ReceiverModel per listener, one slot per route)
that follow the epoch rule of forward_srtp.py.  A plain module, imported as `from tests.forward_srtp_loop import ...`."""
import numpy as np

from hilcodec_amd import forward_srtp, srtp, wire
from tests.forward_loop import random_packet, random_sid


def key(tag, b):
    """the master key and salt named (tag, b)"""
    return bytes([tag & 255, b & 255, tag >> 8] * 5 + [7]), bytes([b & 255, tag & 255] * 7)


class Call:
    """B senders behind one srtp.SenderModel.  A talking slot sends one or two packets per hop with consecutive hop indices; `late`
    slots now and then hold a packet back by one hop, so that it arrives behind a newer one; `first` gives a slot's first hop index
    (0xFFFA: its SEQ wraps soon).  `hop` returns the same arrivals twice, in the same push order: plain and protected."""

    def __init__(self, B, n, T, m, K, seed, first=None, late=()):
        self.B, self.n, self.T, self.m, self.K = B, n, T, m, K
        self.tb = wire.transport_bytes(n, m, T)
        self.rng = np.random.default_rng(seed)
        self.tx = srtp.SenderModel(B, self.tb)
        self.h = np.zeros(B, dtype=np.int64)
        for b, h in (first or {}).items():
            self.h[b] = h
        self.late, self.held = set(late), {}
        self.talking = [True] * B
        self.gen = [0] * B
        self.history = []                                    # every protected arrival: (slot, bytes)

    def rekey(self, b, ssrc=None):
        """a start of sender b under its next key: (master key, master salt, ssrc) for the forwarder's set_uplink_key"""
        self.gen[b] += 1
        mk, ms = key(self.gen[b], b)
        ssrc = 1000 + b if ssrc is None else ssrc
        self.tx.keys.set_key(b, mk, ms, ssrc=ssrc)
        start = np.zeros(self.B, dtype=np.int32)
        start[b] = 1
        self.tx.protect(np.zeros((self.B, self.tb), dtype=np.uint8), np.zeros(self.B, dtype=np.int32), start)
        self.held.pop(b, None)                               # what was under way under the old key is lost
        if self.gen[b] > 1:
            self.h[b] = 0
        return mk, ms, ssrc

    def hop(self, p_flip=0.1, p_two=0.3, p_late=0.25):
        rng, B, tb = self.rng, self.B, self.tb
        rounds = [{}, {}]
        for b in range(B):
            if rng.random() < p_flip:
                self.talking[b] = not self.talking[b]
            count = (1 + int(rng.random() < p_two)) if self.talking[b] else 0
            if not count and self.K is not None and rng.random() < 0.3:
                rounds[0][b] = random_sid(rng, int(self.h[b]), self.K)
                self.h[b] = (self.h[b] + 1) & 0xFFFF
            for r in range(count):
                fec = self.m >= 1 and rng.random() < 0.7
                n_pkt = int(rng.integers(max(self.m, 1) if fec else 1, self.n + 1))
                rounds[r][b] = random_packet(rng, int(self.h[b]), n_pkt, self.T, self.m, fec)[0]
                self.h[b] = (self.h[b] + 1) & 0xFFFF
        sent = []                                            # (slot, plain, protected) in sending order
        for packets in rounds:
            rows, nbytes = np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32)
            for b, p in packets.items():
                rows[b, :len(p)], nbytes[b] = np.frombuffer(p, dtype=np.uint8), len(p)
            out = self.tx.protect(rows, nbytes)
            sent += [(b, p, out["packets"][b, :out["nbytes"][b]].tobytes()) for b, p in packets.items()]
        arrived = []
        for b, p, w in sent:
            if b in self.late and b not in self.held and rng.random() < p_late:
                self.held[b] = (b, p, w, len(self.history))
            else:
                arrived.append((b, p, w))
        for b in [b for b, v in self.held.items() if v[3] < len(self.history)]:
            arrived.append(self.held.pop(b)[:3])             # behind this hop's own packets
        self.history.append([(b, w) for b, _, w in arrived])
        return [(b, p) for b, p, _ in arrived], [(b, w) for b, _, w in arrived]


def forge(p, bit=37):
    """`p` with one bit of its body flipped"""
    bit %= 8 * (len(p) - srtp.TAG_BYTES)
    return p[:bit >> 3] + bytes([p[bit >> 3] ^ (1 << (bit & 7))]) + p[(bit >> 3) + 1:]


class Clients:
    """every listener's client: a srtp.ReceiverModel with one slot per route, re-keyed and restarted by the epoch rule"""

    def __init__(self, B, F, tb):
        self.B, self.F, self.tb = B, F, tb
        self.rx = [srtp.ReceiverModel(F, tb) for _ in range(B)]
        self.epoch = np.zeros((B, F), dtype=np.int64)
        self.keys = [None] * B                               # (master key, master salt, base ssrc)
        self.delivered = 0

    def set_key(self, b, mk, ms, base):
        self.keys[b] = (mk, ms, base)

    def deliver(self, epochs, out, out_nbytes):
        """one hop's protected rows and the epochs signalled with them -> the rows as the clients see them: plain uint8 [B, F, P, tb]
        and their byte counts (0: nothing arrived or it was rejected)"""
        B, F, P = out_nbytes.shape
        plain, counts = np.zeros((B, F, P, self.tb), dtype=np.uint8), np.zeros((B, F, P), dtype=np.int32)
        for b in range(B):
            for j in range(F):
                if epochs[b, j] != self.epoch[b, j] and self.keys[b] is not None:
                    mk, ms, base = self.keys[b]
                    self.rx[b].keys.set_key(j, mk, ms, ssrc=forward_srtp.route_ssrc(base, j, int(epochs[b, j])))
                    start = np.zeros(F, dtype=np.int32)
                    start[j] = 1
                    self.rx[b].start(start)
                    self.epoch[b, j] = epochs[b, j]
                for k in range(P):
                    nb = int(out_nbytes[b, j, k])
                    if nb == 0:
                        continue
                    got = self.rx[b].push(j, out[b, j, k, :nb].tobytes())
                    if got is not None:
                        plain[b, j, k, :len(got)] = np.frombuffer(got, dtype=np.uint8)
                        counts[b, j, k] = len(got)
                        self.delivered += 1
        return plain, counts
