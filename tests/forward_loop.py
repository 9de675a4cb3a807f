"""What the CPU and the GPU tests of the forwarding hop share: a seeded traffic generator (talk spurts, SIDs, silence, duplicates,
overflowing bursts, malformed packets, random pad bits; joins, leaves and layer changes), the host's membership rows, and the small
checkers of what a hop emitted.  A plain module, imported as `from tests.forward_loop import ...`."""
import numpy as np
import torch

from hilcodec_amd import dtx, wire


def random_packet(rng, hop, n_pkt, T, m, fec, pad=True):
    """a headed codes packet of n_pkt stages (and an m-stage redundant section with `fec`), random codes; `pad`: random pad bits
    in its last byte (a receiver ignores them).  Returns (bytes, codes [n_pkt (+ m), T])"""
    codes = torch.from_numpy(rng.integers(0, 1024, (n_pkt + (m if fec else 0), T)))
    body = bytearray(wire.pack_stream_packet(codes))
    spare = 8 * len(body) - 10 * codes.numel()
    if pad and spare:
        body[-1] |= int(rng.integers(0, 1 << spare))
    return wire.pack_transport(hop, bytes(body), n_pkt, fec=fec), codes


def random_sid(rng, hop, K):
    return wire.pack_transport(hop, bytes(rng.integers(0, 256, dtx.sid_bytes(K), dtype=np.uint8)), 0, sid=True)


def malformed(rng, good, n, T, m):
    """one of the ways a packet is malformed, made from the valid codes packet `good`: short, reserved bit set, n = 0, n > n_max,
    wrong length.  Returns (bytes, byte count): the count may differ from len(bytes)"""
    how = int(rng.integers(0, 5))
    p = bytearray(good)
    if how == 0:
        return bytes(p[:2]), int(rng.integers(-1, 3))
    if how == 1:
        p[2] |= wire.RSV_BIT
    elif how == 2:
        p[2] &= ~wire.N_MASK & 0xFF
    elif how == 3:
        p[2] = (p[2] & ~wire.N_MASK & 0xFF) | (n + 1)
    else:
        return bytes(p), len(p) - 1 if len(p) > wire.TRANSPORT_HEADER + 1 else len(p) + 1
    return bytes(p), len(p)


class Membership:
    """the host's rows of a forwarding hop: room (-1: none), layers, and the action row of the next hop"""

    def __init__(self, B, n):
        self.B, self.n = B, n
        self.room = np.full(B, -1, dtype=np.int32)
        self.layers = np.full(B, n, dtype=np.int32)
        self.joined = set()

    def apply(self, events, hop=None):
        """events: ("join", slot, room) / ("leave", slot) / ("layers", slot, L), also sent to a GraphedForwardHop `hop`"""
        for ev in events:
            if ev[0] == "join":
                self.room[ev[1]] = ev[2]
                self.joined.add(ev[1])
                hop is None or hop.join(ev[1], ev[2])
            elif ev[0] == "leave":
                self.room[ev[1]] = -1
                hop is None or hop.leave(ev[1])
            else:
                self.layers[ev[1]] = ev[2]
                hop is None or hop.set_layers(ev[1], ev[2])

    def action(self):
        """this hop's action row; the joins are spent"""
        a = np.zeros(self.B, dtype=np.int32)
        a[sorted(self.joined)] = 1
        self.joined = set()
        return a


class Traffic:
    """seeded arrivals and session events for B slots in `rooms` rooms.  Every slot alternates talk spurts (a codes packet per hop,
    with a redundant section on most hops when m >= 1) and silences (a SID now and then when K is not None, else nothing); on top of
    that come duplicates, a third and further arrivals (overflow), malformed packets and random pad bits.  Each slot draws from a
    generator of its own (`seed`, or `slot_seeds[b]` for slot b), so one slot's traffic does not depend on another's.  `garbage`: the
    slots whose every arrival is replaced by random bytes of a random length."""

    def __init__(self, B, n, T, m, K, rooms, seed, p_event=0.2, garbage=(), slot_seeds=None):
        self.B, self.n, self.T, self.m, self.K, self.rooms = B, n, T, m, K, rooms
        self.rng = np.random.default_rng(seed)              # the events and the push order
        self.slot_rng = [np.random.default_rng([(slot_seeds or {}).get(b, seed), b]) for b in range(B)]
        self.tb = wire.transport_bytes(n, m, T)
        self.talking = [bool(r.random() < 0.5) for r in self.slot_rng]
        self.h = [int(r.integers(0, 65536)) for r in self.slot_rng]
        self.p_event, self.garbage = p_event, set(garbage)

    def initial_events(self):
        return [("join", b, b % self.rooms) for b in range(self.B)]

    def events(self):
        rng, out = self.rng, []
        while rng.random() < self.p_event:
            b, what = int(rng.integers(0, self.B)), rng.random()
            if what < 0.4:
                out.append(("join", b, int(rng.integers(0, self.rooms))))
            elif what < 0.6:
                out.append(("leave", b))
            else:
                out.append(("layers", b, int(rng.integers(1, self.n + 1))))
        return out

    def hop(self):
        """one hop's arrivals in push order: (slots, packets uint8 [A, tb], nbytes)"""
        n, T, m, K = self.n, self.T, self.m, self.K
        arrived = []
        for b in range(self.B):
            rng = self.slot_rng[b]
            if rng.random() < 0.15:
                self.talking[b] = not self.talking[b]
            mine = []
            h = int(self.h[b])
            fec = m >= 1 and rng.random() < 0.7
            n_pkt = int(rng.integers(max(m, 1) if fec else 1, n + 1))
            good = random_packet(rng, h, n_pkt, T, m, fec)[0]
            if self.talking[b]:
                mine.append((good, len(good)))
                self.h[b] = (h + 1) & 0xFFFF
            elif K is not None and rng.random() < 0.3:
                sid = random_sid(rng, h, K)
                mine.append((sid, len(sid)))
                self.h[b] = (h + 1) & 0xFFFF
            if mine and rng.random() < 0.15:
                mine.append(mine[0])                         # a duplicate
            if mine and rng.random() < 0.15:                 # a burst: more arrivals than any `burst` forwards
                for _ in range(int(rng.integers(1, 5))):
                    extra = random_packet(rng, h, n_pkt, T, m, fec)[0]
                    mine.append((extra, len(extra)))
            if rng.random() < 0.12:
                mine.insert(int(rng.integers(0, len(mine) + 1)), malformed(rng, good, n, T, m))
            if b in self.garbage:
                mine = [(bytes(rng.integers(0, 256, self.tb, dtype=np.uint8)), int(rng.integers(-1, self.tb + 3))) for _ in mine]
            arrived += [(b, p, nb) for p, nb in mine]
        keys = self.rng.random(len(arrived))                # push order interleaves the slots and keeps each slot's own order
        for b in range(self.B):
            mine = [i for i, a in enumerate(arrived) if a[0] == b]
            keys[mine] = np.sort(keys[mine])
        arrived = [arrived[i] for i in np.argsort(keys, kind="stable")]
        packets = np.zeros((len(arrived), self.tb), dtype=np.uint8)
        for a, (_, p, _nb) in enumerate(arrived):
            packets[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        return [b for b, _, _ in arrived], packets, [nb for _, _, nb in arrived]


def check_hop(res, records, room, layers, cfg, n, T, m, K, listeners=None):
    """the invariants of one hop's result (a model's or the kernels'; `records`: the hop's staged arrivals): route owners are distinct,
    in the listener's room, not the listener, at most fanout; every non-empty row parses for a receiver of n stages with header n <=
    layers and is zero past its length, every other row is zero.  Returns the recount per listener: int64 [B, 3], the packets, their
    bytes and those whose n was cut (a source's n: header byte 2 of record pick[owner][k])"""
    B = len(room)
    counts = np.zeros((B, 3), dtype=np.int64)
    for b in (range(B) if listeners is None else listeners):
        owners = [int(t) for t in res["routes"][b] if t >= 0]
        assert len(owners) == len(set(owners)) <= cfg.fanout and b not in owners, (b, owners)
        assert all(room[t] == room[b] >= 0 for t in owners), (b, owners)
        for j in range(cfg.fanout):
            for k in range(cfg.burst):
                nb, row = int(res["out_nbytes"][b, j, k]), res["out"][b, j, k]
                assert not row[nb:].any(), (b, j, k)
                if nb == 0:
                    continue
                t = int(res["routes"][b, j])
                assert t >= 0 and k < res["pick_count"][t], (b, j, k)
                _hop, sid, _fec, n_pkt, _body = wire.parse_transport(row, nb, T, n, m, K)
                assert sid or n_pkt <= layers[b], (b, j, k)
                flags = int(records[res["pick"][t, k]].view(np.uint8)[4 + 2])
                counts[b] += (1, nb, int(not sid and (flags & wire.N_MASK) > n_pkt))
    return counts
