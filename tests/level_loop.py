"""What the CPU and the GPU tests of level-based speaker selection share: tests/forward_loop.py's traffic with a level drawn per
arrival, a scripted room of senders without DTX (every slot sends one codes packet per hop; who talks, and how loud, follows a script),
and the count of what a listener heard of it.  A plain module, imported as `from tests.level_loop import ...`."""
import numpy as np

from hilcodec_amd import wire
from tests.forward_loop import Traffic, random_packet


class LevelTraffic:
    """tests.forward_loop.Traffic with one level per arrival, drawn from `choices` (repeats make keys tie; -1: unknown) by a generator
    of its own, so the packets are those of the plain traffic with the same seed"""

    def __init__(self, B, n, T, m, K, rooms, seed, choices=(20, 20, 40, -1), **kw):
        self.traffic = Traffic(B, n, T, m, K, rooms, seed, **kw)
        self.levels_rng = np.random.default_rng([seed, 0x1e7e1])
        self.choices = np.asarray(choices, dtype=np.int64)
        self.tb = self.traffic.tb

    def initial_events(self):
        return self.traffic.initial_events()

    def events(self):
        return self.traffic.events()

    def hop(self):
        """one hop's arrivals in push order: (slots, packets uint8 [A, tb], nbytes, levels)"""
        slots, packets, nbytes = self.traffic.hop()
        return slots, packets, nbytes, self.levels_rng.choice(self.choices, len(slots)).tolist()


# the room scenario's talk script: (slot, from, to, level), the slot talks on the hops from <= h < to
ROOM_SCRIPT = ((4, 20, 120, 20), (5, 60, 200, 26), (2, 150, 260, 15), (3, 240, 330, 30), (1, 300, 380, 22))


class ScriptedRoom:
    """B senders without DTX in one room: every slot sends one n-stage codes packet per hop.  A slot that talks by `script` says the
    script's level + U{-jitter..jitter}, plus 25 with probability `spike_p` (a pause between two words); every other slot says
    `background` + U{-background_jitter..background_jitter}."""

    def __init__(self, B, n, T, script, seed, background=70, background_jitter=3, jitter=4, spike_p=0.15):
        self.B, self.n, self.T, self.script = B, n, T, tuple(script)
        self.rng = np.random.default_rng(seed)
        self.background, self.background_jitter, self.jitter, self.spike_p = background, background_jitter, jitter, spike_p
        self.tb = wire.transport_bytes(n, 0, T)

    def talkers(self, h):
        """the scripted talkers of hop h, in script order"""
        return [s for s, lo, hi, _ in self.script if lo <= h < hi]

    def hop(self, h):
        """hop h's arrivals in slot order: (slots, packets uint8 [B, tb], nbytes, levels)"""
        rng = self.rng
        said = {s: lv for s, lo, hi, lv in self.script if lo <= h < hi}
        packets = np.zeros((self.B, self.tb), dtype=np.uint8)
        levels = []
        for b in range(self.B):
            p = random_packet(rng, h & 0xFFFF, self.n, self.T, 0, False)[0]
            packets[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
            if b in said:
                lv = said[b] + int(rng.integers(-self.jitter, self.jitter + 1)) + (25 if rng.random() < self.spike_p else 0)
            else:
                lv = self.background + int(rng.integers(-self.background_jitter, self.background_jitter + 1))
            levels.append(min(max(lv, 0), 127))
        return list(range(self.B)), packets, [self.tb] * self.B, levels


def heard_of_wanted(net, routes_of_hop, hops, listener=0, most=2):
    """(heard, wanted) at `listener` over `hops` hops: wanted counts the first `most` scripted talkers of each hop other than the
    listener, heard those among its routes; `routes_of_hop(h, slots, packets, nbytes, levels)` runs hop h and returns routes [B, fanout]"""
    heard = wanted = 0
    for h in range(hops):
        routes = routes_of_hop(h, *net.hop(h))
        want = [s for s in net.talkers(h) if s != listener][:most]
        wanted += len(want)
        heard += sum(1 for s in want if s in [int(t) for t in routes[listener]])
    return heard, wanted
