"""Jitter buffer of the graphed receiver (graph_step.GraphedDecodeHop(jitter=JitterConfig(...)), `play()`): the definition, bit for bit,
of hilc_jitter_step (csrc/jitter.hip), and the only module that knows its rules.

Packets carry the transport header of wire.py (hop index h mod 2^16, SID / FEC flags, n).  Per slot the receiver keeps a ring of C
entries indexed by h mod C and a playout clock `next` that starts D hops after the first packet: each hop, the slot's arrivals are
taken in push order, then the entry `next` is played — its codes decoded, its SID turned into comfort noise, a gap filled from the
redundant section of entry next + 1, concealed or held — and `next` advances.  The kernel writes the same control rows that the
caller of `step(packets, n, hold=, lost=, fec=, sid=, silent=)` writes, so every kernel after it is the explicit path's.

Per hop and slot, in this order:
1. action != 0 (a start or a resume on this hop): the state row and the ring are cleared.
2. each arrival, in push order: malformed (wire.parse_transport raises) -> MALFORMED, dropped; a slot not anchored is anchored by it
   (next = h, wait = D) and stores it; else d = int16(h - next): d < 0 LATE, d >= C EARLY, entry h occupied DUPLICATE (the first
   copy stays), else stored.  Stored arrivals count ACCEPTED.
3. play: hold row != 0 (a host hold or stop): nothing (playout pauses, the ring is kept); not anchored: hold 1; wait > 0: wait -= 1,
   hold 1 (priming); else entry h = next: codes -> packet row = body, n row = n, in_dtx = 0 (DECODED); SID -> packet row = SID, hold 2,
   in_dtx = 1 (NOISE); none and in_dtx -> hold 3 (NOISE); none, m >= 1 and entry h + 1 a codes packet with the FEC flag -> fec 1,
   packet and n rows from entry h + 1, which stays (FEC); none and conceal -> lost 1 (LOST); none -> hold 1 (LOST).  Then entry h is
   dropped and next = (next + 1) mod 2^16.
Rows not decided get what the explicit path accepts: n row = the graph's n, packet row zero, lost / fec 0, hold as given.

State row of a slot (int32, ST_WORDS words, updated in place once per hop): ST_ANCHORED, ST_WAIT, ST_NEXT, ST_IN_DTX, ST_MASK (bit i:
ring entry i occupied), then the counters STAT_*.  Ring: one meta word per entry (META_* fields: h | SID << 16 | FEC << 17 | n << 18,
0 when the entry is free) and one body row (the packet body, zero past its length)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import wire

ST_ANCHORED, ST_WAIT, ST_NEXT, ST_IN_DTX, ST_MASK = 0, 1, 2, 3, 4
STAT_ACCEPTED, STAT_DUPLICATE, STAT_LATE, STAT_EARLY, STAT_MALFORMED = 5, 6, 7, 8, 9
STAT_DECODED, STAT_FEC, STAT_LOST, STAT_NOISE = 10, 11, 12, 13
ST_WORDS = 14
STAT_NAMES = ("accepted", "duplicate", "late", "early", "malformed", "decoded", "fec", "lost", "noise")

META_SID, META_FEC, META_N_SHIFT = 1 << 16, 1 << 17, 18


@dataclass(frozen=True)
class JitterConfig:
    """depth D: the hops a slot primes before it plays its first packet (its playout delay); capacity C: ring entries per slot, a
    power of two in [2, 32] (the index h mod C survives the 16-bit wrap and the occupancy mask fits one int32), D <= C - 2 (the
    window holds the D hops of delay, the hop played and the one FEC looks at)"""
    depth: int = 2
    capacity: int = 8

    def __post_init__(self):
        for name in ("depth", "capacity"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"JitterConfig.{name} must be an int, got {v!r}")
        C, D = int(self.capacity), int(self.depth)
        if not 2 <= C <= 32 or C & (C - 1):
            raise ValueError(f"JitterConfig.capacity = {C}: a power of two in [2, 32]")
        if not 0 <= D <= C - 2:
            raise ValueError(f"JitterConfig.depth = {D} outside [0, capacity - 2 = {C - 2}]")


def meta_word(hop: int, sid: bool, fec: bool, n: int) -> int:
    return (int(hop) & 0xFFFF) | (META_SID if sid else 0) | (META_FEC if fec else 0) | (int(n) << META_N_SHIFT)


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


class JitterModel:
    """numpy statement of hilc_jitter_step for `batch` slots of a receiver with n_max stages, m redundant ones (0: no FEC), `frames`
    frames, comfort noise of order K (None: none) and `conceal`.  `state` int32 [B, ST_WORDS] and `meta` int32 [B, C] are the
    kernel's rows; `body` uint8 [B, C, stride] the ring's bodies (stride = wire.packet_bytes(n_max + m, frames))."""

    def __init__(self, batch: int, cfg: JitterConfig, n_max: int, m: int = 0, frames: int = 1, K: Optional[int] = None,
                 conceal: bool = False):
        self.B, self.cfg, self.n_max, self.m, self.T, self.K = int(batch), cfg, int(n_max), int(m), int(frames), K
        self.conceal = bool(conceal)
        self.stride = wire.packet_bytes(self.n_max + self.m, self.T)
        self.tbytes = wire.transport_bytes(self.n_max, self.m, self.T)
        C = cfg.capacity
        self.state = np.zeros((self.B, ST_WORDS), dtype=np.int32)
        self.meta = np.zeros((self.B, C), dtype=np.int32)
        self.body = np.zeros((self.B, C, self.stride), dtype=np.uint8)

    def _arrive(self, b: int, packet, nbytes: int) -> None:
        st, C = self.state[b], self.cfg.capacity
        try:
            hop, sid, fec, n, body = wire.parse_transport(packet, nbytes, self.T, self.n_max, self.m, self.K)
        except ValueError:
            st[STAT_MALFORMED] += 1
            return
        i = hop & (C - 1)
        if not st[ST_ANCHORED]:
            st[ST_ANCHORED], st[ST_NEXT], st[ST_WAIT] = 1, hop, self.cfg.depth
        else:
            d = ((hop - int(st[ST_NEXT]) + 0x8000) & 0xFFFF) - 0x8000
            if d < 0:
                st[STAT_LATE] += 1
                return
            if d >= C:
                st[STAT_EARLY] += 1
                return
            if (int(st[ST_MASK]) >> i) & 1:
                st[STAT_DUPLICATE] += 1
                return
        self.meta[b, i] = _i32(meta_word(hop, sid, fec, n))
        self.body[b, i] = 0
        self.body[b, i, :len(body)] = np.frombuffer(body, dtype=np.uint8)
        st[ST_MASK] = _i32(int(st[ST_MASK]) | (1 << i))
        st[STAT_ACCEPTED] += 1

    def _play(self, b: int, rows: Dict[str, np.ndarray]) -> None:
        st, C = self.state[b], self.cfg.capacity
        if rows["hold"][b] != 0:
            return
        if not st[ST_ANCHORED]:
            rows["hold"][b] = 1
            return
        if st[ST_WAIT] > 0:
            st[ST_WAIT] -= 1
            rows["hold"][b] = 1
            return
        h = int(st[ST_NEXT])
        i, j = h & (C - 1), (h + 1) & (C - 1)
        mask = int(st[ST_MASK]) & 0xFFFFFFFF
        if (mask >> i) & 1:
            mt = int(self.meta[b, i]) & 0xFFFFFFFF
            rows["packets"][b] = self.body[b, i]
            if mt & META_SID:
                rows["hold"][b] = 2
                st[ST_IN_DTX] = 1
                st[STAT_NOISE] += 1
            else:
                rows["n"][b] = mt >> META_N_SHIFT
                st[ST_IN_DTX] = 0
                st[STAT_DECODED] += 1
            st[ST_MASK] = _i32(mask & ~(1 << i))
            self.meta[b, i] = 0
        elif st[ST_IN_DTX]:
            rows["hold"][b] = 3
            st[STAT_NOISE] += 1
        else:
            mt = int(self.meta[b, j]) & 0xFFFFFFFF
            if self.m >= 1 and (mask >> j) & 1 and not mt & META_SID and mt & META_FEC:
                rows["fec"][b] = 1
                rows["packets"][b] = self.body[b, j]
                rows["n"][b] = mt >> META_N_SHIFT
                st[STAT_FEC] += 1
            else:
                if self.conceal:
                    rows["lost"][b] = 1
                else:
                    rows["hold"][b] = 1
                st[STAT_LOST] += 1
        st[ST_NEXT] = (h + 1) & 0xFFFF

    def step(self, action, hold, slots, packets, nbytes) -> Dict[str, np.ndarray]:
        """one hop: `action` / `hold` int [B] (the session rows: a start or resume; a host hold or stop), arrivals `slots` [A],
        `packets` uint8 [A, tbytes], `nbytes` [A] in push order -> the rows the kernel writes: hold, n, lost, fec (int32 [B]) and
        packets (uint8 [B, stride])"""
        B = self.B
        action = np.asarray(action).reshape(-1)
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        packets = np.asarray(packets, dtype=np.uint8).reshape(len(slots), self.tbytes)
        nbytes = np.asarray(nbytes, dtype=np.int64).reshape(-1)
        rows = {"hold": np.asarray(hold, dtype=np.int32).reshape(-1).copy(), "n": np.full(B, self.n_max, dtype=np.int32),
                "lost": np.zeros(B, dtype=np.int32), "fec": np.zeros(B, dtype=np.int32),
                "packets": np.zeros((B, self.stride), dtype=np.uint8)}
        for b in np.nonzero(action != 0)[0]:
            self.state[b] = 0
            self.meta[b] = 0
        for a in range(len(slots)):
            self._arrive(int(slots[a]), packets[a], int(nbytes[a]))
        for b in range(B):
            self._play(b, rows)
        return rows
