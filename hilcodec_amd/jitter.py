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
0 when the entry is free) and one body row (the packet body, zero past its length).

Adaptive playout (JitterConfig(..., adapt=AdaptConfig(...)); hilc_jitter_adapt_step, csrc/jitter_adapt.hip).  The fixed buffer's clock
advances one per hop for ever, so a sender whose clock drifts, a burst of delay or a sender restart leaves it late or early for the
life of the stream.  With `adapt` the slot moves its clock against the sender's by whole hops — an inserted hop (grow), a skipped
entry (shrink) or a new anchor (resync) — decided per slot in the same launch from one more row, the adapt row (int32, AD_WORDS
words): AD_DEBT (hops to move at once; > 0 grow, < 0 shrink), AD_PENDING (hops the windowed estimate wants), AD_STALE (windows in a
row that wanted the same direction and were not served), AD_MIN / AD_COUNT (the window's smallest margin; its hops), AD_RUN /
AD_LAST (the run of out-of-window arrivals; the last one's h), AD_MARGIN (the last full window's smallest margin), then the
counters AD_GROWN, AD_SHRUNK, AD_FORCED, AD_RESYNC.  "The control words are cleared": the words before the counters = 0, then
AD_MIN = C ("no arrival seen") and AD_MARGIN = D.  The margin of an arrival is d = int16(h - next) when it is taken: 0 = it arrived on
the hop that plays it; the fixed buffer's steady state is d = D.  The steps above become:
1. action != 0 clears the whole adapt row too, counters included.
2. each arrival: malformed as above (AD_RUN untouched).  Not anchored: anchored as above, the control words are cleared, stored.
   d < 0 or d >= C: LATE / EARLY is counted; AD_RUN = AD_RUN + 1 if AD_RUN > 0 and |int16(h - AD_LAST)| < C, else 1; AD_LAST = h; at
   AD_RUN >= resync the slot resyncs — next = h, wait = D, in_dtx = 0, the ring is emptied (mask and meta), the control words are
   cleared, AD_RESYNC += 1 and this arrival is stored (ACCEPTED); otherwise it is dropped, and with wait == 0 it first leaves an
   urgent debt: late by L = -d <= max_late: AD_DEBT = max(AD_DEBT, L); early by E = d - (C - 1) <= max_late: AD_DEBT =
   min(AD_DEBT, -E).  Duplicate: as above, AD_RUN = 0.  Stored: as above, AD_RUN = 0 and, with wait == 0, AD_MIN = min(AD_MIN, d).
3. play: held, not anchored or priming: as above.  Else, with h = next, present = entry h occupied, fecable = the FEC condition above
   on entry h + 1, free = not present and (in_dtx or not fecable) (noise or a loss whatever the clock does) and forced =
   force_windows > 0 and AD_STALE >= force_windows, a step is picked: AD_DEBT != 0: step = sign(AD_DEBT), AD_DEBT -= step, and
   AD_PENDING, if of that sign, moves one towards 0 too; else AD_PENDING != 0 and (free or forced): step = sign(AD_PENDING),
   AD_PENDING -= step, AD_FORCED += 1 when not free; else step = 0.  step != 0 restarts the window (AD_MIN = C, AD_COUNT = 0) and sets
   AD_STALE = 0 once AD_PENDING == 0.  step > 0 (grow): AD_GROWN += 1, the hop is an inserted one — hold 3 if in_dtx, else lost 1
   with conceal, else hold 1 — next stands, no STAT_* counter moves and the hop ends.  step < 0 (shrink): entry h is discarded if
   present, next = h + 1, AD_SHRUNK += 1, and the hop goes on with the new next.  Then the play rule above, unchanged; after it
   AD_COUNT += 1, and at AD_COUNT >= window: if AD_MIN < C (an arrival was seen): AD_MARGIN = AD_MIN, want = headroom - AD_MIN,
   AD_STALE = AD_STALE + 1 if want and the old AD_PENDING have the same sign, else 0, AD_PENDING = want; then AD_MIN = C, AD_COUNT = 0.
So urgent late or early arrivals move the clock at once; the windowed estimate moves it by headroom - min margin, one hop per
opportunity, on hops that cost nothing (comfort noise or a loss) and on speech only after force_windows windows of waiting; `resync`
consecutive out-of-window arrivals that agree with each other re-anchor the slot.  DECODED + FEC + LOST + NOISE + AD_GROWN = the hops
past priming that were not held."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import wire
from .sessions import HOLD_HELD, HOLD_SID, HOLD_SILENT

ST_ANCHORED, ST_WAIT, ST_NEXT, ST_IN_DTX, ST_MASK = 0, 1, 2, 3, 4
STAT_ACCEPTED, STAT_DUPLICATE, STAT_LATE, STAT_EARLY, STAT_MALFORMED = 5, 6, 7, 8, 9
STAT_DECODED, STAT_FEC, STAT_LOST, STAT_NOISE = 10, 11, 12, 13
ST_WORDS = 14
STAT_NAMES = ("accepted", "duplicate", "late", "early", "malformed", "decoded", "fec", "lost", "noise")

META_SID, META_FEC, META_N_SHIFT = 1 << 16, 1 << 17, 18

AD_DEBT, AD_PENDING, AD_STALE, AD_MIN, AD_COUNT, AD_RUN, AD_LAST, AD_MARGIN = range(8)
AD_GROWN, AD_SHRUNK, AD_FORCED, AD_RESYNC = 8, 9, 10, 11
AD_WORDS = 12
AD_NAMES = ("grown", "shrunk", "forced", "resync")


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


@dataclass(frozen=True)
class AdaptConfig:
    """adaptive playout of a JitterConfig (the rules: this module's docstring).  headroom: the margin, in hops, the windowed
    estimate steers the earliest arrival of a window to; max_late: how many hops late (or past the window's end) a dropped arrival
    may be and still move the clock at once (None: capacity - 2); window: hops per estimate; resync: consecutive out-of-window
    arrivals that re-anchor the slot; force_windows: windows an estimate waits for a free hop before it cuts or pads speech (0: never)"""
    headroom: int = 1
    max_late: Optional[int] = None
    window: int = 50
    resync: int = 4
    force_windows: int = 4

    def __post_init__(self):
        for name, lo in (("headroom", 0), ("max_late", 1), ("window", 1), ("resync", 2), ("force_windows", 0)):
            v = getattr(self, name)
            if name == "max_late" and v is None:
                continue
            if not _is_int(v):
                raise ValueError(f"AdaptConfig.{name} must be an int, got {v!r}")
            if not lo <= int(v) < 1 << 30:
                raise ValueError(f"AdaptConfig.{name} = {v} below {lo}")

    def max_late_for(self, capacity: int) -> int:
        return int(capacity) - 2 if self.max_late is None else int(self.max_late)


@dataclass(frozen=True)
class JitterConfig:
    """depth D: the hops a slot primes before it plays its first packet (its playout delay); capacity C: ring entries per slot, a
    power of two in [2, 32] (the index h mod C survives the 16-bit wrap and the occupancy mask fits one int32), D <= C - 2 (the
    window holds the D hops of delay, the hop played and the one FEC looks at); adapt: an AdaptConfig for an adaptive playout clock
    (0 <= headroom <= C - 2, 1 <= max_late <= C - 2, so C >= 4), None for the fixed one"""
    depth: int = 2
    capacity: int = 8
    adapt: Optional[AdaptConfig] = None

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
        if self.adapt is not None:
            if not isinstance(self.adapt, AdaptConfig):
                raise ValueError(f"JitterConfig.adapt must be an AdaptConfig or None, got {self.adapt!r}")
            if not 0 <= self.adapt.headroom <= C - 2:
                raise ValueError(f"AdaptConfig.headroom = {self.adapt.headroom} outside [0, capacity - 2 = {C - 2}]")
            if not 1 <= self.adapt.max_late_for(C) <= C - 2:
                raise ValueError(f"AdaptConfig.max_late = {self.adapt.max_late_for(C)} outside [1, capacity - 2 = {C - 2}]")


def meta_word(hop: int, sid: bool, fec: bool, n: int) -> int:
    return (int(hop) & 0xFFFF) | (META_SID if sid else 0) | (META_FEC if fec else 0) | (int(n) << META_N_SHIFT)


def _i16(v: int) -> int:
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


class JitterModel:
    """numpy statement of hilc_jitter_step for `batch` slots of a receiver with n_max stages, m redundant ones (0: no FEC), `frames`
    frames, comfort noise of order K (None: none) and `conceal`.  `state` int32 [B, ST_WORDS] and `meta` int32 [B, C] are the
    kernel's rows; `body` uint8 [B, C, stride] the ring's bodies (stride = wire.packet_bytes(n_max + m, frames)).  With cfg.adapt it
    states hilc_jitter_adapt_step, and `adapt` int32 [B, AD_WORDS] are the adapt rows."""

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
        if cfg.adapt is not None:
            self.adapt = np.zeros((self.B, AD_WORDS), dtype=np.int32)

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
        self._store(b, hop, sid, fec, n, body)

    def _store(self, b: int, hop: int, sid: bool, fec: bool, n: int, body: bytes) -> None:
        st, i = self.state[b], hop & (self.cfg.capacity - 1)
        self.meta[b, i] = _i32(meta_word(hop, sid, fec, n))
        self.body[b, i] = 0
        self.body[b, i, :len(body)] = np.frombuffer(body, dtype=np.uint8)
        st[ST_MASK] = _i32(int(st[ST_MASK]) | (1 << i))
        st[STAT_ACCEPTED] += 1

    def _clear_control(self, b: int) -> None:
        ad = self.adapt[b]
        ad[:AD_GROWN] = 0
        ad[AD_MIN], ad[AD_MARGIN] = self.cfg.capacity, self.cfg.depth

    def _arrive_adapt(self, b: int, packet, nbytes: int) -> None:
        st, ad, C, ac = self.state[b], self.adapt[b], self.cfg.capacity, self.cfg.adapt
        try:
            hop, sid, fec, n, body = wire.parse_transport(packet, nbytes, self.T, self.n_max, self.m, self.K)
        except ValueError:
            st[STAT_MALFORMED] += 1
            return
        if not st[ST_ANCHORED]:
            st[ST_ANCHORED], st[ST_NEXT], st[ST_WAIT] = 1, hop, self.cfg.depth
            self._clear_control(b)
        else:
            d = _i16(hop - int(st[ST_NEXT]))
            if d < 0 or d >= C:
                st[STAT_LATE if d < 0 else STAT_EARLY] += 1
                ad[AD_RUN] = ad[AD_RUN] + 1 if ad[AD_RUN] > 0 and abs(_i16(hop - int(ad[AD_LAST]))) < C else 1
                ad[AD_LAST] = hop
                if ad[AD_RUN] < ac.resync:
                    if st[ST_WAIT] == 0:
                        if d < 0 and -d <= ac.max_late_for(C):
                            ad[AD_DEBT] = max(int(ad[AD_DEBT]), -d)
                        elif d >= C and d - (C - 1) <= ac.max_late_for(C):
                            ad[AD_DEBT] = min(int(ad[AD_DEBT]), (C - 1) - d)
                    return
                st[ST_NEXT], st[ST_WAIT], st[ST_IN_DTX], st[ST_MASK] = hop, self.cfg.depth, 0, 0
                self.meta[b] = 0
                self._clear_control(b)
                ad[AD_RESYNC] += 1
            elif (int(st[ST_MASK]) >> (hop & (C - 1))) & 1:
                st[STAT_DUPLICATE] += 1
                ad[AD_RUN] = 0
                return
            else:
                ad[AD_RUN] = 0
                if st[ST_WAIT] == 0:
                    ad[AD_MIN] = min(int(ad[AD_MIN]), d)
        self._store(b, hop, sid, fec, n, body)

    def _play(self, b: int, rows: Dict[str, np.ndarray]) -> None:
        st, C = self.state[b], self.cfg.capacity
        if rows["hold"][b] != 0:
            return
        if not st[ST_ANCHORED]:
            rows["hold"][b] = HOLD_HELD
            return
        if st[ST_WAIT] > 0:
            st[ST_WAIT] -= 1
            rows["hold"][b] = HOLD_HELD
            return
        if self.cfg.adapt is not None and self._shift(b, rows):
            return
        self._play_entry(b, rows)
        if self.cfg.adapt is not None:
            self._window(b)

    def _fecable(self, b: int, j: int) -> bool:
        mt = int(self.meta[b, j]) & 0xFFFFFFFF
        return bool(self.m >= 1 and (int(self.state[b, ST_MASK]) >> j) & 1 and not mt & META_SID and mt & META_FEC)

    def _shift(self, b: int, rows: Dict[str, np.ndarray]) -> bool:
        """the adaptive step of a playing slot, before its entry is played: True when the hop is an inserted one (grow)"""
        st, ad, C, ac = self.state[b], self.adapt[b], self.cfg.capacity, self.cfg.adapt
        h = int(st[ST_NEXT])
        i, j = h & (C - 1), (h + 1) & (C - 1)
        present = bool((int(st[ST_MASK]) >> i) & 1)
        free = not present and bool(st[ST_IN_DTX] or not self._fecable(b, j))
        forced = ac.force_windows > 0 and ad[AD_STALE] >= ac.force_windows
        sign = lambda v: (int(v) > 0) - (int(v) < 0)
        step = 0
        if ad[AD_DEBT] != 0:
            step = sign(ad[AD_DEBT])
            ad[AD_DEBT] -= step
            if sign(ad[AD_PENDING]) == step:
                ad[AD_PENDING] -= step
        elif ad[AD_PENDING] != 0 and (free or forced):
            step = sign(ad[AD_PENDING])
            ad[AD_PENDING] -= step
            if not free:
                ad[AD_FORCED] += 1
        if step != 0:
            ad[AD_MIN], ad[AD_COUNT] = C, 0
            if ad[AD_PENDING] == 0:
                ad[AD_STALE] = 0
        if step > 0:
            ad[AD_GROWN] += 1
            if st[ST_IN_DTX]:
                rows["hold"][b] = HOLD_SILENT
            elif self.conceal:
                rows["lost"][b] = 1
            else:
                rows["hold"][b] = HOLD_HELD
            return True
        if step < 0:
            if present:
                st[ST_MASK] = _i32(int(st[ST_MASK]) & 0xFFFFFFFF & ~(1 << i))
                self.meta[b, i] = 0
            st[ST_NEXT] = (h + 1) & 0xFFFF
            ad[AD_SHRUNK] += 1
        return False

    def _window(self, b: int) -> None:
        ad, C, ac = self.adapt[b], self.cfg.capacity, self.cfg.adapt
        ad[AD_COUNT] += 1
        if ad[AD_COUNT] >= ac.window:
            if ad[AD_MIN] < C:
                want, old = ac.headroom - int(ad[AD_MIN]), int(ad[AD_PENDING])
                ad[AD_MARGIN] = ad[AD_MIN]
                ad[AD_STALE] = ad[AD_STALE] + 1 if (want > 0 and old > 0) or (want < 0 and old < 0) else 0
                ad[AD_PENDING] = want
            ad[AD_MIN], ad[AD_COUNT] = C, 0

    def _play_entry(self, b: int, rows: Dict[str, np.ndarray]) -> None:
        st, C = self.state[b], self.cfg.capacity
        h = int(st[ST_NEXT])
        i, j = h & (C - 1), (h + 1) & (C - 1)
        mask = int(st[ST_MASK]) & 0xFFFFFFFF
        if (mask >> i) & 1:
            mt = int(self.meta[b, i]) & 0xFFFFFFFF
            rows["packets"][b] = self.body[b, i]
            if mt & META_SID:
                rows["hold"][b] = HOLD_SID
                st[ST_IN_DTX] = 1
                st[STAT_NOISE] += 1
            else:
                rows["n"][b] = mt >> META_N_SHIFT
                st[ST_IN_DTX] = 0
                st[STAT_DECODED] += 1
            st[ST_MASK] = _i32(mask & ~(1 << i))
            self.meta[b, i] = 0
        elif st[ST_IN_DTX]:
            rows["hold"][b] = HOLD_SILENT
            st[STAT_NOISE] += 1
        else:
            mt = int(self.meta[b, j]) & 0xFFFFFFFF
            if self._fecable(b, j):
                rows["fec"][b] = 1
                rows["packets"][b] = self.body[b, j]
                rows["n"][b] = mt >> META_N_SHIFT
                st[STAT_FEC] += 1
            else:
                if self.conceal:
                    rows["lost"][b] = 1
                else:
                    rows["hold"][b] = HOLD_HELD
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
            if self.cfg.adapt is not None:
                self.adapt[b] = 0
        arrive = self._arrive if self.cfg.adapt is None else self._arrive_adapt
        for a in range(len(slots)):
            arrive(int(slots[a]), packets[a], int(nbytes[a]))
        for b in range(B):
            self._play(b, rows)
        return rows
