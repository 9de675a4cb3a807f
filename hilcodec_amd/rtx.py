"""NACK and retransmission of the graphed hops (graph_step.GraphedDecodeHop(nack=NackConfig(...)), GraphedEncodeHop(rtx=RtxConfig(...))):
the definition, bit for bit, of hilc_nack_build and hilc_rtx_step (csrc/rtx.hip), and the only module that knows their rules.  Import
it by name (`from hilcodec_amd import rtx`).

The receiver's jitter buffer keeps D hops of delay per slot, and the 16-bit hop index of the transport header tells it which hops
are missing while there is still time to fetch them.  hilc_nack_build reads each slot's ring after the jitter step and emits a 4-byte
negative acknowledgement (wire.pack_nack: base, bitmap) that a bridge sends back to the client beside the media; the sender keeps a
history of the headed packets it sent, takes the NACKs it was given with a hop (`step(x, nacks=(slots, blobs))`) and hilc_rtx_step
copies the packets asked for into `per_hop` output rows.  A retransmission is the packet that was sent, byte for byte, and reaches the
receiver as an ordinary `play()` arrival: hilc_jitter_step sorts it into the ring like any late, reordered or duplicated packet.

Receiver rule (NackConfig(rtt_hops, retry_hops, max_requests, skip_fecable); per slot and hop, after the jitter step of that hop;
it reads the slot's jitter state row and the ring's meta words only; C = the ring's capacity, m = the receiver's fec_stages):
1. action != 0 (a start or a resume on this hop) clears the NACK row, the slot's NACK bytes and its due flag.
2. due = 0.  A slot that is not anchored does nothing more.  The hold row is not read: arrivals are taken while playout pauses, so
   holes are still worth asking for.
3. housekeeping.  With next = ST_NEXT (already advanced by this hop's play), every entry word with count > 0, d = int16(h - next):
   0 <= d < C and ring entry h mod C occupied: NK_RECOVERED += 1 and the word is freed; d < 0 or d >= C: NK_EXPIRED += 1 and the word
   is freed.  (The window is tested first: outside it the ring entry h mod C belongs to another hop.  A retransmission that arrives
   on the very hop that plays it is decoded, but its entry is gone when this rule runs: it counts EXPIRED.)
4. top = the largest d in [0, C) whose ring entry (next + d) mod C is occupied.  None: the rule ends (a tail loss shows only when a
   later packet arrives).
5. a hole is an unoccupied d in [0, top).  It is skipped when d + 1 < rtt_hops (a request made now is answered among the arrivals of
   the play call rtt_hops later, which plays next + rtt_hops - 1: the hop would come too late); when it lies in a silent stretch (the
   nearest occupied entry below it in the window is a SID, or there is none below it and ST_IN_DTX is set: DTX sends nothing there);
   or when skip_fecable is set, m >= 1 and entry d + 1 is a codes packet with the FEC flag (the jitter buffer repairs it).  A hole
   that is not skipped is eligible when its word is free, or when its age >= retry_hops and its count < max_requests.
6. the eligible holes are taken in increasing d: the first gives base = (next + d) mod 2^16, the others go into the bitmap when they
   lie at most 16 above base (C <= 32: a further one waits for a later hop and is not marked).  Every hole taken sets its word to
   h | (count + 1) << 16 with age 0 and NK_ASKED += 1; every other hole whose word has count > 0 ages by one, saturating at 255.  If
   any hole was taken the slot's NACK bytes become wire.pack_nack(base, bitmap), due = 1 and NK_SENT += 1; else they stay.
NACK row (int32, NK_WORDS words): the counters NK_SENT, NK_ASKED, NK_RECOVERED, NK_EXPIRED (NK_NAMES), then NK_RING_WORDS entry words
from NK_RING, indexed like the jitter ring by h mod C (those past C stay 0): h | count << 16 | age << 24, 0 when free.

Sender rule (RtxConfig(history=R, per_hop); per slot and hop, the sender graph's last launch, after hilc_packet_header; a headed row
is tb = wire.transport_bytes(n, m, T) bytes):
1. action != 0 empties the slot's tags.  The counters stay.
2. nbytes[b] > 0 on this hop: the packet is stored at entry h mod R, h read from the packet's own bytes 0-1: the row zero past its
   min(nbytes, tb) bytes, the tag h | nbytes << 16, RX_STORED += 1.  Held, stopped and DTX-SILENT hops send nothing and store
   nothing; a SID is stored like any packet.
3. a NACK for the slot on this hop (held and stopped slots answer theirs too): RX_REQUESTS += 1, and its hops in wire.nack_hops
   order: a hop whose tag at h mod R is not 0 and carries h goes to the next free output row q < per_hop, byte for byte with its
   nbytes, RX_SENT += 1; a matching hop after the rows are full: RX_DROPPED += 1; a hop that is not in the history (never sent, sent
   before a start, or overwritten R hops later: the tag does not match, so a stale hop is never sent): RX_MISS += 1.
4. the output rows not used are zero with nbytes 0.
State per slot: the ring of R rows, one tag word per entry (0: empty) and the counter row (int32, RX_WORDS words): RX_STORED,
RX_REQUESTS, RX_SENT, RX_MISS, RX_DROPPED (RX_NAMES).

A NACK travels to the sender's graph as two int32 words per slot (nack_words): NACK_PRESENT | base and bitmap, (0, 0) for none.

Two properties of the loop.  A retransmission that still arrives too late is an ordinary LATE arrival: with JitterConfig(adapt=...)
it counts towards the adaptive clock like any other late packet (the jitter rules are unchanged).  A retransmission is not charged
to VBR's token bucket: the bucket meters what the encoder produces, and hilc_rtx_step runs behind it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from . import wire
from .jitter import META_FEC, META_SID, ST_ANCHORED, ST_IN_DTX, ST_MASK, ST_NEXT, ST_WORDS
from .report import _check_ints

NK_SENT, NK_ASKED, NK_RECOVERED, NK_EXPIRED, NK_RING = range(5)
NK_RING_WORDS = 32                                   # the widest jitter ring
NK_WORDS = NK_RING + NK_RING_WORDS
NK_NAMES = ("sent", "asked", "recovered", "expired")

RX_STORED, RX_REQUESTS, RX_SENT, RX_MISS, RX_DROPPED = range(5)
RX_WORDS = 5
RX_NAMES = ("stored", "requests", "sent", "miss", "dropped")

NACK_PRESENT = 1 << 16
MAX_HISTORY, MAX_PER_HOP = 64, 4


@dataclass(frozen=True)
class NackConfig:
    """NACKs of a GraphedDecodeHop (the rules: this module's docstring).  rtt_hops in [1, 30]: the play calls between a request and
    its answer's arrival; retry_hops in [1, 255]: the hops a request waits before it is repeated; max_requests in [1, 255]: the
    requests one hop gets at most; skip_fecable: leave a hole alone that the next packet's redundant section repairs"""
    rtt_hops: int = 2
    retry_hops: int = 3
    max_requests: int = 2
    skip_fecable: bool = False

    def __post_init__(self):
        _check_ints("NackConfig", self, (("rtt_hops", 1, 30), ("retry_hops", 1, 255), ("max_requests", 1, 255)))
        if not isinstance(self.skip_fecable, (bool, np.bool_)):
            raise ValueError(f"NackConfig.skip_fecable must be a bool, got {self.skip_fecable!r}")


@dataclass(frozen=True)
class RtxConfig:
    """retransmission history of a GraphedEncodeHop (the rules: this module's docstring).  history R: the headed packets kept per
    slot, a power of two in [2, 64]; per_hop in [1, 4]: the retransmissions one slot sends per hop at most"""
    history: int = 16
    per_hop: int = 2

    def __post_init__(self):
        _check_ints("RtxConfig", self, (("history", 2, MAX_HISTORY), ("per_hop", 1, MAX_PER_HOP)))
        if int(self.history) & (int(self.history) - 1):
            raise ValueError(f"RtxConfig.history = {self.history}: a power of two in [2, {MAX_HISTORY}]")


def nack_words(base: int, bitmap: int) -> Tuple[int, int]:
    """the two int32 words that carry one NACK to the sender's graph"""
    return NACK_PRESENT | (int(base) & 0xFFFF), int(bitmap) & 0xFFFF


def _i16(v: int) -> int:
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


class NackModel:
    """numpy statement of hilc_nack_build for `batch` slots of a receiver with a jitter ring of `capacity` entries and m =
    `fec_stages` redundant stages.  `state` int32 [B, NK_WORDS] are the kernel's NACK rows, `nacks` uint8 [B, 4] each slot's latest
    NACK and `due` int32 [B] the flags of the last step."""

    def __init__(self, batch: int, cfg: NackConfig, capacity: int, fec_stages: int = 0):
        self.B, self.cfg, self.C, self.m = int(batch), cfg, int(capacity), int(fec_stages)
        if not 2 <= self.C <= NK_RING_WORDS or self.C & (self.C - 1):
            raise ValueError(f"NackModel: capacity = {capacity}: a power of two in [2, {NK_RING_WORDS}]")
        self.state = np.zeros((self.B, NK_WORDS), dtype=np.int32)
        self.nacks = np.zeros((self.B, wire.NACK_BYTES), dtype=np.uint8)
        self.due = np.zeros(self.B, dtype=np.int32)

    def step(self, jitter_state, meta, action) -> Dict[str, np.ndarray]:
        """one hop: `jitter_state` int [B, jitter.ST_WORDS] and `meta` int [B, C] as the jitter step of this hop left them, `action`
        int [B] -> the rows the kernel writes: nacks (uint8 [B, 4]) and due (int32 [B]); `state` is updated in place"""
        C, c = self.C, self.cfg
        js = np.asarray(jitter_state).reshape(self.B, ST_WORDS)
        meta = np.asarray(meta).reshape(self.B, C)
        action = np.asarray(action).reshape(-1)
        for b in range(self.B):
            row = self.state[b]
            if action[b] != 0:
                row[:] = 0
                self.nacks[b] = 0
            self.due[b] = 0
            if not js[b, ST_ANCHORED]:
                continue
            nxt, mask = int(js[b, ST_NEXT]) & 0xFFFF, int(js[b, ST_MASK]) & 0xFFFFFFFF
            occ = [bool((mask >> ((nxt + d) & (C - 1))) & 1) for d in range(C)]
            mt = [int(meta[b, (nxt + d) & (C - 1)]) & 0xFFFFFFFF for d in range(C)]
            words = row[NK_RING:NK_RING + C]
            for i in range(C):
                w = int(words[i]) & 0xFFFFFFFF
                if (w >> 16) & 255:
                    d = _i16((w & 0xFFFF) - nxt)
                    if 0 <= d < C:
                        if (mask >> i) & 1:
                            row[NK_RECOVERED] += 1
                            words[i] = 0
                    else:
                        row[NK_EXPIRED] += 1
                        words[i] = 0
            if not any(occ):
                continue
            top = max(d for d in range(C) if occ[d])
            holes, eligible = [], []
            for d in range(top):
                if occ[d]:
                    continue
                holes.append(d)
                below = [e for e in range(d) if occ[e]]
                silent = bool(mt[below[-1]] & META_SID) if below else bool(js[b, ST_IN_DTX])
                fecable = bool(c.skip_fecable and self.m >= 1 and occ[d + 1] and not mt[d + 1] & META_SID and mt[d + 1] & META_FEC)
                if d + 1 < c.rtt_hops or silent or fecable:
                    continue
                w = int(words[(nxt + d) & (C - 1)]) & 0xFFFFFFFF
                count, age = (w >> 16) & 255, w >> 24
                if count == 0 or (age >= c.retry_hops and count < c.max_requests):
                    eligible.append(d)
            taken = [d for d in eligible if d - eligible[0] <= 16]
            for d in holes:
                i = (nxt + d) & (C - 1)
                w = int(words[i]) & 0xFFFFFFFF
                count, age = (w >> 16) & 255, w >> 24
                if d in taken:
                    words[i] = _i32(((nxt + d) & 0xFFFF) | (count + 1) << 16)
                    row[NK_ASKED] += 1
                elif count:
                    words[i] = _i32((w & 0xFFFFFF) | min(age + 1, 255) << 24)
            if taken:
                base = (nxt + taken[0]) & 0xFFFF
                bitmap = sum(1 << (d - taken[0] - 1) for d in taken[1:])
                self.nacks[b] = np.frombuffer(wire.pack_nack(base, bitmap), dtype=np.uint8)
                self.due[b] = 1
                row[NK_SENT] += 1
        return {"nacks": self.nacks.copy(), "due": self.due.copy()}


class RtxModel:
    """numpy statement of hilc_rtx_step for `batch` slots of a sender whose headed rows are `row_bytes` = wire.transport_bytes(n, m,
    T) bytes.  `ring` uint8 [B, R, row_bytes] and `tags` int32 [B, R] are the history, `state` int32 [B, RX_WORDS] the counter rows."""

    def __init__(self, batch: int, cfg: RtxConfig, row_bytes: int):
        self.B, self.cfg, self.tb = int(batch), cfg, int(row_bytes)
        if self.tb <= wire.TRANSPORT_HEADER:
            raise ValueError(f"RtxModel: row_bytes = {row_bytes} holds no packet")
        self.ring = np.zeros((self.B, cfg.history, self.tb), dtype=np.uint8)
        self.tags = np.zeros((self.B, cfg.history), dtype=np.int32)
        self.state = np.zeros((self.B, RX_WORDS), dtype=np.int32)

    def step(self, packets, nbytes, nacks=None, action=None) -> Dict[str, np.ndarray]:
        """one hop: `packets` uint8 [B, row_bytes] and `nbytes` int [B] as hilc_packet_header left them, `nacks` int [B, 2] (nack_words
        per slot, (0, 0): none; None: none at all), `action` int [B] (None: zeros) -> packets (uint8 [B, per_hop, row_bytes]) and nbytes
        (int32 [B, per_hop]): the retransmissions of this hop; the history and `state` are updated in place"""
        B, R, P, tb = self.B, self.cfg.history, self.cfg.per_hop, self.tb
        packets = np.asarray(packets, dtype=np.uint8).reshape(B, tb)
        nbytes = np.asarray(nbytes, dtype=np.int64).reshape(-1)
        nacks = np.zeros((B, 2), dtype=np.int64) if nacks is None else np.asarray(nacks, dtype=np.int64).reshape(B, 2)
        action = np.zeros(B, dtype=np.int64) if action is None else np.asarray(action).reshape(-1)
        out = np.zeros((B, P, tb), dtype=np.uint8)
        out_nbytes = np.zeros((B, P), dtype=np.int32)
        for b in range(B):
            row = self.state[b]
            if action[b] != 0:
                self.tags[b] = 0
            nb = min(int(nbytes[b]), tb)
            if nb > 0:
                h = (int(packets[b, 0]) << 8) | int(packets[b, 1])
                e = h & (R - 1)
                self.ring[b, e] = 0
                self.ring[b, e, :nb] = packets[b, :nb]
                self.tags[b, e] = h | nb << 16
                row[RX_STORED] += 1
            word, bitmap = int(nacks[b, 0]), int(nacks[b, 1]) & 0xFFFF
            if word & NACK_PRESENT:
                row[RX_REQUESTS] += 1
                q = 0
                for h in wire.nack_hops(word & 0xFFFF, bitmap):
                    tag = int(self.tags[b, h & (R - 1)])
                    if tag == 0 or tag & 0xFFFF != h:
                        row[RX_MISS] += 1
                    elif q >= P:
                        row[RX_DROPPED] += 1
                    else:
                        out[b, q] = self.ring[b, h & (R - 1)]
                        out_nbytes[b, q] = tag >> 16
                        row[RX_SENT] += 1
                        q += 1
        return {"packets": out, "nbytes": out_nbytes}
