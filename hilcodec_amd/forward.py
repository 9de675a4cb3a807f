"""Selective forwarding of the graphed hops (graph_step.GraphedForwardHop): the definition, bit for bit, of hilc_forward_classify and
hilc_forward_route (csrc/forward.hip), and the only module that knows their rules.  Import it by name (`from hilcodec_amd import
forward`).

A conference through GraphedDecodeHop(mix=) and GraphedEncodeHop decodes and re-encodes every participant on every hop.  The residual
VQ allows a cheaper server: the first L stages of an n-stage packet are a valid L-stage encoding, and packets are stage-major, so
those stages are a bit prefix of the body (wire.py).  The forwarding hop takes each hop's arrivals of B participant slots and emits,
for every listener, the packets of its room's active other members, each cut to that listener's number of stages — without running the
model.  The receiving client is a GraphedDecodeHop(jitter=, mix=) that plays the few streams it is sent.

Trim rule (trim_packet, in `wire` functions only; a receiver of n_max stages, m redundant ones, comfort noise of order K):
1. hop, sid, fec, n, body = wire.parse_transport(packet, nbytes, T, n_max, m, K); it raises where that raises.
2. a SID is returned byte for byte.
3. keep = min(n, L): the primary is the first `keep` stages.
4. the redundant section survives only if fec and keep_fec and keep >= m (a receiver refuses the FEC flag with n < m).
5. the result is wire.pack_transport(hop, wire.pack_fec_packet(codes[:keep], red or None), keep, fec=red is not None): canonical, the
   pad bits of its last byte zero whatever the input's were.
In bits (trim_bits, the way the kernel cuts): behind the header, output bit i is source bit i while i < 10 keep T, source bit
i + 10 (n - keep) T while inside the redundant section, else 0; header byte 2 is rewritten.

Each slot is both a sender and a listener.  One hop's inputs: the arrivals in GraphedDecodeHop.play's record form (arrival_records:
grouped by slot, stable), room int32 [B] (-1: no room, else a room id in [0, B)), layers int32 [B] in [1, n], action int32 [B]
(non-zero: the slot was joined on this hop).

Sender rule (ForwardConfig(fanout, burst, hang_hops, keep_fec); hilc_forward_classify, per slot b):
1. action[b] != 0 clears the sender row.
2. the arrivals in push order.  Malformed (parse_transport raises for n_max = n, m, K): SD_MALFORMED += 1, nothing else.  Valid:
   SD_CODES or SD_SIDS += 1; the first `burst` valid arrivals are picked: pick[b][k] = their record index, pick_count[b] their number
   (pick is -1 behind it); each further valid arrival: SD_OVERFLOW += 1, not forwarded.
3. talk = a valid codes arrival was seen on this hop.
4. SD_HANG = hang_hops + 1 if talk, else max(SD_HANG - 1, 0).
5. SD_SINCE = min(SD_SINCE + 1, MAX_SINCE) if SD_HANG > 0 after the update, else 0.
Slots without a room are classified like any other slot.

Listener rule (hilc_forward_route, per slot b, after the sender rule has run for every slot):
1. action[b] != 0 clears the listener row: its routes become -1, its counters 0.
2. with r = room[b], the candidates are the slots t != b with room[t] == r >= 0 and SD_HANG[t] > 0, ordered by (SD_HANG descending,
   SD_SINCE descending, slot ascending); the selected set is the first min(fanout, count) of them; r < 0 selects nothing.
3. a route is freed (owner -1) when its owner is not selected or has action != 0 on this hop.  The selected slots without a route
   take the free routes: ascending slot order, lowest free route index first.  An owner keeps its route index while it stays selected.
4. new_routes[b][j] = 1 exactly on a hop where route j gets an owner that differs from the owner before this hop; LR_SWITCHES counts.
5. for route j with owner t and k < pick_count[t], output row (b, j, k) is trim_packet(arrival pick[t][k], L = layers[b] clamped to
   [1, n]), zero past its length, its byte count beside it; every other row is zero with count 0.
6. LR_PACKETS and LR_BYTES count the rows written and their bytes, LR_TRIMMED the packets whose n was cut.

Limits.  By these two rules alone, speaker selection rests on the senders' DTX: silence arrives as SIDs or as nothing.  Against
senders without DTX every member is always active and the earliest ones keep the routes: use fanout >= room size - 1 there, or the
senders' audio levels (below).  hang_hops should exceed the sender's DTX hang-over, so that the first SID of a silence is still
forwarded.

Feedback.  Answering listeners' NACKs from a history at the forwarder, per-listener byte budgets and deriving the layers from receiver
reports are downlink.py's (GraphedForwardHop(downlink=)): two further launches that read what these two wrote; `layers` stays the cap.

Senders without DTX.  Level-based selection is audio_level.py's (GraphedForwardHop(speakers=)): the senders say how loud each hop was,
one further launch between these two keeps a smoothed loudness per sender and hands hilc_forward_route shadow sender rows whose
(SD_HANG, SD_SINCE) order is the loudness order; the rules above stay what they are.

Protected calls.  SRTP hop by hop is forward_srtp.py's (GraphedForwardHop(srtp=)): hilc_srtp_unprotect in front of these two launches
hands them plain records (a rejected arrival is a record of 0 bytes: malformed by rule 2 of the sender rule), one launch behind
them protects every output row under its listener's key and its route's own SSRC; the rules above stay what they are.

Out of scope: re-stamping hop indices; more than one room per slot."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import wire
from .report import _check_ints

SD_HANG, SD_SINCE, SD_CODES, SD_SIDS, SD_MALFORMED, SD_OVERFLOW = range(6)
SD_WORDS = 6
SD_NAMES = ("hang", "since", "codes", "sids", "malformed", "overflow")

LR_PACKETS, LR_BYTES, LR_TRIMMED, LR_SWITCHES = range(4)
LR_WORDS = 4
LR_NAMES = ("packets", "bytes", "trimmed", "switches")

MAX_FANOUT, MAX_BURST, MAX_HANG_HOPS, MAX_SINCE = 8, 4, 255, 65535


@dataclass(frozen=True)
class ForwardConfig:
    """selective forwarding of a GraphedForwardHop (the rules: this module's docstring).  fanout in [1, 8]: the routes of one listener;
    burst in [1, 4]: the arrivals of one sender forwarded per hop; hang_hops in [0, 255]: the hops a sender stays active after its last
    codes packet; keep_fec: keep a packet's redundant section where the rules allow"""
    fanout: int = 3
    burst: int = 2
    hang_hops: int = 8
    keep_fec: bool = True

    def __post_init__(self):
        _check_ints("ForwardConfig", self, (("fanout", 1, MAX_FANOUT), ("burst", 1, MAX_BURST), ("hang_hops", 0, MAX_HANG_HOPS)))
        if not isinstance(self.keep_fec, (bool, np.bool_)):
            raise ValueError(f"ForwardConfig.keep_fec must be a bool, got {self.keep_fec!r}")


def trim_packet(packet, nbytes: int, L: int, T: int, n_max: int, m: int, K, keep_fec: bool) -> bytes:
    """the headed packet `packet[:nbytes]` cut to at most `L` stages (the trim rule of this module's docstring); ValueError where
    wire.parse_transport raises"""
    hop, sid, fec, n, body = wire.parse_transport(packet, nbytes, T, n_max, m, K)
    if sid:
        return bytes(packet[:int(nbytes)])
    if int(L) < 1:
        raise ValueError(f"trim_packet: L = {L} must be >= 1")
    keep = min(n, int(L))
    codes = wire.unpack_stream_packet(body, n + (int(m) if fec else 0), T)
    red = codes[n:] if fec and keep_fec and keep >= int(m) else None
    return wire.pack_transport(hop, wire.pack_fec_packet(codes[:keep], red), keep, fec=red is not None)


def trim_bits(row, L: int, T: int, m: int, keep_fec: bool) -> Tuple[np.ndarray, int]:
    """the kernel's cut of a valid headed packet `row` (uint8, its exact bytes): (the output bytes, their number).  Bytes 0-1 are copied,
    byte 2 is keep | FEC_BIT, and behind the header output bit i is source bit i for i < 10 keep T, source bit i + 10 (n - keep) T for
    10 keep T <= i < 10 (keep + m) T when the redundant section survives, else 0"""
    row = np.asarray(row, dtype=np.uint8)
    flags = int(row[2])
    if flags & wire.SID_BIT:
        return row.copy(), len(row)
    n, fec = flags & wire.N_MASK, bool(flags & wire.FEC_BIT)
    keep = min(n, int(L))
    red = fec and bool(keep_fec) and keep >= int(m)
    prim, shift = 10 * keep * T, 10 * (n - keep) * T
    end = prim + (10 * int(m) * T if red else 0)
    src = np.unpackbits(row[wire.TRANSPORT_HEADER:])
    body = (end + 7) // 8
    i = np.arange(8 * body)
    from_src = np.where(i < prim, i, i + shift)
    bits = np.where(i < end, src[np.minimum(from_src, len(src) - 1)], 0).astype(np.uint8)
    out = np.concatenate([row[:2], np.array([keep | (wire.FEC_BIT if red else 0)], dtype=np.uint8), np.packbits(bits)])
    return out, wire.TRANSPORT_HEADER + body


def arrival_records(slots, packets, nbytes, row_bytes: int, batch: int, max_arrivals: Optional[int] = None):
    """one hop's arrivals in push order -> the record form GraphedDecodeHop.play stages: (records int32 [max_arrivals, 1 + ceil(row_bytes
    / 4)]: byte count, then the headed packet; grouped by slot, stable) and (offsets int32 [batch + 1])"""
    sl = np.asarray(slots, dtype=np.int64).reshape(-1)
    A = len(sl)
    aw = 1 + (int(row_bytes) + 3) // 4
    rec = np.zeros((A if max_arrivals is None else int(max_arrivals), aw), dtype=np.int32)
    order = np.argsort(sl, kind="stable")
    offs = np.zeros(int(batch) + 1, dtype=np.int32)
    offs[1:] = np.cumsum(np.bincount(sl, minlength=int(batch)))
    if A:
        rec[:A, 0] = np.clip(np.asarray(nbytes, dtype=np.int64).reshape(-1)[order], -1, 1 << 20)
        rec.view(np.uint8)[:A, 4:4 + row_bytes] = np.asarray(packets, dtype=np.uint8).reshape(A, row_bytes)[order]
    return rec, offs


class _Shape:
    def __init__(self, batch: int, cfg: ForwardConfig, n: int, T: int, m: int = 0, K=None):
        self.B, self.cfg, self.n, self.T, self.m, self.K = int(batch), cfg, int(n), int(T), int(m), K
        if self.B < 1 or self.T < 1 or not 1 <= self.n <= 31 or not 0 <= self.m <= self.n or self.n + self.m > wire.MAX_STAGES:
            raise ValueError(f"forward: batch = {batch}, n = {n}, T = {T}, m = {m} outside what a headed packet holds")
        self.tb = wire.transport_bytes(self.n, self.m, self.T)

    def _packet(self, rec, a: int):
        """(the bytes, the byte count) of record a"""
        return rec[a].view(np.uint8)[4:4 + self.tb], int(rec[a, 0])


class SenderModel(_Shape):
    """numpy statement of hilc_forward_classify for `batch` slots.  `state` int32 [B, SD_WORDS] are the kernel's sender rows."""

    def __init__(self, batch: int, cfg: ForwardConfig, n: int, T: int, m: int = 0, K=None):
        super().__init__(batch, cfg, n, T, m, K)
        self.state = np.zeros((self.B, SD_WORDS), dtype=np.int32)

    def step(self, records, offsets, action) -> Dict[str, np.ndarray]:
        """one hop: `records`, `offsets` (arrival_records) and `action` int [B] -> pick (int32 [B, burst]) and pick_count (int32
        [B]); `state` is updated in place"""
        rec = np.ascontiguousarray(records, dtype=np.int32)
        offs = np.clip(np.asarray(offsets, dtype=np.int64), 0, len(rec))
        action = np.asarray(action).reshape(-1)
        pick = np.full((self.B, self.cfg.burst), -1, dtype=np.int32)
        count = np.zeros(self.B, dtype=np.int32)
        for b in range(self.B):
            row = self.state[b]
            if action[b] != 0:
                row[:] = 0
            talk = False
            for a in range(int(offs[b]), int(max(offs[b], offs[b + 1]))):
                data, nb = self._packet(rec, a)
                try:
                    _hop, sid, _fec, _n, _body = wire.parse_transport(data, nb, self.T, self.n, self.m, self.K)
                except ValueError:
                    row[SD_MALFORMED] += 1
                    continue
                row[SD_SIDS if sid else SD_CODES] += 1
                talk = talk or not sid
                if count[b] < self.cfg.burst:
                    pick[b, count[b]] = a
                    count[b] += 1
                else:
                    row[SD_OVERFLOW] += 1
            row[SD_HANG] = self.cfg.hang_hops + 1 if talk else max(int(row[SD_HANG]) - 1, 0)
            row[SD_SINCE] = min(int(row[SD_SINCE]) + 1, MAX_SINCE) if row[SD_HANG] > 0 else 0
        return {"pick": pick, "pick_count": count}


class ListenerModel(_Shape):
    """numpy statement of hilc_forward_route for `batch` slots.  `routes` int32 [B, fanout] are the routes' owners (-1: free), `state`
    int32 [B, LR_WORDS] the kernel's listener rows."""

    def __init__(self, batch: int, cfg: ForwardConfig, n: int, T: int, m: int = 0, K=None):
        super().__init__(batch, cfg, n, T, m, K)
        self.routes = np.full((self.B, cfg.fanout), -1, dtype=np.int32)
        self.state = np.zeros((self.B, LR_WORDS), dtype=np.int32)

    def step(self, records, action, room, layers, sender_state, pick, pick_count) -> Dict[str, np.ndarray]:
        """one hop: `records` (arrival_records), `action`, `room`, `layers` int [B], and `sender_state`, `pick`, `pick_count` as the
        sender rule of this hop left them -> out (uint8 [B, fanout, burst, tb]), out_nbytes (int32 [B, fanout, burst]), routes and
        new_routes (int32 [B, fanout]); `routes` and `state` are updated in place"""
        c, B, F, P = self.cfg, self.B, self.cfg.fanout, self.cfg.burst
        rec = np.ascontiguousarray(records, dtype=np.int32)
        action, room, layers = (np.asarray(v).reshape(-1) for v in (action, room, layers))
        sd = np.asarray(sender_state).reshape(B, SD_WORDS)
        out = np.zeros((B, F, P, self.tb), dtype=np.uint8)
        out_nbytes = np.zeros((B, F, P), dtype=np.int32)
        new_routes = np.zeros((B, F), dtype=np.int32)
        for b in range(B):
            row, routes = self.state[b], self.routes[b]
            if action[b] != 0:
                row[:] = 0
                routes[:] = -1
            before = routes.copy()
            r = int(room[b])
            cands = [t for t in range(B) if t != b and r >= 0 and int(room[t]) == r and sd[t, SD_HANG] > 0]
            cands.sort(key=lambda t: (-int(sd[t, SD_HANG]), -int(sd[t, SD_SINCE]), t))
            selected = set(cands[:F])
            for j in range(F):
                if routes[j] >= 0 and (int(routes[j]) not in selected or action[routes[j]] != 0):
                    routes[j] = -1
            fresh = sorted(selected - {int(t) for t in routes if t >= 0})
            for j in range(F):
                if routes[j] < 0 and fresh:
                    routes[j] = fresh.pop(0)
            L = min(max(int(layers[b]), 1), self.n)
            for j in range(F):
                t = int(routes[j])
                if t >= 0 and t != before[j]:
                    new_routes[b, j] = 1
                    row[LR_SWITCHES] += 1
                if t < 0:
                    continue
                for k in range(min(int(pick_count[t]), P)):
                    data, nb = self._packet(rec, int(pick[t, k]))
                    cut, length = trim_bits(data[:nb], L, self.T, self.m, c.keep_fec)
                    out[b, j, k, :length] = cut
                    out_nbytes[b, j, k] = length
                    row[LR_PACKETS] += 1
                    row[LR_BYTES] += length
                    row[LR_TRIMMED] += int(not data[2] & wire.SID_BIT and (int(data[2]) & wire.N_MASK) > L)
        return {"out": out, "out_nbytes": out_nbytes, "routes": self.routes.copy(), "new_routes": new_routes}


class ForwardModel(_Shape):
    """SenderModel then ListenerModel: one GraphedForwardHop of `batch` slots with n stages, T frames, m redundant stages and comfort
    noise of order K (None: SIDs are malformed)"""

    def __init__(self, batch: int, cfg: ForwardConfig, n: int, T: int, m: int = 0, K=None):
        super().__init__(batch, cfg, n, T, m, K)
        self.sender = SenderModel(batch, cfg, n, T, m, K)
        self.listener = ListenerModel(batch, cfg, n, T, m, K)

    def step_records(self, records, offsets, action, room, layers) -> Dict[str, np.ndarray]:
        """one hop on staged arrivals (arrival_records): everything both kernels write"""
        res = self.sender.step(records, offsets, action)
        res.update(self.listener.step(records, action, room, layers, self.sender.state, res["pick"], res["pick_count"]))
        return res

    def step(self, slots, packets, nbytes, room, layers, action=None) -> Dict[str, np.ndarray]:
        """one hop: this hop's arrivals in push order (`slots`, `nbytes`: A ints; `packets` uint8 [A, tb]), `room`, `layers` int [B] and
        `action` int [B] (None: zeros) -> out, out_nbytes, routes, new_routes, pick, pick_count"""
        rec, offs = arrival_records(slots, packets, nbytes, self.tb, self.B)
        return self.step_records(rec, offs, np.zeros(self.B, dtype=np.int32) if action is None else action, room, layers)
