"""SRTP on the selective forwarding hop (graph_step.GraphedForwardHop(srtp=SrtpConfig())): the definition, bit for bit, of
hilc_srtp_protect_routes (csrc/srtp.hip), and the only module that knows its rules.  Import it by name (`from hilcodec_amd import
forward_srtp`).  The primitives — the transform, key rows, KeyTable, protect_packet, unprotect_packet — are srtp.py's and are not
restated here.

The forwarder parses headers and cuts packets to a listener's layers, so it cannot pass ciphertext through: SRTP runs hop by hop.
Arrivals are protected under each sender's uplink key and are unprotected on ingress; the rows a listener is sent are protected again
under that listener's downlink key.

Keys.  Two srtp.KeyTables: an uplink key per slot (what that participant's GraphedEncodeHop(srtp=) protects with) and a downlink key
per slot (one per listener, shared by its routes).

Route SSRC.  A listener's F routes share one key, and a forwarded packet keeps its sender's hop index as SEQ, so two routes, or two
successive owners of one route, would meet the same (key, SSRC, index): a two-time pad.  Each route therefore runs under its own
SSRC, which changes whenever the stream on it restarts: route_ssrc(base, route, epoch) = (base + forward.MAX_FANOUT epoch + route)
mod 2^32, with `base` the downlink key row's KEY_SSRC and `epoch` a per-(listener, route) counter on the device.  The transport header
carries no SSRC, so the epoch is signalled to the client like `new_routes` is (GraphedForwardHop.route_epoch): whenever the epoch of
route j differs from the one the client has, it calls set_key(j, master_key, master_salt, ssrc=route_ssrc(base, j, epoch)) and
start(j) on its GraphedDecodeHop(srtp=) in front of that hop's rows.  srtp.KeyTable takes the same master key under a new SSRC as a
fresh key.

Route row, int32 [B, fanout, RT_WORDS]: RT_EPOCH; the index state RT_ROC, RT_SL (the SEQ of the highest index sent), RT_SEEN (0: nothing
sent since the restart, 1: sent, SEEN_EXHAUSTED: see rule 4), RT_WIN_LO, RT_WIN_HI (bit k of the 64: the index k below the highest
one sent has been sent); then the counters RT_PROTECTED, RT_NOKEY, RT_STALE, RT_EXHAUSTED.

Egress rule (hilc_srtp_protect_routes; per listener b and route j, over the hop's final rows (b, j, k) in k order — the route
launch's, or hilc_downlink_step's with downlink= — and t = routes[b][j] after the route launch):
1. restart: new_routes[b][j], action[b], rekey_down[b] (b was given a downlink key for this hop) or, with 0 <= t < B, action[t] or
   rekey_up[t] (t was given an uplink key: its stream restarts at SEQ 0) non-zero: RT_EPOCH += 1 while it is below MAX_EPOCH; RT_ROC,
   RT_SL, RT_SEEN and the window are cleared.  Counters and epoch survive everything but reset().
2. nb = min(nbytes, row bytes).  nb < 3 (no packet): the output row is zero with count 0, nothing else moves.
3. without a valid downlink key: zero row, count 0, RT_NOKEY += 1.  Plaintext never leaves a keyed hop.
4. a restart at RT_EPOCH = MAX_EPOCH finds no SSRC left: the epoch stays and RT_SEEN becomes SEEN_EXHAUSTED, which no later restart
   leaves.  Every row of such a route: zero row, count 0, RT_EXHAUSTED += 1.
5. otherwise the index is estimated as srtp.py's receiver rule does it (its steps 2, 3 and 5) on (RT_SL, RT_ROC, RT_SEEN, window): v
   from RFC 3711 3.3.1, the first packet since the restart taking v = RT_ROC; v = -1, an index more than 63 below the highest sent,
   or an index whose window bit is set: not sent — zero row, count 0, RT_STALE += 1.  An accepted index moves the highest index and
   the window as the receiver's would.  So "no (key, SSRC, index) is encrypted twice" is a property of the route row itself, whatever
   order, repetition or owner change the arrivals had, and the client's own estimate of v agrees with the one used here.
6. the row goes out as srtp.protect_packet(the downlink key row with SSRC = route_ssrc(KEY_SSRC, j, RT_EPOCH), row[:nb], v): nb + 10
   bytes, zero past them; RT_PROTECTED += 1.
hilc_srtp_protect's sender rule ("SEQ < last SEQ: the counter wrapped") is not used: it holds for a sender that emits its own hops in
order, not for a relay of arrivals.

Ingress.  hilc_srtp_unprotect (srtp.ReceiverModel, unchanged) is the graph's first launch, on the arrival region widened by 10 bytes,
into a device-only plain buffer that every later launch reads.  Its clear row is rekey_up: an RX row lives as long as its key, so a
join under the same key does not reopen the replay window.  A rejected arrival becomes a record of 0 bytes, which
hilc_forward_classify counts as SD_MALFORMED.

Not covered: NACK answers (downlink.history > 0 raises with srtp=: an answer is cut again at answer time, so it could put other
plaintext under an index already used; a per-route history of ciphertext is the follow-up), SRTCP, key exchange, re-stamping hop
indices, the timing of table lookups on a GPU that others share."""
from __future__ import annotations

import hashlib
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import audio_level as level_def
from . import downlink as downlink_def
from . import forward as forward_def
from . import srtp as srtp_def
from . import wire

RT_EPOCH, RT_ROC, RT_SL, RT_SEEN, RT_WIN_LO, RT_WIN_HI, RT_PROTECTED, RT_NOKEY, RT_STALE, RT_EXHAUSTED = range(10)
RT_WORDS = 10
RT_NAMES = ("protected", "nokey", "stale", "exhausted")

SEEN_EXHAUSTED = 2
MAX_EPOCH = (1 << 28) - 1


def route_ssrc(base: int, route: int, epoch: int) -> int:
    """the SSRC of route `route` of a listener whose downlink key has SSRC `base`, in the route's epoch `epoch`"""
    return (int(base) + forward_def.MAX_FANOUT * int(epoch) + int(route)) & 0xFFFFFFFF


class ForwardKeys:
    """the host's side of a protected forwarder's keys: the uplink table `up` and the downlink table `down` (srtp.KeyTable each) and
    the slots given a key since the last hop, which `take` turns into that hop's one-hop rows rekey_up / rekey_down.  A key serves
    one stream: each set counts as that key's start, so KeyTable refuses a key the slot had before."""

    def __init__(self, batch: int):
        self.B = int(batch)
        self.up, self.down = srtp_def.KeyTable(self.B), srtp_def.KeyTable(self.B)
        self._rekeyed: Tuple[set, set] = (set(), set())

    def reset(self) -> None:
        self.up.reset()
        self.down.reset()
        self._rekeyed = (set(), set())

    def _set(self, which: int, slot, master_key, master_salt, ssrc, roc) -> None:
        table = (self.up, self.down)[which]
        table.set_key(slot, master_key, master_salt, ssrc, roc)
        table.started(slot)
        self._rekeyed[which].add(int(slot))

    def set_uplink_key(self, slot, master_key, master_salt, ssrc: Optional[int] = None, roc: int = 0) -> None:
        self._set(0, slot, master_key, master_salt, ssrc, roc)

    def set_downlink_key(self, slot, master_key, master_salt, ssrc: Optional[int] = None) -> None:
        self._set(1, slot, master_key, master_salt, ssrc, 0)

    def clear_keys(self, slot) -> None:
        self.up.clear_key(slot)
        self.down.clear_key(slot)

    @property
    def pending(self) -> bool:
        return bool(self._rekeyed[0] or self._rekeyed[1])

    def take(self) -> Tuple[List[int], List[int]]:
        """the slots given an uplink / a downlink key since the last call, sorted; forgets them"""
        up, down = sorted(self._rekeyed[0]), sorted(self._rekeyed[1])
        self._rekeyed = (set(), set())
        return up, down

    def __repr__(self):
        return f"ForwardKeys(up={self.up!r}, down={self.down!r})"


def _flags(B: int, v) -> np.ndarray:
    return np.zeros(B, dtype=np.int64) if v is None else np.asarray(v).reshape(-1)


def _marks(B: int, slots) -> np.ndarray:
    row = np.zeros(B, dtype=np.int32)
    row[list(slots)] = 1
    return row


class RouteModel:
    """numpy statement of hilc_srtp_protect_routes for `batch` listeners of `fanout` routes and `burst` rows each, whose plain rows are
    `row_bytes` = wire.transport_bytes(n, m, T) bytes.  `keys` (a srtp.KeyTable) holds the downlink key rows, `state` int32 [B, fanout,
    RT_WORDS] the kernel's route rows.  `sent`: None, or a list that takes (digest of the key material, SSRC, index) of every row
    protected."""

    def __init__(self, batch: int, fanout: int, burst: int, row_bytes: int):
        self.B, self.F, self.P, self.tb = int(batch), int(fanout), int(burst), int(row_bytes)
        if not 1 <= self.F <= forward_def.MAX_FANOUT or not 1 <= self.P <= forward_def.MAX_BURST:
            raise ValueError(f"forward_srtp.RouteModel: fanout = {fanout}, burst = {burst} outside [1, {forward_def.MAX_FANOUT}] and "
                             f"[1, {forward_def.MAX_BURST}]")
        if not wire.TRANSPORT_HEADER < self.tb <= srtp_def.MAX_ROW_BYTES:
            raise ValueError(f"forward_srtp.RouteModel: row_bytes = {row_bytes} outside ({wire.TRANSPORT_HEADER}, {srtp_def.MAX_ROW_BYTES}]")
        self.keys = srtp_def.KeyTable(self.B)
        self.state = np.zeros((self.B, self.F, RT_WORDS), dtype=np.int32)
        self.sent: Optional[list] = None

    def _admit(self, row, seq: int) -> Optional[int]:
        """rule 5 on one route row: the rollover counter the index is sent under (the row moves), or None (refused, the row stays)"""
        roc, s_l, seen = srtp_def._u32(row[RT_ROC]), int(row[RT_SL]) & 0xFFFF, row[RT_SEEN] == 1
        if not seen:
            v = roc
        elif s_l < 32768:
            v = roc - 1 if seq - s_l > 32768 else roc
        else:
            v = (roc + 1) & 0xFFFFFFFF if s_l - 32768 > seq else roc
        if v < 0:
            return None
        window = srtp_def._u32(row[RT_WIN_LO]) | srtp_def._u32(row[RT_WIN_HI]) << 32
        delta = ((v << 16) | seq) - ((roc << 16) | s_l) if seen else 1
        if delta <= 0 and (-delta >= srtp_def.WINDOW or (window >> -delta) & 1):
            return None
        if delta > 0:
            window = 1 if not seen or delta >= srtp_def.WINDOW else ((window << delta) | 1) & ((1 << srtp_def.WINDOW) - 1)
            row[RT_SL], row[RT_ROC], row[RT_SEEN] = seq, srtp_def._i32(v), 1
        else:
            window |= 1 << -delta
        row[RT_WIN_LO], row[RT_WIN_HI] = srtp_def._i32(window), srtp_def._i32(window >> 32)
        return v

    def protect(self, rows, nbytes, routes, new_routes, action=None, rekey_up=None, rekey_down=None) -> Dict[str, np.ndarray]:
        """one hop: the final `rows` uint8 [B, fanout, burst, row_bytes] and `nbytes` int [B, fanout, burst], `routes` and `new_routes`
        int [B, fanout] as the route launch left them, `action`, `rekey_up`, `rekey_down` int [B] (None: zeros) -> out (uint8 [B,
        fanout, burst, row_bytes + 10]) and out_nbytes (int32 [B, fanout, burst]); `state` is updated in place"""
        B, F, P, tb = self.B, self.F, self.P, self.tb
        rows = np.asarray(rows, dtype=np.uint8).reshape(B, F, P, tb)
        nbytes = np.asarray(nbytes, dtype=np.int64).reshape(B, F, P)
        routes, new_routes = np.asarray(routes).reshape(B, F), np.asarray(new_routes).reshape(B, F)
        action, rekey_up, rekey_down = _flags(B, action), _flags(B, rekey_up), _flags(B, rekey_down)
        out = np.zeros((B, F, P, tb + srtp_def.TAG_BYTES), dtype=np.uint8)
        out_nbytes = np.zeros((B, F, P), dtype=np.int32)
        for b in range(B):
            key = self.keys.rows[b]
            valid = key[srtp_def.KEY_VALID] != 0
            digest = hashlib.sha256(key[srtp_def.KEY_RK:].tobytes()).digest() if self.sent is not None else None
            for j in range(F):
                row, t = self.state[b, j], int(routes[b, j])
                restart = new_routes[b, j] != 0 or action[b] != 0 or rekey_down[b] != 0
                if 0 <= t < B:
                    restart = restart or action[t] != 0 or rekey_up[t] != 0
                if restart:
                    if row[RT_EPOCH] < MAX_EPOCH:
                        row[RT_EPOCH] += 1
                        row[RT_SEEN] = 0
                    else:
                        row[RT_SEEN] = SEEN_EXHAUSTED
                    row[RT_ROC] = row[RT_SL] = row[RT_WIN_LO] = row[RT_WIN_HI] = 0
                ssrc = route_ssrc(srtp_def._u32(key[srtp_def.KEY_SSRC]), j, int(row[RT_EPOCH]))
                for k in range(P):
                    nb = min(int(nbytes[b, j, k]), tb)
                    if nb < wire.TRANSPORT_HEADER:
                        continue
                    if not valid:
                        row[RT_NOKEY] += 1
                        continue
                    if row[RT_SEEN] == SEEN_EXHAUSTED:
                        row[RT_EXHAUSTED] += 1
                        continue
                    seq = (int(rows[b, j, k, 0]) << 8) | int(rows[b, j, k, 1])
                    v = self._admit(row, seq)
                    if v is None:
                        row[RT_STALE] += 1
                        continue
                    route_key = key.copy()
                    route_key[srtp_def.KEY_SSRC] = srtp_def._i32(ssrc)
                    blob = srtp_def.protect_packet(route_key, rows[b, j, k, :nb].tobytes(), v)
                    out[b, j, k, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
                    out_nbytes[b, j, k] = len(blob)
                    row[RT_PROTECTED] += 1
                    if self.sent is not None:
                        self.sent.append((digest, ssrc, (v << 16) | seq))
        return {"out": out, "out_nbytes": out_nbytes}


class ForwarderModel:
    """srtp.ReceiverModel on the uplink keys, forward.SenderModel (audio_level.RankModel with `speakers`), forward.ListenerModel
    (downlink.DownlinkModel with `downlink`) and RouteModel on the downlink keys: one GraphedForwardHop(srtp=SrtpConfig()) of `batch`
    slots.  `keys` (a ForwardKeys) takes the keys; its two tables are the ingress model's and the egress model's."""

    def __init__(self, batch: int, cfg: forward_def.ForwardConfig, n: int, T: int, m: int = 0, K=None,
                 downlink: Optional[downlink_def.DownlinkConfig] = None, speakers: Optional[level_def.SpeakerConfig] = None):
        shape = forward_def._Shape(batch, cfg, n, T, m, K)
        self.B, self.cfg, self.tb, self.speakers = shape.B, cfg, shape.tb, speakers
        if downlink is not None and downlink.history > 0:
            raise ValueError("forward_srtp: downlink.history > 0 with srtp: a NACK answer is cut again at answer time, so it could put "
                             "other plaintext under an index already used")
        self.keys = ForwardKeys(self.B)
        self.ingress = srtp_def.ReceiverModel(self.B, self.tb)
        self.ingress.keys = self.keys.up
        self.sender = forward_def.SenderModel(batch, cfg, n, T, m, K)
        self.rank = None if speakers is None else level_def.RankModel(batch, cfg, speakers)
        self.listener = forward_def.ListenerModel(batch, cfg, n, T, m, K)
        self.downlink = None if downlink is None else downlink_def.DownlinkModel(batch, downlink, cfg, n, T, m, K)
        self.egress = RouteModel(self.B, cfg.fanout, cfg.burst, self.tb)
        self.egress.keys = self.keys.down

    def step(self, slots, packets, nbytes, room, layers, action=None, levels=None, reports=None) -> Dict[str, np.ndarray]:
        """one hop: this hop's protected arrivals in push order (`slots`, `nbytes`: A ints; `packets` uint8 [A, tb + 10]), `room`,
        `layers` int [B], `action` int [B] (None: zeros), `levels` (with speakers) and `reports` (with a downlink rate) as
        GraphedForwardHop.forward takes them -> what the hop's launches write: plain (the ingress records), pick, pick_count, routes,
        new_routes, plain_out / plain_nbytes (the final rows in front of the egress) and out / out_nbytes (the protected rows)"""
        B = self.B
        rec, offs = forward_def.arrival_records(slots, packets, nbytes, self.tb + srtp_def.TAG_BYTES, B)
        action = np.zeros(B, dtype=np.int32) if action is None else np.asarray(action)
        up, down = self.keys.take()
        rekey_up, rekey_down = _marks(B, up), _marks(B, down)
        plain = self.ingress.unprotect(rec, offs, rekey_up)
        res = self.sender.step(plain, offs, action)
        ranked = self.sender.state
        if self.rank is not None:
            ranked = res["shadow"] = self.rank.step(self.sender.state, level_def.loud_row(B, slots, levels, self.speakers), room, action)
        res.update(self.listener.step(plain, action, room, layers, ranked, res["pick"], res["pick_count"]))
        if self.downlink is not None:
            fb = downlink_def.feedback_rows(B, self.cfg.fanout, reports, None)
            res.update(self.downlink.step(res["routes"], res["new_routes"], res["out"], res["out_nbytes"], layers, action,
                                          report=fb["report"]))
        res["plain"], res["plain_out"], res["plain_nbytes"] = plain, res["out"], res["out_nbytes"]
        res.update(self.egress.protect(res["out"], res["out_nbytes"], res["routes"], res["new_routes"], action, rekey_up, rekey_down))
        return res
