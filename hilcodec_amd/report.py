"""Receiver reports and loss-adaptive in-band FEC of the graphed hops (graph_step.GraphedDecodeHop(report=ReportConfig(...)),
GraphedEncodeHop(fec_adapt=FecAdaptConfig(...))): the definition, bit for bit, of hilc_rx_report and hilc_fec_adapt (csrc/report.hip),
and the only module that knows their rules.  Import it by name (`from hilcodec_amd import report`).

The receiver's jitter buffer counts, per slot, the hops it decoded, repaired from a redundant section, lost or played as noise
(jitter.STAT_DECODED / STAT_FEC / STAT_LOST / STAT_NOISE).  hilc_rx_report turns those counters into a 3-byte report per slot
(wire.pack_report: seq, loss_q8, residual_q8) that a bridge sends back to the client beside the media; the sender takes the reports
it was given with a hop (`step(x, reports=(slots, blobs))`) and hilc_fec_adapt switches each slot's redundant section on or off.
The switch is word 0 ("valid") of the slot's previous-codes row: hilc_pack_codes_10bit_fec appends the redundant section only when
it is non-zero, hilc_packet_header derives the FEC flag from the packet's length and the receiver takes packets with or without the
section, so no other kernel changes; the packer still stores every hop's codes, so switching on takes effect on the next packet.

Receiver rule (ReportConfig(window=W, interval=R); per slot and hop, after the jitter step of that hop):
1. action != 0 (a start or a resume on this hop) clears the report row: the slot's report bytes and its due flag become 0 and the
   remembered counters are taken as 0.
2. the hop's class is whichever of STAT_DECODED, STAT_FEC, STAT_LOST, STAT_NOISE moved since the previous hop (the row remembers
   the four counters; at most one moves; were it more, the first in that order).  jitter.py guarantees DECODED + FEC + LOST + NOISE +
   AD_GROWN = the hops past priming that were not held, so a held, priming or inserted (grown) hop has no class and changes nothing
   but the due flag, which is 0.
3. D, F and L hops enter a sliding window of the slot's last W such hops: 2 bits each (CLASS_D / CLASS_F / CLASS_L) in a ring of
   ceil(W / 16) words, entry i in bits [2 (i mod 16), 2 (i mod 16) + 2) of word i // 16, RP_HEAD the entry written next; with N = W
   the entry at RP_HEAD, the oldest, leaves the counts first.  RP_N, RP_F, RP_L are the window's entries and its F and L hops, kept
   incrementally.  NOISE hops do not enter the window (DTX says nothing about the link).  Every class counts towards the interval:
   RP_PHASE += 1.
4. at RP_PHASE >= R: RP_PHASE = 0 and, with N >= 1, a report is emitted: seq = (seq + 1) mod 256 (the first report carries 1),
   loss_q8 = min(255, (256 (F + L) + N // 2) // N), residual_q8 = min(255, (256 L + N // 2) // N), RP_REPORTS += 1, the slot's
   report bytes = (seq, loss_q8, residual_q8) and due = 1 on that hop, 0 on every other.  With N = 0 (noise only) nothing is emitted
   and the interval starts again.  loss_q8 counts repaired hops as missing on purpose: it must not depend on whether the sender's
   FEC is on; residual_q8 is what the listener actually lost.
Report row (int32, RP_WORDS words): RP_SEQ, RP_LOSS, RP_RESIDUAL (the last report), RP_PHASE, RP_N, RP_F, RP_L, RP_HEAD, RP_DECODED,
RP_FEC, RP_LOST, RP_NOISE (the remembered counters), RP_REPORTS, then RP_RING_WORDS ring words from RP_RING (those past
ceil(W / 16) stay 0).

Sender rule (FecAdaptConfig(on_q8, off_q8, calm_reports, timeout_hops, initial_on); per slot and hop, before the packer):
1. action != 0 clears the row: ON = initial_on, CALM = 0, no sequence number seen, AGE = 0, the stored loss and residual and the
   counters 0.
2. a report for the slot on this hop (held and stopped slots take theirs too) is accepted if the slot has seen none since it was
   cleared, or if d = (seq - last) mod 256 is in [1, 127]; otherwise FA_STALE += 1 and it is dropped.  An accepted report sets
   SEEN = 1, last = seq, AGE = 0, stores its loss and residual and counts FA_REPORTS; then loss >= on_q8: CALM = 0 and ON = 1
   (FA_TURNED_ON += 1 if ON was 0); loss <= off_q8: CALM += 1 and at CALM >= calm_reports ON = 0 (FA_TURNED_OFF += 1 if ON was 1);
   in between: CALM = 0.
3. not held: AGE += 1, and with timeout_hops > 0 and AGE >= timeout_hops: ON = initial_on, CALM = 0, SEEN = 0, AGE = 0,
   FA_TIMEOUT += 1 (the stored sequence number, loss and residual stay; with SEEN = 0 any seq is accepted next).
4. not held and ON == 0: word 0 of the slot's previous-codes row of this hop's parity is set to 0.  Nothing else in that row is
   touched, and a held slot's row is never touched: it keeps its previous codes.
5. fec_on[b] = ON.
Adapt row (int32, FA_WORDS words): FA_ON, FA_CALM, FA_SEEN, FA_LAST, FA_AGE, FA_LOSS, FA_RESIDUAL, then the counters FA_REPORTS,
FA_STALE, FA_TURNED_ON, FA_TURNED_OFF, FA_TIMEOUT (FA_NAMES).

A report travels to the sender's graph as one int32 word per slot (report_word): REPORT_PRESENT | seq << 16 | loss_q8 << 8 |
residual_q8, 0 for no report."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from .jitter import ST_WORDS, STAT_DECODED, STAT_FEC, STAT_LOST, STAT_NOISE

RP_SEQ, RP_LOSS, RP_RESIDUAL, RP_PHASE, RP_N, RP_F, RP_L, RP_HEAD = range(8)
RP_DECODED, RP_FEC, RP_LOST, RP_NOISE, RP_REPORTS, RP_RING = 8, 9, 10, 11, 12, 13
RP_RING_WORDS = 16                                   # ceil(256 / 16): the widest window's ring
RP_WORDS = RP_RING + RP_RING_WORDS
RP_NAMES = ("seq", "loss", "residual", "phase", "n", "f", "l", "head", "decoded", "fec", "lost", "noise", "reports")
CLASS_NONE, CLASS_D, CLASS_F, CLASS_L, CLASS_NOISE = 0, 1, 2, 3, 4

FA_ON, FA_CALM, FA_SEEN, FA_LAST, FA_AGE, FA_LOSS, FA_RESIDUAL = range(7)
FA_REPORTS, FA_STALE, FA_TURNED_ON, FA_TURNED_OFF, FA_TIMEOUT = 7, 8, 9, 10, 11
FA_WORDS = 12
FA_NAMES = ("reports", "stale", "turned_on", "turned_off", "timeout")

REPORT_PRESENT = 1 << 24


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_ints(who: str, obj, bounds) -> None:
    for name, lo, hi in bounds:
        v = getattr(obj, name)
        if not _is_int(v):
            raise ValueError(f"{who}.{name} must be an int, got {v!r}")
        if not lo <= int(v) <= hi:
            raise ValueError(f"{who}.{name} = {v} outside [{lo}, {hi}]")


@dataclass(frozen=True)
class ReportConfig:
    """receiver reports of a GraphedDecodeHop (the rules: this module's docstring).  window W: the D / F / L hops a report looks
    back on, in [8, 256]; interval R: the classed hops between two reports, in [1, 1024]"""
    window: int = 64
    interval: int = 16

    def __post_init__(self):
        _check_ints("ReportConfig", self, (("window", 8, 256), ("interval", 1, 1024)))


@dataclass(frozen=True)
class FecAdaptConfig:
    """loss-adaptive FEC of a GraphedEncodeHop (the rules: this module's docstring).  on_q8 / off_q8: the reported loss_q8 (loss x
    256) at or above which the redundant section is switched on / at or below which a report is calm, 0 <= off_q8 < on_q8 <= 255;
    calm_reports >= 1: calm reports in a row that switch it off; timeout_hops >= 0: hops without an accepted report after which the
    slot falls back to `initial_on` (0: never); initial_on: the switch of a slot that has heard nothing"""
    on_q8: int = 8
    off_q8: int = 3
    calm_reports: int = 4
    timeout_hops: int = 0
    initial_on: bool = True

    def __post_init__(self):
        _check_ints("FecAdaptConfig", self, (("on_q8", 1, 255), ("off_q8", 0, 254), ("calm_reports", 1, (1 << 30) - 1),
                                             ("timeout_hops", 0, (1 << 30) - 1)))
        if not self.off_q8 < self.on_q8:
            raise ValueError(f"FecAdaptConfig: off_q8 = {self.off_q8} must be below on_q8 = {self.on_q8}")
        if not isinstance(self.initial_on, (bool, np.bool_)):
            raise ValueError(f"FecAdaptConfig.initial_on must be a bool, got {self.initial_on!r}")


def report_word(seq: int, loss_q8: int, residual_q8: int) -> int:
    """the int32 word that carries one report to the sender's graph"""
    return REPORT_PRESENT | (int(seq) & 255) << 16 | (int(loss_q8) & 255) << 8 | (int(residual_q8) & 255)


class ReportModel:
    """numpy statement of hilc_rx_report for `batch` slots.  `state` int32 [B, RP_WORDS] are the kernel's report rows, `reports` uint8
    [B, 3] each slot's latest report and `due` int32 [B] the flags of the last step."""

    def __init__(self, batch: int, cfg: ReportConfig):
        self.B, self.cfg = int(batch), cfg
        self.state = np.zeros((self.B, RP_WORDS), dtype=np.int32)
        self.reports = np.zeros((self.B, 3), dtype=np.uint8)
        self.due = np.zeros(self.B, dtype=np.int32)

    def _enter(self, row: np.ndarray, cls: int) -> None:
        W = self.cfg.window
        head = int(row[RP_HEAD])
        w, sh = RP_RING + head // 16, 2 * (head % 16)
        word = int(row[w]) & 0xFFFFFFFF
        if row[RP_N] >= W:                                  # the oldest entry leaves the counts
            old = (word >> sh) & 3
            row[RP_F] -= old == CLASS_F
            row[RP_L] -= old == CLASS_L
        else:
            row[RP_N] += 1
        word = (word & ~(3 << sh)) | (cls << sh)
        row[w] = np.uint32(word).astype(np.int32)
        row[RP_F] += cls == CLASS_F
        row[RP_L] += cls == CLASS_L
        row[RP_HEAD] = (head + 1) % W

    def step(self, jitter_state, action) -> Dict[str, np.ndarray]:
        """one hop: `jitter_state` int [B, jitter.ST_WORDS] as the jitter step of this hop left it, `action` int [B] -> the rows
        the kernel writes: reports (uint8 [B, 3]) and due (int32 [B]); `state` is updated in place"""
        js = np.asarray(jitter_state).reshape(self.B, ST_WORDS)
        action = np.asarray(action).reshape(-1)
        R = self.cfg.interval
        for b in range(self.B):
            row = self.state[b]
            if action[b] != 0:
                row[:] = 0
                self.reports[b] = 0
            self.due[b] = 0
            cls = CLASS_NONE
            for c, (mine, theirs) in zip((CLASS_D, CLASS_F, CLASS_L, CLASS_NOISE),
                                         ((RP_DECODED, STAT_DECODED), (RP_FEC, STAT_FEC), (RP_LOST, STAT_LOST), (RP_NOISE, STAT_NOISE))):
                if cls == CLASS_NONE and js[b, theirs] != row[mine]:
                    cls = c
                row[mine] = js[b, theirs]
            if cls == CLASS_NONE:
                continue
            if cls != CLASS_NOISE:
                self._enter(row, cls)
            row[RP_PHASE] += 1
            if row[RP_PHASE] < R:
                continue
            row[RP_PHASE] = 0
            N = int(row[RP_N])
            if N < 1:
                continue
            row[RP_SEQ] = (int(row[RP_SEQ]) + 1) & 255
            row[RP_LOSS] = min(255, (256 * int(row[RP_F] + row[RP_L]) + N // 2) // N)
            row[RP_RESIDUAL] = min(255, (256 * int(row[RP_L]) + N // 2) // N)
            row[RP_REPORTS] += 1
            self.reports[b] = (row[RP_SEQ], row[RP_LOSS], row[RP_RESIDUAL])
            self.due[b] = 1
        return {"reports": self.reports.copy(), "due": self.due.copy()}


class FecAdaptModel:
    """numpy statement of hilc_fec_adapt for `batch` slots of a sender with m = `fec_stages` redundant stages and `frames` frames per
    hop.  `state` int32 [B, FA_WORDS] are the kernel's adapt rows (as after a clear: ON = initial_on)."""

    def __init__(self, batch: int, cfg: FecAdaptConfig, fec_stages: int, frames: int = 1):
        self.B, self.cfg, self.m, self.T = int(batch), cfg, int(fec_stages), int(frames)
        if self.m < 1 or self.T < 1:
            raise ValueError(f"FecAdaptModel: fec_stages = {fec_stages} and frames = {frames} must be >= 1")
        self.state = np.zeros((self.B, FA_WORDS), dtype=np.int32)
        self.state[:, FA_ON] = int(cfg.initial_on)

    def step(self, words=None, action=None, hold=None, prev: Optional[np.ndarray] = None) -> np.ndarray:
        """one hop: `words` int [B] (report_word per slot, 0: none), `action` / `hold` int [B] (None: zeros), `prev` int32 [B, 1 + m T]
        (the previous-codes rows of this hop's parity, updated in place; None: not modelled) -> fec_on int32 [B]; `state` is updated in
        place"""
        B, c = self.B, self.cfg
        zeros = np.zeros(B, dtype=np.int64)
        words = zeros if words is None else np.asarray(words, dtype=np.int64).reshape(-1)
        action = zeros if action is None else np.asarray(action).reshape(-1)
        hold = zeros if hold is None else np.asarray(hold).reshape(-1)
        if prev is not None and prev.shape != (B, 1 + self.m * self.T):
            raise ValueError(f"FecAdaptModel.step: prev must be [{B}, {1 + self.m * self.T}]")
        on0 = int(c.initial_on)
        for b in range(B):
            row = self.state[b]
            if action[b] != 0:
                row[:] = 0
                row[FA_ON] = on0
            w = int(words[b])
            if w & REPORT_PRESENT:
                seq, loss, residual = (w >> 16) & 255, (w >> 8) & 255, w & 255
                d = (seq - int(row[FA_LAST])) & 255
                if row[FA_SEEN] and not 1 <= d <= 127:
                    row[FA_STALE] += 1
                else:
                    row[FA_SEEN], row[FA_LAST], row[FA_AGE], row[FA_LOSS], row[FA_RESIDUAL] = 1, seq, 0, loss, residual
                    row[FA_REPORTS] += 1
                    if loss >= c.on_q8:
                        row[FA_CALM] = 0
                        row[FA_TURNED_ON] += row[FA_ON] == 0
                        row[FA_ON] = 1
                    elif loss <= c.off_q8:
                        row[FA_CALM] += 1
                        if row[FA_CALM] >= c.calm_reports:
                            row[FA_TURNED_OFF] += row[FA_ON] == 1
                            row[FA_ON] = 0
                    else:
                        row[FA_CALM] = 0
            if hold[b] == 0:
                row[FA_AGE] += 1
                if c.timeout_hops > 0 and row[FA_AGE] >= c.timeout_hops:
                    row[FA_ON], row[FA_CALM], row[FA_SEEN], row[FA_AGE] = on0, 0, 0, 0
                    row[FA_TIMEOUT] += 1
                if prev is not None and row[FA_ON] == 0:
                    prev[b, 0] = 0
        return self.state[:, FA_ON].copy()
