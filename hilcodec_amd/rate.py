"""Report-driven rate control of the graphed sender (graph_step.GraphedEncodeHop(rate=RateConfig(...))): the definition, bit for bit, of
hilc_rate_ceiling and hilc_rate_charge (csrc/rate.hip), and the only module that knows their rules.  Import it by name (`from hilcodec_amd
import rate`).

Receiver reports (report.py) tell the sender how much of a slot's stream went missing.  FEC, retransmission and VBR answer loss by
sending as much or more; when the link itself is the reason for the loss that makes it worse.  This rule lowers a slot's bit rate
instead: each slot has a rate (bits per hop, kept in Q8: bits x 256) that follows the reports, and a token bucket filled at that rate
and charged with every byte the slot really sends.  What the bucket can pay for is the most quantiser stages the slot may use on the
hop, n_ceil; the residual quantiser is trained with quantiser dropout, so cutting a slot to fewer stages is exact (vbr.py).  All
arithmetic is integer.

Bits.  bucket(cfg, T, m, header): x_bits = floor(x_kbps 1000 T 320 / 24000) for min, max and start (start_kbps None: max), as
       vbr.bucket_bits; stage_bits = 10 T.  min <= start <= max; min_bits >= 8 TRANSPORT_HEADER header + 10 T (max(m, 1) + m): the
       floor of a hop (the header, the fewest primary stages, the redundant section) is always payable; max_bits burst_hops <=
       vbr.MAX_BURST_BITS and max_bits <= MAX_RATE_BITS, so the credit and the Q8 rate fit an int32.

Ceiling rule (hilc_rate_ceiling; per slot and hop, in front of the quantiser):
1. action != 0 (a start or a resume on this hop) resets the slot: RC_RATE_Q8 = 256 start_bits, RC_CREDIT = burst_hops start_bits, the
   report memory (RC_SEEN, RC_LAST, RC_AGE, RC_LOSS) and the counters 0.
2. a report for the slot on this hop (report.report_word; held and stopped slots take theirs too) is accepted by exactly
   hilc_fec_adapt's rule: if the slot has seen none since it was reset, or d = (seq - RC_LAST) mod 256 is in [1, 127]; otherwise
   RC_STALE += 1 and it is dropped.  An accepted report sets RC_SEEN = 1, RC_LAST = seq, RC_AGE = 0, RC_LOSS = loss_q8, RC_REPORTS += 1;
   then loss >= high_q8: rate = max(256 min_bits, (rate (512 - loss)) >> 9) (a 64-bit product: the 1 - p / 2 of Google Congestion
   Control's loss-based rule), RC_DECREASED += 1; loss <= low_q8: rate = min(256 max_bits, rate + max(256, (rate increase_q8) >> 8)),
   RC_INCREASED += 1; in between the rate is kept.  loss_q8 is used, not residual_q8: it counts repaired hops as missing, so the rule
   does not depend on whether FEC is on.
3. not held: RC_AGE += 1, and with timeout_hops > 0 and RC_AGE >= timeout_hops: rate = 256 start_bits, RC_SEEN = 0, RC_AGE = 0,
   RC_TIMEOUT += 1.
4. not held: RC_CREDIT = min(RC_CREDIT + (rate >> 8), burst_hops (rate >> 8)).
5. overhead = 8 TRANSPORT_HEADER header + 10 m T [a redundant section will be sent]: m >= 1, no action on this hop, and word 0 of the
   slot's previous-codes row of this hop's parity is non-zero (after hilc_fec_adapt, when the sender has one).
6. n_ceil = clamp(max(0, RC_CREDIT - overhead) // (10 T), min(n_slot, max(m, 1)), n_slot), n_slot the slot's own ceiling (the graph's
   n, `start(n=)`, `set_bitrate`) clamped to [1, n].
7. not held: RC_LIMITED += n_ceil < n_slot.  A held slot reports n_ceil = n_slot.

Charge rule (hilc_rate_charge; per slot and hop, the graph's last launch):
   RC_CREDIT = max(RC_CREDIT - 8 (nbytes[b] + the sum over q of rtx_nbytes[b, q]), -burst_hops (rate >> 8)).
What the slot really put on the wire this hop is charged: the header, the primary codes with their padding, the redundant section, a
SID, nothing for a DTX silent hop, what VBR saved, and retransmissions.  A held or stopped slot's packet is 0 bytes, but the NACKs it
answered are still charged.  The credit may go below 0 (the floor of a hop costs more than a low rate pays, padding, retransmissions):
the debt is paid back before the ceiling rises again, and it is bounded by burst_hops hops of the rate.

Rate row (int32, RC_WORDS words): RC_RATE_Q8, RC_CREDIT, RC_SEEN, RC_LAST, RC_AGE, RC_LOSS, then the counters RC_REPORTS, RC_STALE,
RC_DECREASED, RC_INCREASED, RC_TIMEOUT, RC_LIMITED (RC_NAMES)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

from .report import REPORT_PRESENT, _check_ints
from .vbr import MAX_BURST_BITS
from .wire import MAX_STAGES, TRANSPORT_HEADER

RC_RATE_Q8, RC_CREDIT, RC_SEEN, RC_LAST, RC_AGE, RC_LOSS = range(6)
RC_REPORTS, RC_STALE, RC_DECREASED, RC_INCREASED, RC_TIMEOUT, RC_LIMITED = 6, 7, 8, 9, 10, 11
RC_WORDS = 12
RC_NAMES = ("reports", "stale", "decreased", "increased", "timeout", "limited")
MAX_RATE_BITS = 1 << 22                           # 256 rate_bits, and one increase on top of it, fit an int32


@dataclass(frozen=True)
class RateConfig:
    """rate control of a GraphedEncodeHop (the rules: this module's docstring).  min_kbps <= start_kbps <= max_kbps (finite, > 0;
    start_kbps None: max_kbps): the bounds of a slot's rate and the rate of a slot that has heard nothing; high_q8 / low_q8: the
    reported loss_q8 (loss x 256) at or above which the rate falls / at or below which it rises, 0 <= low_q8 < high_q8 <= 255;
    increase_q8 in [0, 65535]: the rise per calm report, as a fraction x 256 of the rate (never less than one bit per hop);
    burst_hops >= 1: the hops of the rate the bucket holds, and the debt it allows; timeout_hops >= 0: hops without an accepted report
    after which the slot falls back to start_kbps (0: never)"""
    min_kbps: float
    max_kbps: float
    start_kbps: Optional[float] = None
    high_q8: int = 26
    low_q8: int = 5
    increase_q8: int = 13
    burst_hops: int = 8
    timeout_hops: int = 0

    def __post_init__(self):
        for name in ("min_kbps", "max_kbps", "start_kbps"):
            v = getattr(self, name)
            if v is None and name == "start_kbps":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                    or not float(v) > 0.0:
                raise ValueError(f"RateConfig: {name} must be a finite number > 0, got {v!r}")
            object.__setattr__(self, name, float(v))
        _check_ints("RateConfig", self, (("high_q8", 1, 255), ("low_q8", 0, 254), ("increase_q8", 0, 65535),
                                         ("burst_hops", 1, (1 << 30) - 1), ("timeout_hops", 0, (1 << 30) - 1)))
        if not self.low_q8 < self.high_q8:
            raise ValueError(f"RateConfig: low_q8 = {self.low_q8} must be below high_q8 = {self.high_q8}")
        if not self.min_kbps <= self.start <= self.max_kbps:
            raise ValueError(f"RateConfig: min_kbps = {self.min_kbps} <= start_kbps = {self.start} <= max_kbps = {self.max_kbps} must hold")

    @property
    def start(self) -> float:
        """start_kbps, or max_kbps when it is None"""
        return self.max_kbps if self.start_kbps is None else self.start_kbps


class Bucket(NamedTuple):
    """what bucket() returns, in bits per hop"""
    stage_bits: int
    min_bits: int
    max_bits: int
    start_bits: int
    header_bits: int


def floor_bits(frames: int, fec_stages: int = 0, header: bool = False) -> int:
    """the bits of the smallest hop the ceiling rule can ask for: the header, max(m, 1) primary stages and the redundant section"""
    m = int(fec_stages)
    return 8 * TRANSPORT_HEADER * bool(header) + 10 * int(frames) * (max(m, 1) + m)


def bucket(cfg: RateConfig, frames: int, fec_stages: int = 0, header: bool = False) -> Bucket:
    """cfg's rates in bits per hop of `frames` frames, for a sender with m = `fec_stages` and the transport header or not.  ValueError
    when min_kbps does not pay for the floor of every hop or a bound of the int32 rows is passed"""
    if not isinstance(cfg, RateConfig):
        raise ValueError(f"cfg must be a RateConfig, got {cfg!r}")
    T, m = int(frames), int(fec_stages)
    if T < 1 or m < 0:
        raise ValueError(f"frames = {frames!r} must be >= 1 and fec_stages = {fec_stages!r} >= 0")
    lo, hi, start = (math.floor(Fraction(k) * 1000 * T * 320 / 24000) for k in (cfg.min_kbps, cfg.max_kbps, cfg.start))
    need = floor_bits(T, m, header)
    if lo < need:
        raise ValueError(f"RateConfig: min_kbps = {cfg.min_kbps} is {lo} bits per hop, the floor of a hop (header, {max(m, 1)} stages, "
                         f"{m} redundant ones) needs {need}")
    if hi * cfg.burst_hops > MAX_BURST_BITS or hi > MAX_RATE_BITS:
        raise ValueError(f"RateConfig: max_kbps = {cfg.max_kbps} is {hi} bits per hop: more than {MAX_RATE_BITS}, or a burst of more than "
                         f"{MAX_BURST_BITS}")
    return Bucket(10 * T, lo, hi, start, 8 * TRANSPORT_HEADER * bool(header))


def kbps(row_or_rows, frames: int):
    """RC_RATE_Q8 of one rate row (-> float) or of rows [B, RC_WORDS] (-> float64 [B]) back in kbps, on the host"""
    rows = row_or_rows.detach().cpu().numpy() if hasattr(row_or_rows, "detach") else np.asarray(row_or_rows)
    out = rows[..., RC_RATE_Q8].astype(np.float64) * 24000.0 / (256.0 * 1000.0 * 320.0 * int(frames))
    return float(out) if out.ndim == 0 else out


class RateModel:
    """numpy statement of hilc_rate_ceiling (`ceiling`) and hilc_rate_charge (`charge`) for `batch` slots of an n-stage sender with
    `frames` frames per hop, m = `fec_stages` redundant stages and the transport header or not.  `state` int32 [B, RC_WORDS] are the
    kernels' rate rows (as after a reset)."""

    def __init__(self, batch: int, cfg: RateConfig, n: int, frames: int = 1, fec_stages: int = 0, header: bool = False):
        self.B, self.cfg, self.n, self.T, self.m = int(batch), cfg, int(n), int(frames), int(fec_stages)
        if not 1 <= self.n <= MAX_STAGES:
            raise ValueError(f"n = {n} outside [1, {MAX_STAGES}]")
        self.bits = bucket(cfg, self.T, self.m, header)
        self.state = np.zeros((self.B, RC_WORDS), dtype=np.int32)
        self._reset(self.state)

    def _reset(self, rows: np.ndarray) -> None:
        rows[...] = 0
        rows[..., RC_RATE_Q8] = 256 * self.bits.start_bits
        rows[..., RC_CREDIT] = self.cfg.burst_hops * self.bits.start_bits

    def ceiling(self, words=None, action=None, hold=None, n_slot=None, prev: Optional[np.ndarray] = None) -> np.ndarray:
        """the head of one hop: `words` int [B] (report_word per slot, 0: none), `action` / `hold` int [B] (None: zeros), `n_slot` int
        [B] (None: n), `prev` int [B, 1 + m T] or [B] (the previous-codes rows of this hop's parity, or their words 0; None: no
        redundant section is live) -> n_ceil int32 [B]; `state` is updated in place"""
        B, c, bits = self.B, self.cfg, self.bits
        zeros = np.zeros(B, dtype=np.int64)
        words = zeros if words is None else np.asarray(words, dtype=np.int64).reshape(-1)
        action = zeros if action is None else np.asarray(action).reshape(-1)
        hold = zeros if hold is None else np.asarray(hold).reshape(-1)
        n_slot = np.full(B, self.n) if n_slot is None else np.clip(np.asarray(n_slot, dtype=np.int64).reshape(-1), 1, self.n)
        valid = zeros if prev is None else np.asarray(prev).reshape(B, -1)[:, 0]
        lo_q8, hi_q8 = 256 * bits.min_bits, 256 * bits.max_bits
        out = np.zeros(B, dtype=np.int32)
        for b in range(B):
            row = self.state[b]
            if action[b] != 0:
                self._reset(row)
            rate = int(row[RC_RATE_Q8])
            w = int(words[b])
            if w & REPORT_PRESENT:
                seq, loss = (w >> 16) & 255, (w >> 8) & 255
                d = (seq - int(row[RC_LAST])) & 255
                if row[RC_SEEN] and not 1 <= d <= 127:
                    row[RC_STALE] += 1
                else:
                    row[RC_SEEN], row[RC_LAST], row[RC_AGE], row[RC_LOSS] = 1, seq, 0, loss
                    row[RC_REPORTS] += 1
                    if loss >= c.high_q8:
                        rate = max(lo_q8, (rate * (512 - loss)) >> 9)
                        row[RC_DECREASED] += 1
                    elif loss <= c.low_q8:
                        rate = min(hi_q8, rate + max(256, (rate * c.increase_q8) >> 8))
                        row[RC_INCREASED] += 1
            held = hold[b] != 0
            if not held:
                row[RC_AGE] += 1
                if c.timeout_hops > 0 and row[RC_AGE] >= c.timeout_hops:
                    rate = 256 * bits.start_bits
                    row[RC_SEEN], row[RC_AGE] = 0, 0
                    row[RC_TIMEOUT] += 1
                row[RC_CREDIT] = min(int(row[RC_CREDIT]) + (rate >> 8), c.burst_hops * (rate >> 8))
            row[RC_RATE_Q8] = rate
            redundant = self.m >= 1 and action[b] == 0 and valid[b] != 0
            overhead = bits.header_bits + bits.stage_bits * self.m * int(redundant)
            ns = int(n_slot[b])
            n_ceil = min(max(max(0, int(row[RC_CREDIT]) - overhead) // bits.stage_bits, min(ns, max(self.m, 1))), ns)
            if held:
                n_ceil = ns
            else:
                row[RC_LIMITED] += n_ceil < ns
            out[b] = n_ceil
        return out

    def charge(self, nbytes, rtx_nbytes=None) -> None:
        """the tail of one hop: `nbytes` int [B] (the hop's packets as sent, header included), `rtx_nbytes` int [B, per_hop] or None
        (its retransmissions); `state` is updated in place"""
        sent = np.asarray(nbytes, dtype=np.int64).reshape(self.B)
        if rtx_nbytes is not None:
            sent = sent + np.asarray(rtx_nbytes, dtype=np.int64).reshape(self.B, -1).sum(axis=1)
        floor = -self.cfg.burst_hops * (self.state[:, RC_RATE_Q8].astype(np.int64) >> 8)
        self.state[:, RC_CREDIT] = np.maximum(self.state[:, RC_CREDIT].astype(np.int64) - 8 * sent, floor).astype(np.int32)
