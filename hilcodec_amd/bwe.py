"""Delay-based bandwidth estimation of the graphed hops (graph_step.GraphedDecodeHop(bwe=BweConfig(...)),
GraphedEncodeHop(cap=CapConfig(...))): the definition, bit for bit, of hilc_rx_bwe and hilc_rate_cap (csrc/bwe.hip), and the only module
that knows their rules.  Import it by name (`from hilcodec_amd import bwe`).

Loss-based rate control (rate.py) reacts once a drop-tail queue is full, so every delivered packet still waits behind a full queue.
The receiver can see the queue grow long before that: packets sent one hop apart arrive more than one hop apart.  hilc_rx_bwe measures
that delay gradient per slot (the arrival-time filter, trendline and over-use detector of Google Congestion Control), runs an AIMD
controller on the incoming rate it measures and emits a 3-byte cap (wire.pack_cap); hilc_rate_cap, in front of hilc_rate_ceiling, clamps
the sender's rate to the latest cap.  The sender's rate is therefore the smaller of the loss-based rate and the receiver's estimate:
the loss rule keeps probing upward and handles the standing queue that a gradient cannot see, the estimate keeps the queue short.
All arithmetic is integer; `>>` and `//` round towards minus infinity.

Time.  Ticks of 1/24000 s: a hop of T frames is HOP_TICKS T = 320 T ticks, so send-time differences are exact integers from the
       header's hop index.  Arrival times are host ints taken mod 2^32 (stored as int32 words); differences are taken as int32.
Bits.  bits(cfg, T): x_bits = floor(x_kbps 1000 T 320 / 24000) for min and max, as rate.bucket; 1 <= min_bits <= max_bits <=
       MAX_CAP_BITS = 65535 (a cap is a uint16 on the wire; ValueError otherwise).

Receiver rule (hilc_rx_bwe; per slot and hop, directly behind the jitter step; it reads the hop's arrival region, the parallel arrival
times, `action` and its own row, never the jitter state):
1. action != 0 (a start or a resume on this hop) clears the row: BW_RATE_Q8 = 256 max_bits, BW_THR = THR_START, everything else 0,
   counters included; the slot's cap bytes become 0.
2. each arrival of the slot, in push order, parsed by wire.parse_transport (malformed: BW_MALFORMED += 1, skipped), with its hop index
   h, its arrival time t and its size bits = 8 nbytes:
   - a slot that has seen nothing (BW_SEEN = 0) only remembers it: BW_SEEN = 1, BW_LAST_H = h, BW_LAST_T = t, and the rate ring starts
     with (t, bits), or stays empty for a SID.
   - else dh = int16(h - BW_LAST_H); dh <= 0 (a retransmission, a duplicate, a reordered packet): BW_OLD += 1, skipped entirely.
   - da = int32(t - BW_LAST_T); da < 0 or da > reset_ticks: the estimator restarts with this arrival as its first: BW_RESET += 1,
     BW_LAST_H = h, BW_LAST_T = t, BW_THR = THR_START, BW_ACC = BW_SM = BW_COUNT = BW_PREV_M = BW_OVER_TICKS = BW_OVER_COUNT =
     BW_SIGNAL = BW_N = BW_HEAD = 0, the rate ring as for a first arrival.  BW_RATE_Q8 and BW_STATE are kept.
   - else BW_LAST_H = h, BW_LAST_T = t, the rate ring takes the arrival (3.), and one sample is taken (BW_SAMPLES += 1):
     a. d = clamp(da - 320 T dh, -ACC_MAX, ACC_MAX)
     b. BW_ACC = clamp(BW_ACC + d, -ACC_MAX, ACC_MAX): the accumulated delay in ticks
     c. BW_SM += ((256 BW_ACC - BW_SM) alpha_q8) >> 8: the smoothed delay in Q8
     d. (t, BW_SM) enters the trend ring of the last `window` samples (BW_N entries, BW_HEAD the next to be written)
     e. BW_COUNT = min(BW_COUNT + 1, COUNT_MAX = 60)
     f. with a full window, the least-squares slope of the smoothed delay over arrival time, x_i = uint32(t_i - t_0) >> 4 (16-tick
        units) and y_i = sm_i - sm_0 (Q8) relative to the oldest sample: num = N sum(x y) - sum(x) sum(y), den = N sum(x x) - sum(x)^2,
        slope = clamp((16 num) // den, -SLOPE_MAX, SLOPE_MAX) in Q16, 0 when den <= 0 or the window is not full yet
     g. the modified trend m = slope BW_COUNT 4
     h. detector: m > BW_THR: BW_OVER_TICKS += da, BW_OVER_COUNT += 1 (both saturate at 2^30), and once BW_OVER_TICKS > OVER_TICKS = 240 (10 ms),
        BW_OVER_COUNT > 1 and m >= BW_PREV_M: BW_SIGNAL = OVERUSE, BW_OVERUSE += 1, both cleared (until then the signal stays what it
        was); m < -BW_THR: BW_SIGNAL = UNDERUSE, BW_UNDERUSE += 1 when it was not, both cleared; else BW_SIGNAL = NORMAL, both cleared.
        Then BW_PREV_M = m.
     i. the threshold adapts unless |m| - BW_THR > 15 2^16: BW_THR += ((|m| - BW_THR) min(da, 2400) k) >> 24, k = K_DOWN (0.039 / 24
        in Q24) when |m| < BW_THR, K_UP (0.0087 / 24 in Q24) otherwise, clamped to [THR_MIN, THR_MAX] = [6, 600] 2^16; THR_START =
        12.5 2^16.
     j. AIMD on BW_SIGNAL (4.).
3. incoming rate: a ring of the last `rate_window` sampled codes packets (t, bits) (BW_RN entries, BW_RHEAD the next to be written).
   A SID arrival or an estimator restart empties it: a sender in DTX is not sending at its rate.  R_q8 = (the bits of all but the
   oldest) 256 320 T // uint32(t_newest - t_oldest), valid with at least RATE_MIN = 4 entries and a positive span.
4. AIMD:
   - OVERUSE: with a valid R, new = max(256 min_bits, (R_q8 beta_q8) >> 8); only a lower value replaces BW_RATE_Q8, which counts
     BW_DECREASED and makes the cap due on this hop.  BW_STATE = HOLD.
   - UNDERUSE: BW_STATE = HOLD (the queue is draining: wait).
   - NORMAL: BW_STATE = INCREASE, and BW_RATE_Q8 = min(256 max_bits, BW_RATE_Q8 + max(1, (BW_RATE_Q8 increase_q16 dh) >> 16)),
     BW_INCREASED += 1 (increase_q16 None: 70 T, about 8 % per second).
5. emission, every hop: BW_PHASE += 1; when a decrease happened on this hop, or BW_PHASE >= interval and BW_SEEN: BW_PHASE = 0,
   BW_SEQ = (BW_SEQ + 1) mod 256, the slot's cap bytes = wire.pack_cap(BW_SEQ, min(65535, BW_RATE_Q8 >> 8)), due = 1, BW_CAPS += 1;
   due = 0 on every other hop and the cap bytes stay.

Bounds that keep every product inside int64 (the model asserts them): |BW_ACC| <= ACC_MAX = 2^20 ticks, so |BW_SM| <= 2^28 and |y| <=
2^29; reset_ticks <= MAX_RESET_TICKS = 2^17 and window <= MAX_WINDOW = 32, so a window spans less than 2^22 ticks and x < 2^18; then
|N sum(x y)|, |sum(x) sum(y)| <= 2^57, |16 num| <= 2^62, den <= 2^46.  SLOPE_MAX = 2^22, so |m| <= 2^22 240 < 2^30 fits a word and the
threshold's product is below 2^30 2^12 2^15.  T <= MAX_FRAMES = 1024 and an arrival of at most MAX_ROW_BYTES = 2^15 bytes: 320 T dh <
2^34, the rate's numerator < 2^23 2^8 2^19 = 2^50, R_q8 beta_q8 < 2^58.  BW_RATE_Q8 <= 2^24: the increase's product < 2^24 2^16 2^15.

Sender rule (hilc_rate_cap; per slot and hop, directly in front of hilc_rate_ceiling, which is unchanged, as are RateModel and RC_*):
1. action != 0 clears the cap row.
2. a cap word for the slot on this hop (cap_word: CAP_PRESENT | seq << 16 | cap_bits, a one-hop row like the report's; held and stopped
   slots take theirs too) is accepted by exactly hilc_rate_ceiling's sequence rule: the first since the row was cleared (or timed out), or
   (seq - CP_LAST) mod 256 in [1, 127]; otherwise CP_STALE += 1 and it is dropped.  An accepted word sets CP_SEEN = 1, CP_LAST = seq,
   CP_AGE = 0, CP_CAP_Q8 = 256 clamp(cap_bits, min_bits, max_bits) (the rate's bounds) and CP_CAPS += 1.
3. not held: CP_AGE += 1, and with timeout_hops > 0 and CP_AGE >= timeout_hops the cap is forgotten: CP_SEEN = 0, CP_AGE = 0,
   CP_TIMEOUT += 1.
4. while CP_SEEN: RC_RATE_Q8 = min(RC_RATE_Q8, CP_CAP_Q8) in the slot's rate row, CP_CLAMPED += 1 when that lowered it.
hilc_rate_ceiling then runs on the clamped rate: its own report may still lower it, its increase starts from the cap, and on a hop with
an action it resets the rate row as always.

Rows (int32).  The estimate: BW_RATE_Q8, BW_THR, BW_SEEN, BW_LAST_H, BW_LAST_T, BW_ACC, BW_SM, BW_COUNT, BW_PREV_M, BW_OVER_TICKS,
BW_OVER_COUNT, BW_SIGNAL, BW_STATE, BW_PHASE, BW_SEQ, BW_N, BW_HEAD, BW_RN, BW_RHEAD, the counters BW_SAMPLES, BW_OLD, BW_RESET,
BW_MALFORMED, BW_OVERUSE, BW_UNDERUSE, BW_DECREASED, BW_INCREASED, BW_CAPS (BW_NAMES), then the trend ring at BW_TREND (MAX_WINDOW pairs
t, sm) and the rate ring at BW_RING (MAX_WINDOW pairs t, bits): BW_WORDS words.  The cap: CP_CAP_Q8, CP_SEEN, CP_LAST, CP_AGE, the
counters CP_CAPS, CP_STALE, CP_TIMEOUT, CP_CLAMPED (CP_NAMES): CP_WORDS words."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, NamedTuple, Optional

import numpy as np

from . import wire
from .rate import RC_RATE_Q8, RC_WORDS
from .report import _check_ints

HOP_TICKS = 320                                   # ticks of 1/24000 s per frame
BW_RATE_Q8, BW_THR, BW_SEEN, BW_LAST_H, BW_LAST_T, BW_ACC, BW_SM, BW_COUNT, BW_PREV_M, BW_OVER_TICKS = range(10)
BW_OVER_COUNT, BW_SIGNAL, BW_STATE, BW_PHASE, BW_SEQ, BW_N, BW_HEAD, BW_RN, BW_RHEAD = range(10, 19)
BW_SAMPLES, BW_OLD, BW_RESET, BW_MALFORMED, BW_OVERUSE, BW_UNDERUSE, BW_DECREASED, BW_INCREASED, BW_CAPS = range(19, 28)
BW_TREND = 28
MAX_WINDOW = 32
BW_RING = BW_TREND + 2 * MAX_WINDOW
BW_WORDS = BW_RING + 2 * MAX_WINDOW
BW_NAMES = ("samples", "old", "reset", "malformed", "overuse", "underuse", "decreased", "increased", "caps")
SIGNAL_NORMAL, SIGNAL_OVERUSE, SIGNAL_UNDERUSE = 0, 1, 2
STATE_HOLD, STATE_INCREASE = 0, 1
THR_START, THR_MIN, THR_MAX = 25 << 15, 6 << 16, 600 << 16
THR_SKIP = 15 << 16
K_UP, K_DOWN = 6082, 27263                        # 0.0087 / 24 and 0.039 / 24 per tick in Q24, rounded to nearest
OVER_TICKS, ADAPT_TICKS = 240, 2400
COUNT_MAX, RATE_MIN = 60, 4
ACC_MAX, SLOPE_MAX = 1 << 20, 1 << 22
MAX_RESET_TICKS, MAX_FRAMES, MAX_ROW_BYTES, MAX_CAP_BITS = 1 << 17, 1024, 1 << 15, 65535

CP_CAP_Q8, CP_SEEN, CP_LAST, CP_AGE, CP_CAPS, CP_STALE, CP_TIMEOUT, CP_CLAMPED = range(8)
CP_WORDS = 8
CP_NAMES = ("caps", "stale", "timeout", "clamped")
CAP_PRESENT = 1 << 24

_I64 = 1 << 63


def _kbps(who: str, obj, names) -> None:
    for name in names:
        v = getattr(obj, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                or not float(v) > 0.0:
            raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")
        object.__setattr__(obj, name, float(v))


@dataclass(frozen=True)
class BweConfig:
    """delay-based estimate of a GraphedDecodeHop (the rules: this module's docstring).  min_kbps <= max_kbps (finite, > 0): the bounds
    of the estimate, which starts at max_kbps; window in [2, 32]: the samples of the trendline; rate_window in [4, 32]: the codes packets
    the incoming rate is measured over; alpha_q8 in [1, 256]: the smoothing of the accumulated delay (x 256); beta_q8 in [1, 255]: the
    fraction x 256 of the incoming rate an over-use falls to; increase_q16 in [0, 65535] or None (70 per frame of the hop): the rise per
    hop index and calm sample, as a fraction x 65536 of the estimate; interval in [1, 1024]: the hops between two caps when nothing
    decreases; reset_ticks in [1, 2^17]: an arrival gap (ticks of 1/24000 s) above which the estimator restarts"""
    min_kbps: float
    max_kbps: float
    window: int = 20
    rate_window: int = 16
    alpha_q8: int = 26
    beta_q8: int = 218
    increase_q16: Optional[int] = None
    interval: int = 8
    reset_ticks: int = 72000

    def __post_init__(self):
        _kbps("BweConfig", self, ("min_kbps", "max_kbps"))
        bounds = (("window", 2, MAX_WINDOW), ("rate_window", RATE_MIN, MAX_WINDOW), ("alpha_q8", 1, 256), ("beta_q8", 1, 255),
                  ("interval", 1, 1024), ("reset_ticks", 1, MAX_RESET_TICKS))
        _check_ints("BweConfig", self, bounds + ((("increase_q16", 0, 65535),) if self.increase_q16 is not None else ()))
        if not self.min_kbps <= self.max_kbps:
            raise ValueError(f"BweConfig: min_kbps = {self.min_kbps} <= max_kbps = {self.max_kbps} must hold")

    def increase(self, frames: int) -> int:
        """increase_q16, or 70 per frame of the hop (at most 65535) when it is None"""
        return min(65535, 70 * int(frames)) if self.increase_q16 is None else int(self.increase_q16)


@dataclass(frozen=True)
class CapConfig:
    """rate caps of a GraphedEncodeHop (the rules: this module's docstring).  timeout_hops >= 0: hops without an accepted cap after which
    the slot forgets its cap (0: never)"""
    timeout_hops: int = 0

    def __post_init__(self):
        _check_ints("CapConfig", self, (("timeout_hops", 0, (1 << 30) - 1),))


class Bits(NamedTuple):
    """what bits() returns, in bits per hop"""
    min_bits: int
    max_bits: int


def bits(cfg: BweConfig, frames: int) -> Bits:
    """cfg's bounds in bits per hop of `frames` frames.  ValueError when min_kbps is less than one bit per hop, max_kbps more than
    MAX_CAP_BITS, or frames outside [1, MAX_FRAMES]"""
    if not isinstance(cfg, BweConfig):
        raise ValueError(f"cfg must be a BweConfig, got {cfg!r}")
    T = int(frames)
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"frames = {frames!r} outside [1, {MAX_FRAMES}]")
    lo, hi = (math.floor(Fraction(k) * 1000 * T * HOP_TICKS / 24000) for k in (cfg.min_kbps, cfg.max_kbps))
    if lo < 1 or hi > MAX_CAP_BITS:
        raise ValueError(f"BweConfig: min_kbps = {cfg.min_kbps} is {lo} and max_kbps = {cfg.max_kbps} is {hi} bits per hop, outside "
                         f"[1, {MAX_CAP_BITS}]")
    return Bits(lo, hi)


def cap_word(seq: int, cap_bits: int) -> int:
    """a cap as the sender's graph takes it: one int32 word per slot, 0 for none"""
    return CAP_PRESENT | (int(seq) & 255) << 16 | (int(cap_bits) & 0xFFFF)


def kbps(row_or_rows, frames: int):
    """BW_RATE_Q8 of one estimate row (-> float) or of rows [B, BW_WORDS] (-> float64 [B]) back in kbps, on the host"""
    rows = row_or_rows.detach().cpu().numpy() if hasattr(row_or_rows, "detach") else np.asarray(row_or_rows)
    out = rows[..., BW_RATE_Q8].astype(np.float64) * 24000.0 / (256.0 * 1000.0 * HOP_TICKS * int(frames))
    return float(out) if out.ndim == 0 else out


def _i16(v: int) -> int:
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def _i32(v: int) -> int:
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else (hi if v > hi else v)


def _fits(*values: int) -> None:
    """the products the kernel forms in 64 bits"""
    for v in values:
        assert -_I64 <= v < _I64, v


class BweModel:
    """numpy statement of hilc_rx_bwe for `batch` slots of a receiver of n_max stages, m = `fec_stages` redundant ones, `frames` frames
    per hop and comfort noise of order K (None: none).  `state` int32 [B, BW_WORDS] are the kernel's rows (as after a reset), `caps`
    uint8 [B, CAP_BYTES] each slot's latest cap, `due` int32 [B] the flags of the last hop."""

    def __init__(self, batch: int, cfg: BweConfig, n_max: int, fec_stages: int = 0, frames: int = 1, K: Optional[int] = None):
        self.B, self.cfg, self.n_max, self.m, self.T, self.K = int(batch), cfg, int(n_max), int(fec_stages), int(frames), K
        self.bits = bits(cfg, self.T)
        self.tbytes = wire.transport_bytes(self.n_max, self.m, self.T)
        if self.tbytes > MAX_ROW_BYTES:
            raise ValueError(f"an arrival of {self.tbytes} bytes, at most {MAX_ROW_BYTES}")
        self.inc = cfg.increase(self.T)
        self.state = np.zeros((self.B, BW_WORDS), dtype=np.int32)
        self.caps = np.zeros((self.B, wire.CAP_BYTES), dtype=np.uint8)
        self.due = np.zeros(self.B, dtype=np.int32)
        self._reset(self.state)

    def _reset(self, rows: np.ndarray) -> None:
        rows[...] = 0
        rows[..., BW_RATE_Q8] = 256 * self.bits.max_bits
        rows[..., BW_THR] = THR_START

    # ---- the two rings
    @staticmethod
    def _push(r: np.ndarray, base: int, n_word: int, head_word: int, size: int, a: int, b: int) -> None:
        head = int(r[head_word])
        r[base + 2 * head], r[base + 2 * head + 1] = a, b
        r[head_word] = (head + 1) % size
        r[n_word] = min(int(r[n_word]) + 1, size)

    @staticmethod
    def _entries(r: np.ndarray, base: int, n_word: int, head_word: int, size: int):
        n, head = int(r[n_word]), int(r[head_word])
        first = (head - n) % size
        return [(int(r[base + 2 * ((first + i) % size)]), int(r[base + 2 * ((first + i) % size) + 1])) for i in range(n)]

    def _start_rate_ring(self, r: np.ndarray, sid: bool, t: int, nbits: int) -> None:
        r[BW_RN] = r[BW_RHEAD] = 0
        if not sid:
            self._push(r, BW_RING, BW_RN, BW_RHEAD, self.cfg.rate_window, t, nbits)

    def incoming_q8(self, r: np.ndarray) -> Optional[int]:
        """R_q8 of one row, or None when it is not valid"""
        e = self._entries(r, BW_RING, BW_RN, BW_RHEAD, self.cfg.rate_window)
        if len(e) < RATE_MIN:
            return None
        span = (e[-1][0] - e[0][0]) & 0xFFFFFFFF
        if span <= 0:
            return None
        num = sum(b for _, b in e[1:]) * 256 * HOP_TICKS * self.T
        _fits(num)
        return num // span

    def slope_q16(self, r: np.ndarray) -> int:
        """the trendline's slope of one row in Q16, 0 until the window is full"""
        W = self.cfg.window
        e = self._entries(r, BW_TREND, BW_N, BW_HEAD, W)
        if len(e) < W:
            return 0
        t0, y0 = e[0]
        xs = [((t - t0) & 0xFFFFFFFF) >> 4 for t, _ in e]
        ys = [y - y0 for _, y in e]
        assert max(xs) < 1 << 18 and max(abs(y) for y in ys) <= 1 << 29
        sx, sy, sxy, sxx = sum(xs), sum(ys), sum(x * y for x, y in zip(xs, ys)), sum(x * x for x in xs)
        num, den = W * sxy - sx * sy, W * sxx - sx * sx
        _fits(W * sxy, sx * sy, 16 * num, W * sxx, sx * sx)
        if den <= 0:
            return 0
        return _clamp((16 * num) // den, -SLOPE_MAX, SLOPE_MAX)

    # ---- one arrival
    def _arrival(self, r: np.ndarray, packet, nbytes: int, t: int) -> bool:
        """-> whether the rate decreased"""
        c, T = self.cfg, self.T
        try:
            h, sid, _fec, _n, _body = wire.parse_transport(packet, nbytes, T, self.n_max, self.m, self.K)
        except ValueError:
            r[BW_MALFORMED] += 1
            return False
        t, nbits = _i32(t), 8 * int(nbytes)
        if not r[BW_SEEN]:
            r[BW_SEEN], r[BW_LAST_H], r[BW_LAST_T] = 1, h, t
            self._start_rate_ring(r, sid, t, nbits)
            return False
        dh = _i16(h - int(r[BW_LAST_H]))
        if dh <= 0:
            r[BW_OLD] += 1
            return False
        da = _i32(t - int(r[BW_LAST_T]))
        r[BW_LAST_H], r[BW_LAST_T] = h, t
        if da < 0 or da > c.reset_ticks:
            r[BW_RESET] += 1
            r[BW_THR] = THR_START
            for k in (BW_ACC, BW_SM, BW_COUNT, BW_PREV_M, BW_OVER_TICKS, BW_OVER_COUNT, BW_SIGNAL, BW_N, BW_HEAD):
                r[k] = 0
            self._start_rate_ring(r, sid, t, nbits)
            return False
        if sid:
            r[BW_RN] = r[BW_RHEAD] = 0
        else:
            self._push(r, BW_RING, BW_RN, BW_RHEAD, c.rate_window, t, nbits)
        r[BW_SAMPLES] += 1
        _fits(HOP_TICKS * T * dh)
        d = _clamp(da - HOP_TICKS * T * dh, -ACC_MAX, ACC_MAX)
        acc = _clamp(int(r[BW_ACC]) + d, -ACC_MAX, ACC_MAX)
        sm = int(r[BW_SM])
        sm += ((256 * acc - sm) * c.alpha_q8) >> 8
        assert abs(sm) <= ACC_MAX << 8
        r[BW_ACC], r[BW_SM] = acc, sm
        self._push(r, BW_TREND, BW_N, BW_HEAD, c.window, t, sm)
        count = min(int(r[BW_COUNT]) + 1, COUNT_MAX)
        r[BW_COUNT] = count
        m = self.slope_q16(r) * count * 4
        thr = int(r[BW_THR])
        if m > thr:
            r[BW_OVER_TICKS] = min(int(r[BW_OVER_TICKS]) + da, 1 << 30)
            r[BW_OVER_COUNT] = min(int(r[BW_OVER_COUNT]) + 1, 1 << 30)
            if r[BW_OVER_TICKS] > OVER_TICKS and r[BW_OVER_COUNT] > 1 and m >= r[BW_PREV_M]:
                r[BW_SIGNAL] = SIGNAL_OVERUSE
                r[BW_OVERUSE] += 1
                r[BW_OVER_TICKS] = r[BW_OVER_COUNT] = 0
        else:
            if m < -thr:
                r[BW_UNDERUSE] += r[BW_SIGNAL] != SIGNAL_UNDERUSE
                r[BW_SIGNAL] = SIGNAL_UNDERUSE
            else:
                r[BW_SIGNAL] = SIGNAL_NORMAL
            r[BW_OVER_TICKS] = r[BW_OVER_COUNT] = 0
        r[BW_PREV_M] = m
        if abs(m) - thr <= THR_SKIP:
            prod = (abs(m) - thr) * min(da, ADAPT_TICKS) * (K_DOWN if abs(m) < thr else K_UP)
            _fits(prod)
            r[BW_THR] = _clamp(thr + (prod >> 24), THR_MIN, THR_MAX)
        # AIMD
        rate, decreased = int(r[BW_RATE_Q8]), False
        if r[BW_SIGNAL] == SIGNAL_OVERUSE:
            R = self.incoming_q8(r)
            if R is not None:
                _fits(R * c.beta_q8)
                new = max(256 * self.bits.min_bits, (R * c.beta_q8) >> 8)
                if new < rate:
                    rate, decreased = new, True
                    r[BW_DECREASED] += 1
            r[BW_STATE] = STATE_HOLD
        elif r[BW_SIGNAL] == SIGNAL_UNDERUSE:
            r[BW_STATE] = STATE_HOLD
        else:
            r[BW_STATE] = STATE_INCREASE
            rate = min(256 * self.bits.max_bits, rate + max(1, (rate * self.inc * dh) >> 16))
            r[BW_INCREASED] += 1
        r[BW_RATE_Q8] = rate
        return decreased

    def step(self, action, slots, packets, nbytes, times) -> Dict[str, np.ndarray]:
        """one hop: `action` int [B] (None: zeros), arrivals `slots` [A], `packets` uint8 [A, tbytes], `nbytes` [A] and `times` [A]
        (ticks, any int: taken mod 2^32) in push order -> the slot's cap bytes uint8 [B, CAP_BYTES] and due flags int32 [B] (copies);
        `state`, `caps` and `due` are updated in place"""
        B = self.B
        action = np.zeros(B, dtype=np.int64) if action is None else np.asarray(action).reshape(-1)
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        packets = np.asarray(packets, dtype=np.uint8).reshape(len(slots), self.tbytes)
        nbytes = np.asarray(nbytes, dtype=np.int64).reshape(-1)
        times = [int(t) for t in np.asarray(times, dtype=object).reshape(-1)]
        if not len(slots) == len(nbytes) == len(times):
            raise ValueError(f"{len(slots)} slots, {len(nbytes)} byte counts and {len(times)} times")
        decreased = np.zeros(B, dtype=bool)
        for b in range(B):
            if action[b] != 0:
                self._reset(self.state[b])
                self.caps[b] = 0
        for a in range(len(slots)):
            b = int(slots[a])
            decreased[b] |= self._arrival(self.state[b], packets[a], int(nbytes[a]), times[a])
        for b in range(B):
            r = self.state[b]
            r[BW_PHASE] += 1
            emit = bool(decreased[b]) or (r[BW_PHASE] >= self.cfg.interval and r[BW_SEEN] != 0)
            if emit:
                r[BW_PHASE] = 0
                r[BW_SEQ] = (int(r[BW_SEQ]) + 1) & 255
                r[BW_CAPS] += 1
                self.caps[b] = np.frombuffer(wire.pack_cap(int(r[BW_SEQ]), min(MAX_CAP_BITS, int(r[BW_RATE_Q8]) >> 8)), dtype=np.uint8)
            self.due[b] = int(emit)
        return {"caps": self.caps.copy(), "due": self.due.copy()}


class CapModel:
    """numpy statement of hilc_rate_cap for `batch` slots of a sender whose rate is bounded by [min_bits, max_bits] bits per hop (its
    rate.bucket).  `state` int32 [B, CP_WORDS] are the kernel's cap rows (as after a reset)."""

    def __init__(self, batch: int, cfg: CapConfig, min_bits: int, max_bits: int):
        if not isinstance(cfg, CapConfig):
            raise ValueError(f"cfg must be a CapConfig, got {cfg!r}")
        self.B, self.cfg, self.min_bits, self.max_bits = int(batch), cfg, int(min_bits), int(max_bits)
        if not 1 <= self.min_bits <= self.max_bits <= 1 << 22:
            raise ValueError(f"1 <= min_bits = {min_bits} <= max_bits = {max_bits} <= 2^22 must hold")
        self.state = np.zeros((self.B, CP_WORDS), dtype=np.int32)

    def step(self, rate_rows: np.ndarray, words=None, action=None, hold=None) -> None:
        """the head of one hop, in front of RateModel.ceiling: `rate_rows` int32 [B, rate.RC_WORDS] (RC_RATE_Q8 is clamped in place),
        `words` int [B] (cap_word per slot, 0: none), `action` / `hold` int [B] (None: zeros); `state` is updated in place"""
        B, c = self.B, self.cfg
        assert rate_rows.shape == (B, RC_WORDS)
        zeros = np.zeros(B, dtype=np.int64)
        words = zeros if words is None else np.asarray(words, dtype=np.int64).reshape(-1)
        action = zeros if action is None else np.asarray(action).reshape(-1)
        hold = zeros if hold is None else np.asarray(hold).reshape(-1)
        for b in range(B):
            row = self.state[b]
            if action[b] != 0:
                row[...] = 0
            w = int(words[b])
            if w & CAP_PRESENT:
                seq, cap = (w >> 16) & 255, w & 0xFFFF
                d = (seq - int(row[CP_LAST])) & 255
                if row[CP_SEEN] and not 1 <= d <= 127:
                    row[CP_STALE] += 1
                else:
                    row[CP_SEEN], row[CP_LAST], row[CP_AGE] = 1, seq, 0
                    row[CP_CAP_Q8] = 256 * _clamp(cap, self.min_bits, self.max_bits)
                    row[CP_CAPS] += 1
            if hold[b] == 0:
                row[CP_AGE] += 1
                if c.timeout_hops > 0 and row[CP_AGE] >= c.timeout_hops:
                    row[CP_SEEN], row[CP_AGE] = 0, 0
                    row[CP_TIMEOUT] += 1
            if row[CP_SEEN] and rate_rows[b, RC_RATE_Q8] > row[CP_CAP_Q8]:
                rate_rows[b, RC_RATE_Q8] = row[CP_CAP_Q8]
                row[CP_CLAMPED] += 1
