"""Room mixing of the graphed receiver (graph_step.GraphedDecodeHop(mix=MixConfig(...)), `hilcodec_amd.mix_rooms`): the definition, bit
for bit, of hilc_mix_levels, hilc_mix_gains, hilc_mix_rooms and hilc_mix_rooms_dyn (csrc/mix.hip), and the only module that knows the
rules.  Inputs are assumed finite.

A conference bridge: every slot of a room hears the room's loudest other members.  Per hop the inputs are the receiver's final output
rows `wav` fp32 [B, 1, L] (whatever produced them: decoded, concealed, FEC, comfort noise, or the zeros of a held slot), `room` int32
[B] (-1: in no room, else a room id in [0, B)), `action` int32 [B] or None (the session row: a start or a resume on this hop) and the
state: `score` float64 [B] and, with the two options of MixConfig, `gains` float64 [B, 2], `power` float64 [B] and `limiter` float64
[B, 2].  A hop with action[b] != 0 first resets slot b's state rows to their cleared values: score 0, gains (1, 1), power 0, limiter
(0, 1).

Level.   p[l] = the sum over i = l (mod 64), i ascending, of (double)x[i] (double)x[i], l = 0..63; E = p[0] + p[1] + ... + p[63] in that
         order.  Every product and every sum is rounded on its own in float64 (the idiom of hilc_dtx_encode's lag sums).
Score.   score[b] = max(E[b], 0.5 prev[b]).  Every slot, every hop, whatever its room.  The halving (a peak hold) keeps the speaker
         set from flipping on every 13 ms hop.
Gain.    (MixConfig.level = LevelConfig(...); every slot, every hop, whatever its room.)  Every operation is one float64 operation
         rounded on its own; gate2 = gate_rms gate_rms, lo = target_rms target_rms / band, hi = target_rms target_rms band are computed
         once, here, as Python floats.  m = E / L; g0 = the previous hop-end gain, pw = the previous power.  If m >= gate2: pw = m when
         pw == 0, else pw + smooth (m - pw); v = (g0 g0) pw; v < lo: g1 = min(g0 up, max_gain); v > hi: g1 = max(g0 down, min_gain);
         else g1 = g0.  Otherwise pw and g1 = g0 stay: silence, comfort noise under the gate and held rows never pump the gain.
         gains[b] = (g0, g1), power[b] = pw.
Select.  The candidates of room r are the slots with room == r and score > 0, ordered by (score descending, slot ascending); the first
         min(top_k, count) are the room's speakers: speakers[b] = 1 for them, 0 for every other slot.  (The raw score: levelling does
         not change who speaks.)
Mix.     For a slot b with room[b] = r >= 0 the terms are the speakers of r other than b in ascending slot order: per sample acc =
         s[t0][i], then acc = acc + s[t1][i], ... (every sum rounded in fp32).  Without `level` s[j][i] = wav[j][i]; with it s[j][i] =
         fp32((double)wav[j][i] (g0 + (g1 - g0) ((double)(i + 1) / (double)L))) with slot j's (g0, g1): the gain moves linearly over
         the hop.  No terms, or room[b] < 0: acc is a row of zeros.  A held listener still gets its mix; a speaker hears the other
         speakers only (k - 1 terms).
Limit.   Without `limit`, mixed[b][i] = min(max(acc, -1), 1).  With MixConfig.limit = LimitConfig(ceiling, release, sub), per listener
         (a row of zeros runs through it as well, so its state releases): sub-frame s covers the samples [s sub, min((s + 1) sub, L)),
         n_s of them; p_s = max |acc[i]| over it (fp32, exact); e_s = max(p_s, release e_(s-1)); G_s = ceiling / e_s when e_s >
         ceiling, else 1 (float64, each operation rounded on its own); e_(-1), G_(-1) are limiter[b].  The gain of the sample at
         offset k of sub-frame s is G_s when G_s <= G_(s-1) (an immediate attack) and G_(s-1) + (G_s - G_(s-1)) ((double)(k + 1) /
         (double)n_s) otherwise; mixed = min(max(fp32((double)acc g), -1), 1); limiter[b] = (e_last, G_last).  g <= ceiling / p_s in
         every sub-frame, so |mixed| <= fp32(ceiling) up to one fp32 ulp: the clamp only guards against non-finite input.

Out of scope: room ids >= B, a host-set volume or mute row, selection on levelled scores."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

MAX_TOP_K = 8
LANES = 64
MIN_SUB = 16                # LimitConfig.sub, samples of a limiter sub-frame
MAX_SUB = 512
MAX_LIMIT_L = 8192          # the longest hop the limiter takes: at most MAX_LIMIT_L / MIN_SUB = 512 sub-frames


def _reals(cfg, *names) -> None:
    """the fields `names` of a config are finite real numbers (no bool): ValueError otherwise"""
    for name in names:
        v = getattr(cfg, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{type(cfg).__name__}.{name} must be a finite number, got {v!r}")


def _holds(cfg, ok: bool, what: str) -> None:
    if not ok:
        raise ValueError(f"{type(cfg).__name__}: {what} does not hold in {cfg!r}")


@dataclass(frozen=True)
class LevelConfig:
    """per-speaker levelling (the module docstring's "Gain"): a slot whose smoothed power, as heard, lies outside [target_rms^2 / band,
    target_rms^2 band] moves its gain by `up` / `down` per hop inside [min_gain, max_gain]; hops under `gate_rms` do not count."""
    target_rms: float = 0.1
    gate_rms: float = 0.01
    band: float = 1.6
    up: float = 1.01
    down: float = 0.97
    min_gain: float = 0.125
    max_gain: float = 8.0
    smooth: float = 0.25

    def __post_init__(self):
        _reals(self, "target_rms", "gate_rms", "band", "up", "down", "min_gain", "max_gain", "smooth")
        _holds(self, 0 < self.gate_rms and 0 < self.target_rms, "0 < gate_rms, 0 < target_rms")
        _holds(self, self.band > 1 and self.up > 1 and 0 < self.down < 1, "band > 1, up > 1, 0 < down < 1")
        _holds(self, 0 < self.min_gain <= 1 <= self.max_gain, "0 < min_gain <= 1 <= max_gain")
        _holds(self, 0 < self.smooth <= 1, "0 < smooth <= 1")

    # the derived constants, computed once here and handed to the entry point as doubles
    @property
    def gate2(self) -> float:
        return float(self.gate_rms) * float(self.gate_rms)

    @property
    def lo(self) -> float:
        return float(self.target_rms) * float(self.target_rms) / float(self.band)

    @property
    def hi(self) -> float:
        return float(self.target_rms) * float(self.target_rms) * float(self.band)


@dataclass(frozen=True)
class LimitConfig:
    """the per-listener limiter (the module docstring's "Limit"): the mix never exceeds `ceiling`; the envelope falls by `release` per
    sub-frame of `sub` samples"""
    ceiling: float = 0.9
    release: float = 0.99
    sub: int = 32

    def __post_init__(self):
        _reals(self, "ceiling", "release")
        _holds(self, 0 < self.ceiling <= 1 and 0 < self.release < 1, "0 < ceiling <= 1, 0 < release < 1")
        v = self.sub
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not MIN_SUB <= int(v) <= MAX_SUB:
            raise ValueError(f"LimitConfig.sub must be an int in [{MIN_SUB}, {MAX_SUB}], got {v!r}")


@dataclass(frozen=True)
class MixConfig:
    """top_k: the most speakers of a room that are mixed, an int in [1, 8]; level: per-speaker levelling (LevelConfig) or None; limit:
    the per-listener limiter (LimitConfig) or None: the plain clamp"""
    top_k: int = 3
    level: Optional[LevelConfig] = None
    limit: Optional[LimitConfig] = None

    def __post_init__(self):
        v = self.top_k
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"MixConfig.top_k must be an int, got {v!r}")
        if not 1 <= int(v) <= MAX_TOP_K:
            raise ValueError(f"MixConfig.top_k = {v} outside [1, {MAX_TOP_K}]")
        _check_dynamics("MixConfig", self.level, self.limit)


def _check_dynamics(who: str, level, limit) -> None:
    if level is not None and not isinstance(level, LevelConfig):
        raise ValueError(f"{who}.level must be a mixer.LevelConfig or None, got {level!r}")
    if limit is not None and not isinstance(limit, LimitConfig):
        raise ValueError(f"{who}.limit must be a mixer.LimitConfig or None, got {limit!r}")


def _np(a, dtype) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def levels(wav) -> np.ndarray:
    """E float64 [B] of wav fp32 [B, 1, L] (or [B, L])"""
    x = _np(wav, np.float32)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    B, L = x.shape
    p = np.zeros((B, LANES), dtype=np.float64)
    for base in range(0, L, LANES):
        w = min(LANES, L - base)
        v = x[:, base:base + w]
        p[:, :w] = p[:, :w] + v * v
    E = p[:, 0].copy()
    for lane in range(1, LANES):
        E = E + p[:, lane]
    return E


def update_score(score: np.ndarray, E: np.ndarray, action=None) -> np.ndarray:
    prev = np.asarray(score, dtype=np.float64)
    if action is not None:
        prev = np.where(_np(action, np.int64).reshape(-1) != 0, 0.0, prev)
    return np.maximum(E, 0.5 * prev)


def select(room: np.ndarray, score: np.ndarray, top_k: int) -> np.ndarray:
    """speakers int32 [B]"""
    B = len(room)
    speakers = np.zeros(B, dtype=np.int32)
    for r in np.unique(room[room >= 0]):
        cand = [b for b in range(B) if room[b] == r and score[b] > 0]
        cand.sort(key=lambda b: (-score[b], b))
        speakers[cand[:top_k]] = 1
    return speakers


def _resets(action, B: int) -> np.ndarray:
    return np.zeros(B, dtype=bool) if action is None else _np(action, np.int64).reshape(-1) != 0


def update_gains(gains: np.ndarray, power: np.ndarray, E: np.ndarray, L: int, cfg: LevelConfig, action=None):
    """(gains float64 [B, 2], power float64 [B]) after a hop of L samples with energies E (the module docstring's "Gain")"""
    gains, power = np.array(gains, dtype=np.float64), np.array(power, dtype=np.float64)
    reset = _resets(action, len(E))
    gate2, lo, hi = cfg.gate2, cfg.lo, cfg.hi
    up, down, smooth = float(cfg.up), float(cfg.down), float(cfg.smooth)
    min_gain, max_gain = float(cfg.min_gain), float(cfg.max_gain)
    for b in range(len(E)):
        g0, pw = (1.0, 0.0) if reset[b] else (float(gains[b, 1]), float(power[b]))
        g1 = g0
        m = float(E[b]) / float(L)
        if m >= gate2:
            pw = m if pw == 0.0 else pw + smooth * (m - pw)
            v = (g0 * g0) * pw
            if v < lo:
                g1 = min(g0 * up, max_gain)
            elif v > hi:
                g1 = max(g0 * down, min_gain)
        gains[b] = (g0, g1)
        power[b] = pw
    return gains, power


def sums(wav: np.ndarray, room: np.ndarray, speakers: np.ndarray, gains: Optional[np.ndarray] = None) -> np.ndarray:
    """acc fp32 [B, L] of wav fp32 [B, L]: every listener's sum before the clamp or the limiter; gains float64 [B, 2]: levelled terms"""
    B, L = wav.shape
    out = np.zeros((B, L), dtype=np.float32)
    ramp = np.arange(1, L + 1, dtype=np.float64) / np.float64(L)

    def term(t):
        if gains is None:
            return wav[t]
        g = gains[t, 0] + (gains[t, 1] - gains[t, 0]) * ramp
        with np.errstate(over="ignore", invalid="ignore"):
            return (wav[t].astype(np.float64) * g).astype(np.float32)

    for b in range(B):
        if room[b] < 0:
            continue
        terms = [t for t in range(B) if room[t] == room[b] and speakers[t] and t != b]
        if not terms:
            continue
        acc = term(terms[0]).copy()
        for t in terms[1:]:
            acc = (acc + term(t)).astype(np.float32)
        out[b] = acc
    return out


def clamp(acc: np.ndarray) -> np.ndarray:
    return np.minimum(np.maximum(acc, np.float32(-1)), np.float32(1))


def mix(wav: np.ndarray, room: np.ndarray, speakers: np.ndarray) -> np.ndarray:
    """mixed fp32 [B, L] of wav fp32 [B, L]: the plain mix (no levelling, no limiter)"""
    return clamp(sums(wav, room, speakers))


def limit(acc: np.ndarray, state: np.ndarray, cfg: LimitConfig, action=None):
    """(mixed fp32 [B, L], state float64 [B, 2]) of the sums acc fp32 [B, L] and the limiter rows (the module docstring's "Limit")"""
    B, L = acc.shape
    state = np.array(state, dtype=np.float64)
    reset = _resets(action, B)
    ceiling, release, sub = float(cfg.ceiling), float(cfg.release), int(cfg.sub)
    gain = np.empty((B, L), dtype=np.float64)
    for b in range(B):
        e, G = (0.0, 1.0) if reset[b] else (float(state[b, 0]), float(state[b, 1]))
        for lo in range(0, L, sub):
            n = min(sub, L - lo)
            p = float(np.fmax.reduce(np.abs(acc[b, lo:lo + n])))
            r = release * e
            e = p if p > r else r
            Gs = ceiling / e if e > ceiling else 1.0
            if Gs <= G:
                gain[b, lo:lo + n] = Gs
            else:
                gain[b, lo:lo + n] = G + (Gs - G) * (np.arange(1, n + 1, dtype=np.float64) / np.float64(n))
            G = Gs
        state[b] = (e, G)
    with np.errstate(over="ignore", invalid="ignore"):
        return clamp((acc.astype(np.float64) * gain).astype(np.float32)), state


class MixModel:
    """numpy statement of hilc_mix_levels (+ hilc_mix_gains) + hilc_mix_rooms / hilc_mix_rooms_dyn for `batch` slots; `score` float64
    [B], and with cfg.level `gains` float64 [B, 2] and `power` float64 [B], with cfg.limit `limiter` float64 [B, 2], are the kernels'
    state rows.  (No room ids >= B: see the module docstring.)"""

    def __init__(self, batch: int, cfg: Optional[MixConfig] = None):
        self.B, self.cfg = int(batch), cfg if cfg is not None else MixConfig()
        self.score = torch.zeros(self.B, dtype=torch.float64)
        self.gains, self.power, self.limiter = cleared_rows(self.B, self.cfg.level, self.cfg.limit)

    def step(self, wav, room, action=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """one hop: wav fp32 [B, 1, L], room int [B], action int [B] or None -> (mixed fp32 [B, 1, L], speakers int32 [B]); the state
        rows advance"""
        x = _np(wav, np.float32)
        if x.shape[0] != self.B or x.size == 0:
            raise ValueError(f"MixModel.step: wav must be [{self.B}, 1, L >= 1]")
        x = x.reshape(self.B, -1)
        rm = _np(room, np.int64).reshape(-1)
        if len(rm) != self.B:
            raise ValueError(f"MixModel.step: room needs {self.B} entries")
        E = levels(x)
        score = update_score(self.score.numpy(), E, action)
        self.score = torch.from_numpy(score)
        speakers = select(rm, score, int(self.cfg.top_k))
        gains = None
        if self.cfg.level is not None:
            gains, power = update_gains(self.gains.numpy(), self.power.numpy(), E, x.shape[1], self.cfg.level, action)
            self.gains, self.power = torch.from_numpy(gains), torch.from_numpy(power)
        acc = sums(x, rm, speakers, gains)
        if self.cfg.limit is not None:
            if x.shape[1] > MAX_LIMIT_L:
                raise ValueError(f"MixModel.step: the limiter takes hops of at most {MAX_LIMIT_L} samples")
            mixed, state = limit(acc, self.limiter.numpy(), self.cfg.limit, action)
            self.limiter = torch.from_numpy(state)
        else:
            mixed = clamp(acc)
        return torch.from_numpy(mixed).view(self.B, 1, -1), torch.from_numpy(speakers)


def cleared_rows(batch: int, level, limit, device=None):
    """(gains float64 [B, 2] = (1, 1) or None, power float64 [B] = 0 or None, limiter float64 [B, 2] = (0, 1) or None)"""
    kw = dict(dtype=torch.float64, device=device)
    gains = torch.ones(batch, 2, **kw) if level is not None else None
    power = torch.zeros(batch, **kw) if level is not None else None
    limiter = torch.tensor([0.0, 1.0], **kw).repeat(batch, 1) if limit is not None else None
    return gains, power, limiter


class Dynamics:
    """The levelling and limiter state of `hilcodec_amd.mix_rooms(..., dynamics=)` for `batch` slots, updated in place by every call:
    `gains` float64 [B, 2] and `power` float64 [B] (with `level`), `limiter` float64 [B, 2] (with `limit`), on `device` (None: the
    current GPU).  `reset(slots)` puts the rows of `slots` (None: all) back as constructed: what a start does in the graphed hop."""

    def __init__(self, batch: int, level: Optional[LevelConfig] = None, limit: Optional[LimitConfig] = None, device=None):
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"Dynamics: batch must be an int >= 1, got {batch!r}")
        _check_dynamics("Dynamics", level, limit)
        self.batch, self.level, self.limit = int(batch), level, limit
        self.device = torch.device("cuda" if device is None else device)
        self.gains, self.power, self.limiter = cleared_rows(self.batch, level, limit, self.device)

    def reset(self, slots=None) -> None:
        idx = slice(None) if slots is None else torch.as_tensor(sorted(slots), dtype=torch.long, device=self.device)
        fresh = cleared_rows(1, self.level, self.limit, self.device)
        for row, new in zip((self.gains, self.power, self.limiter), fresh):
            if row is not None:
                row[idx] = new[0]
