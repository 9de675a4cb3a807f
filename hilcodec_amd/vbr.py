"""Quality-targeted variable bitrate (VBR) of the graphed sender (graph_step.GraphedEncodeHop(vbr=VbrConfig(...))): the definition, bit
for bit, of hilc_vbr_select (csrc/vbr.hip), and the only module that knows the rules.  Import it by name (`from hilcodec_amd import vbr`).

The residual quantiser is trained with quantiser dropout, so the first s stages of an n-stage code are a valid s-stage code, and the
encoder's caches do not depend on the quantiser: a slot's code can be cut to fewer stages after the fact, exactly.  Per slot and hop
the rule sends the fewest stages whose quantisation error is `target_db` below the energy of the quantiser's input, under an optional
ceiling on the bit rate.  Inputs are assumed finite.  No claim about audio quality is made here: the rule is stated on the quantiser's
own error, and the trained weights are not in this tree.

Per hop the inputs are `z` fp32 [B, T, C] (the quantiser's input, channel-last), `idx` int64 [n, B, T] (stage-major), `codebooks` fp32
[Nq, K, C], `n_b` int [B] (the slot's ceiling, clamped to [1, n]; None: n), `action` / `hold` int [B] or None (the session rows).

Distortion.  Per frame t ascending, r = z[b, t, :]; for s = 0 .. n_b: e(t, s) = |r|^2, then (s < n_b) r[c] = r[c] - codebooks[s, k, c]
             with k = idx[s, b, t] clamped to [0, K): one fp32 subtraction per channel, rvq_encode_kernel's chain.  |r|^2 in float64:
             p[l] = the sum over c = l (mod 64), c ascending, of (double)r[c] (double)r[c], l = 0..63; e = p[0] + p[1] + ... + p[63] in
             that order; every product and every sum is rounded on its own (the idiom of mixer.levels).  D[b, s] = the sum over t
             ascending of e(t, s); D[b, s > n_b] = D[b, n_b].
Quality.     n_q = the smallest s in [lo, n_b] with D[b, s] <= rho D[b, 0] (float64, one rounded product), else n_b; rho =
             10^(-target_db / 10), lo = min(n_b, max(n_min, fec_stages, 1)) (an FEC sender's next packet repeats the first fec_stages
             stages of this hop, so they must exist).
Cap.         An integer token bucket per slot, in bits: stage_bits = 10 T, rate_bits = floor(cap_kbps 1000 T 320 / 24000), burst_bits =
             rate_bits burst_hops, and rate_bits >= stage_bits max(n_min, fec_stages, 1), so the credit never goes negative.  Per hop:
             credit = min(credit + rate_bits, burst_bits); n_cap = clamp(credit // stage_bits, lo, n_b); n_eff = min(n_q, n_cap);
             credit -= n_eff stage_bits.  Without a cap n_eff = n_q.  The cap counts the primary codes only: not the transport
             header, not the redundant FEC section, and a hop that DTX turns into a SID or into silence is still charged.
Sessions.    A slot with an action this hop (a start, a resume) starts from credit = burst_bits, before anything else.  A held slot
             keeps its credit (after such a refill), reports n_eff = n_b and a zero D row.
Indices.     Rows s >= n_eff[b] of slot b's indices become -1, as the quantiser leaves the rows past a slot's n."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from .wire import MAX_STAGES

LANES = 64
MAX_BURST_BITS = 1 << 30                          # credit + rate_bits fits an int32


@dataclass(frozen=True)
class VbrConfig:
    """target_db (> 0): a hop is good enough at the first stage count whose quantisation error is this far below the quantiser input's
    energy; n_min (int >= 1): never fewer stages than this; cap_kbps (None or > 0): the ceiling on the primary codes' bit rate, as a
    token bucket that holds at most burst_hops (int >= 1) hops of it"""
    target_db: float
    n_min: int = 1
    cap_kbps: Optional[float] = None
    burst_hops: int = 8

    def __post_init__(self):
        for name, optional in (("target_db", False), ("cap_kbps", True)):
            v = getattr(self, name)
            if v is None and optional:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                    or not float(v) > 0.0:
                raise ValueError(f"VbrConfig: {name} must be a finite number > 0{' or None' if optional else ''}, got {v!r}")
            object.__setattr__(self, name, float(v))
        for name in ("n_min", "burst_hops"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError(f"VbrConfig: {name} must be an int >= 1, got {v!r}")
            object.__setattr__(self, name, int(v))
        if not 0.0 < self.rho < 1.0:
            raise ValueError(f"VbrConfig: target_db = {self.target_db} gives rho = {self.rho}, outside (0, 1)")

    @property
    def rho(self) -> float:
        """the bar on D[s] / D[0], computed in float64 on the host; the kernel receives this value"""
        return 10.0 ** (-self.target_db / 10.0)


def floor_stages(cfg: VbrConfig, fec_stages: int = 0) -> int:
    """max(n_min, fec_stages, 1): the fewest stages the rule sends (a slot whose ceiling n_b is lower sends n_b)"""
    return max(cfg.n_min, int(fec_stages), 1)


def bucket_bits(cfg: VbrConfig, frames: int, fec_stages: int = 0) -> Tuple[int, int, int]:
    """(stage_bits, rate_bits, burst_bits) of a hop of `frames` frames; (10 frames, 0, 0) without a cap.  ValueError when the rate does
    not pay for the floor of every hop"""
    T = int(frames)
    if T < 1:
        raise ValueError(f"frames must be >= 1, got {frames!r}")
    stage_bits = 10 * T
    if cfg.cap_kbps is None:
        return stage_bits, 0, 0
    rate_bits = math.floor(Fraction(cfg.cap_kbps) * 1000 * T * 320 / 24000)
    need = stage_bits * floor_stages(cfg, fec_stages)
    if rate_bits < need:
        raise ValueError(f"VbrConfig: cap_kbps = {cfg.cap_kbps} is {rate_bits} bits per hop, the floor of {floor_stages(cfg, fec_stages)} "
                         f"stages needs {need}")
    burst_bits = rate_bits * cfg.burst_hops
    if burst_bits > MAX_BURST_BITS:
        raise ValueError(f"VbrConfig: a burst of {burst_bits} bits is more than {MAX_BURST_BITS}")
    return stage_bits, rate_bits, burst_bits


def _np(a, dtype) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def _energy(r: np.ndarray) -> np.ndarray:
    """float64 [...] of fp32 [..., C]: 64 lane partials over the channels, added in lane order"""
    x = r.astype(np.float64)
    C = x.shape[-1]
    p = np.zeros(x.shape[:-1] + (LANES,), dtype=np.float64)
    for base in range(0, C, LANES):
        w = min(LANES, C - base)
        v = x[..., base:base + w]
        p[..., :w] = p[..., :w] + v * v
    e = p[..., 0].copy()
    for lane in range(1, LANES):
        e = e + p[..., lane]
    return e


def _ceilings(n_b, B: int, n: int) -> np.ndarray:
    if n_b is None:
        return np.full(B, n, dtype=np.int64)
    nb = _np(n_b, np.int64).reshape(-1)
    if len(nb) != B:
        raise ValueError(f"n_b needs {B} entries, got {len(nb)}")
    return np.clip(nb, 1, n)


def distortions(z, idx, codebooks, n_b=None) -> np.ndarray:
    """D float64 [B, n + 1] of one hop: z fp32 [B, T, C], idx int64 [n, B, T], codebooks fp32 [Nq, K, C], n_b int [B] or None"""
    z = _np(z, np.float32)
    idx = _np(idx, np.int64)
    cb = _np(codebooks, np.float32)
    if z.ndim != 3 or idx.ndim != 3 or cb.ndim != 3 or idx.shape[1:] != z.shape[:2] or cb.shape[2] != z.shape[2]:
        raise ValueError("distortions: z must be [B, T, C], idx [n, B, T] and codebooks [Nq, K, C]")
    n, B, T = idx.shape
    if not 1 <= n <= min(cb.shape[0], MAX_STAGES):
        raise ValueError(f"distortions: n = {n} outside [1, {min(cb.shape[0], MAX_STAGES)}]")
    K = cb.shape[1]
    nb = _ceilings(n_b, B, n)
    D = np.zeros((B, n + 1), dtype=np.float64)
    r = z.copy()
    for s in range(n + 1):
        e = _energy(r)                                    # [B, T]
        d = e[:, 0].copy()
        for t in range(1, T):
            d = d + e[:, t]
        D[:, s] = np.where(s <= nb, d, D[:, s - 1]) if s else d
        if s < n:
            k = np.clip(idx[s], 0, K - 1)                 # [B, T]
            cut = (r - cb[s][k]).astype(np.float32)
            r = np.where((s < nb)[:, None, None], cut, r)
    return D


def choose(D: np.ndarray, n_b: np.ndarray, lo: np.ndarray, rho: float) -> np.ndarray:
    """n_q int64 [B]: the smallest s in [lo, n_b] with D[b, s] <= rho D[b, 0], else n_b"""
    B = D.shape[0]
    out = np.asarray(n_b, dtype=np.int64).copy()
    bar = np.float64(rho) * D[:, 0]
    for b in range(B):
        for s in range(int(lo[b]), int(n_b[b]) + 1):
            if D[b, s] <= bar[b]:
                out[b] = s
                break
    return out


class VbrModel:
    """numpy statement of hilc_vbr_select for `batch` slots of an n-stage sender with `frames` frames per hop; `credit` int32 [B] is the
    kernel's state row (all zero and unused without a cap)"""

    def __init__(self, batch: int, cfg: VbrConfig, n: int, frames: int, fec_stages: int = 0):
        if not isinstance(cfg, VbrConfig):
            raise ValueError(f"cfg must be a VbrConfig, got {cfg!r}")
        self.B, self.cfg, self.n, self.T = int(batch), cfg, int(n), int(frames)
        if not 1 <= self.n <= MAX_STAGES:
            raise ValueError(f"n = {n} outside [1, {MAX_STAGES}]")
        self.n_lo = floor_stages(cfg, fec_stages)
        self.stage_bits, self.rate_bits, self.burst_bits = bucket_bits(cfg, self.T, fec_stages)
        self.capped = cfg.cap_kbps is not None
        self.credit = torch.full((self.B,), self.burst_bits, dtype=torch.int32)

    def step(self, z, idx, codebooks, n_b=None, action=None, hold=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """one hop -> (n_eff int32 [B], D float64 [B, n + 1], idx_out int64 [n, B, T]); `credit` advances"""
        B, n = self.B, self.n
        idx = _np(idx, np.int64)
        if idx.ndim != 3 or idx.shape[0] != n or idx.shape[1] != B or idx.shape[2] != self.T:
            raise ValueError(f"VbrModel.step: idx must be [{n}, {B}, {self.T}]")
        nb = _ceilings(n_b, B, n)
        lo = np.minimum(nb, self.n_lo)
        fresh = np.zeros(B, dtype=bool) if action is None else _np(action, np.int64).reshape(-1) != 0
        held = np.zeros(B, dtype=bool) if hold is None else _np(hold, np.int64).reshape(-1) != 0
        if len(fresh) != B or len(held) != B:
            raise ValueError(f"VbrModel.step: action and hold need {B} entries")
        D = distortions(z, idx, codebooks, nb)
        n_eff = choose(D, nb, lo, self.cfg.rho)
        if self.capped:
            credit = self.credit.numpy().astype(np.int64)
            credit = np.where(fresh, self.burst_bits, credit)
            filled = np.minimum(credit + self.rate_bits, self.burst_bits)
            n_cap = np.clip(filled // self.stage_bits, lo, nb)
            n_eff = np.minimum(n_eff, n_cap)
            credit = np.where(held, credit, filled - n_eff * self.stage_bits)
            self.credit = torch.from_numpy(credit.astype(np.int32))
        n_eff = np.where(held, nb, n_eff)
        D[held] = 0.0
        out = idx.copy()
        stage = np.arange(n, dtype=np.int64)[:, None]
        out[np.broadcast_to((stage >= n_eff[None, :])[:, :, None], out.shape)] = -1
        return torch.from_numpy(n_eff.astype(np.int32)), torch.from_numpy(D), torch.from_numpy(out)
