"""Polyphase sample-rate conversion between 24 kHz (the codec's rate) and 8 / 16 / 22.05 / 32 / 44.1 / 48 kHz.

The reference loads every input with `librosa.load(PATH, sr=sr)` (test_onnx.py:52), which resamples a file of any rate to the model's
rate.  This is the project's own converter for that step (not librosa's: soxr is neither installed nor bit-reproducible), run by
one HIP kernel (`hilc_resample_poly`, csrc/resample.hip) offline (`hilcodec_amd.resample`), eagerly with a carried history
(`Resampler`) or inside the graphed sender and receiver (graph_step.GraphedEncodeHop(input_rate=), GraphedDecodeHop(output_rate=)).

Definition.  With g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, Z = 40, Q = ceil(2 Z max(L, M) / L) taps per output and
K = L Q, the filter is designed once in float64 and rounded once to fp32:
    fc = 0.93 * 0.5 / max(L, M),  n = k - (K - 1) / 2,  h[k] = L * 2 fc * sinc(2 fc n) * kaiser(K, beta = 8.6)[k]
and stored phase-major, taps[p][j] = h[p + j L].  Output sample m, with ph = (m M) mod L and base = (m M - ph) / L, is
    y[m] = sum_{j = 0 .. Q-1} taps[ph][j] * x[base - j]
summed in order of j from 0, each product and each sum rounded to fp32 on its own: `scipy.signal.upfirdn(h, x, L, M)[:len]` up to
that rounding.  x[i < 0] comes from the history (the last Q - 1 input samples, zero for a fresh stream and offline).  An offline
call on T samples returns ceil(T L / M) of them, as `resample_poly` does.  A streaming hop of 320 F samples at 24 kHz takes
`hop_samples(F, rate)` samples at the other rate; every hop then has the same phase pattern, so hops that start from zero history
give exactly the bits of one offline call on the concatenated signal.

`reference` is the torch CPU statement of this definition, the executable definition the tests compare the kernel against."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

BASE_RATE = 24000
RATES = (8000, 16000, 22050, 32000, 44100, 48000)      # the other side of a conversion; BASE_RATE on both sides: no resampler
ZERO_CROSSINGS = 40
CUTOFF = 0.93
BETA = 8.6
HOP = 320                                                 # codec samples per frame at 24 kHz


@dataclass(frozen=True, eq=False)
class Spec:
    """One direction of conversion: `taps` fp32 `[L, Q]` (phase-major, CPU; do not modify), `delay` the filter's group delay in
    input samples, (K - 1) / (2 L)."""
    sr_in: int
    sr_out: int
    L: int
    M: int
    Q: int
    taps: Tensor
    delay: float

    @property
    def delay_seconds(self) -> float:
        return self.delay / self.sr_in

    @property
    def history(self) -> int:
        """input samples of history a stream carries: Q - 1"""
        return self.Q - 1

    def out_len(self, T: int) -> int:
        """outputs of an offline call on T input samples: ceil(T L / M)"""
        return (int(T) * self.L + self.M - 1) // self.M


def check_rates(sr_in: int, sr_out: int) -> None:
    """ValueError unless one side is 24 000 Hz and the other a supported rate (24 000 included: no resampler)"""
    ok = (sr_in == BASE_RATE and (sr_out == BASE_RATE or sr_out in RATES)) or (sr_out == BASE_RATE and sr_in in RATES)
    if not ok:
        raise ValueError(f"unsupported conversion {sr_in} -> {sr_out} Hz: one side must be {BASE_RATE} and the other one of "
                         f"{RATES} (or {BASE_RATE})")


@lru_cache(maxsize=None)
def design(sr_in: int, sr_out: int) -> Spec:
    """the filter of one direction (see the module docstring); ValueError for an unsupported pair or for 24 000 -> 24 000"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    check_rates(sr_in, sr_out)
    if sr_in == sr_out:
        raise ValueError(f"{sr_in} -> {sr_out} Hz needs no resampler")
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    Q = -(-2 * ZERO_CROSSINGS * max(L, M) // L)
    K = L * Q
    fc = CUTOFF * 0.5 / max(L, M)
    n = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    h = L * 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(K, BETA)
    taps = torch.from_numpy(h.reshape(Q, L).T.copy()).float().contiguous()     # taps[p][j] = h[p + j L]
    return Spec(sr_in, sr_out, L, M, Q, taps, (K - 1) / (2.0 * L))


def hop_samples(frames: int, rate: int) -> int:
    """samples at `rate` of a hop of `frames` codec frames (320 each at 24 kHz); ValueError for an unsupported rate or when that is
    not an integer (naming the smallest frame count it is an integer for)"""
    rate = int(rate)
    if rate != BASE_RATE and rate not in RATES:
        raise ValueError(f"unsupported sample rate {rate}: expected {BASE_RATE} or one of {RATES}")
    if isinstance(frames, bool) or int(frames) != frames or frames < 1:
        raise ValueError(f"frames must be an int >= 1, got {frames!r}")
    num = HOP * int(frames) * rate
    if num % BASE_RATE:
        step = BASE_RATE // math.gcd(HOP * rate, BASE_RATE)
        raise ValueError(f"a hop of {frames} frames is not a whole number of samples at {rate} Hz: frames must be a multiple of {step}")
    return num // BASE_RATE


def reference(x: Tensor, spec: Spec, hist: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """torch CPU statement of the definition: x `[B, 1, T]` (any device; read as fp32) and the history `[B, 1, Q - 1]` (None:
    zeros) -> (y fp32 `[B, 1, ceil(T L / M)]`, the new history `[B, 1, Q - 1]` = the last Q - 1 samples of history || x), on the CPU"""
    x = x.detach().to("cpu", torch.float32)
    if x.dim() != 3 or x.shape[1] != 1:
        raise ValueError(f"x must be [B, 1, T], got {tuple(x.shape)}")
    B, _, T = x.shape
    L, M, Q = spec.L, spec.M, spec.Q
    h = torch.zeros(B, Q - 1) if hist is None else hist.detach().to("cpu", torch.float32).reshape(B, Q - 1)
    ext = torch.cat([h, x.reshape(B, T)], dim=1)                        # x[g] at ext[:, g + Q - 1]
    m = torch.arange(spec.out_len(T), dtype=torch.int64)
    ph, base = (m * M) % L, (m * M) // L
    idx = base[:, None] + (Q - 1) - torch.arange(Q)[None, :]
    tw = spec.taps[ph]
    acc = torch.zeros(B, m.numel())
    for j in range(Q):
        acc = acc + tw[:, j] * ext[:, idx[:, j]]                        # one rounding per product and per sum
    return acc.view(B, 1, -1), ext[:, ext.shape[1] - (Q - 1):].reshape(B, 1, Q - 1).clone()


_DEVICE_TAPS: Dict[Tuple[int, int, str], Tensor] = {}


def device_taps(spec: Spec, device) -> Tensor:
    """the fp32 `[L, Q]` tap table of `spec` on `device`, built once per (rates, device) — before a graph capture"""
    key = (spec.sr_in, spec.sr_out, str(torch.device(device)))
    if key not in _DEVICE_TAPS:
        _DEVICE_TAPS[key] = spec.taps.to(device)
    return _DEVICE_TAPS[key]


def resample(wav: Tensor, orig_sr: int, target_sr: int) -> Tensor:
    """offline: wav fp32 `[B, 1, T]` on the GPU at `orig_sr` -> `[B, 1, ceil(T L / M)]` at `target_sr` (zero history; one kernel
    launch).  One side must be 24 000 Hz, the other a supported rate; equal rates return `wav` itself."""
    from . import ops
    check_rates(int(orig_sr), int(target_sr))
    if int(orig_sr) == int(target_sr):
        return wav
    spec = design(int(orig_sr), int(target_sr))
    return ops.resample_poly(wav, device_taps(spec, wav.device), spec.L, spec.M)


class Resampler:
    """Eager streaming conversion of `batch` streams that carries each stream's history: `y = r(x)` for consecutive chunks x `[batch,
    1, T]` gives the bits of one offline call on their concatenation when every chunk but the last is a multiple of M samples
    (a hop of `hop_samples` is).  `history` `[batch, 1, Q - 1]` is the current history; `reset(history=None)` zeroes or loads it."""

    def __init__(self, orig_sr: int, target_sr: int, batch: int, device):
        self.spec = design(int(orig_sr), int(target_sr))
        self.taps = device_taps(self.spec, device)
        self.history = torch.zeros(int(batch), 1, self.spec.Q - 1, device=device)

    def reset(self, history: Optional[Tensor] = None) -> None:
        if history is None:
            self.history.zero_()
        else:
            self.history = history.to(self.history.device, torch.float32).reshape(self.history.shape).clone()

    def __call__(self, x: Tensor) -> Tensor:
        from . import ops
        hist_out = torch.empty_like(self.history)
        y = ops.resample_poly(x, self.taps, self.spec.L, self.spec.M, hist=self.history, hist_out=hist_out)
        self.history = hist_out
        return y
