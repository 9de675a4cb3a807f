"""Discontinuous transmission (DTX) and comfort noise (CN) of the graphed sender and receiver
(graph_step.GraphedEncodeHop(dtx=DtxConfig(...)), GraphedDecodeHop(cng_order=K)): the definition, the host tables the kernels
receive, a numpy statement of both kernels (hilc_dtx_encode, hilc_cng_synth in csrc/dtx.hip) that the tests match bit for bit, and
the silence-descriptor (SID) wire helpers.  Import it by name (`from hilcodec_amd import dtx`).

Sender, per stream and hop (S = 320 T samples at 24 kHz, what the encoder sees — after the input resampler when there is one):
  * autocorrelation in float64: lane l of 64 sums x[s] x[s - k] over s = l (mod 64), s >= k, in increasing s (each product of two
    fp32 samples is exact in float64); R[k] = the 64 partials summed in lane order, k = 0..K;
  * the hop is active iff E = R[0] / S >= thr_vad = 10^(threshold_db / 10);
  * Levinson-Durbin in float64 on R'[0] = R[0] (1 + 2^-13), R'[k] = R[k] (`levinson`), reflection coefficients k_1..k_K and the
    residual energy E_K;
  * level L = #{j in 0..126 : E_K / S < thr[j]}, thr[j] = 10^(-(j + 0.5) / 10) (`level_table`): the residual power in 1 dB steps;
  * q_i = clamp(rint(128 k_i), -127, 127) (int8);
  * the state machine of `next_run` / `kind_of` turns the activity into SPEECH / SID / SILENT.
SID packet: byte 0 = L, bytes 1..K = q_i (two's complement): `sid_bytes(K)` = 1 + K bytes.

Receiver, per slot producing noise (c = its count of noise hops since its start, b = its slot index):
  u[s] = fp32(h >> 8) 2^-23 - 1, h = lowbias32(key ^ seed_b), key = (c S + s) mod 2^32, seed_b = (b + 1) 0x9E3779B9 mod 2^32;
  y[s] = g u[s] - a_K y[s - K] - ... - a_1 y[s - 1] in fp32, every product and difference rounded on its own, left to right;
  g = `gain_table()[L]` = sqrt(3) 10^(-L / 20) rounded once to fp32 (sqrt(3): the uniform excitation's variance is 1/3); a = the
  direct-form coefficients of k^_i = q_i / 128 by the step-up recursion in float64, rounded once to fp32 (|k^_i| < 1: the
  synthesis filter is stable in exact arithmetic); y[-K..-1] is the slot's filter memory.  In fp32 a SID whose poles sit at the
  unit circle (e.g. every q_i = -127 at K = 16) can still make the direct form diverge: a hop with some |y[s]| >= NOISE_BOUND or
  a value that is not finite is replaced by zeros and the filter memory is cleared (the hop still counts in c), so a hostile or
  degenerate SID costs silence, never an overflow that would reach the resampler's history."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

HELD, SPEECH, SID, SILENT = 0, 1, 2, 3           # kind of a sender's hop (SILENT: a DTX hop without a packet)
MAX_ORDER = 16
LANES = 64                                        # partial sums of the autocorrelation: one per lane of a wave
LEVELS = 128                                      # L in 0..127
NOISE_FLOOR = 1.0 + 2.0 ** -13                    # R'[0] = R[0] (1 + 2^-13): white-noise correction of the Levinson input
GOLDEN = 0x9E3779B9
NOISE_BOUND = 16.0                                # a noise hop with some |y[s]| >= 16 (or not finite) becomes silence
_MAX_RUN = 1 << 30                                # hangover and sid_interval: run = H + I fits an int32

# CN state row of a receiver slot (int32 words, 3 + 2 K): has-SID, L, c, q_1..q_K, then the K fp32 filter-memory words (y[-K]..y[-1])
ST_HAS, ST_LEVEL, ST_COUNT, ST_Q = 0, 1, 2, 3


def state_words(order: int) -> int:
    return ST_Q + 2 * int(order)


@dataclass(frozen=True)
class DtxConfig:
    """threshold_db: the activity threshold on the hop's mean power (dBFS, a finite float in [-127, 0]); hangover H (int >= 0): the
    inactive hops still sent as speech; sid_interval I (int >= 1): one SID every I hops after the hangover; order K (int in 0..16)"""
    threshold_db: float = -60.0
    hangover: int = 8
    sid_interval: int = 8
    order: int = 8

    def __post_init__(self):
        t = self.threshold_db
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(float(t)) or not -127.0 <= float(t) <= 0.0:
            raise ValueError(f"DtxConfig: threshold_db must be a finite float in [-127, 0], got {t!r}")
        object.__setattr__(self, "threshold_db", float(t))
        for name, lo, hi in (("hangover", 0, _MAX_RUN), ("sid_interval", 1, _MAX_RUN), ("order", 0, MAX_ORDER)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"DtxConfig: {name} must be an int in [{lo}, {hi}], got {v!r}")
            object.__setattr__(self, name, int(v))

    @property
    def thr_vad(self) -> float:
        """the activity threshold on E = R[0] / S, computed in float64 on the host"""
        return 10.0 ** (self.threshold_db / 10.0)


def check_order(order: int, packet_bytes: int, who: str) -> None:
    """a SID of order K must fit the packet row the dequantiser already reads: 1 + K <= packet_bytes"""
    if sid_bytes(order) > packet_bytes:
        raise ValueError(f"{who}: a SID of order {order} needs {sid_bytes(order)} bytes, a packet row holds {packet_bytes}: "
                         f"order must be <= {packet_bytes - 1}")


# ---------------------------------------------------------------- host tables
def level_table() -> np.ndarray:
    """float64 [127]: thr[j] = 10^(-(j + 0.5) / 10), the level thresholds on E_K / S"""
    return np.array([10.0 ** (-(j + 0.5) / 10.0) for j in range(LEVELS - 1)], dtype=np.float64)


def gain_table() -> np.ndarray:
    """float32 [128]: gain[L] = sqrt(3) 10^(-L / 20), computed in float64 and rounded once"""
    return np.array([math.sqrt(3.0) * 10.0 ** (-L / 20.0) for L in range(LEVELS)], dtype=np.float64).astype(np.float32)


# ---------------------------------------------------------------- SID wire helpers
def sid_bytes(order: int) -> int:
    return 1 + int(order)


def pack_sid(level: int, q) -> bytes:
    """(L in 0..127, q_1..q_K int8) -> the 1 + K SID bytes"""
    L = int(level)
    if not 0 <= L < LEVELS:
        raise ValueError(f"level {level} outside [0, 127]")
    q = [int(v) for v in q]
    if any(not -128 <= v <= 127 for v in q):
        raise ValueError("q: int8 values expected")
    return bytes([L] + [v & 0xFF for v in q])


def parse_sid(packet: bytes, order: int) -> Tuple[int, np.ndarray]:
    """the first 1 + K bytes of `packet` -> (L, q int8 [K])"""
    K = int(order)
    blob = bytes(packet)
    if len(blob) < sid_bytes(K):
        raise ValueError(f"a SID of order {K} has {sid_bytes(K)} bytes, got {len(blob)}")
    return blob[0], np.frombuffer(blob[1:1 + K], dtype=np.int8).copy()


# ---------------------------------------------------------------- analysis (hilc_dtx_encode)
def autocorrelation(x, order: int) -> np.ndarray:
    """x fp32 [B, S] (S a multiple of 64) -> R float64 [B, K + 1], summed as the kernel sums"""
    x = np.asarray(x, dtype=np.float32)
    B, S = x.shape
    if S % LANES:
        raise ValueError(f"S = {S} must be a multiple of {LANES}")
    xd = x.astype(np.float64)
    R = np.zeros((B, order + 1))
    for k in range(order + 1):
        prod = np.zeros((B, S))
        prod[:, k:] = xd[:, k:] * xd[:, :S - k]                     # exact: 24-bit x 24-bit mantissas
        prod = prod.reshape(B, S // LANES, LANES)
        part = np.zeros((B, LANES))
        for j in range(S // LANES):                                 # lane l: s = l, l + 64, ... in increasing s
            part = part + prod[:, j]
        r = np.zeros(B)
        for lane in range(LANES):                                   # the partials in lane order
            r = r + part[:, lane]
        R[:, k] = r
    return R


def levinson(R: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """R float64 [B, K + 1] -> (k float64 [B, K] reflection coefficients, E_K float64 [B]), on R'[0] = R[0] (1 + 2^-13).
    k_i = -(R[i] + sum_{j<i} a_j R[i - j]) / E_{i-1} (the sum from R[i] in increasing j), a_i = k_i, a_j += k_i a_{i-j},
    E_i = E_{i-1} (1 - k_i^2); E_{i-1} <= 0 or |k_i| >= 1: k_i..k_K = 0 and the recursion stops (E_K = E_{i-1})"""
    R = np.asarray(R, dtype=np.float64)
    B, K = R.shape[0], R.shape[1] - 1
    a = np.zeros((B, K + 1))
    k = np.zeros((B, K))
    E = R[:, 0] * NOISE_FLOOR
    alive = np.ones(B, dtype=bool)
    for i in range(1, K + 1):
        acc = R[:, i].copy()
        for j in range(1, i):
            acc = acc + a[:, j] * R[:, i - j]
        ok = alive & (E > 0)
        with np.errstate(all="ignore"):
            ki = np.where(ok, -acc / np.where(ok, E, 1.0), 0.0)
        ok &= np.abs(ki) < 1
        ki = np.where(ok, ki, 0.0)
        alive = ok
        new = a.copy()
        for j in range(1, i):
            new[:, j] = a[:, j] + ki * a[:, i - j]
        new[:, i] = ki
        a = np.where(ok[:, None], new, a)
        E = np.where(ok, E * (1.0 - ki * ki), E)
        k[:, i - 1] = ki
    return k, E


def quantize(k: np.ndarray) -> np.ndarray:
    """reflection coefficients -> q int8 = clamp(rint(128 k), -127, 127)"""
    return np.clip(np.rint(np.asarray(k, dtype=np.float64) * 128.0), -127, 127).astype(np.int8)


def analyze(x, cfg: DtxConfig):
    """x fp32 [B, S] -> (active bool [B], level int [B], q int8 [B, K], k float64 [B, K], E_K float64 [B]): hilc_dtx_encode's analysis"""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, Tensor) else x, dtype=np.float32)
    S = x.shape[1]
    R = autocorrelation(x, cfg.order)
    active = R[:, 0] / float(S) >= cfg.thr_vad
    k, E = levinson(R)
    level = (np.asarray(E / float(S))[:, None] < level_table()[None, :]).sum(axis=1)
    return active, level.astype(np.int64), quantize(k), k, E


def next_run(run: int, active: bool, cfg: DtxConfig) -> int:
    """the sender's per-slot counter after one (not held) hop"""
    H, I = cfg.hangover, cfg.sid_interval
    if active:
        return 0
    if run <= H:
        return run + 1
    return H + 1 + (run - H) % I


def kind_of(run: int, active: bool, cfg: DtxConfig) -> int:
    """the kind of a (not held) hop from its NEW run"""
    if active or run <= cfg.hangover:
        return SPEECH
    return SID if run == cfg.hangover + 1 else SILENT


def encode_model(x, run, action, hold, packets, nbytes, indices, prev, cfg: DtxConfig):
    """hilc_dtx_encode on host copies.  x fp32 [B, S]; run int32 [B]; action / hold int32 [B] or None; packets uint8 [B, stride],
    nbytes int32 [B], indices int64 [n, B, T] (what the packer wrote); prev int32 [B, 1 + m T] (the FEC row the packer just wrote)
    or None.  Returns (run, kind, packets, nbytes, indices, prev), new tensors"""
    x = x.detach().cpu().reshape(x.shape[0], -1)
    B = x.shape[0]
    active, level, q, _, _ = analyze(x, cfg)
    run = run.detach().cpu().clone()
    kind = torch.zeros(B, dtype=torch.int32)
    packets, nbytes, indices = packets.detach().cpu().clone(), nbytes.detach().cpu().clone(), indices.detach().cpu().clone()
    prev = None if prev is None else prev.detach().cpu().clone()
    for b in range(B):
        r = 0 if action is not None and int(action[b]) != 0 else int(run[b])
        if hold is not None and int(hold[b]) != 0:
            run[b], kind[b] = r, HELD
            continue
        r = next_run(r, bool(active[b]), cfg)
        kd = kind_of(r, bool(active[b]), cfg)
        run[b], kind[b] = r, kd
        if kd == SPEECH:
            continue
        packets[b] = 0
        if kd == SID:
            blob = pack_sid(int(level[b]), q[b])
            packets[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
            nbytes[b] = len(blob)
        else:
            nbytes[b] = 0
        indices[:, b] = -1
        if prev is not None:
            prev[b, 0] = 0
    return run, kind, packets, nbytes, indices, prev


# ---------------------------------------------------------------- synthesis (hilc_cng_synth)
def lowbias32(h: np.ndarray) -> np.ndarray:
    """the 32-bit integer hash of the excitation (uint32 in, uint32 out; multiplications mod 2^32)"""
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def excitation(slot: int, count: int, S: int) -> np.ndarray:
    """u fp32 [S] of slot b's noise hop c: uniform in [-1, 1)"""
    key = (np.uint64(count) * np.uint64(S) + np.arange(S, dtype=np.uint64)) & 0xFFFFFFFF
    seed = ((int(slot) + 1) * GOLDEN) & 0xFFFFFFFF
    h = lowbias32(key ^ np.uint64(seed))
    return (h >> 8).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)


def step_up(q) -> np.ndarray:
    """q int8 [K] -> the direct-form a_1..a_K (fp32) of k^_i = q_i / 128: the step-up recursion in float64, rounded once"""
    q = np.clip(np.asarray(q, dtype=np.int64), -127, 127)
    K = q.shape[0]
    a = np.zeros(K + 1)
    for i in range(1, K + 1):
        kh = float(q[i - 1]) / 128.0
        new = a.copy()
        for j in range(1, i):
            new[j] = a[j] + kh * a[i - j]
        new[i] = kh
        a = new
    return a[1:].astype(np.float32)


def synthesize(level: int, q, slot: int, count: int, S: int, memory=None) -> Tuple[np.ndarray, np.ndarray]:
    """one noise hop: -> (y fp32 [S], the new filter memory fp32 [K] = y[S - K..S - 1]); `memory` fp32 [K] (y[-K]..y[-1]; None: 0)"""
    q = np.asarray(q)
    K = q.shape[0]
    a = step_up(q)
    g = gain_table()[min(max(int(level), 0), LEVELS - 1)]
    e = g * excitation(slot, count, S)
    y = np.zeros(K + S, dtype=np.float32)
    if memory is not None and K:
        y[:K] = np.asarray(memory, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        _recurse_one(y, e, a, K, S)
    out, mem = y[K:].copy(), y[S:].copy()
    with np.errstate(invalid="ignore"):
        if not np.all(np.abs(out) < NOISE_BOUND):
            out[:], mem[:] = 0.0, 0.0
    return out, mem


def _recurse_one(y, e, a, K, S):
    for s in range(S):
        acc = e[s]
        for j in range(K, 0, -1):
            acc = np.float32(acc - np.float32(a[j - 1] * y[K + s - j]))
        y[K + s] = acc


def _synth_rows(level, q, slots, counts, S, memory) -> Tuple[np.ndarray, np.ndarray]:
    """`synthesize` over several slots at once (the same arithmetic, vectorised over the slots): level int [N], q int8 [N, K],
    slots / counts int [N], memory fp32 [N, K] -> (y [N, S], memory [N, K])"""
    N, K = q.shape
    a = np.stack([step_up(q[i]) for i in range(N)]) if N else np.zeros((0, K), np.float32)
    g = gain_table()[np.clip(level, 0, LEVELS - 1)]
    e = np.stack([g[i] * excitation(slots[i], counts[i], S) for i in range(N)]) if N else np.zeros((0, S), np.float32)
    y = np.zeros((N, K + S), dtype=np.float32)
    y[:, :K] = memory
    with np.errstate(over="ignore", invalid="ignore"):
        _recurse_rows(y, e, a, K, S)
    out, mem = y[:, K:].copy(), y[:, S:].copy()
    with np.errstate(invalid="ignore"):
        wild = ~np.all(np.abs(out) < NOISE_BOUND, axis=1)
    out[wild], mem[wild] = 0.0, 0.0
    return out, mem


def _recurse_rows(y, e, a, K, S):
    for s in range(S):
        acc = e[:, s].copy()
        for j in range(K, 0, -1):
            acc = (acc - (a[:, j - 1] * y[:, K + s - j]).astype(np.float32)).astype(np.float32)
        y[:, K + s] = acc


def cng_model(state, packets, hold, action, order: int, frames: int):
    """hilc_cng_synth on host copies.  state int32 [B, 3 + 2 K] (`state_words`); packets uint8 [B, stride] (a SID slot's row holds
    the SID); hold int32 [B]: 2 = a SID arrived, 3 = silent (DTX, nothing arrived), 0 = decoded this hop, anything else = held;
    action int32 [B] or None (!= 0: a start on this hop clears the state first).  Returns (state, hold, restore, noise), new
    tensors: noise fp32 [B, S] holds the rows of the slots that produce noise (restore[b] = 1; hold[b] becomes 0), a silent slot
    without a SID gets hold[b] = 1."""
    K, S = int(order), 320 * int(frames)
    st = state.detach().cpu().clone()
    hold = hold.detach().cpu().clone()
    pk = packets.detach().cpu()
    B = st.shape[0]
    if action is not None:
        st[action.detach().cpu() != 0] = 0
    restore = torch.zeros(B, dtype=torch.int32)
    noise = torch.zeros(B, S, dtype=torch.float32)
    mem = st[:, ST_Q + K:].contiguous().view(torch.float32)
    make = []
    for b in range(B):
        h = int(hold[b])
        if h == 2:
            L, q = parse_sid(bytes(pk[b].tolist()), K)
            if int(st[b, ST_HAS]) == 0:
                mem[b] = 0
            st[b, ST_HAS], st[b, ST_LEVEL] = 1, min(int(L), LEVELS - 1)
            st[b, ST_Q:ST_Q + K] = torch.from_numpy(np.clip(q.astype(np.int64), -127, 127)).to(torch.int32)
            make.append(b)
        elif h == 3:
            if int(st[b, ST_HAS]):
                make.append(b)
            else:
                hold[b] = 1
        elif h == 0:
            st[b, ST_HAS] = 0
    if make:
        idx = torch.tensor(make)
        counts = (st[idx, ST_COUNT].numpy().astype(np.int64) & 0xFFFFFFFF)
        y, m = _synth_rows(st[idx, ST_LEVEL].numpy().astype(np.int64), st[idx, ST_Q:ST_Q + K].numpy().astype(np.int8),
                           np.array(make), counts, S, mem[idx].numpy())
        noise[idx] = torch.from_numpy(y)
        mem[idx] = torch.from_numpy(m)
        st[idx, ST_COUNT] = torch.from_numpy(((counts + 1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
        hold[idx] = 0
        restore[idx] = 1
    st[:, ST_Q + K:] = mem.view(torch.int32)
    return st, hold, restore, noise


def round_trip(x, cfg: DtxConfig, hops: int, slot: int = 0) -> np.ndarray:
    """`analyze` one hop x fp32 [S] and `synthesize` `hops` consecutive noise hops from its SID (filter memory carried): fp32 [hops S]"""
    x = np.asarray(x, dtype=np.float32).reshape(1, -1)
    _, level, q, _, _ = analyze(x, cfg)
    S = x.shape[1]
    out, mem = [], None
    for c in range(hops):
        y, mem = synthesize(int(level[0]), q[0], slot, c, S, mem)
        out.append(y)
    return np.concatenate(out)
