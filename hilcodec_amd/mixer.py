"""Room mixing of the graphed receiver (graph_step.GraphedDecodeHop(mix=MixConfig(...)), `hilcodec_amd.mix_rooms`): the definition, bit
for bit, of hilc_mix_levels and hilc_mix_rooms (csrc/mix.hip), and the only module that knows the rules.  Inputs are assumed finite.

A conference bridge: every slot of a room hears the room's loudest other members.  Per hop the inputs are the receiver's final output
rows `wav` fp32 [B, 1, L] (whatever produced them: decoded, concealed, FEC, comfort noise, or the zeros of a held slot), `room` int32
[B] (-1: in no room, else a room id in [0, B)), `action` int32 [B] or None (the session row: a start or a resume on this hop) and the
state `score` float64 [B].

Level.   p[l] = the sum over i = l (mod 64), i ascending, of (double)x[i] (double)x[i], l = 0..63; E = p[0] + p[1] + ... + p[63] in that
         order.  Every product and every sum is rounded on its own in float64 (the idiom of hilc_dtx_encode's lag sums).
Score.   score[b] = max(E[b], 0.5 prev[b]), prev[b] = 0 when action[b] != 0.  Every slot, every hop, whatever its room.  The halving
         (a peak hold) keeps the speaker set from flipping on every 13 ms hop.
Select.  The candidates of room r are the slots with room == r and score > 0, ordered by (score descending, slot ascending); the first
         min(top_k, count) are the room's speakers: speakers[b] = 1 for them, 0 for every other slot.
Mix.     For a slot b with room[b] = r >= 0 the terms are the speakers of r other than b in ascending slot order: per sample acc =
         wav[t0][i], then acc = acc + wav[t1][i], ... (every sum rounded in fp32), mixed[b][i] = min(max(acc, -1), 1).  No terms, or
         room[b] < 0: the row is 0.  A held listener still gets its mix; a speaker hears the other speakers only (k - 1 terms).

Out of scope: a stateful soft limiter (the clamp is memoryless), per-speaker gains, and room ids >= B."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

MAX_TOP_K = 8
LANES = 64


@dataclass(frozen=True)
class MixConfig:
    """top_k: the most speakers of a room that are mixed, an int in [1, 8]"""
    top_k: int = 3

    def __post_init__(self):
        v = self.top_k
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"MixConfig.top_k must be an int, got {v!r}")
        if not 1 <= int(v) <= MAX_TOP_K:
            raise ValueError(f"MixConfig.top_k = {v} outside [1, {MAX_TOP_K}]")


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


def mix(wav: np.ndarray, room: np.ndarray, speakers: np.ndarray) -> np.ndarray:
    """mixed fp32 [B, L] of wav fp32 [B, L]"""
    B, L = wav.shape
    out = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        if room[b] < 0:
            continue
        terms = [t for t in range(B) if room[t] == room[b] and speakers[t] and t != b]
        if not terms:
            continue
        acc = wav[terms[0]].copy()
        for t in terms[1:]:
            acc = (acc + wav[t]).astype(np.float32)
        out[b] = np.minimum(np.maximum(acc, np.float32(-1)), np.float32(1))
    return out


class MixModel:
    """numpy statement of hilc_mix_levels + hilc_mix_rooms for `batch` slots; `score` float64 [B] is the kernels' state row.  (No soft
    limiter with state, no per-speaker gains, no room ids >= B: see the module docstring.)"""

    def __init__(self, batch: int, cfg: Optional[MixConfig] = None):
        self.B, self.cfg = int(batch), cfg if cfg is not None else MixConfig()
        self.score = torch.zeros(self.B, dtype=torch.float64)

    def step(self, wav, room, action=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """one hop: wav fp32 [B, 1, L], room int [B], action int [B] or None -> (mixed fp32 [B, 1, L], speakers int32 [B]); `score`
        advances"""
        x = _np(wav, np.float32)
        if x.shape[0] != self.B or x.size == 0:
            raise ValueError(f"MixModel.step: wav must be [{self.B}, 1, L >= 1]")
        x = x.reshape(self.B, -1)
        rm = _np(room, np.int64).reshape(-1)
        if len(rm) != self.B:
            raise ValueError(f"MixModel.step: room needs {self.B} entries")
        score = update_score(self.score.numpy(), levels(x), action)
        self.score = torch.from_numpy(score)
        speakers = select(rm, score, int(self.cfg.top_k))
        mixed = mix(x, rm, speakers)
        return torch.from_numpy(mixed).view(self.B, 1, -1), torch.from_numpy(speakers)
