"""Audio level and level-based speaker selection of the graphed hops (graph_step.GraphedEncodeHop(audio_level=True),
GraphedForwardHop(speakers=SpeakerConfig(...))): the definition, bit for bit, of hilc_audio_level and hilc_forward_rank
(csrc/audio_level.hip), and the only module that knows their rules.  Import it by name (`from hilcodec_amd import audio_level`).

The forwarding hop (forward.py) never decodes, so it cannot measure who speaks; by itself it selects the senders from whom a codes packet
arrived recently, which tells nothing about senders without DTX.  So the sender says how loud its hop was, as RTP senders do with the
RFC 6464 audio level, and the forwarder ranks by what it was told.

Level of a hop (hilc_audio_level; hop_level(x), x fp32 [B, 1, L] or [B, L], the 24 kHz hop the encoder reads):
  E is mixer.py's "Level" energy: p[l] = the sum over i = l (mod 64), i ascending, of (double)x[i] (double)x[i], E = p[0] + ... + p[63]
  in that order, every product and every sum rounded on its own in float64; m = E / (double)L, one float64 division; level = #{j in
  0..126 : m < thr[j]}, thr = dtx.level_table(), thr[j] = 10^(-(j + 0.5) / 10).  That is -dBov in 1 dB steps in [0, 127]: silence gives
  127, a full-scale square 0, a full-scale sine 3, a sine of amplitude 0.1 gives 23.  A held or stopped slot gives 127 and its row is not
  read.  A row with a NaN gives 0 (a NaN is below no threshold); inputs are assumed finite.

The level travels beside the packet (the wire format is unchanged).  The forwarder takes one level per arrival, 0..127, or -1 for
"unknown", which counts as SpeakerConfig.floor_level; the host reduces them to the loudest per slot (loud_row) and hands the kernel
loud[b] = 128 - level in [1, 128], 0 for a slot without an arrival on this hop.

Rank rule (SpeakerConfig(floor_level, attack_shift, decay_q8, margin_db); hilc_forward_rank, per slot b, after hilc_forward_classify has
finished for every slot and before hilc_forward_route; integer arithmetic only).  Inputs: this hop's sender rows sd (forward.SD_*), the
one-hop row loud (clamped to [0, 128]), the room and action rows, and the PREVIOUS hop's shadow rows.  Outputs: this hop's shadow rows
int32 [B, forward.SD_WORDS] and the speaker rows int32 [B, SP_WORDS]: SP_SCORE, SP_RANK, SP_STAGE and the counters SP_LEVELLED, SP_STAGED.
1. action[b] != 0 clears the speaker row and counts b's previous shadow row as all zero.
2. talk = sd[b][SD_HANG] == hang_hops + 1, a valid codes arrival on this hop.  l = loud[b] if talk, else 0.  SP_LEVELLED += 1 when talk
   and loud[b] > 0.
3. target = 256 l.  With score = SP_SCORE (read clamped to [0, 256 * 128]): if target > score, score += (target - score + 2^a - 1) >> a,
   a = attack_shift; otherwise score = max(target, score - decay_q8).  A fast attack, a linear decay of decay_q8 / 256 dB per hop.
4. SP_RANK = -1 unless room[b] >= 0, action[b] == 0 and b's previous shadow SD_HANG > 0.  Otherwise it is the number of slots s != b with
   room[s] == room[b], action[s] == 0 and a previous shadow SD_HANG > 0 that are ahead of b in the order hilc_forward_route uses, applied
   to the previous shadow rows: SD_HANG descending, SD_SINCE descending, slot ascending (SD_HANG clamped to at most 256, SD_SINCE to [0,
   65535], as that kernel reads them).  SP_STAGE = 0 <= SP_RANK < fanout: the slot was among its room's first `fanout` speakers.
   SP_STAGED += SP_STAGE.
5. candidate = sd[b][SD_HANG] > 0 and score >= 256 (128 - floor_level).
6. key = ((score + (SP_STAGE ? 256 margin_db : 0)) << 8) | min(max(sd[b][SD_SINCE], 0), 255).  score <= 32768 and margin_db <= 32 keep key
   below 2^24.
7. the shadow row is a copy of sd[b] with two words replaced: SD_HANG = candidate ? 1 + (key >> 16) : 0 and SD_SINCE = candidate ? key &
   0xFFFF : 0.  So the shadow SD_HANG is at most 161.

Why shadow rows.  hilc_forward_route clamps SD_HANG to [0, 256] and SD_SINCE to [0, 65535] and sorts by exactly that pair, which is the
key's order.  Handed the shadow rows in place of the sender rows it ranks by key without a change to it, and forward.ListenerModel.step(...,
sender_state=shadow, ...) is its model as it stands.  The real sender rows, GraphedForwardHop.sender_state and everything downlink.py
reads stay what they were.  Why the previous hop's rows in step 4: no slot reads what another writes in the same launch; the price is
that SP_RANK and the margin are one hop behind.

Hysteresis.  The margin goes to a room's first `fanout` ranks only: a newcomer must be margin_db louder than a speaker on stage to take
its place, and the speaker that lost it must be margin_db louder to take it back.  (With fanout + 1 ranks both parties of a duel for the
last route would hold the margin and it would cancel.)  The case this leaves without hysteresis: a listener that is itself on stage
does not hear itself, so its last route goes to the room's rank `fanout`, which holds no margin; two senders duelling for that rank flip
that one route of the `fanout` listeners on stage, and of nobody else.

Ties.  Equal keys fall back to tenure, min(SD_SINCE, 255), then to the lower slot.  With every level unknown all senders that talk settle
at the same score, and once they have, the selected sets are those of the plain hop for as long as every sender has been active for 255
hops or fewer — except that a sender is dropped as soon as its score has decayed under the floor, not after hang_hops.

Out of scope: carrying the level inside the packet; a voice-activity flag; levels of retransmissions (downlink.py answers NACKs from its
history whatever the level was)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import dtx, mixer
from . import forward as forward_def
from .forward import SD_HANG, SD_SINCE, SD_WORDS
from .report import _check_ints

SP_SCORE, SP_RANK, SP_STAGE, SP_LEVELLED, SP_STAGED = range(5)
SP_WORDS = 5
SP_NAMES = ("score", "rank", "stage", "levelled", "staged")

MAX_LEVEL = dtx.LEVELS - 1                                  # 127: silence
MAX_LOUD = 128                                              # loud = MAX_LOUD - level
MAX_ATTACK_SHIFT, MAX_DECAY_Q8, MAX_MARGIN_DB = 4, 32768, 32
UNKNOWN = -1                                                # an arrival without a level


@dataclass(frozen=True)
class SpeakerConfig:
    """level-based speaker selection of a GraphedForwardHop (the rules: this module's docstring).  floor_level in [0, 127]: a sender
    quieter than this level (a larger number) is no candidate, and an unknown level counts as it; attack_shift in [0, 4]: the score
    moves by 2^-attack_shift of its distance to a louder hop; decay_q8 in [1, 32768]: it falls by decay_q8 / 256 dB per hop; margin_db
    in [0, 32]: what a newcomer must be louder by than a speaker on stage"""
    floor_level: int = 60
    attack_shift: int = 1
    decay_q8: int = 192
    margin_db: int = 6

    def __post_init__(self):
        _check_ints("SpeakerConfig", self, (("floor_level", 0, MAX_LEVEL), ("attack_shift", 0, MAX_ATTACK_SHIFT),
                                            ("decay_q8", 1, MAX_DECAY_Q8), ("margin_db", 0, MAX_MARGIN_DB)))


def hop_level(x) -> np.ndarray:
    """level int32 [B] of x fp32 [B, 1, L] (or [B, L]): the module docstring's "Level of a hop" """
    E = mixer.levels(x)
    L = int(np.prod(np.shape(x)[1:]))
    m = E / float(L)
    return (m[:, None] < dtx.level_table()[None, :]).sum(axis=1).astype(np.int32)


def loud_row(batch: int, slots, levels, cfg: SpeakerConfig) -> np.ndarray:
    """one hop's arrivals -> the one-hop row loud int32 [batch]: 128 - the loudest (smallest) level among slot b's arrivals, an unknown
    one counting as cfg.floor_level; 0 for a slot without an arrival.  `slots`: A host ints; `levels`: A host ints in [-1, 127], or
    None: every arrival is unknown.  ValueError for another length or a value outside that range"""
    sl = np.asarray(slots, dtype=np.int64).reshape(-1)
    loud = np.zeros(int(batch), dtype=np.int32)
    if levels is None:
        loud[sl] = MAX_LOUD - int(cfg.floor_level)
        return loud
    raw = np.asarray(levels.numpy() if hasattr(levels, "numpy") else levels)
    if raw.size and (raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer)):
        raise ValueError(f"levels must be ints in [{UNKNOWN}, {MAX_LEVEL}], got {raw.dtype}")
    lv = raw.reshape(-1)
    if len(lv) != len(sl):
        raise ValueError(f"levels: {len(sl)} slots but {len(lv)} levels")
    if len(lv):
        if lv.min() < UNKNOWN or lv.max() > MAX_LEVEL:
            raise ValueError(f"levels must be ints in [{UNKNOWN}, {MAX_LEVEL}]")
        np.maximum.at(loud, sl, (MAX_LOUD - np.where(lv < 0, int(cfg.floor_level), lv)).astype(np.int32))
    return loud


def _order_word(hang, since):
    """the pair hilc_forward_route sorts a sender row by, as one int"""
    return (min(int(hang), forward_def.MAX_HANG_HOPS + 1) << 16) | min(max(int(since), 0), forward_def.MAX_SINCE)


class RankModel:
    """numpy statement of hilc_forward_rank for `batch` slots.  `state` int32 [B, SP_WORDS] are the kernel's speaker rows, `shadow`
    int32 [B, forward.SD_WORDS] the shadow rows of the last hop."""

    def __init__(self, batch: int, cfg: forward_def.ForwardConfig, speakers: SpeakerConfig):
        self.B, self.cfg, self.speakers = int(batch), cfg, speakers
        self.state = np.zeros((self.B, SP_WORDS), dtype=np.int32)
        self.shadow = np.zeros((self.B, SD_WORDS), dtype=np.int32)

    def step(self, sender_state, loud, room, action=None) -> np.ndarray:
        """one hop: `sender_state` int [B, SD_WORDS] as the sender rule of this hop left it, `loud`, `room` and `action` int [B]
        (None: zeros) -> this hop's shadow rows (a copy); `state` and `shadow` are updated in place"""
        B, c, sp = self.B, self.cfg, self.speakers
        sd = np.asarray(sender_state).reshape(B, SD_WORDS)
        loud, room = (np.asarray(v).reshape(-1) for v in (loud, room))
        action = np.zeros(B, dtype=np.int32) if action is None else np.asarray(action).reshape(-1)
        prev = np.where((action != 0)[:, None], 0, self.shadow)
        new = sd.astype(np.int32).copy()
        # the slots that count in step 4, per room, each with its place in the route kernel's order (smaller: ahead)
        order = [(-_order_word(prev[s, SD_HANG], prev[s, SD_SINCE]), s) for s in range(B)]
        ranked = {}
        for s in range(B):
            if room[s] >= 0 and action[s] == 0 and prev[s, SD_HANG] > 0:
                ranked.setdefault(int(room[s]), []).append(order[s])
        for b in range(B):
            row = self.state[b]
            if action[b] != 0:
                row[:] = 0
            talk = int(sd[b, SD_HANG]) == c.hang_hops + 1
            said = min(max(int(loud[b]), 0), MAX_LOUD)
            row[SP_LEVELLED] += int(talk and said > 0)
            target = 256 * said if talk else 0
            score = min(max(int(row[SP_SCORE]), 0), 256 * MAX_LOUD)
            if target > score:
                score += (target - score + (1 << sp.attack_shift) - 1) >> sp.attack_shift
            else:
                score = max(target, score - sp.decay_q8)
            rank = -1
            if room[b] >= 0 and action[b] == 0 and prev[b, SD_HANG] > 0:
                rank = sum(1 for other in ranked[int(room[b])] if other < order[b])
            stage = 0 <= rank < c.fanout
            row[SP_SCORE], row[SP_RANK], row[SP_STAGE] = score, rank, int(stage)
            row[SP_STAGED] += int(stage)
            candidate = sd[b, SD_HANG] > 0 and score >= 256 * (MAX_LOUD - sp.floor_level)
            key = ((score + (256 * sp.margin_db if stage else 0)) << 8) | min(max(int(sd[b, SD_SINCE]), 0), 255)
            new[b, SD_HANG] = 1 + (key >> 16) if candidate else 0
            new[b, SD_SINCE] = key & 0xFFFF if candidate else 0
        self.shadow = new
        return new.copy()


class SpeakerForwardModel(forward_def._Shape):
    """SenderModel, RankModel, then ListenerModel on the shadow rows: one GraphedForwardHop(speakers=) of `batch` slots"""

    def __init__(self, batch: int, cfg: forward_def.ForwardConfig, speakers: SpeakerConfig, n: int, T: int, m: int = 0, K=None):
        super().__init__(batch, cfg, n, T, m, K)
        self.speakers = speakers
        self.sender = forward_def.SenderModel(batch, cfg, n, T, m, K)
        self.rank = RankModel(batch, cfg, speakers)
        self.listener = forward_def.ListenerModel(batch, cfg, n, T, m, K)

    def step_records(self, records, offsets, loud, action, room, layers) -> Dict[str, np.ndarray]:
        """one hop on staged arrivals (forward.arrival_records) and the one-hop row `loud` (loud_row): everything the three kernels
        write, `shadow` among it"""
        res = self.sender.step(records, offsets, action)
        res["shadow"] = self.rank.step(self.sender.state, loud, room, action)
        res.update(self.listener.step(records, action, room, layers, res["shadow"], res["pick"], res["pick_count"]))
        return res

    def step(self, slots, packets, nbytes, levels, room, layers, action=None) -> Dict[str, np.ndarray]:
        """one hop: this hop's arrivals in push order with one level each (`levels`: A ints in [-1, 127], or None: all unknown)"""
        rec, offs = forward_def.arrival_records(slots, packets, nbytes, self.tb, self.B)
        action = np.zeros(self.B, dtype=np.int32) if action is None else action
        return self.step_records(rec, offs, loud_row(self.B, slots, levels, self.speakers), action, room, layers)
