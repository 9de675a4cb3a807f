"""CPU: the rules of hilcodec_amd/audio_level.py — the level of a hop, SpeakerConfig's ranges, the bounds that let the unchanged route
kernel sort by the key, and what the rule is for: a room of senders without DTX in which the plain forwarding hop keeps its routes on
the earliest slots, a duel that flips without the margin, and unknown levels, which fall back to the plain selection.  No kernel is
launched here; the conditions of the scenarios are stated by the feature's specification, not measured."""
import itertools

import numpy as np
import pytest

from hilcodec_amd import audio_level, dtx, forward
from hilcodec_amd.audio_level import (MAX_LOUD, SP_LEVELLED, SP_RANK, SP_SCORE, SP_STAGE, SP_STAGED, RankModel, SpeakerConfig,
                                      SpeakerForwardModel, hop_level, loud_row)
from hilcodec_amd.forward import LR_SWITCHES, SD_HANG, SD_SINCE, SD_WORDS, ForwardConfig, ForwardModel
from tests.hops import assert_entry_points
from tests.level_loop import ROOM_SCRIPT, ScriptedRoom, heard_of_wanted


def test_entry_points_and_rows():
    assert_entry_points(("hilc_audio_level", "hilc_forward_rank"), in_abi16_line=True)
    import re
    from tests.hops import HEADER
    defines = dict(re.findall(r"^#define HILC_SPEAKER_(\w+) (\d+)$", open(HEADER).read(), re.M))
    names = dict(SCORE=SP_SCORE, RANK=SP_RANK, STAGE=SP_STAGE, LEVELLED=SP_LEVELLED, STAGED=SP_STAGED, WORDS=audio_level.SP_WORDS,
                 MAX_LOUD=MAX_LOUD, MAX_ATTACK_SHIFT=audio_level.MAX_ATTACK_SHIFT, MAX_DECAY_Q8=audio_level.MAX_DECAY_Q8,
                 MAX_MARGIN_DB=audio_level.MAX_MARGIN_DB)
    assert {k: int(v) for k, v in defines.items()} == names
    from hilcodec_amd import sessions
    assert "loud" in sessions.ONE_HOP_ROWS and audio_level.MAX_LEVEL == dtx.LEVELS - 1 == 127


def test_hop_level_of_known_signals():
    L = 960
    t = np.arange(L)
    sine = np.sin(2 * np.pi * 10 * t / L)                    # whole periods: a mean square of one half
    rows = np.stack([np.zeros(L), np.where(t % 2 == 0, 1.0, -1.0), sine, 0.1 * sine]).astype(np.float32)
    assert hop_level(rows).tolist() == [127, 0, 3, 23]
    assert hop_level(rows[:, None, :]).tolist() == [127, 0, 3, 23]
    assert hop_level(np.full((1, 1), 1e-30, dtype=np.float32)).tolist() == [127]
    # every step of the table, from both sides of each threshold: the level is -dBov rounded to the nearest dB
    for db in (0.4, 0.6, 59.4, 59.6, 125.4, 125.6, 126.4, 126.6):
        x = np.full((1, 64), 10.0 ** (-db / 20.0), dtype=np.float32)
        assert hop_level(x).tolist() == [int(round(db))], db


def test_config_ranges():
    c = SpeakerConfig()
    assert (c.floor_level, c.attack_shift, c.decay_q8, c.margin_db) == (60, 1, 192, 6)
    for field, lo, hi in (("floor_level", 0, 127), ("attack_shift", 0, 4), ("decay_q8", 1, 32768), ("margin_db", 0, 32)):
        SpeakerConfig(**{field: lo})
        SpeakerConfig(**{field: hi})
        for bad in (lo - 1, hi + 1, 1.5, True, None, "3"):
            with pytest.raises(ValueError):
                SpeakerConfig(**{field: bad})


def test_loud_row_and_its_checks():
    c = SpeakerConfig(floor_level=50)
    assert loud_row(5, [3, 1, 3, 4], [30, 127, 20, -1], c).tolist() == [0, 1, 0, 108, 78]
    assert loud_row(3, [0, 0], None, c).tolist() == [78, 0, 0] and loud_row(2, [], None, c).tolist() == [0, 0]
    assert loud_row(2, [1], np.array([0]), c).tolist() == [0, 128]
    for bad in ([128], [-2], [1.0], [True], [1, 2]):
        with pytest.raises(ValueError):
            loud_row(2, [0], bad, c)


def test_key_bounds_at_every_corner():
    """key < 2^24 and the shadow SD_HANG <= 256, which the route kernel's clamps need, at every corner of the config ranges and for
    the loudest sender on stage; the shadow row keeps the counters"""
    corners = itertools.product((0, 127), (0, 4), (1, 32768), (0, 32), (1, 8), (0, 255))
    for floor, attack, decay, margin, fanout, hang in corners:
        cfg, sp = ForwardConfig(fanout=fanout, hang_hops=hang), SpeakerConfig(floor, attack, decay, margin)
        model = RankModel(2, cfg, sp)
        sd = np.zeros((2, SD_WORDS), dtype=np.int32)
        sd[:, SD_HANG], sd[:, SD_SINCE], sd[:, 2:] = hang + 1, 65535, 7
        for _ in range(200):                                 # long enough for the slowest attack to reach full scale
            shadow = model.step(sd, [400, 128], [0, 0])      # 400: clamped to 128
        assert model.state[:, SP_SCORE].tolist() == [256 * 128] * 2 and model.state[:, SP_STAGE].tolist() == [1, int(fanout > 1)]
        key = ((shadow[:, SD_HANG].astype(np.int64) - 1) << 16) | shadow[:, SD_SINCE]
        assert key.max() < 1 << 24 and shadow[:, SD_HANG].max() <= 256 and shadow[:, SD_SINCE].max() <= 65535
        assert key[0] == ((256 * 128 + 256 * margin) << 8) | 255 and (shadow[:, 2:] == 7).all()


def test_score_rank_and_reset():
    cfg, sp = ForwardConfig(fanout=1, hang_hops=2), SpeakerConfig(floor_level=60, attack_shift=1, decay_q8=192, margin_db=6)
    model = RankModel(3, cfg, sp)
    room = np.array([0, 0, 1])
    sd = np.zeros((3, SD_WORDS), dtype=np.int32)
    sd[:, SD_HANG], sd[:, SD_SINCE] = 3, 1
    scores = []
    for h in range(20):
        sd[:, SD_SINCE] = h + 1
        model.step(sd, [108, 98, 108], room)
        scores.append(int(model.state[0, SP_SCORE]))
    assert scores[:3] == [13824, 20736, 24192] and scores[-1] == 256 * 108          # ceil((target - score) / 2) per hop
    assert model.state[:, SP_RANK].tolist() == [0, 1, 0] and model.state[:, SP_STAGE].tolist() == [1, 0, 1]
    assert model.state[:, SP_LEVELLED].tolist() == [20, 20, 20] and model.state[0, SP_STAGED] > 10
    key0 = ((256 * 108 + 256 * 6) << 8) | 20
    assert model.shadow[0].tolist()[:2] == [1 + (key0 >> 16), key0 & 0xFFFF]
    # silence within the hang-over: no level counts, the score decays linearly and the slot leaves the candidates under the floor
    sd[0, SD_HANG] = 2
    model.step(sd, [108, 98, 108], room)
    assert model.state[0, SP_SCORE] == 256 * 108 - 192 and model.state[0, SP_LEVELLED] == 20
    # a join clears the row, and the others see its previous shadow row as zero on that hop
    model.step(sd, [108, 98, 108], room, action=[1, 0, 0])
    assert model.state[0].tolist() == [0, -1, 0, 0, 0] and model.state[1, SP_RANK] == 0 and model.shadow[0, SD_HANG] == 0
    # a slot in no room has no rank but keeps its score
    model.step(sd, [0, 98, 108], np.array([-1, 0, 1]))
    assert model.state[0, SP_RANK] == -1


def _plain_and_ruled(B, cfg, sp, n, T):
    return ForwardModel(B, cfg, n, T), SpeakerForwardModel(B, cfg, sp, n, T)


def test_room_of_senders_without_dtx():
    """6 senders that never stop sending, fanout 2: the plain hop hears at most half of the scripted talkers (its routes sit on the
    earliest slots), the rule at least 95 % of them"""
    B, n, T, hops = 6, 8, 1, 400
    cfg, sp = ForwardConfig(fanout=2, burst=1, hang_hops=8), SpeakerConfig()
    room, layers = np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32)
    join = lambda h: np.full(B, int(h == 0), dtype=np.int32)
    plain, ruled = _plain_and_ruled(B, cfg, sp, n, T)
    heard_p, wanted_p = heard_of_wanted(ScriptedRoom(B, n, T, ROOM_SCRIPT, seed=1), lambda h, s, p, nb, lv:
                                        plain.step(s, p, nb, room, layers, join(h))["routes"], hops)
    heard_r, wanted_r = heard_of_wanted(ScriptedRoom(B, n, T, ROOM_SCRIPT, seed=1), lambda h, s, p, nb, lv:
                                        ruled.step(s, p, nb, lv, room, layers, join(h))["routes"], hops)
    print(f"plain: {heard_p} of {wanted_p}; with the rule: {heard_r} of {wanted_r}, "
          f"{int(ruled.listener.state[0, LR_SWITCHES])} route switches at listener 0")
    assert wanted_p == wanted_r == 520
    assert heard_p <= 0.5 * wanted_p
    assert heard_r >= 0.95 * wanted_r
    assert plain.listener.routes[0].tolist() == [1, 2]                     # for good


def _duel_switches(margin_db):
    B, n, T = 4, 8, 1
    cfg, sp = ForwardConfig(fanout=1, burst=1, hang_hops=8), SpeakerConfig(margin_db=margin_db)
    model = SpeakerForwardModel(B, cfg, sp, n, T)
    net = ScriptedRoom(B, n, T, ((1, 0, 300, 20), (2, 0, 300, 21)), seed=2, background_jitter=0, spike_p=0.0)
    room, layers = np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32)
    for h in range(300):
        slots, packets, nbytes, levels = net.hop(h)
        model.step(slots, packets, nbytes, levels, room, layers, np.full(B, int(h == 0), dtype=np.int32))
    return int(model.listener.state[0, LR_SWITCHES])


def test_duel_needs_the_margin():
    """two talkers 1 dB apart, fanout 1: without a margin listener 0's route flips again and again, with 6 dB it settles"""
    loose, tight = _duel_switches(0), _duel_switches(6)
    print(f"route switches at listener 0 over 300 hops: {loose} with margin_db = 0, {tight} with margin_db = 6")
    assert loose >= 20
    assert tight <= 3


def _settle_hops(sp):
    """the hops the attack of the module docstring's step 3 takes from 0 to the floor's score"""
    target, score, hops = 256 * (MAX_LOUD - sp.floor_level), 0, 0
    while score < target:
        score += (target - score + (1 << sp.attack_shift) - 1) >> sp.attack_shift
        hops += 1
    return hops


def test_unknown_levels_select_as_the_plain_hop():
    """every level -1: all senders settle at the floor's score, keys tie, and tenure then slot decide as in the plain hop.  Senders join
    at different hops, one leaves and joins again; the selected sets are compared on every hop on which every sender has had the
    attack's time to settle since the last join, and has been active for 255 hops or fewer"""
    B, n, T = 6, 8, 1
    cfg, sp = ForwardConfig(fanout=2, burst=1, hang_hops=8), SpeakerConfig()
    plain, ruled = _plain_and_ruled(B, cfg, sp, n, T)
    net = ScriptedRoom(B, n, T, (), seed=3)
    joins = {0: [0, 1], 3: [2], 5: [3, 4], 9: [5], 100: [1]}
    settle = _settle_hops(sp)
    assert settle == 15
    room, layers = np.full(B, -1, dtype=np.int32), np.full(B, n, dtype=np.int32)
    compared = 0
    for h in range(255):
        action = np.zeros(B, dtype=np.int32)
        for b in joins.get(h, ()):
            room[b], action[b] = 0, 1
        slots, packets, nbytes, _ = net.hop(h)
        here = [a for a, b in enumerate(slots) if room[b] >= 0]            # a slot sends from its join on
        args = ([slots[a] for a in here], packets[here], [nbytes[a] for a in here])
        want = plain.step(*args, room, layers, action)["routes"]
        got = ruled.step(*args, [-1] * len(here), room, layers, action)["routes"]
        assert plain.sender.state[:, SD_SINCE].max() <= 255
        if all(h >= j + settle for j in joins if j <= h):
            compared += 1
            assert [set(r) for r in got.tolist()] == [set(r) for r in want.tolist()], h
    assert compared > 200 and (ruled.rank.state[:, SP_SCORE] == 256 * (MAX_LOUD - sp.floor_level)).all()
    assert ruled.rank.state[:, SP_LEVELLED].min() > 150                    # an unknown level counts as a level: the floor's
