"""GPU: the audio level and level-based speaker selection (hilcodec_amd/audio_level.py).  hilc_audio_level against hop_level;
hilc_forward_rank and the unchanged hilc_forward_route on its shadow rows against RankModel + ListenerModel under
tests/level_loop.py's traffic; GraphedForwardHop(speakers=) against the three ops called eagerly and the models, with the downlink
launches behind it, and room by room; GraphedEncodeHop(audio_level=True) against hop_level of its input, against the hop without the
option, behind the input resampler and in front of a forwarder.  Everything is an integer or one defined float64 chain: every
comparison is bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import audio_level, downlink, dtx, forward, synth, wire
from hilcodec_amd.audio_level import (SP_LEVELLED, SP_RANK, SP_STAGED, SP_WORDS, SpeakerConfig, SpeakerForwardModel, hop_level, loud_row)
from hilcodec_amd.downlink import DownlinkConfig, ForwardDownlinkModel
from hilcodec_amd.forward import LR_SWITCHES, LR_WORDS, SD_WORDS, ForwardConfig
from hilcodec_amd.rate import RateConfig
from tests.downlink_loop import Feedback
from tests.forward_loop import Membership
from tests.hops import caches_equal
from tests.level_loop import LevelTraffic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
INTS = dict(dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


@pytest.fixture(scope="module")
def thr():
    return torch.from_numpy(dtx.level_table()).to(DEV)


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


# ---------------------------------------------------------------- hilc_audio_level
def level_rows(B, L, seed):
    """rows of zeros, full scale, 1e-30 and random values at scales from full scale down to under the quietest level"""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        kind = (b + seed) % 5
        if kind == 1:
            x[b] = np.where(rng.random(L) < 0.5, 1.0, -1.0)
        elif kind == 2:
            x[b] = 1e-30
        elif kind >= 3:
            x[b] = np.clip(rng.standard_normal(L) * 10.0 ** (-rng.uniform(0.0, 7.0)), -1.0, 1.0)
    return x


# one wave, a ragged last workgroup of four waves, more than 64 slots; a hop shorter than a wave, around its 64 lanes, 1 and 3 frames
@pytest.mark.parametrize("L", [1, 63, 65, 320, 960])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_audio_level_against_hop_level(B, L, thr):
    from hilcodec_amd import ops
    x = level_rows(B, L, seed=B + L)
    want = hop_level(x)
    xd = torch.from_numpy(x).to(DEV)
    level = torch.full((B,), -9, **INTS)
    assert ops.audio_level(xd.view(B, 1, L), thr, level) is level
    assert np.array_equal(level.cpu().numpy(), want), (level.tolist(), want.tolist())
    assert np.array_equal(ops.audio_level(xd, thr).cpu().numpy(), want)          # [B, L], a new tensor
    if B >= 5:
        assert {0, 127} <= set(want.tolist()) and (B < 70 or len(set(want.tolist())) >= 4)
    # a NaN row beside the others does not change them
    b_nan = B // 2
    xn = xd.clone()
    xn[b_nan, L // 2] = float("nan")
    got = ops.audio_level(xn, thr).cpu().numpy()
    keep = np.arange(B) != b_nan
    assert np.array_equal(got[keep], want[keep]) and got[b_nan] == hop_level(xn.cpu().numpy())[b_nan] == 0
    # hold marks give 127, whatever the row holds
    hold = np.zeros(B, dtype=np.int32)
    hold[::2] = np.arange(1, 1 + len(hold[::2]))
    got = ops.audio_level(xn, thr, hold=dev(hold)).cpu().numpy()
    assert np.array_equal(got, np.where(hold != 0, 127, hop_level(xn.cpu().numpy())))


# ---------------------------------------------------------------- hilc_forward_rank, then hilc_forward_route
class Rows:
    """the device rows of the three launches for B slots, filled so that an element a launch does not write shows"""

    def __init__(self, B, cfg, tb):
        F, P = cfg.fanout, cfg.burst
        self.sd, self.lr = torch.zeros(B, SD_WORDS, **INTS), torch.zeros(B, LR_WORDS, **INTS)
        self.shadow, self.sp = torch.zeros(2, B, SD_WORDS, **INTS), torch.zeros(B, SP_WORDS, **INTS)
        self.pick, self.pick_count = torch.zeros(B, P, **INTS), torch.zeros(B, **INTS)
        self.routes, self.new_routes = torch.full((B, F), -1, **INTS), torch.zeros(B, F, **INTS)
        self.out, self.out_nbytes = torch.zeros(B, F, P, tb, dtype=torch.uint8, device=DEV), torch.zeros(B, F, P, **INTS)
        self.p = 0

    def run(self, arr, offs, loud, action, room, layers, cfg, sp, n, T, m, K):
        from hilcodec_amd import ops
        for t in (self.pick, self.pick_count, self.new_routes, self.out_nbytes, self.shadow[self.p ^ 1]):
            t.fill_(-9)
        self.out.fill_(0xEE)
        ops.forward_classify(arr, offs, self.sd, self.pick, self.pick_count, cfg, n, T, m, K, action=action)
        ops.forward_rank(self.sd, loud, room, self.shadow[self.p], self.shadow[self.p ^ 1], self.sp, cfg, sp, action=action)
        self.p ^= 1                                          # the parities alternate: this hop's rows are the next hop's previous ones
        ops.forward_route(arr, room, layers, self.shadow[self.p], self.pick, self.pick_count, self.routes, self.new_routes, self.lr,
                          self.out, self.out_nbytes, cfg, n, T, m, K, action=action)

    def differs_from(self, res, model):
        """None, or the name of the first row that is not the model's"""
        got = dict(pick=self.pick, pick_count=self.pick_count, shadow=self.shadow[self.p], routes=self.routes,
                   new_routes=self.new_routes, out=self.out, out_nbytes=self.out_nbytes)
        for name, t in got.items():
            if not np.array_equal(t.cpu().numpy(), res[name]):
                return name
        for name, t, want in (("sender_state", self.sd, model.sender.state), ("speaker_state", self.sp, model.rank.state),
                              ("listener_state", self.lr, model.listener.state)):
            if not np.array_equal(t.cpu().numpy(), want):
                return name
        return None


SPEAKERS = {1: SpeakerConfig(), 3: SpeakerConfig(floor_level=50, attack_shift=0, decay_q8=1000, margin_db=0),
            8: SpeakerConfig(floor_level=70, attack_shift=2, decay_q8=64, margin_db=32)}
# (B, rooms, T): the ragged last workgroup of 4 waves, one and three frames; one room whose candidate scan goes past 64 lanes; nobody to rank
RANK_CASES = [(B, rooms, T, F) for B, rooms, T in ((5, 2, 1), (5, 2, 3), (70, 1, 1), (1, 1, 1)) for F in (1, 3, 8)]


@pytest.mark.parametrize("case", RANK_CASES, ids=lambda c: "B{}-rooms{}-T{}-F{}".format(*c))
def test_rank_and_route_against_the_models(case):
    """64 hops of the generator's traffic with joins, leaves and layer changes and levels that tie: every row of the three launches is
    the models' on every hop"""
    B, rooms, T, F = case
    n, m, K = (8, 2, 8) if T == 3 else (8, 0, None)
    cfg, sp = ForwardConfig(fanout=F, burst=2, hang_hops=3), SPEAKERS[F]
    model, mem = SpeakerForwardModel(B, cfg, sp, n, T, m, K), Membership(B, n)
    net = LevelTraffic(B, n, T, m, K, rooms, seed=B + 7 * T + F, p_event=0.3)
    tb = model.tb
    rows = Rows(B, cfg, tb)
    mem.apply(net.initial_events())
    for h in range(64):
        mem.apply(net.events())
        slots, packets, nbytes, levels = net.hop()
        rec, offs = forward.arrival_records(slots, packets, nbytes, tb, B, 8 * B)
        loud, action = loud_row(B, slots, levels, sp), mem.action()
        want = model.step_records(rec, offs, loud, action, mem.room, mem.layers)
        rows.run(dev(rec), dev(offs), dev(loud), dev(action), dev(mem.room), dev(mem.layers), cfg, sp, n, T, m, K)
        assert rows.differs_from(want, model) is None, (h, rows.differs_from(want, model))
    spk, lr = model.rank.state, model.listener.state
    if B > 1:                                                # the traffic reached the rule
        assert spk[:, SP_LEVELLED].sum() > 0 and spk[:, SP_STAGED].sum() > 0 and lr[:, LR_SWITCHES].sum() > 0
        assert not np.array_equal(model.rank.shadow, model.sender.state)
    else:
        assert spk[0, SP_RANK] in (-1, 0) and not lr.any()
    # without an action row no slot is cleared
    want = model.step_records(rec, offs, loud, np.zeros(B, dtype=np.int32), mem.room, mem.layers)
    rows.run(dev(rec), dev(offs), dev(loud), None, dev(mem.room), dev(mem.layers), cfg, sp, n, T, m, K)
    assert rows.differs_from(want, model) is None


def test_rank_argument_checks(thr):
    """every bad argument returns its error code and launches nothing; the ops check the widths of their rows"""
    from hilcodec_amd import _lib, ops
    lib = _lib.lib
    SHAPE, NULL, UNSUPPORTED, RANGE = -1, -2, -4, -5
    B = 3
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    sd, loud, room, act, prev, sp = z(B, SD_WORDS), z(B), z(B), z(B), z(B, SD_WORDS), z(B, SP_WORDS)
    shadow = torch.full((B, SD_WORDS), -9, **INTS)
    p = lambda t: t.data_ptr()
    good = [p(sd), p(loud), p(room), p(act), p(prev), p(shadow), p(sp), B, 3, 8, 60, 1, 192, 6, None]
    for i in (0, 1, 2, 4, 5, 6):
        assert lib.hilc_forward_rank(*[None if j == i else v for j, v in enumerate(good)]) == NULL, i
    for i, v, code in ((7, 0, SHAPE), (8, 0, RANGE), (8, 9, RANGE), (9, -1, RANGE), (9, 256, RANGE), (10, -1, RANGE), (10, 128, RANGE),
                       (11, -1, RANGE), (11, 5, RANGE), (12, 0, RANGE), (12, 32769, RANGE), (13, -1, RANGE), (13, 33, RANGE),
                       (5, p(prev), UNSUPPORTED), (5, p(sd), UNSUPPORTED)):
        assert lib.hilc_forward_rank(*[v if j == i else w for j, w in enumerate(good)]) == code, (i, v)
    x, level = torch.ones(B, 8, device=DEV), torch.full((B,), -9, **INTS)
    good_l = [p(x), p(thr), None, p(level), B, 8, None]
    for i in (0, 1, 3):
        assert lib.hilc_audio_level(*[None if j == i else v for j, v in enumerate(good_l)]) == NULL, i
    for i in (4, 5):
        assert lib.hilc_audio_level(*[0 if j == i else v for j, v in enumerate(good_l)]) == SHAPE, i
    torch.cuda.synchronize()
    assert bool((shadow == -9).all()) and bool((level == -9).all()) and not sp.any()      # a refused call launches nothing
    assert lib.hilc_forward_rank(*good) == 0 and lib.hilc_audio_level(*good_l) == 0
    assert lib.hilc_forward_rank(*[None if j == 3 else v for j, v in enumerate(good)]) == 0      # the action row is optional
    torch.cuda.synchronize()
    assert not shadow.any() and level.tolist() == [0] * B
    cfg, spk = ForwardConfig(), SpeakerConfig()
    args = dict(sender_rows=sd, loud=loud, room=room, shadow_prev=prev, shadow=shadow, rows=sp)
    for name, bad in (("sender_rows", z(B, SD_WORDS + 1)), ("loud", z(B + 1)), ("shadow_prev", z(B + 1, SD_WORDS)), ("shadow", z(B, 5)),
                      ("rows", z(B, SP_WORDS + 1)), ("room", z(B).cpu())):
        with pytest.raises(RuntimeError):
            ops.forward_rank(**{**args, name: bad}, cfg=cfg, speakers=spk)
    for bad in (dict(x=x.cpu()), dict(thr=thr[:-1]), dict(x=torch.ones(B + 1, 8, device=DEV)), dict(hold=z(B + 1))):
        with pytest.raises(RuntimeError):
            ops.audio_level(**{**dict(x=x, thr=thr, level=level), **bad})


# ---------------------------------------------------------------- the graphed forwarding hop
def rate_for(T, m, fcfg):
    """a RateConfig whose minimum just pays for the floor of a hop, so that the bucket limits some hops and not others"""
    kbps = (downlink.floor_bits(T, m, fcfg.fanout, fcfg.keep_fec) + 1) * 24000.0 / (1000.0 * T * 320.0)
    return RateConfig(min_kbps=kbps, max_kbps=2 * kbps, start_kbps=kbps, burst_hops=3, timeout_hops=10)


def test_graph_against_eager_and_models():
    """GraphedForwardHop(speakers=).forward over 48 replays (some without arrivals, some without levels) equals the three ops called
    eagerly on the same staged inputs and the models; sender_state stays the real rows; the argument checks of `levels`"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T, m, K = 9, 8, 1, 2, 8
    cfg, sp = ForwardConfig(fanout=3, burst=2, hang_hops=3), SpeakerConfig(floor_level=50, margin_db=3)
    hop = GraphedForwardHop(B, T, n, DEV, fec_stages=m, cng_order=K, cfg=cfg, max_arrivals=8 * B, speakers=sp)
    model, mem = SpeakerForwardModel(B, cfg, sp, n, T, m, K), Membership(B, n)
    net = LevelTraffic(B, n, T, m, K, 2, seed=31, p_event=0.15)
    tb = model.tb
    eager = Rows(B, cfg, tb)
    assert not hop.speaker_state.any() and tuple(hop.speaker_rank.shape) == (B,)
    mem.apply(net.initial_events(), hop)
    quiet_hops = unknown_hops = 0
    for h in range(48):
        mem.apply(net.events() if h % 3 == 0 else [], hop)
        slots, packets, nbytes, levels = net.hop() if h % 7 != 5 else ([], np.zeros((0, tb), dtype=np.uint8), [], [])
        if h % 5 == 4:
            levels = None                                    # every arrival unknown
        elif h % 2:
            levels = torch.tensor(levels, dtype=torch.int64)
        quiet_hops += not slots
        unknown_hops += levels is None
        t_packets = torch.from_numpy(packets).to(DEV) if h % 2 else torch.from_numpy(packets)
        out, out_nbytes = hop.forward(slots, t_packets, nbytes, levels)
        action = mem.action()
        want = model.step(slots, packets, nbytes, levels, mem.room, mem.layers, action)
        st = hop.stage
        loud = loud_row(B, slots, levels, sp)
        assert np.array_equal(st.row["loud"].cpu().numpy(), loud), h         # exactly this hop's levels are on the device
        assert np.array_equal(st.row["action"].cpu().numpy(), action) and np.array_equal(st.row["room"].cpu().numpy(), mem.room)
        eager.run(hop.arrivals.clone(), hop.offsets.clone(), st.row["loud"].clone(), st.row["action"].clone(), st.row["room"].clone(),
                  st.row["layers"].clone(), cfg, sp, n, T, m, K)
        assert eager.differs_from(want, model) is None, (h, eager.differs_from(want, model))
        for name, t in (("out", out), ("out_nbytes", out_nbytes), ("routes", hop.routes), ("new_routes", hop.new_routes)):
            assert np.array_equal(t.cpu().numpy(), want[name]), (h, name)
        assert torch.equal(hop.sender_state, eager.sd) and torch.equal(hop.listener_state, eager.lr), h
        assert np.array_equal(hop.sender_state.cpu().numpy(), model.sender.state), h     # the real rows, not the shadow ones
        assert torch.equal(hop.speaker_state, eager.sp) and torch.equal(hop.speaker_rank, eager.sp[:, SP_RANK]), h
    assert quiet_hops >= 3 and unknown_hops >= 8 and model.rank.state[:, SP_STAGED].sum() > 20
    assert not np.array_equal(model.rank.shadow, model.sender.state)
    before = hop.speaker_state.clone()
    one = ([0], torch.zeros(1, tb, dtype=torch.uint8), [5])
    for bad in ([128], [-2], [0, 1], [], [0.5], torch.zeros(1, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError):
            hop.forward(*one, bad)
    assert torch.equal(hop.speaker_state, before)            # nothing ran
    plain = GraphedForwardHop(3, T, n, DEV, cfg=cfg)
    with pytest.raises(ValueError):
        plain.forward([0], torch.zeros(1, plain.tstride, dtype=torch.uint8), [5], levels=[20])
    for bad in (lambda: plain.speaker_state, lambda: plain.speaker_rank):
        with pytest.raises(RuntimeError):
            bad()
    assert "loud" not in plain.stage.row
    with pytest.raises(ValueError):
        GraphedForwardHop(3, T, n, DEV, cfg=cfg, speakers=cfg)


class _Ranked:
    """SpeakerForwardModel in ForwardDownlinkModel's `forward` seat: the hop's loudness row is set beside the call"""

    def __init__(self, model):
        self.model, self.loud = model, None
        self.cfg, self.B, self.tb, self.listener, self.sender = model.cfg, model.B, model.tb, model.listener, model.sender

    def step_records(self, records, offsets, action, room, layers):
        return self.model.step_records(records, offsets, self.loud, action, room, layers)


def test_graph_with_the_downlink_launches():
    """GraphedForwardHop(speakers=, downlink=): the downlink launches follow unchanged on the routes the shadow rows selected — the
    hop equals ForwardDownlinkModel fed the shadow-ranked routes, on every hop of 48"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T, m, K = 9, 8, 1, 2, 8
    fcfg, sp = ForwardConfig(fanout=3, burst=2, hang_hops=3), SpeakerConfig(floor_level=50)
    dcfg = DownlinkConfig(rate=rate_for(T, m, fcfg), history=8, per_hop=2)
    hop = GraphedForwardHop(B, T, n, DEV, fec_stages=m, cng_order=K, cfg=fcfg, max_arrivals=8 * B, downlink=dcfg, speakers=sp)
    model, mem = ForwardDownlinkModel(B, fcfg, dcfg, n, T, m, K), Membership(B, n)
    ranked = model.forward = _Ranked(SpeakerForwardModel(B, fcfg, sp, n, T, m, K))
    net, fbk = LevelTraffic(B, n, T, m, K, 2, seed=37, p_event=0.15), Feedback(B, fcfg.fanout, dcfg.history, 37, p_report=0.3, p_nack=0.3)
    mem.apply(net.initial_events(), hop)
    VIEWS = ("routes", "new_routes", "eff_layers", "rtx_packets", "rtx_nbytes", "rtx_routes")
    for h in range(48):
        mem.apply(net.events() if h % 3 == 0 else [], hop)
        reports, nacks = fbk.hop(ranked.listener.routes, net.traffic.h)
        if h % 5 in (3, 4):
            reports = nacks = None
        slots, packets, nbytes, levels = net.hop()
        out, out_nbytes = hop.forward(slots, torch.from_numpy(packets), nbytes, levels, reports=reports, nacks=nacks)
        ranked.loud = loud_row(B, slots, levels, sp)
        want = model.step(slots, packets, nbytes, mem.room, mem.layers, mem.action(), reports=reports, nacks=nacks)
        got = dict(out=out, out_nbytes=out_nbytes, **{v: getattr(hop, v) for v in VIEWS})
        for name, t in got.items():
            assert np.array_equal(t.cpu().numpy(), want[name]), (h, name)
        for name, t, rows in (("downlink_state", hop.downlink_state, model.downlink.state), ("sender_state", hop.sender_state, ranked.sender.state),
                              ("listener_state", hop.listener_state, ranked.listener.state), ("speaker_state", hop.speaker_state, ranked.model.rank.state),
                              ("history_state", hop.history_state, model.downlink.sender_state)):
            assert np.array_equal(t.cpu().numpy(), rows), (h, name)
    d = model.downlink.state
    assert all(d[:, w].sum() > 0 for w in (downlink.DL_REPORTS, downlink.DL_PACKETS))
    assert ranked.model.rank.state[:, SP_STAGED].sum() > 20


def test_rooms_do_not_hear_each_others_levels():
    """two rooms, the same packets, other levels in room B: every row of room A's slots is the same"""
    from hilcodec_amd.graph_step import GraphedForwardHop
    B, n, T = 10, 8, 1
    cfg, sp = ForwardConfig(fanout=2, burst=2, hang_hops=3), SpeakerConfig()
    hops = [GraphedForwardHop(B, T, n, DEV, cfg=cfg, max_arrivals=8 * B, speakers=sp) for _ in (0, 1)]
    nets = [LevelTraffic(B, n, T, 0, None, 2, seed=41, p_event=0.0) for _ in (0, 1)]
    rng = np.random.default_rng(43)
    in_a = np.arange(B) % 2 == 0                             # initial_events: slot b joins room b % 2
    for hop, net in zip(hops, nets):
        Membership(B, n).apply(net.initial_events(), hop)
    differed = 0
    for h in range(40):
        (slots, packets, nbytes, levels), (slots_b, packets_b, _nb, _lv) = nets[0].hop(), nets[1].hop()
        assert slots == slots_b and np.array_equal(packets, packets_b)
        other = [int(rng.choice([10, 30, 90, -1])) if not in_a[s] else lv for s, lv in zip(slots, levels)]
        res = []
        for hop, lv in zip(hops, (levels, other)):
            out, out_nbytes = hop.forward(slots, torch.from_numpy(packets), nbytes, lv)
            res.append([t.cpu().numpy() for t in (out, out_nbytes, hop.routes, hop.new_routes, hop.listener_state, hop.speaker_state)])
        for x, y in zip(*res):
            assert np.array_equal(x[in_a], y[in_a]), h
        differed += not np.array_equal(res[0][2][~in_a], res[1][2][~in_a])
    assert differed > 0                                      # room B's routes did follow its own levels


# ---------------------------------------------------------------- the graphed sender
def test_sender_measures_its_hop(speech):
    """GraphedEncodeHop(audio_level=True, header=True): `audio_level` is hop_level of the input on every hop, 127 for a held slot, and
    it stays valid for one further step; packets, byte counts, indices and caches are those of the hop without the option"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, n, hops = 4, 8, 8
    kw = dict(sessions=True, header=True)
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, audio_level=True, **kw)
    plain = GraphedEncodeHop(speech, B, HOP, n, DEV, **kw)
    x = synth.synth_clips(B, HOP * hops, seed=21)
    x = (x * torch.tensor([1.0, 0.1, 0.003, 0.0]).view(B, 1, 1)).to(DEV)
    assert tx.audio_level.tolist() == [127] * B
    with pytest.raises(RuntimeError):
        plain.audio_level
    held = None
    for h in range(hops):
        xs = x[:, :, HOP * h:HOP * (h + 1)].contiguous()
        hold = [1] if h in (3, 4) else None
        packets, nbytes = tx.step(xs, hold=hold)
        p_packets, p_nbytes = plain.step(xs, hold=hold)
        want = hop_level(xs.cpu().numpy())
        if hold:
            want[1] = 127
        level = tx.audio_level
        assert np.array_equal(level.cpu().numpy(), want), (h, level.tolist(), want.tolist())
        assert torch.equal(packets, p_packets) and torch.equal(nbytes, p_nbytes) and torch.equal(tx.indices, plain.indices), h
        assert caches_equal(tx.cache_enc, plain.cache_enc) and torch.equal(tx.hop_index, plain.hop_index), h
        if held is not None:
            assert np.array_equal(held[0].cpu().numpy(), held[1]), h
        held = (level, want)
    assert want[3] == 127 and want[0] < want[1] < want[2] < 127
    tx.reset()
    assert tx.audio_level.tolist() == [127] * B


def test_sender_measures_behind_the_resampler(speech, thr):
    """input_rate=16000: the level is that of the 24 kHz hop the encoder reads — resample_poly and audio_level called eagerly"""
    from hilcodec_amd import ops
    from hilcodec_amd.graph_step import GraphedEncodeHop
    from hilcodec_amd.resample import BASE_RATE, design, device_taps, hop_samples
    B, n, frames, rate = 4, 8, 3, 16000
    n_in = hop_samples(frames, rate)
    tx = GraphedEncodeHop(speech, B, HOP * frames, n, DEV, input_rate=rate, audio_level=True)
    s = design(rate, BASE_RATE)
    taps = device_taps(s, DEV)
    x = synth.synth_clips(B, n_in * 4, seed=22)
    x = (x * torch.tensor([1.0, 0.2, 0.01, 0.0005]).view(B, 1, 1)).to(DEV)
    hist = torch.zeros(B, 1, s.history, device=DEV)
    seen = set()
    for h in range(4):
        xs = x[:, :, n_in * h:n_in * (h + 1)].contiguous()
        tx.step(xs)
        hist_out = torch.empty_like(hist)
        y = ops.resample_poly(xs, taps, s.L, s.M, hist=hist, hist_out=hist_out)
        hist = hist_out
        assert tuple(y.shape) == (B, 1, HOP * frames)
        assert torch.equal(tx.audio_level, ops.audio_level(y, thr)), h
        assert np.array_equal(tx.audio_level.cpu().numpy(), hop_level(y.cpu().numpy())), h
        seen |= set(tx.audio_level.tolist())
    assert len(seen) >= 4


def test_sender_levels_steer_the_forwarder(speech):
    """six senders without DTX into one room, fanout 1: the levels the senders measured, fed to the forwarder beside their packets,
    make listener 0's route follow whoever is loud — slot 4, then the louder slot 2 — where the plain hop stays on slot 1"""
    from hilcodec_amd.graph_step import GraphedEncodeHop, GraphedForwardHop
    B, n, hops = 6, 8, 56
    talk = {4: (5, 28, 0.1), 2: (30, 56, 1.0)}               # slot: from, to, amplitude; everybody else murmurs
    cfg, sp = ForwardConfig(fanout=1, burst=1, hang_hops=8), SpeakerConfig()
    tx = GraphedEncodeHop(speech, B, HOP, n, DEV, header=True, audio_level=True)
    fwd = GraphedForwardHop(B, 1, n, DEV, cfg=cfg, speakers=sp)
    plain = GraphedForwardHop(B, 1, n, DEV, cfg=cfg)
    model = SpeakerForwardModel(B, cfg, sp, n, 1)
    room, layers = np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32)
    for b in range(B):
        fwd.join(b, 0)
        plain.join(b, 0)
    x = synth.synth_clips(B, HOP * hops, seed=23)
    x = x / x.abs().amax(dim=2, keepdim=True)
    owners = []
    for h in range(hops):
        gain = torch.tensor([next((a for s, (lo, hi, a) in talk.items() if s == b and lo <= h < hi), 0.0003) for b in range(B)])
        xs = (x[:, :, HOP * h:HOP * (h + 1)] * gain.view(B, 1, 1)).contiguous().to(DEV)
        packets, nbytes = tx.step(xs)
        levels, counts = tx.audio_level.tolist(), nbytes.tolist()
        assert levels == hop_level(xs.cpu().numpy()).tolist()
        fwd.forward(list(range(B)), packets, counts, levels)
        plain.forward(list(range(B)), packets, counts)
        want = model.step(list(range(B)), packets.cpu().numpy(), counts, levels, room, layers, np.full(B, int(h == 0), dtype=np.int32))
        assert np.array_equal(fwd.routes.cpu().numpy(), want["routes"]), h
        owners.append(int(fwd.routes[0, 0]))
        assert int(plain.routes[0, 0]) == 1, h               # the earliest other slot, whoever talks
    # the attack takes two hops to pass the floor from silence; slot 2 is 20 dB louder than slot 4 was, which decays by 0.75 dB per
    # hop and holds the margin of 6 dB: a few hops of attack overtake it
    assert owners[:5] == [-1] * 5 and set(owners[8:28]) == {4} and set(owners[36:]) == {2}, owners
    assert int(fwd.speaker_rank[2]) == 0 and int(fwd.listener_state[0, LR_SWITCHES]) == 2
