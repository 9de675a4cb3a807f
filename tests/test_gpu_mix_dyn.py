"""GPU: per-speaker levelling and the limiter of the room mixer (MixConfig(level=, limit=), hilcodec_amd.mix_rooms(dynamics=)).
hilc_mix_gains and hilc_mix_rooms_dyn against the definition (mixer.py), hilc_mix_rooms_dyn without its optional rows against
hilc_mix_rooms, the receiver's `mixed` / `speakers` / `levels` / `gains` / `limiter_state` against mixer.MixModel applied to the
waveform it returned (next to an identical receiver without the mixer, which must return the same waveform and caches), and the
two-replay bridge — every comparison bit for bit (torch.equal / np.array_equal); the one bound is the limiter's ceiling."""
import numpy as np
import pytest
import torch

import hilcodec_amd
from hilcodec_amd import mixer, synth
from hilcodec_amd.mixer import Dynamics, LevelConfig, LimitConfig, MixConfig, MixModel
from tests.hops import rooms_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
B8, N = 8, 8
FAST = LevelConfig(up=1.5, down=0.7)                        # a dozen hops reach the band and the bounds


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def under_ceiling(mixed, cfg):
    """g <= ceiling / p_s in every sub-frame, so |acc g| <= ceiling (1 + 2^-52)^2 in float64: at most one fp32 ulp over fp32(ceiling)"""
    top = float(np.abs(np.asarray(mixed)).max())
    return top <= float(np.nextafter(np.float32(cfg.ceiling), np.float32(2)))


# ---------------------------------------------------------------- hilc_mix_gains against mixer.update_gains
def gain_rows(L, seed):
    """[3, 1, L]: a zero row, a loud one, one under the gate (rms 0.003 < gate_rms 0.01)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((3, 1, L), dtype=np.float32)
    x[1, 0] = rng.uniform(-0.9, 0.9, L)
    x[1, 0, L - 1] = 0.9
    x[2, 0] = 0.005 * rng.uniform(-1.0, 1.0, L)
    return x


@pytest.mark.parametrize("L", [1, 63, 64, 65, 294, 320, 960])
def test_mix_gains_kernel(L):
    from hilcodec_amd import ops
    gains0 = np.array([[0.5, 0.8], [2.0, 3.0], [1.2, 1.7]])
    power0 = np.array([0.02, 0.0005, 0.003])
    gains, power = dev(gains0.copy()), dev(power0.copy())
    # hop 1: slot 2 (under the gate) starts on this hop: its row is the cleared one and stays
    x = gain_rows(L, L)
    action = np.array([0, 0, 1], dtype=np.int32)
    ops.mix_gains(dev(x), gains, power, FAST, i32(action))
    want_g, want_p = mixer.update_gains(gains0, power0, mixer.levels(x), L, FAST, action)
    assert np.array_equal(gains.cpu().numpy(), want_g) and np.array_equal(power.cpu().numpy(), want_p)
    assert want_g[0].tolist() == [0.8, 0.8] and want_p[0] == 0.02                # the zero row: gain and power held
    assert want_g[1, 0] == 3.0 and want_g[1, 1] != 3.0 and want_p[1] != 0.0005   # the loud row moved both
    assert want_g[2].tolist() == [1.0, 1.0] and want_p[2] == 0.0                 # reset, then gated
    # hop 2, no action row, the rows rotated: slot 2 is loud from power 0 (pw = m), slot 0 under the gate, slot 1 zero
    x2 = np.ascontiguousarray(np.roll(gain_rows(L, L + 1000), 1, axis=0))
    ops.mix_gains(dev(x2), gains, power, FAST)
    got_g, got_p = mixer.update_gains(want_g, want_p, mixer.levels(x2), L, FAST)
    assert np.array_equal(gains.cpu().numpy(), got_g) and np.array_equal(power.cpu().numpy(), got_p)
    assert got_p[2] == mixer.levels(x2)[2] / L and got_g[2, 1] == 0.7
    assert got_g[0].tolist() == [0.8, 0.8] and got_g[1].tolist() == [want_g[1, 1]] * 2


def test_mix_gains_depend_on_the_slots_own_row_only():
    from hilcodec_amd import ops
    B, L = 5, 294
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.5, 0.5, (B, 1, L)).astype(np.float32)
    gains0, power0 = rng.uniform(0.5, 2.0, (B, 2)), rng.uniform(0.0, 0.1, B)
    action = np.array([0, 1, 0, 0, 0], dtype=np.int32)

    def run(rows):
        gains, power = dev(gains0.copy()), dev(power0.copy())
        ops.mix_gains(dev(rows), gains, power, FAST, i32(action))
        return gains.cpu().numpy(), power.cpu().numpy()

    base_g, base_p = run(x)
    for b in range(B):
        for fill in (np.nan, np.inf, 0.0, 7.0):
            other = np.full_like(x, fill)
            other[b] = x[b]
            g, p = run(other)
            assert np.array_equal(g[b], base_g[b]) and p[b] == base_p[b], (b, fill)


# ---------------------------------------------------------------- hilc_mix_rooms_dyn
@pytest.mark.parametrize("top_k", [1, 3, 8])
@pytest.mark.parametrize("case", ["b6", "b70", "b300"])
def test_mix_rooms_dyn_without_rows_is_mix_rooms(case, top_k):
    from hilcodec_amd import ops
    room = rooms_case(case)
    B, L = len(room), 70
    rng = np.random.default_rng(B + top_k)
    for trial in range(2):
        score = dev(rng.choice(np.array([0.0, 0.25, 1.0, 4.0]), B))
        wav = dev(rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32))
        want, want_sp = torch.full((B, 1, L), 7.0, device=DEV), torch.full((B,), -9, dtype=torch.int32, device=DEV)
        got, got_sp = torch.full((B, 1, L), 5.0, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
        ops.mix_rooms(wav, i32(room), score, top_k, want, want_sp)
        ops.mix_rooms_dyn(wav, i32(room), score, top_k, got, got_sp, action=i32(np.ones(B)))     # an action row without rows: unread
        assert torch.equal(got, want) and torch.equal(got_sp, want_sp), trial
        if top_k > 1 and B > 6:
            assert got.abs().max().item() == 1.0


RUNS = [("b6", 1), ("b70", 3), ("b300", 8)]


@pytest.mark.parametrize("sub", [16, 32])
@pytest.mark.parametrize("L", [33, 70, 320])
@pytest.mark.parametrize("case,top_k", RUNS, ids=[f"{c}-k{k}" for c, k in RUNS])
def test_mix_rooms_dyn_kernel(case, top_k, L, sub):
    """levelling and the limiter against the model over two hops: the second starts from the first's rows, and three slots start again
    on it"""
    from hilcodec_amd import ops
    room = rooms_case(case)
    B = len(room)
    cfg = MixConfig(top_k, level=FAST, limit=LimitConfig(sub=sub))
    rng = np.random.default_rng(B + top_k + L + sub)
    model = MixModel(B, cfg)
    model.score = torch.from_numpy(rng.choice(np.array([0.0, 0.25, 1.0, 4.0]), B))
    model.gains = torch.from_numpy(np.repeat(rng.uniform(0.5, 2.0, (B, 1)), 2, axis=1))
    model.power = torch.from_numpy(rng.uniform(0.0, 0.5, B))
    model.limiter = torch.from_numpy(np.stack([rng.uniform(0.0, 2.0, B), rng.uniform(0.3, 1.0, B)], axis=1))
    score, gains, power, limiter = (t.clone().to(DEV) for t in (model.score, model.gains, model.power, model.limiter))
    mixed = torch.full((B, 1, L), 7.0, device=DEV)
    sp = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    loud = 0
    for hop in range(2):
        wav = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
        wav[rng.integers(0, B)] = 0                          # a silent slot
        action = np.zeros(B, dtype=np.int32)
        if hop == 1:
            action[[0, B // 2, B - 1]] = 1
        x, act = dev(wav), i32(action)
        ops.mix_levels(x, score, act)
        ops.mix_gains(x, gains, power, cfg.level, act)
        ops.mix_rooms_dyn(x, i32(room), score, top_k, mixed, sp, gains, limiter, cfg.limit, act)
        want_mixed, want_sp = model.step(wav, room, action)
        assert torch.equal(score.cpu(), model.score), hop
        assert torch.equal(gains.cpu(), model.gains) and torch.equal(power.cpu(), model.power), hop
        assert torch.equal(sp.cpu(), want_sp), hop
        assert torch.equal(limiter.cpu(), model.limiter), hop
        assert torch.equal(mixed.cpu(), want_mixed), hop
        assert under_ceiling(want_mixed, cfg.limit) and under_ceiling(mixed.cpu(), cfg.limit), hop
        raw = mixer.sums(wav.reshape(B, L), room, want_sp.numpy(), model.gains.numpy())
        loud += int((np.abs(raw) > 1.0).sum())
        assert bool((model.limiter[torch.from_numpy(room < 0), 0] <= 2.0 * 0.99).all())          # listeners in no room: the envelope only releases
    if top_k > 1:
        assert loud > 0 and model.limiter[:, 1].min().item() < 1.0             # the raw sums clip: the limiter was at work


@pytest.mark.parametrize("L,sub", [(1024, 32), (1025, 32), (3200, 512), (8192, 16)])
def test_mix_rooms_dyn_long_hops(L, sub):
    """either side of the hop length at which the limiter's kernel takes its longer LDS row, the product's longest hop, and the longest
    hop of all at the shortest sub-frame (512 sub-frames)"""
    from hilcodec_amd import ops
    room = rooms_case("b6")
    B, top_k = len(room), 3
    cfg = MixConfig(top_k, level=FAST, limit=LimitConfig(sub=sub))
    rng = np.random.default_rng(L)
    model = MixModel(B, cfg)
    score = torch.zeros(B, dtype=torch.float64, device=DEV)
    gains, power, limiter = mixer.cleared_rows(B, cfg.level, cfg.limit, DEV)
    mixed = torch.full((B, 1, L), 7.0, device=DEV)
    sp = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    for hop in range(2):
        wav = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
        wav[:, :, L // 2:] *= np.float32(0.05)               # a quiet second half: the envelope releases inside the hop
        x = dev(wav)
        ops.mix_levels(x, score)
        ops.mix_gains(x, gains, power, cfg.level)
        ops.mix_rooms_dyn(x, i32(room), score, top_k, mixed, sp, gains, limiter, cfg.limit)
        want_mixed, want_sp = model.step(wav, room)
        assert torch.equal(sp.cpu(), want_sp) and torch.equal(gains.cpu(), model.gains), hop
        assert torch.equal(limiter.cpu(), model.limiter), hop
        assert torch.equal(mixed.cpu(), want_mixed), hop
        assert under_ceiling(mixed.cpu(), cfg.limit), hop
        raw = mixer.sums(wav.reshape(B, L), room, want_sp.numpy(), model.gains.numpy())
        assert np.abs(raw).max() > 1.0                       # two speakers per listener in the room of three: the raw sums clip


@pytest.mark.parametrize("which", ["level", "limit"])
def test_mix_rooms_dyn_one_row(which):
    """each optional row alone: levelled terms under the plain clamp, raw terms under the limiter"""
    from hilcodec_amd import ops
    room = rooms_case("b70")
    B, L, top_k = len(room), 294, 3
    cfg = MixConfig(top_k, level=FAST) if which == "level" else MixConfig(top_k, limit=LimitConfig(sub=32))
    rng = np.random.default_rng(70)
    model = MixModel(B, cfg)
    score = torch.zeros(B, dtype=torch.float64, device=DEV)
    gains, power, limiter = mixer.cleared_rows(B, cfg.level, cfg.limit, DEV)
    mixed = torch.full((B, 1, L), 7.0, device=DEV)
    sp = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    for hop in range(3):
        wav = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
        x = dev(wav)
        ops.mix_levels(x, score)
        if cfg.level is not None:
            ops.mix_gains(x, gains, power, cfg.level)
        ops.mix_rooms_dyn(x, i32(room), score, top_k, mixed, sp, gains, limiter, cfg.limit)
        want_mixed, want_sp = model.step(wav, room)
        assert torch.equal(mixed.cpu(), want_mixed) and torch.equal(sp.cpu(), want_sp), hop
        if cfg.level is not None:
            assert torch.equal(gains.cpu(), model.gains) and torch.equal(power.cpu(), model.power), hop
        else:
            assert torch.equal(limiter.cpu(), model.limiter) and under_ceiling(mixed.cpu(), cfg.limit), hop
    if which == "level":
        assert want_mixed.abs().max().item() <= 1.0 and model.gains[:, 1].max().item() < 1.0


def test_mix_rooms_dynamics_six_hops():
    B, L = 6, 320
    room = i32([0, 0, 0, 1, -1, 1])
    cfg = MixConfig(2, level=FAST, limit=LimitConfig())
    model = MixModel(B, cfg)
    dyn = Dynamics(B, cfg.level, cfg.limit)
    rng = np.random.default_rng(6)
    score = None
    for k in range(6):
        amp = np.array([0.9, 0.8, 0.03, 0.005, 0.5, 0.0 if k < 3 else 0.9]).reshape(B, 1, 1)
        wav = torch.from_numpy((amp * rng.uniform(-1.0, 1.0, (B, 1, L))).astype(np.float32))
        mixed, sp, score = hilcodec_amd.mix_rooms(wav.to(DEV), room, score, top_k=2, dynamics=dyn)
        want_mixed, want_sp = model.step(wav, room.cpu())
        assert torch.equal(mixed.cpu(), want_mixed) and torch.equal(sp.cpu(), want_sp), k
        assert torch.equal(score.cpu(), model.score), k
        assert torch.equal(dyn.gains.cpu(), model.gains) and torch.equal(dyn.power.cpu(), model.power), k
        assert torch.equal(dyn.limiter.cpu(), model.limiter), k
        assert under_ceiling(mixed.cpu(), cfg.limit)
        if k == 0:
            assert model.limiter[2, 0] > cfg.limit.ceiling                       # slot 2 hears 0 and 1 at gain 1: over the ceiling
    assert model.gains[0, 1] < 1.0 < model.gains[2, 1] and model.gains[3].tolist() == [1.0, 1.0]    # loud down, quiet up, gated held
    dyn.reset([0])
    assert dyn.gains[0].tolist() == [1.0, 1.0] and dyn.gains[1, 1].item() == model.gains[1, 1].item()
    plain = Dynamics(B)                                                          # no options: the plain mixer
    got = hilcodec_amd.mix_rooms(wav.to(DEV), room, None, top_k=2, dynamics=plain)
    want = hilcodec_amd.mix_rooms(wav.to(DEV), room, None, top_k=2)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        hilcodec_amd.mix_rooms(wav.to(DEV), room, dynamics=Dynamics(B + 1, cfg.level, cfg.limit))
    with pytest.raises(ValueError):
        hilcodec_amd.mix_rooms(wav.to(DEV), room, dynamics=Dynamics(B, cfg.level, cfg.limit, device="cpu"))


# ---------------------------------------------------------------- the graphed receiver against MixModel
def set_rooms(rx, k):
    """the membership changes before hop k"""
    if k == 0:
        for s in range(6):
            rx.join(s, 3)
        rx.join(6, 0)
        rx.join(7, 0)
    if k == 3:
        rx.leave(1)
        rx.join(6, 3)
    if k == 7:
        rx.join(1, 0)
        rx.leave(7)


def step_hop(rx, k, rng):
    """hop k: slot 2 is held on hops 4-6, slot 5 starts again on hop 5, slot 0 resumes from its own export on hop 8; returns (wav,
    action)"""
    packets = torch.from_numpy(rng.integers(0, 256, (B8, rx.stride)).astype(np.uint8))
    action = np.zeros(B8, dtype=np.int32)
    if k == 5:
        rx.start(5)
        action[5] = 1
    if k == 8:
        rx.start(0, cache_dec=rx.export(0))
        action[0] = 1
    wav = rx.step(packets, [N] * B8, hold=[2] if k in (4, 5, 6) else None)
    return wav, action


@pytest.mark.parametrize("kw", [dict(), dict(output_rate=22050)], ids=["24000", "22050"])
def test_receiver_dynamics_match_model(speech, kw):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    cfg = MixConfig(2, level=FAST, limit=LimitConfig())
    mx = GraphedDecodeHop(speech, B8, 1, N, DEV, sessions=True, mix=cfg, **kw)
    pl = GraphedDecodeHop(speech, B8, 1, N, DEV, sessions=True, **kw)
    L = 294 if kw else HOP
    assert mx.mixed.shape == (B8, 1, L) and not mx.mixed.any()
    assert mx.gains.tolist() == [[1.0, 1.0]] * B8 and mx.limiter_state.tolist() == [[0.0, 1.0]] * B8    # cleared after the warm-up
    model = MixModel(B8, cfg)
    moved = 0
    for k in range(12):
        set_rooms(mx, k)
        wav, action = step_hop(mx, k, np.random.default_rng(200 + k))
        wav = wav.clone()
        ref, _ = step_hop(pl, k, np.random.default_rng(200 + k))
        assert wav.shape == (B8, 1, L)
        assert torch.equal(wav, ref), k
        for x, y in zip(mx.cache_dec, pl.cache_dec):
            assert torch.equal(x, y), k
        want_mixed, want_sp = model.step(wav, mx.rooms, action)
        assert torch.equal(mx.levels.cpu(), model.score), k
        assert torch.equal(mx.gains.cpu(), model.gains), k
        assert torch.equal(mx.speakers.cpu(), want_sp), k
        assert torch.equal(mx.limiter_state.cpu(), model.limiter), k
        assert torch.equal(mx.mixed.cpu(), want_mixed), k
        assert under_ceiling(mx.mixed.cpu(), cfg.limit), k
        if k in (4, 5, 6):
            assert not wav[2].any() and model.gains[2, 0] == model.gains[2, 1]   # a held slot's zeros do not move its gain
        if k == 5:
            assert model.gains[5, 0].item() == 1.0                               # the start cleared the row inside the graph
        if k == 8:
            assert model.gains[0, 0].item() == 1.0 and wav[0].any()              # so did the resume
        moved += int((model.gains[:, 0] != model.gains[:, 1]).sum())
    assert mx.rooms == (3, 0, 3, 3, 3, 3, 3, -1)
    assert moved > 0 and bool((model.gains != 1.0).any()) and want_mixed.any()
    torch.cuda.synchronize()


def test_receiver_dynamics_views_need_their_option(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    rx = GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, mix=MixConfig(2))
    for what in ("gains", "limiter_state"):
        with pytest.raises(RuntimeError):
            getattr(rx, what)
    rx = GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, mix=MixConfig(2, limit=LimitConfig()))
    assert rx.limiter_state.shape == (2, 2) and rx.limiter_state.dtype == torch.float64
    with pytest.raises(RuntimeError):
        rx.gains
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, mix=LimitConfig())


# ---------------------------------------------------------------- the bridge: two replays per hop, no host copy
def test_bridge_feeds_a_sender_from_limited_mix(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    cfg = MixConfig(2, level=FAST, limit=LimitConfig())
    tx = GraphedEncodeHop(speech, B8, HOP, N, DEV)
    rx = GraphedDecodeHop(speech, B8, 1, N, DEV, sessions=True, mix=cfg)
    out_a = GraphedEncodeHop(speech, B8, HOP, N, DEV)
    out_b = GraphedEncodeHop(speech, B8, HOP, N, DEV)
    for s in range(B8):
        rx.join(s, s % 2)                                  # two rooms of four
    model = MixModel(B8, cfg)
    x = synth.synth_clips(B8, 4 * HOP, seed=21).to(DEV)
    x[5] = 0                                               # a silent participant
    for k in range(4):
        pk, _ = tx.step(x[:, :, k * HOP:(k + 1) * HOP].contiguous())
        wav = rx.step(pk, [N] * B8)
        got_pk, got_nb = out_a.step(rx.mixed)              # fed the static device view directly
        want_mixed, _ = model.step(wav, rx.rooms)
        want_pk, want_nb = out_b.step(want_mixed.to(DEV))
        assert torch.equal(got_pk, want_pk), k
        assert torch.equal(got_nb, want_nb), k
        assert torch.equal(out_a.indices, out_b.indices), k
        assert want_mixed.any() and int(got_nb.min()) > 0
    torch.cuda.synchronize()
