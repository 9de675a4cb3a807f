"""GPU: the room mixer of the graphed receiver (GraphedDecodeHop(mix=MixConfig(...)), hilcodec_amd.mix_rooms).  The two kernels
against the definition (mixer.py), the receiver's `mixed` / `speakers` / `levels` against mixer.MixModel applied to the waveform it
returned (next to an identical receiver without the mixer, which must return the same waveform and caches), and the two-replay bridge
into a second sender — every comparison bit for bit (torch.equal / np.array_equal)."""
import numpy as np
import pytest
import torch

import hilcodec_amd
from hilcodec_amd import dtx, mixer, synth, wire
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.mixer import MixConfig, MixModel
from tests.hops import rooms_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
B8, N, K = 8, 8, 8


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)


# ---------------------------------------------------------------- the kernels against mixer.py
@pytest.mark.parametrize("L", [1, 63, 64, 65, 294, 320, 960])
def test_mix_levels_kernel(L):
    from hilcodec_amd import ops
    B = 3
    rng = np.random.default_rng(L)
    x = np.zeros((B, 1, L), dtype=np.float32)
    x[1, 0] = rng.uniform(-3.0, 3.0, L)                     # row 0 stays zero
    x[1, 0, 0] = 3.0
    x[1, 0, L - 1] = -3.0
    x[2, 0] = 0.1 * rng.standard_normal(L)
    prev = rng.random(B) * np.array([1.0, 0.0, 1e4])        # slot 0: only the halved score; slot 1: 0; slot 2: far above E
    action = np.array([0, 0, 1], dtype=np.int32)            # ... but slot 2 starts on this hop
    model = MixModel(B, MixConfig(1))
    model.score = torch.from_numpy(prev.copy())
    score = torch.from_numpy(prev.copy()).to(DEV)
    wav = torch.from_numpy(x).to(DEV)
    ops.mix_levels(wav, score, i32(action))
    model.step(x, [-1] * B, action)
    assert torch.equal(score.cpu(), model.score)
    assert score[0].item() == 0.5 * prev[0] and score[2].item() == mixer.levels(x)[2] and score[2].item() > 0
    # again without an action row: slot 1's level is held at E, slot 2's halves against a quieter hop
    x2 = (0.25 * x).astype(np.float32)
    ops.mix_levels(torch.from_numpy(x2).to(DEV), score, None)
    model.step(x2, [-1] * B)
    assert torch.equal(score.cpu(), model.score)
    assert score[1].item() == 0.5 * mixer.levels(x)[1]


@pytest.mark.parametrize("top_k", [1, 3, 8])
@pytest.mark.parametrize("case", ["b6", "b70", "b300"])
def test_mix_rooms_kernel(case, top_k):
    from hilcodec_amd import ops
    room = rooms_case(case)
    B, L = len(room), 70
    rng = np.random.default_rng(B + top_k)
    for trial in range(2):
        score = rng.choice(np.array([0.0, 0.25, 1.0, 4.0]), B)     # four values: ties cross lanes, waves and blocks
        wav = rng.uniform(-0.9, 0.9, (B, L)).astype(np.float32)
        speakers = mixer.select(room, score, top_k)
        want = mixer.mix(wav, room, speakers)
        mixed = torch.full((B, 1, L), 7.0, device=DEV)
        sp = torch.full((B,), -9, dtype=torch.int32, device=DEV)
        ops.mix_rooms(torch.from_numpy(wav).to(DEV).view(B, 1, L), i32(room), torch.from_numpy(score).to(DEV), top_k, mixed, sp)
        assert np.array_equal(sp.cpu().numpy(), speakers), trial
        assert np.array_equal(mixed.cpu().numpy().reshape(B, L), want), trial
        for r in np.unique(room[room >= 0]):
            members = (room == r)
            assert speakers[members].sum() == min(top_k, int((score[members] > 0).sum()))
        if top_k > 1 and B > 6:
            assert np.abs(want).max() == 1.0                # the clamp was reached


def test_six_hops_speaker_hold():
    """slot 0 speaks on the first hop only: it stays the room's speaker exactly while its halved score beats (or ties, as the lower
    slot) slot 1's constant one"""
    B, L = 4, 64
    room = i32([0, 0, 0, -1])
    model = MixModel(B, MixConfig(1))
    score, got = None, []
    for k in range(6):
        amp = [1.0 if k == 0 else 0.0, 0.25, 0.125, 0.5]
        wav = torch.tensor(amp).view(B, 1, 1).repeat(1, 1, L).contiguous()
        mixed, sp, score = hilcodec_amd.mix_rooms(wav.to(DEV), room, score, top_k=1)
        want_mixed, want_sp = model.step(wav, room.cpu())
        assert torch.equal(mixed.cpu(), want_mixed) and torch.equal(sp.cpu(), want_sp), k
        assert torch.equal(score.cpu(), model.score), k
        got.append(sp.cpu().tolist())
    # scores of slot 0: 64, 32, 16, 8, 4 (a tie with slot 1's 64 / 16 = 4: the lower slot), 2
    assert [g[0] for g in got] == [1, 1, 1, 1, 1, 0]
    assert [g[1] for g in got] == [0, 0, 0, 0, 0, 1]
    assert score.cpu().tolist() == [2.0, 4.0, 1.0, 16.0]


# ---------------------------------------------------------------- the graphed receiver against MixModel
def set_rooms(rx, k):
    """the membership changes before hop k"""
    if k == 0:
        for s in range(6):
            rx.join(s, 3)
        rx.join(6, 0)
        rx.join(7, 0)
    if k == 2:
        rx.leave(1)
        rx.join(6, 3)
    if k == 4:
        rx.join(1, 0)
        rx.leave(7)


def step_hop(rx, k, rng):
    """hop k of the explicit script: slot 2 held on hops 1-2, slot 3 lost on hop 2, slot 4 a SID on hop 3 and silent after it, slot 5
    started on hop 3; returns (wav, action)"""
    packets = torch.from_numpy(rng.integers(0, 256, (B8, rx.stride)).astype(np.uint8))
    action = np.zeros(B8, dtype=np.int32)
    if k == 3:
        rx.start(5)
        action[5] = 1
    wav = rx.step(packets, [N] * B8, hold=[2] if k in (1, 2) else None, lost=[3] if k == 2 else None,
                  sid=[4] if k == 3 else None, silent=[4] if k > 3 else None)
    return wav, action


def play_hop(rx, k, rng):
    """hop k of an in-order trace into a jitter receiver (depth 2): slot 3's packet 1 never arrives, slot 4 sends a SID as packet 2 and
    nothing after it, slot 2 is held on hop 3, slot 5 is started on hop 4; returns (wav, action)"""
    slots, rows, nbytes = [], [], []
    for b in range(B8):
        if (b == 3 and k == 1) or (b == 4 and k > 2):
            continue
        if b == 4 and k == 2:
            pkt = wire.pack_transport(k, rng.integers(0, 256, dtx.sid_bytes(K)).astype(np.uint8).tobytes(), 0, sid=True)
        else:
            pkt = wire.pack_transport(k, rng.integers(0, 256, wire.packet_bytes(N, 1)).astype(np.uint8).tobytes(), N)
        row = np.zeros(rx.tstride, dtype=np.uint8)
        row[:len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
        slots.append(b)
        rows.append(row)
        nbytes.append(len(pkt))
    action = np.zeros(B8, dtype=np.int32)
    if k == 4:
        rx.start(5)
        action[5] = 1
    wav = rx.play(slots, torch.from_numpy(np.stack(rows)), nbytes, hold=[2] if k == 3 else None)
    return wav, action


RECEIVERS = [
    ("step", 6, step_hop, dict()),
    ("step-22050", 6, step_hop, dict(output_rate=22050)),
    ("play", 8, play_hop, dict(jitter=JitterConfig())),
]


@pytest.mark.parametrize("name,hops,hop,kw", RECEIVERS, ids=[r[0] for r in RECEIVERS])
def test_receiver_mix_matches_model(speech, name, hops, hop, kw):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    cfg = MixConfig(2)
    base = dict(sessions=True, conceal=True, cng_order=K, **kw)
    mx = GraphedDecodeHop(speech, B8, 1, N, DEV, mix=cfg, **base)
    pl = GraphedDecodeHop(speech, B8, 1, N, DEV, **base)
    L = 294 if "output_rate" in kw else HOP
    assert mx.rooms == (-1,) * B8 and mx.mixed.shape == (B8, 1, L) and not mx.mixed.any()
    model = MixModel(B8, cfg)
    spoke = np.zeros(B8, dtype=np.int64)
    heard = 0
    for k in range(hops):
        set_rooms(mx, k)
        wav, action = hop(mx, k, np.random.default_rng(100 + k))
        wav = wav.clone()
        ref, _ = hop(pl, k, np.random.default_rng(100 + k))
        assert wav.shape == (B8, 1, L)
        assert torch.equal(wav, ref), k
        for x, y in zip(mx.cache_dec, pl.cache_dec):
            assert torch.equal(x, y), k
        want_mixed, want_sp = model.step(wav, mx.rooms, action)
        assert torch.equal(mx.levels.cpu(), model.score), k
        assert torch.equal(mx.speakers.cpu(), want_sp), k
        assert torch.equal(mx.mixed.cpu(), want_mixed), k
        spoke += want_sp.numpy()
        heard += int(want_mixed.any(dim=2).sum())
    assert mx.rooms == (3, 0, 3, 3, 3, 3, 3, -1)
    assert spoke.sum() > 0 and heard > 0 and model.score[4] > 0          # the comfort-noise slot has a level: mixed after the noise
    mx.stop(0)
    assert mx.rooms[0] == 3                                # a stop does not leave the room
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the bridge: two replays per hop, no host copy
def test_bridge_feeds_a_sender_from_mixed(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    cfg = MixConfig(2)
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


# ---------------------------------------------------------------- errors
def test_mix_receiver_arguments(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, N, DEV, mix=MixConfig(2))                         # needs sessions
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, mix=2)
    plain = GraphedDecodeHop(speech, 2, 1, N, DEV)
    for what in ("mixed", "speakers", "levels", "rooms"):
        with pytest.raises(RuntimeError):
            getattr(plain, what)
    with pytest.raises(RuntimeError):
        plain.join(0, 0)
    rx = GraphedDecodeHop(speech, 2, 1, N, DEV, sessions=True, mix=MixConfig(2))
    for slot in (-1, 2):
        with pytest.raises(IndexError):
            rx.join(slot, 0)
        with pytest.raises(IndexError):
            rx.leave(slot)
    for room in (-1, 2, True, 0.5):
        with pytest.raises(ValueError):
            rx.join(0, room)
    rx.join(1, 1)
    assert rx.rooms == (-1, 1)
    rx.leave(1)
    assert rx.rooms == (-1, -1)
