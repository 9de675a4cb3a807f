"""GPU: loss concealment of the graphed receiver (GraphedDecodeHop(conceal=True), `step(..., lost=slots)`).  The prepare kernel
against a host model of its table, the gain kernel against the fp32 torch ramp, and the receiver against an eager reference: a
conceal=False receiver fed host-built substitute packets (wire.conceal_packet) and host holds, its output times the ramp — every
comparison bit for bit (torch.equal), except the oracle leg (the project's waveform bar, 1e-4)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth, wire
from tests.hops import CONCEAL_FADE as F
from tests.hops import build_streaming, caches_equal, prepare_model, put_row, row_bytes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320


@pytest.fixture(scope="module")
def built():
    return build_streaming()


@pytest.fixture(scope="module")
def speech(built):
    return built[0]


def ramp_torch(wav_rows, a, c, G, W):
    """wav * (G[a] + (G[c] - G[a]) * W), fp32, one rounding per operation (CPU torch: no contraction)"""
    gain = G[a] + (G[c] - G[a]) * W
    return wav_rows * gain


def random_packets(B, n_max, T, gen):
    """a hop of random packets (uint8 [B, stride], host) with a random n per stream"""
    n_list = torch.randint(1, n_max + 1, (B,), generator=gen).tolist()
    idx = torch.randint(0, 1024, (n_max, B, T), generator=gen)
    out = torch.zeros(B, wire.packet_bytes(n_max, T), dtype=torch.uint8)
    for b in range(B):
        put_row(out, b, wire.pack_stream_packet(idx[:n_list[b], b]))
    return out, n_list


# ---------------------------------------------------------------- hilc_conceal_prepare against its host model (tests/hops.py)


@pytest.mark.parametrize("B", [37, 1024])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("n_max", [8, 12])
def test_prepare_kernel(B, T, n_max):
    from hilcodec_amd import ops
    gen = torch.Generator().manual_seed(B + 10 * T + n_max)
    for trial in range(3):
        state = torch.zeros(B, n_max + 3, dtype=torch.int32)
        state[:, 0] = torch.randint(0, F + 2, (B,), generator=gen)       # F + 1: a stored run past F counts as F
        state[:, 1] = torch.randint(0, 2, (B,), generator=gen)
        state[:, 2] = torch.randint(0, n_max + 1, (B,), generator=gen)   # 0: clamped to 1
        state[:, 3:] = torch.randint(0, 2048, (B, n_max), generator=gen)  # codes past 10 bits: masked
        kind = torch.randint(0, 8, (B,), generator=gen)
        hold = (kind == 0).to(torch.int32)
        lost = ((kind >= 1) & (kind <= 4)).to(torch.int32)
        action = torch.zeros(B, dtype=torch.int32)
        starts = torch.randint(0, 6, (B,), generator=gen) == 0
        action[starts] = torch.where(torch.randint(0, 2, (B,), generator=gen) == 0, -1, 1)[starts].to(torch.int32)
        packets, n_list = random_packets(B, n_max, T, gen)
        n_slot = torch.tensor(n_list, dtype=torch.int32)
        n_slot[lost.bool() | hold.bool()] = n_max
        exp = prepare_model(state, action, hold, lost, n_slot, packets, T, F)
        d = [t.to(DEV) for t in (state, action, hold, lost, n_slot, packets)]
        ramp = ops.conceal_prepare(d[0], d[1], d[2], d[3], d[4], d[5], T, F)
        torch.cuda.synchronize()
        got = (d[0].cpu(), d[2].cpu(), d[4].cpu(), d[5].cpu(), ramp.cpu())
        for name, g, e in zip(("state", "hold", "n_slot", "packets", "ramp"), got, exp):
            assert torch.equal(g, e), f"trial {trial}: {name}"
        assert torch.equal(d[1].cpu(), action) and torch.equal(d[3].cpu(), lost)      # read-only rows


@pytest.mark.parametrize("B,S", [(37, 320), (37, 640), (1024, 320)])
def test_gain_kernel(B, S):
    from hilcodec_amd import ops
    gen = torch.Generator().manual_seed(B + S)
    G, W = wire.conceal_tables(F, S)
    wav = torch.randn(B, 1, S, generator=gen)
    ramp = torch.randint(-F - 1, F + 2, (B,), generator=gen, dtype=torch.int32)   # +-(F + 1): out of range, not touched
    ramp[:2 + 2 * F] = torch.tensor([0, F + 1] + list(range(-F, 0)) + list(range(1, F + 1)), dtype=torch.int32)
    exp = wav.clone()
    for b in range(B):
        r = int(ramp[b])
        if r == 0 or abs(r) > F:
            continue
        a, c = (r - 1, r) if r > 0 else (-r, 0)
        exp[b] = ramp_torch(wav[b], a, c, G, W)
    occurring = {int(r) for r in ramp if 0 < abs(int(r)) <= F}
    assert occurring == set(range(-F, 0)) | set(range(1, F + 1))      # every (a, c) the receiver makes
    got = wav.to(DEV)
    ops.conceal_gain(got, ramp.to(DEV), G.to(DEV), W.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), exp)
    idle = wav.to(DEV)
    ops.conceal_gain(idle, torch.zeros(B, dtype=torch.int32, device=DEV), G.to(DEV), W.to(DEV))
    assert torch.equal(idle.cpu(), wav)


# ---------------------------------------------------------------- the eager reference receiver
class Reference:
    """a conceal=False, sessions=True receiver plus the host's concealment state: per slot the last received packet and its n,
    and the run k.  `step` builds the substitute packets and holds of the table on the host and applies the ramps in fp32 torch."""

    def __init__(self, model, B, frames, n, fade_hops=F):
        from hilcodec_amd.graph_step import GraphedDecodeHop
        self.r = GraphedDecodeHop(model, B, frames, n, DEV, sessions=True)
        self.B, self.T, self.n, self.F = B, frames, n, fade_hops
        self.last = [None] * B
        self.k = [0] * B
        self.G, self.W = wire.conceal_tables(fade_hops, HOP * frames)

    def start(self, slot, cache_dec=None):
        self.r.start(slot, cache_dec)
        self.last[slot], self.k[slot] = None, 0

    def stop(self, slot):
        self.r.stop(slot)

    def step(self, packets, n_list, hold=(), lost=()):
        pk = packets.cpu().clone()
        n_list = list(n_list)
        holds = set(hold)
        ramps = {}
        for b in range(self.B):
            if b in hold or b in self.r.stopped:
                continue
            if b not in lost:
                if self.k[b]:
                    ramps[b] = (self.k[b], 0)
                self.last[b] = (row_bytes(pk, b), n_list[b])
                self.k[b] = 0
            elif self.last[b] is not None and self.k[b] < self.F:
                blob, nb = self.last[b]
                put_row(pk, b, wire.conceal_packet(blob, nb, self.T))
                n_list[b] = nb
                ramps[b] = (self.k[b], self.k[b] + 1)
                self.k[b] += 1
            else:
                holds.add(b)
        for b in holds:
            n_list[b] = self.n
        wav = self.r.step(pk, n_list, hold=sorted(holds)).cpu().clone()
        for b, (a, c) in ramps.items():
            wav[b] = ramp_torch(wav[b], a, c, self.G, self.W)
        return wav


def _compare(c, ref, wav, ref_wav, h):
    assert torch.equal(wav.cpu(), ref_wav), f"hop {h}: wav"
    assert caches_equal(c.cache_dec, ref.r.cache_dec), f"hop {h}: caches"
    assert torch.equal(c.concealed.cpu(), torch.tensor(ref.k, dtype=torch.int32)), f"hop {h}: concealed"


def run_plan(model, B, frames, hops, seed, n=8):
    """isolated losses every hop; slot 5 a burst of 7 > F hops (2..8) then recovery; slot 3 lost from hop 0 (nothing received
    yet); slot 9 lost on its start hop 4; slot 11 resumed at hop 5 and lost at hops 6-7; slot 13 held at hops 3-4 beside slot 14
    lost there; slot 15 lost at 2, held at 3, received at 4 (fade-in from G[1]); slot 20 stopped at hop 7, started at 10;
    a random n per stream and hop"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    c = GraphedDecodeHop(model, B, frames, n, DEV, sessions=True, conceal=True, fade_hops=F)
    ref = Reference(model, B, frames, n)
    special = {3, 5, 9, 11, 13, 14, 15, 20}
    pool = [b for b in range(B) if b not in special]
    for h in range(hops):
        packets, n_list = random_packets(B, n, frames, gen)
        lost = set(rng.choice(pool, size=max(2, B // 12), replace=False).tolist()) if h else set()
        hold = set()
        if h == 0:
            lost.add(3)
        if 2 <= h <= 8:
            lost.add(5)
        if h == 4:
            for side in (c, ref):
                side.start(9)
            lost.add(9)
        if h == 5:
            enc = c.export(12)
            for side in (c, ref):
                side.start(11, enc)
        if h in (6, 7):
            lost.add(11)
        if h in (3, 4):
            hold.add(13)
            lost.add(14)
        if h == 2:
            lost.add(15)
        if h == 3:
            hold.add(15)
        if h == 7:
            for side in (c, ref):
                side.stop(20)
        if h == 10:
            for side in (c, ref):
                side.start(20)
        garbage = packets.clone()
        for b in lost | hold:                             # rows that are not read
            garbage[b] = torch.randint(0, 256, (garbage.shape[1],), generator=gen, dtype=torch.uint8)
        n_in = [0 if b in lost | hold else n_list[b] for b in range(B)]
        ref_wav = ref.step(packets, n_list, hold=hold, lost=lost)
        wav = c.step(garbage.to(DEV) if h % 2 else garbage, n_in, hold=sorted(hold), lost=sorted(lost))
        _compare(c, ref, wav, ref_wav, h)
        assert bool(torch.isfinite(wav).all())
        if h == 8:
            assert int(c.concealed[5]) == F                 # faded out: held by the graph
        if h == 9:
            assert int(c.concealed[5]) == 0
    return c, ref


@pytest.mark.parametrize("B,frames", [(37, 1), (37, 2), (1024, 1)])
def test_receiver_conceal_equals_reference(speech, B, frames):
    run_plan(speech, B, frames, hops=12, seed=B + frames)


def test_no_loss_identity(speech):
    """conceal=True with `lost` always empty: the conceal=False receiver's bits, over hops with starts, holds and stops"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B, frames, hops = 37, 2, 8
    gen = torch.Generator().manual_seed(71)
    plain = GraphedDecodeHop(speech, B, frames, 8, DEV, sessions=True)
    c = GraphedDecodeHop(speech, B, frames, 8, DEV, sessions=True, conceal=True)
    for h in range(hops):
        packets, n_list = random_packets(B, 8, frames, gen)
        hold = [2, 30] if h in (1, 2) else []
        if h == 3:
            for side in (plain, c):
                side.stop(4)
        if h == 5:
            rec = plain.export(7)
            for side in (plain, c):
                side.start(4)
                side.start(8, rec)
        w0 = plain.step(packets, n_list, hold=hold).clone()
        w1 = c.step(packets, n_list, hold=hold, lost=[])
        assert torch.equal(w0, w1), f"hop {h}"
        assert caches_equal(plain.cache_dec, c.cache_dec), f"hop {h}"
        assert not bool(c.concealed.any())


def test_production_shape(speech):
    """sender -> receiver at 1 024 streams, n = 8, 10 % of the slots lost per hop (a new seeded set each hop)"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    B, hops = 1024, 8
    x = synth.synth_clips(B, HOP * hops, seed=72).to(DEV)
    rng = np.random.default_rng(73)
    s = GraphedEncodeHop(speech, B, HOP, 8, DEV)
    from hilcodec_amd.graph_step import GraphedDecodeHop
    c = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True)
    ref = Reference(speech, B, 1, 8)
    n_list = [8] * B
    for h in range(hops):
        packets, _ = s.step(x[:, :, HOP * h: HOP * (h + 1)].contiguous())
        lost = set(rng.permutation(B)[:B // 10].tolist())
        ref_wav = ref.step(packets, n_list, lost=lost)
        wav = c.step(packets, n_list, lost=sorted(lost))
        _compare(c, ref, wav, ref_wav, h)
        assert bool(torch.isfinite(wav).all())
    assert int(c.concealed.max()) >= 2


def test_oracle_leg(built):
    """3 streams on the CPU oracle (stream_dequantize + stream_decoder of the same repeated codes, the fp32 ramp): within 1e-4"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    from oracle import hilcodec_oracle as O
    model, mk, sd = built
    p = O.stream_prepare(sd, mk)
    B, T, hops = 3, 1, 9
    gen = torch.Generator().manual_seed(74)
    lost_plan = {0: [2], 1: [0], 2: [0, 1], 3: [0], 4: [0], 5: [0], 6: [0], 7: [], 8: [1]}   # stream 0: a burst past F
    c = GraphedDecodeHop(model, B, T, 8, DEV, sessions=True, conceal=True)
    G, W = wire.conceal_tables(F, HOP * T)
    oc = [O.stream_init_cache(mk, 1)[1] for _ in range(B)]
    last, k = [None] * B, [0] * B
    for h in range(hops):
        packets, n_list = random_packets(B, 8, T, gen)
        lost = lost_plan[h]
        wav = c.step(packets, n_list, lost=lost).cpu()
        for b in range(B):
            ramp = None
            if b not in lost:
                codes, n = wire.unpack_stream_packet(row_bytes(packets, b), n_list[b], T), n_list[b]
                if k[b]:
                    ramp = (k[b], 0)
                last[b], k[b] = (codes[:, -1], n), 0
            elif last[b] is not None and k[b] < F:
                n = last[b][1]
                codes = last[b][0].view(n, 1).expand(n, T)
                ramp = (k[b], k[b] + 1)
                k[b] += 1
            else:
                assert not bool(wav[b].any()), f"hop {h} stream {b}: held"
                continue
            wo, oc[b] = O.stream_decoder(p, mk, O.stream_dequantize(p, codes.reshape(n, 1, T).long(), n), oc[b])
            if ramp is not None:
                wo = ramp_torch(wo, ramp[0], ramp[1], G, W)
            assert (wav[b:b + 1] - wo).abs().max() < 1e-4, f"hop {h} stream {b}"
    assert c.concealed.cpu().tolist() == [0, 1, 0]


def test_conceal_checks(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    B = 3
    with pytest.raises(ValueError):
        GraphedDecodeHop(speech, B, 1, 8, DEV, conceal=True)                       # needs sessions
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True, fade_hops=bad)
    pk = torch.zeros(B, wire.packet_bytes(8, 1), dtype=torch.uint8)
    plain = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True)
    with pytest.raises(RuntimeError):
        plain.step(pk, [8] * B, lost=[1])
    with pytest.raises(RuntimeError):
        plain.concealed
    plain.step(pk, [8] * B, lost=[])
    c = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True, fade_hops=2)
    before = c.cache_dec[0].clone()
    with pytest.raises(ValueError):
        c.step(pk, [8] * B, hold=[1], lost=[1])                                    # lost and held
    with pytest.raises(IndexError):
        c.step(pk, [8] * B, lost=[3])
    with pytest.raises(IndexError):
        c.step(pk, [8] * B, lost=[-1])
    with pytest.raises(ValueError):
        c.step(pk, [8] * B, lost=torch.tensor([1], device=DEV))                    # host ints only
    c.stop(2)
    with pytest.raises(ValueError):
        c.step(pk, [8] * B, lost=[2])                                              # stopped
    assert c.parity == 0 and torch.equal(c.cache_dec[0], before)                   # nothing was launched
    c.step(pk, [8, 0, 8], lost=[1])                                                # a lost slot's n is not checked
    assert c.concealed.cpu().tolist() == [0, 0, 0]                                 # nothing received yet: held
    with pytest.raises(ValueError):
        c.step(pk, [8, 0, 8], lost=[0])                                            # slot 1 is not lost: its n is checked
