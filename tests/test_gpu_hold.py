"""GPU: held streams of the graphed hops (`step(..., hold=slots)`, `stop(slot)`).  The hold kernel against a host model of it,
and the loopback, sender and receiver against an eager full-batch loop that copies the previous cache rows back into held rows
after each hop — every comparison bit for bit (torch.equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth, wire
from tests.hops import caches_equal, chunk, same_indices

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


class EagerHeld:
    """the eager full-batch hop (encoder -> quantizer -> dequantizer -> decoder) with held rows: rows in `zero` start fresh
    before the hop, rows in `held` get their caches of before the hop back after it, and their outputs are wav 0 / indices -1"""

    def __init__(self, model, B):
        self.model = model
        self.ce, self.cd = model.initialize_cache(torch.zeros(B, 1, 1, device=DEV))

    def step(self, x, held=(), n=8, zero=()):
        m = self.model
        held, zero = list(held), list(zero)
        if zero:
            for c in list(self.ce) + list(self.cd):
                c[zero] = 0
        old = [c[held].clone() for c in list(self.ce) + list(self.cd)] if held else None
        with torch.no_grad():
            z, self.ce = m.encoder(x, *self.ce)
            idx = m.quantizer(z, n)
            wav, self.cd = m.decoder(m.dequantizer(idx, n), *self.cd)
        idx, wav = idx.clone(), wav.clone()
        if held:
            for c, o in zip(list(self.ce) + list(self.cd), old):
                c[held] = o
            idx[:, held] = -1
            wav[held] = 0
        return idx, wav


def hold_plan(B, hops, seed):
    """per hop: none, a few, stream 7 held three hops in a row, and every stream"""
    rng = np.random.default_rng(seed)
    plan = []
    for h in range(hops):
        s = set(rng.permutation(B)[:4].tolist()) if h not in (0, 5) else set()
        if h in (2, 3, 4):
            s.add(7)
        if h == 6:
            s = set(range(B))
        plan.append(sorted(s))
    return plan


def garbage_rows(x, held, seed):
    """x with the held rows replaced by other audio: a held row's input must not matter"""
    if not held:
        return x
    x = x.clone()
    x[held] = synth.synth_clips(len(held), x.shape[-1], seed=seed).to(DEV).view(len(held), 1, -1)
    return x


def _views(buf, layout):
    return [buf[o:o + s[0] * n].view(s) for s, o, n in zip(layout.shapes, layout.off, layout.lens)]


@pytest.mark.parametrize("B", [37, 1024])
@pytest.mark.parametrize("side", ["both", "enc", "dec"])
def test_hold_kernel(speech, B, side):
    from hilcodec_amd import ops
    from hilcodec_amd.graph_step import state_layout
    layout = state_layout(speech, B, side)
    gen = torch.Generator(device=DEV).manual_seed(B + len(side))
    src = torch.randn(layout.total, device=DEV, generator=gen)
    dst = torch.randn(layout.total, device=DEV, generator=gen)
    T, stride = 2, wire.packet_bytes(8, 2)
    outs = dict(wav=torch.randn(B, 1, HOP * T, device=DEV, generator=gen),
                indices=torch.randint(-1, 1024, (8, B, T), device=DEV, generator=gen),
                packets=torch.randint(0, 256, (B, stride), device=DEV, generator=gen, dtype=torch.uint8),
                nbytes=torch.randint(1, stride + 1, (B,), device=DEV, generator=gen, dtype=torch.int32))
    given = {"both": ("wav", "indices"), "enc": ("indices", "packets", "nbytes"), "dec": ("wav",)}[side]
    rng = np.random.default_rng(B)
    held = sorted({0, B - 1} | set(rng.permutation(B)[:max(3, B // 8)].tolist()))
    hold = torch.zeros(B, dtype=torch.int32)
    hold[held] = torch.tensor([1, 7, -2] * len(held), dtype=torch.int32)[:len(held)]   # any non-zero entry holds

    # all-zero hold: nothing changes
    d0 = dst.clone()
    o0 = {k: v.clone() for k, v in outs.items()}
    ops.state_slots_hold(src, d0, layout, torch.zeros(B, dtype=torch.int32, device=DEV), **{k: o0[k] for k in given})
    torch.cuda.synchronize()
    assert torch.equal(d0, dst) and all(torch.equal(o0[k], outs[k]) for k in outs)

    exp = dst.clone()
    for e, s in zip(_views(exp, layout), _views(src, layout)):
        e[held] = s[held]
    exp_out = {k: v.clone() for k, v in outs.items()}
    exp_out["wav"][held] = 0
    exp_out["indices"][:, held] = -1
    exp_out["packets"][held] = 0
    exp_out["nbytes"][held] = 0
    got = {k: v.clone() for k, v in outs.items()}
    ops.state_slots_hold(src, dst, layout, hold.to(DEV), **{k: got[k] for k in given})
    torch.cuda.synchronize()
    assert torch.equal(dst, exp)                          # held rows copied, every other float (padding included) untouched
    for k in outs:
        assert torch.equal(got[k], exp_out[k] if k in given else outs[k]), k


@pytest.mark.parametrize("groups", [1, 2])
def test_loopback_hold_equals_eager(speech, groups):
    from hilcodec_amd.graph_step import GraphedHop
    B, hops = 37, 8
    x = synth.synth_clips(B, HOP * hops, seed=201).to(DEV)
    plan = hold_plan(B, hops, seed=202)
    g = GraphedHop(speech, B, HOP, 8, DEV, groups=groups, sessions=True)
    e = EagerHeld(speech, B)
    for h in range(hops):
        e_idx, e_wav = e.step(chunk(x, h), plan[h])
        idx, wav = g.step(garbage_rows(chunk(x, h), plan[h], seed=300 + h), hold=plan[h])
        assert torch.equal(idx, e_idx) and torch.equal(wav, e_wav), f"hop {h}"
        assert caches_equal(g.cache_enc, e.ce) and caches_equal(g.cache_dec, e.cd), f"hop {h}"


def test_sender_receiver_hold_equals_loopback(speech):
    """the same holds on both sides (slot 5 by stop() on the split sides from hop 3 to its start at hop 6, by hold= on the
    loopback): held rows have nbytes 0, zero packet rows and zero wav; everything else equals the loopback bit for bit"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedHop
    B, hops = 37, 8
    x = synth.synth_clips(B, HOP * hops, seed=203).to(DEV)
    plan = hold_plan(B, hops, seed=202)
    loop = GraphedHop(speech, B, HOP, 8, DEV, sessions=True)
    s = GraphedEncodeHop(speech, B, HOP, 8, DEV, sessions=True)
    r = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True)
    gen = torch.Generator().manual_seed(5)
    for h in range(hops):
        if h == 3:
            s.stop(5)
            r.stop(5)
            assert s.stopped == (5,) and r.stopped == (5,)
        if h == 6:
            for side in (loop, s, r):
                side.start(5)
        held = sorted(set(plan[h]) | ({5} if 3 <= h < 6 else set()))
        explicit = plan[h]                                # the split sides get slot 5 from their stop
        xin = garbage_rows(chunk(x, h), held, seed=400 + h)
        idx, wav = loop.step(xin, hold=held)
        packets, nbytes = s.step(xin, hold=explicit)
        assert torch.equal(s.indices, idx), f"hop {h}"
        exp_n = torch.tensor([0 if b in held else wire.packet_bytes(8, 1) for b in range(B)], dtype=torch.int32)
        assert torch.equal(nbytes.cpu(), exp_n), f"hop {h}"
        if held:
            assert not bool(packets[held].any()), f"hop {h}"
        n_list = [0 if b in held else 8 for b in range(B)]   # a held slot's n need not be valid
        pk = packets.clone()
        if held:
            pk[held] = torch.randint(0, 256, (len(held), pk.shape[1]), generator=gen, dtype=torch.uint8).to(DEV)
        r_wav = r.step(pk, n_list, hold=explicit)
        assert torch.equal(r_wav, wav), f"hop {h}"
        if held:
            assert not bool(r_wav[held].any())
        assert caches_equal(s.cache_enc, loop.cache_enc) and caches_equal(r.cache_dec, loop.cache_dec), f"hop {h}"
    assert s.stopped == () and r.stopped == ()


def test_lifecycle(speech):
    """stop(3) at hop 2, export(3) at hop 4 = the caches after hop 1, start(3) at hop 5; start(1) with hold [1] at hop 6 leaves
    slot 1 fresh; set_bitrate(4, 2) on a slot held at hop 6 applies from hop 7"""
    from hilcodec_amd.graph_step import GraphedHop
    B, hops = 6, 9
    x = synth.synth_clips(B, HOP * hops, seed=204).to(DEV)
    g = GraphedHop(speech, B, HOP, 8, DEV, sessions=True)
    e = EagerHeld(speech, B)
    n_list = [8] * B
    snap = None
    for h in range(hops):
        held, zero, hold = [], [], None
        if h == 2:
            g.stop(3)
            assert g.stopped == (3,)
        if 2 <= h < 5:
            held = [3]
        if h == 4:
            enc, dec = g.export(3)
            assert caches_equal(enc + dec, snap)
        if h == 5:
            g.start(3)
            assert g.stopped == ()
            zero = [3]
        if h == 6:
            g.start(1)
            g.set_bitrate(4, 2)
            hold = held = [1, 4]
            zero = [1]
        if h >= 6:
            n_list[4] = 2
        e_idx, e_wav = e.step(chunk(x, h), held, n=list(n_list), zero=zero)
        idx, wav = g.step(chunk(x, h), hold=hold)
        assert same_indices(idx, e_idx) and torch.equal(wav, e_wav), f"hop {h}"
        assert caches_equal(g.cache_enc, e.ce) and caches_equal(g.cache_dec, e.cd), f"hop {h}"
        if h == 1:
            snap = [c[3:4].clone() for c in list(e.ce) + list(e.cd)]
        if h == 6:
            enc, dec = g.export(1)
            assert not any(bool(c.any()) for c in enc + dec)          # fresh, and nothing more
        if h >= 7:
            assert bool((idx[2:, 4] == -1).all()) and bool((idx[:2, 4] >= 0).all())
    g.stop(2)
    g.reset()
    assert g.stopped == ()


def test_hold_at_production_shape(speech):
    """1 024 streams, n = 8, 10 hops, 64 seeded random held streams per hop, against the eager loop"""
    from hilcodec_amd.graph_step import GraphedHop
    B, hops = 1024, 10
    x = synth.synth_clips(B, HOP * hops, seed=205).to(DEV)
    rng = np.random.default_rng(206)
    g = GraphedHop(speech, B, HOP, 8, DEV, groups=2, sessions=True)
    e = EagerHeld(speech, B)
    for h in range(hops):
        held = sorted(rng.permutation(B)[:64].tolist())
        e_idx, e_wav = e.step(chunk(x, h), held)
        idx, wav = g.step(chunk(x, h), hold=held)
        assert torch.equal(idx, e_idx), f"hop {h} indices"
        assert torch.equal(wav, e_wav), f"hop {h} wav"
    assert caches_equal(g.cache_enc, e.ce) and caches_equal(g.cache_dec, e.cd)


def test_hold_checks(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedHop
    B = 3
    x = synth.synth_clips(B, HOP, seed=207).to(DEV)
    plain = GraphedHop(speech, B, HOP, 8, DEV)
    ref_idx, ref_wav = [t.clone() for t in plain.step(x)]
    plain.reset()
    with pytest.raises(RuntimeError):
        plain.step(x, hold=[1])
    with pytest.raises(RuntimeError):
        plain.stop(1)
    assert plain.stopped == ()
    idx, wav = plain.step(x, hold=[])                     # empty: accepted, the hop of earlier rounds
    assert torch.equal(idx, ref_idx) and torch.equal(wav, ref_wav)
    plain.step(x, hold=None)
    s = GraphedEncodeHop(speech, B, HOP, 8, DEV)
    with pytest.raises(RuntimeError):
        s.step(x, hold=[0])
    with pytest.raises(RuntimeError):
        s.stop(0)
    r = GraphedDecodeHop(speech, B, 1, 8, DEV)
    pk = torch.zeros(B, wire.packet_bytes(8, 1), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        r.step(pk, [8] * B, hold=[2])
    with pytest.raises(RuntimeError):
        r.stop(2)
    r.step(pk, [8] * B, hold=[])
    sess = GraphedHop(speech, B, HOP, 8, DEV, sessions=True)
    with pytest.raises(IndexError):
        sess.step(x, hold=[0, 3])
    with pytest.raises(ValueError):
        sess.step(x, hold=torch.tensor([1], device=DEV))
    with pytest.raises(IndexError):
        sess.stop(-1)
    rs = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True)
    with pytest.raises(ValueError):
        rs.step(pk, [8, 0, 8], hold=[2])                  # slot 1 is not held: its n is checked
    rs.step(pk, [8, 0, 8], hold=[1])
