"""GPU: per-stream sessions of the graphed hop (GraphedHop(sessions=True)): idle sessions change no bit, a stream started,
resumed or re-rated in one slot equals the eager loop that does the same to that row of its caches, bit for bit, and the
per-stream bitrate agrees with the oracle."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from tests.hops import build_streaming, chunk, same_indices

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320


def eager_hop(model, x, ce, cd, n):
    with torch.no_grad():
        z, ce = model.encoder(x, *ce)
        idx = model.quantizer(z, n)
        wav, cd = model.decoder(model.dequantizer(idx, n), *cd)
    return z, idx, wav, ce, cd


def caches_equal(g, ce, cd, rows=None):
    ge, gd = g.cache_enc, g.cache_dec
    for a, b in zip(list(ge) + list(gd), list(ce) + list(cd)):
        if rows is not None:
            a, b = a[rows], b[rows]
        if not torch.equal(a, b):
            return False
    return True


@pytest.mark.parametrize("groups", [1, 2])
def test_idle_sessions_equal_plain_graph(groups):
    from hilcodec_amd.graph_step import GraphedHop
    model, _, _ = build_streaming()
    B, hops = 5, 4
    x = synth.synth_clips(B, HOP * hops, seed=91).to(DEV)
    plain = GraphedHop(model, B, HOP, 8, DEV, groups=groups)
    sess = GraphedHop(model, B, HOP, 8, DEV, groups=groups, sessions=True)
    for h in range(hops):
        i0, w0 = plain.step(chunk(x, h))
        i1, w1 = sess.step(chunk(x, h))
        assert torch.equal(i0, i1) and torch.equal(w0, w1), f"hop {h}"
    for a, b in zip(list(plain.cache_enc) + list(plain.cache_dec), list(sess.cache_enc) + list(sess.cache_dec)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("groups", [1, 2])
def test_start_mid_run(groups):
    """B = 6; at hop 3 slot 2 starts a new stream: its outputs and caches equal an eager run of the new signal from zero caches in
    row 2, every other slot equals the uninterrupted run"""
    from hilcodec_amd.graph_step import GraphedHop
    model, _, _ = build_streaming()
    B, hops, at = 6, 6, 3
    x = synth.synth_clips(B, HOP * hops, seed=92).to(DEV)
    fresh = synth.synth_clips(1, HOP * (hops - at), seed=93).to(DEV)
    xs = x.clone()
    xs[2:3, :, HOP * at:] = fresh
    ce, cd = model.initialize_cache(x)
    ce2, cd2 = model.initialize_cache(x)
    ref, ref2 = [], []
    for h in range(hops):
        _, idx, wav, ce, cd = eager_hop(model, chunk(x, h), ce, cd, 8)
        ref.append((idx.clone(), wav.clone()))
        if h == at:
            for c in list(ce2) + list(cd2):
                c[2].zero_()
        _, idx, wav, ce2, cd2 = eager_hop(model, chunk(xs, h), ce2, cd2, 8)
        ref2.append((idx.clone(), wav.clone()))
    g = GraphedHop(model, B, HOP, 8, DEV, groups=groups, sessions=True)
    others = [b for b in range(B) if b != 2]
    for h in range(hops):
        if h == at:
            g.start(2)
        idx, wav = g.step(chunk(xs, h))
        assert torch.equal(idx, ref2[h][0]) and torch.equal(wav, ref2[h][1]), f"hop {h}"
        assert torch.equal(idx[:, others], ref[h][0][:, others]) and torch.equal(wav[others], ref[h][1][others]), f"hop {h}"
    assert caches_equal(g, ce2, cd2)
    assert caches_equal(g, ce, cd, rows=others)


def test_resume_elsewhere(tmp_path):
    """export(4) of graph A (B = 6) after its hop 2, through the npz cache format, into slot 0 of graph B (B = 3, groups 2) at
    its hop 1: the slot continues bit-identical to the uninterrupted stream 4"""
    from hilcodec_amd import wire
    from hilcodec_amd.graph_step import GraphedHop
    model, _, _ = build_streaming()
    B, hops = 6, 6
    x = synth.synth_clips(B, HOP * hops, seed=94).to(DEV)
    other = synth.synth_clips(3, HOP * 4, seed=95).to(DEV)
    ce, cd = model.initialize_cache(x)
    ref = []
    for h in range(hops):
        _, idx, wav, ce, cd = eager_hop(model, chunk(x, h), ce, cd, 8)
        ref.append((idx.clone(), wav.clone()))
    ga = GraphedHop(model, B, HOP, 8, DEV, sessions=True)
    for h in range(3):
        ga.step(chunk(x, h))
    enc, dec = ga.export(4)
    assert len(enc) == 22 and len(dec) == 30 and all(c.shape[0] == 1 for c in enc + dec)
    wire.save_cache_npz(str(tmp_path / "enc.npz"), enc, "e_in")
    wire.save_cache_npz(str(tmp_path / "dec.npz"), dec, "d_in")
    enc = wire.load_cache_npz(str(tmp_path / "enc.npz"), "e_in", batch=1)          # host tensors: the pinned upload path
    dec = wire.load_cache_npz(str(tmp_path / "dec.npz"), "d_in", DEV, batch=1)     # device tensors: a device copy
    gb = GraphedHop(model, 3, HOP, 8, DEV, groups=2, sessions=True)
    gb.step(chunk(other, 0))
    gb.start(0, enc, dec)
    for k, h in enumerate(range(3, hops)):
        xin = chunk(other, k + 1).clone()
        xin[0] = chunk(x, h)[4]
        idx, wav = gb.step(xin)
        assert torch.equal(idx[:, 0], ref[h][0][:, 4]) and torch.equal(wav[0], ref[h][1][4]), f"hop {h}"
    e2, d2 = gb.export(0)
    for a, b in zip(e2 + d2, list(ce) + list(cd)):
        assert torch.equal(a[0], b[4])


def test_per_stream_bitrate():
    """slots at n in {1, 2, 4, 8}, changed at hop 2: the eager loop with a per-clip n list on every hop, bit for bit; and three
    streams with a per-hop n against the oracle's streaming functions at the streaming bars"""
    from hilcodec_amd.graph_step import GraphedHop
    from oracle import hilcodec_oracle as O
    model, mk, sd = build_streaming(seed=11)
    B, hops = 4, 4
    x = synth.synth_clips(B, HOP * hops, seed=96).to(DEV)
    plan = [[1, 2, 4, 8]] * 2 + [[8, 4, 1, 2]] * 2
    g = GraphedHop(model, B, HOP, 8, DEV, sessions=True)
    ce, cd = model.initialize_cache(x)
    for h in range(hops):
        if h in (0, 2):
            for b in range(B):
                g.set_bitrate(b, plan[h][b])
        _, e_idx, e_wav, ce, cd = eager_hop(model, chunk(x, h), ce, cd, plan[h])
        idx, wav = g.step(chunk(x, h))
        assert same_indices(idx, e_idx) and torch.equal(wav, e_wav), f"hop {h}"
        for b in range(B):
            assert bool((idx[plan[h][b]:, b] == -1).all())
    assert caches_equal(g, ce, cd)

    # oracle leg: 3 streams, one n per stream and hop
    B = 3
    per_hop = [[1, 8, 4], [1, 8, 4], [4, 2, 8], [4, 2, 8]]
    p = O.stream_prepare(sd, mk)
    x = synth.synth_clips(B, HOP * hops, seed=97)
    g = GraphedHop(model, B, HOP, 8, DEV, sessions=True)
    ce, cd = model.initialize_cache(x.to(DEV))
    oc = [O.stream_init_cache(mk, 1) for _ in range(B)]
    for h in range(hops):
        for b in range(B):
            g.set_bitrate(b, per_hop[h][b])
        xin = chunk(x, h)
        idx, wav = g.step(xin.to(DEV))
        z, _, _, ce, cd = eager_hop(model, xin.to(DEV), ce, cd, per_hop[h])
        for b in range(B):
            n = per_hop[h][b]
            oe, od = oc[b]
            zo, oe = O.stream_encoder(p, mk, xin[b:b + 1], oe)
            io = O.stream_quantize(p, zo, n)
            wo, od = O.stream_decoder(p, mk, O.stream_dequantize(p, io, n), od)
            oc[b] = (oe, od)
            assert (z[b:b + 1].cpu() - zo).abs().max() < 2e-5
            assert torch.equal(idx[:n, b:b + 1].cpu(), io) and bool((idx[n:, b] == -1).all()), f"hop {h} stream {b}"
            assert (wav[b:b + 1].cpu() - wo).abs().max() < 1e-4
            for a, o in zip(list(g.cache_enc) + list(g.cache_dec), list(oe) + list(od)):
                assert (a[b:b + 1].cpu() - o).abs().max() < 5e-5


def test_sessions_at_production_shape():
    """B = 1 024 (the stage launches' production tile forms), 6 hops, every hop 16 fresh starts, 2 resumes and 8 bitrate changes at
    seeded random slots, against an eager B = 1 024 loop that does the same with per-slot zero_() / copy_() on its cache views and
    a per-clip n: bit-identical"""
    from hilcodec_amd.graph_step import GraphedHop
    model, _, _ = build_streaming()
    B, hops = 1024, 6
    x = synth.synth_clips(B, HOP * hops, seed=98).to(DEV)
    rng = np.random.default_rng(1234)
    g = GraphedHop(model, B, HOP, 8, DEV, groups=2, sessions=True)
    ce, cd = model.initialize_cache(x)
    n_list = [8] * B
    for h in range(hops):
        slots = rng.permutation(B)[:26].tolist()
        starts, resumes, rates = slots[:16], slots[16:18], slots[18:]
        if h > 0:
            sources = rng.integers(0, B, size=2).tolist()
            snaps = [[c[s:s + 1].clone() for c in list(ce) + list(cd)] for s in sources]   # before any action of this hop
            for dst, src, snap in zip(resumes, sources, snaps):
                enc, dec = g.export(src)
                assert all(torch.equal(a, b) for a, b in zip(enc + dec, snap))
                g.start(dst, enc, dec)
                for c, s in zip(list(ce) + list(cd), snap):
                    c[dst].copy_(s[0])
                n_list[dst] = 8
        for s in starts:
            g.start(s)
            for c in list(ce) + list(cd):
                c[s].zero_()
            n_list[s] = 8
        for s in rates:
            v = int(rng.choice([1, 2, 4, 8]))
            g.set_bitrate(s, v)
            n_list[s] = v
        _, e_idx, e_wav, ce, cd = eager_hop(model, chunk(x, h), ce, cd, list(n_list))
        idx, wav = g.step(chunk(x, h))
        assert same_indices(idx, e_idx), f"hop {h} indices"
        assert torch.equal(wav, e_wav), f"hop {h} wav"
    assert caches_equal(g, ce, cd)
