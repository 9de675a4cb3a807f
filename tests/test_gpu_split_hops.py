"""GPU: the sender / receiver split of the graphed hop.  The packet kernel against the host packer, the packed dequantiser against
rvq_decode, GraphedEncodeHop and GraphedDecodeHop against their eager loops, sender -> receiver against the loopback GraphedHop,
and per-side sessions — every comparison bit for bit (torch.equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth, wire
from tests.hops import chunk

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def host_packets(idx, n_list):
    """[n_max, B, T] indices + per-stream n -> the host reference batch (uint8 [B, stride], int32 [B])"""
    n_max, B, T = idx.shape
    idx = idx.cpu()
    out = torch.zeros(B, wire.packet_bytes(n_max, T), dtype=torch.uint8)
    nbytes = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        blob = wire.pack_stream_packet(idx[:n_list[b], b])
        out[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        nbytes[b] = len(blob)
    return out, nbytes


def ragged(B, n_max, T, seed):
    g = torch.Generator().manual_seed(seed)
    n_list = torch.randint(1, n_max + 1, (B,), generator=g).tolist()
    idx = torch.randint(0, 1024, (n_max, B, T), generator=g)
    for b, n in enumerate(n_list):
        idx[n:, b] = -1                                   # as the streaming quantiser writes rows >= a stream's n
    return idx, n_list


@pytest.mark.parametrize("B", [1, 37, 1024])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_pack_codes_matches_host(B, T):
    from hilcodec_amd import ops
    for n_max in (8, 12):
        idx, n_list = ragged(B, n_max, T, seed=B * 100 + T + n_max)
        ref, ref_n = host_packets(idx, n_list)
        n_clip = torch.tensor(n_list, dtype=torch.int32, device=DEV)
        packets, nbytes = ops.pack_codes_10bit(idx.to(DEV), n_clip)
        torch.cuda.synchronize()
        assert torch.equal(packets.cpu(), ref), (n_max, B, T)
        assert torch.equal(nbytes.cpu(), ref_n)
        full = idx.clamp(min=0)
        packets, nbytes = ops.pack_codes_10bit(full.to(DEV))                 # no n_clip: every stream n_max stages
        assert torch.equal(packets.cpu(), host_packets(full, [n_max] * B)[0])
        assert bool((nbytes == wire.packet_bytes(n_max, T)).all())


def test_pack_codes_clamps_out_of_range():
    from hilcodec_amd import ops
    idx = torch.tensor([[[5, -3]], [[2000, 1023]]])       # [2, 1, 2]
    packets, _ = ops.pack_codes_10bit(idx.to(DEV))
    assert torch.equal(packets.cpu(), host_packets(torch.tensor([[[5, 0]], [[1023, 1023]]]), [2])[0])


@pytest.mark.parametrize("name,n_max", [("hil_speech", 8), ("hil_music", 12)])
def test_rvq_decode_packed_matches_rvq_decode(name, n_max):
    from hilcodec_amd import ops
    model = synth.streaming_model(name, 3)
    cb = model.dequantizer._tables(DEV).codebooks
    for B, T in ((37, 1), (37, 2), (1024, 1), (5, 5)):
        idx, n_list = ragged(B, n_max, T, seed=B + 10 * T + n_max)
        n_clip = torch.tensor(n_list, dtype=torch.int32, device=DEV)
        ref = ops.rvq_decode(idx.to(DEV), cb, n_max, n_clip=n_clip)
        packets = host_packets(idx, n_list)[0].to(DEV)
        q = ops.rvq_decode_packed(packets, cb, n_max, T, n_clip=n_clip)
        assert q.shape == (B, T, cb.shape[2])
        assert torch.equal(q, ref), (name, B, T)
        assert torch.equal(model.dequantizer.decode_packed(packets, n_clip, n_max, T), ref)
        full = idx.clamp(min=0)
        assert torch.equal(ops.rvq_decode_packed(host_packets(full, [n_max] * B)[0].to(DEV), cb, n_max, T),
                           ops.rvq_decode(full.to(DEV), cb, n_max))


@pytest.mark.parametrize("B", [37, 1024])
def test_sender_equals_eager(speech, B):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    model, hops = speech, 6
    x = synth.synth_clips(B, HOP * hops, seed=101).to(DEV)
    s = GraphedEncodeHop(model, B, HOP, 8, DEV)
    assert len(s.cache_enc) == 22 and s.state_bytes == 2 * 4 * s.state[0].layout.total
    ce, _ = model.initialize_cache(x)
    for h in range(hops):
        with torch.no_grad():
            z, ce = model.encoder(chunk(x, h), *ce)
            idx = model.quantizer(z, 8)
        packets, nbytes = s.step(chunk(x, h))
        assert torch.equal(s.indices, idx), f"hop {h}"
        ref, ref_n = host_packets(idx, [8] * B)
        assert torch.equal(packets.cpu(), ref) and torch.equal(nbytes.cpu(), ref_n), f"hop {h}"
    assert all(torch.equal(a, b) for a, b in zip(s.cache_enc, ce))


@pytest.mark.parametrize("B,frames", [(37, 1), (37, 2), (1024, 1)])
def test_receiver_equals_eager(speech, B, frames):
    from hilcodec_amd import ops
    from hilcodec_amd.graph_step import GraphedDecodeHop
    model, hops = speech, 6
    r = GraphedDecodeHop(model, B, frames, 8, DEV)
    assert len(r.cache_dec) == 30
    _, cd = model.initialize_cache(torch.zeros(B, 1, 1, device=DEV))
    for h in range(hops):
        idx, n_list = ragged(B, 8, frames, seed=1000 * h + B + frames)
        if h % 2:
            packets = host_packets(idx, n_list)[0]                                  # host packets: the pinned upload
        else:
            packets = ops.pack_codes_10bit(idx.to(DEV), torch.tensor(n_list, dtype=torch.int32, device=DEV))[0]
        with torch.no_grad():
            wav_ref, cd = model.decoder(model.dequantizer(idx.to(DEV)[:max(n_list)].contiguous(), n_list), *cd)
        wav = r.step(packets, n_list)
        assert wav.shape == (B, 1, HOP * frames)
        assert torch.equal(wav, wav_ref), f"hop {h}"
    assert all(torch.equal(a, b) for a, b in zip(r.cache_dec, cd))
    bad = list(n_list)
    bad[0] = 9
    with pytest.raises(ValueError):
        r.step(packets, bad)
    with pytest.raises(ValueError):
        r.step(packets, n_list[:-1])
    with pytest.raises(ValueError):
        r.step(packets[:, :-1], n_list)


def test_sender_to_receiver_equals_loopback(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedHop
    model, B, hops = speech, 37, 6
    x = synth.synth_clips(B, HOP * hops, seed=102).to(DEV)
    loop = GraphedHop(model, B, HOP, 8, DEV, sessions=True)
    s = GraphedEncodeHop(model, B, HOP, 8, DEV, sessions=True)
    r = GraphedDecodeHop(model, B, 1, 8, DEV, sessions=True)
    n_list = [8] * B
    rng = np.random.default_rng(7)
    for h in range(hops):
        if h in (2, 4):
            for b in rng.permutation(B)[:12].tolist():
                v = int(rng.choice([1, 2, 4, 8]))
                loop.set_bitrate(b, v)
                s.set_bitrate(b, v)
                n_list[b] = v
        idx, wav = loop.step(chunk(x, h))
        packets, nbytes = s.step(chunk(x, h))
        assert torch.equal(s.indices, idx), f"hop {h}"
        assert nbytes.tolist() == [wire.packet_bytes(n, 1) for n in n_list]
        assert torch.equal(r.step(packets, n_list), wav), f"hop {h}"


def _eager_loop(model, x, hops, restart=None):
    """eager encoder -> RVQ -> dequantiser -> decoder, n = 8; `restart` = (hop, slot): that slot's caches zeroed before that hop"""
    ce, cd = model.initialize_cache(x)
    out = []
    for h in range(hops):
        if restart is not None and h == restart[0]:
            for c in list(ce) + list(cd):
                c[restart[1]].zero_()
        with torch.no_grad():
            z, ce = model.encoder(chunk(x, h), *ce)
            idx = model.quantizer(z, 8)
            wav, cd = model.decoder(model.dequantizer(idx, 8), *cd)
        out.append((idx.clone(), wav.clone()))
    return out, ce, cd


def test_sessions_on_each_side(speech):
    """start mid-run on both sides; resume from each side's export; resume from a loopback GraphedHop.export split in halves"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedHop
    model, B, hops, at = speech, 6, 6, 3
    x = synth.synth_clips(B, HOP * hops, seed=103).to(DEV)
    xs = x.clone()
    xs[2:3, :, HOP * at:] = synth.synth_clips(1, HOP * (hops - at), seed=104).to(DEV)
    ref, _, _ = _eager_loop(model, x, hops)
    ref2, ce2, cd2 = _eager_loop(model, xs, hops, restart=(at, 2))
    s = GraphedEncodeHop(model, B, HOP, 8, DEV, sessions=True)
    r = GraphedDecodeHop(model, B, 1, 8, DEV, sessions=True)
    loop = GraphedHop(model, B, HOP, 8, DEV, sessions=True)
    others = [b for b in range(B) if b != 2]
    saved = {}
    for h in range(hops):
        if h == at:
            s.start(2)
            r.start(2)
        packets, _ = s.step(chunk(xs, h))
        wav = r.step(packets, [8] * B)
        loop.step(chunk(x, h))
        assert torch.equal(s.indices, ref2[h][0]) and torch.equal(wav, ref2[h][1]), f"hop {h}"
        assert torch.equal(wav[others], ref[h][1][others]), f"hop {h}"
        if h == 2:
            saved["split"] = (s.export(4), r.export(4))
            saved["loop"] = loop.export(5)
            assert all(torch.equal(a[0], b[4]) for a, b in zip(saved["split"][0], s.cache_enc))
    assert all(torch.equal(a, b) for a, b in zip(s.cache_enc, ce2))
    assert all(torch.equal(a, b) for a, b in zip(r.cache_dec, cd2))
    # resume: slot 0 from the sender's / receiver's exports of stream 4, slot 1 from the loopback's export of stream 5 (host copies)
    enc4, dec4 = saved["split"]
    enc5, dec5 = [[c.cpu() for c in part] for part in saved["loop"]]
    other = synth.synth_clips(3, HOP * 4, seed=105).to(DEV)
    s2 = GraphedEncodeHop(model, 3, HOP, 8, DEV, sessions=True)
    r2 = GraphedDecodeHop(model, 3, 1, 8, DEV, sessions=True)
    p, _ = s2.step(chunk(other, 0))
    r2.step(p, [8] * 3)
    s2.start(0, enc4)
    r2.start(0, dec4)
    s2.start(1, enc5)
    r2.start(1, dec5)
    for k, h in enumerate(range(3, hops)):
        xin = chunk(other, k + 1).clone()
        xin[0] = chunk(x, h)[4]
        xin[1] = chunk(x, h)[5]
        p, _ = s2.step(xin)
        wav = r2.step(p, [8] * 3)
        assert torch.equal(s2.indices[:, :2], ref[h][0][:, 4:6]), f"hop {h}"
        assert torch.equal(wav[:2], ref[h][1][4:6]), f"hop {h}"
    with pytest.raises(RuntimeError):
        GraphedDecodeHop(model, 2, 1, 8, DEV).start(0)
