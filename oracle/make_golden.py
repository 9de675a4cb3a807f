"""Generate `tests/golden/*.npz` from the REAL reference (aask1357/hilcodec) — build container only.

Run:  python oracle/make_golden.py            (needs /root/reference; CPU, ~1 min)

Every expected output below is produced by the reference's own PyTorch modules
(`models/hilcodec/models.py`, `models/hilcodec/streaming.py`, `models/hilcodec/modules/*.py`,
`models/hilcodec/vector_quantize.py`, `modules/vector_quantize.py`,
`modules/weight_standardization.py`) on deterministic synthetic weights/inputs that are
*regenerated from seeds* (`hilcodec_amd/synth.py`) by the tests; only expected outputs (and tiny
op-level inputs) are stored.  The fixtures are data: nothing of the reference's source is kept.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hilcodec_amd import synth  # noqa: E402
from oracle import refimport as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 7
CLIP_SEED = 1234


def t2n(t):
    return t.detach().cpu().numpy()


def offline_golden(ref, name: str, n_clips: int, partial_n: int):
    mk = synth.model_kwargs(name)
    sd = synth.synth_state_dict(name, seed=WEIGHT_SEED)
    model = R.build_offline(ref, mk, sd)
    x = synth.synth_clips(n_clips, 24000, seed=CLIP_SEED)
    out = {}
    with torch.no_grad():
        z = model.encoder(x.clone())
        q, num_replaces, loss, idx = model.quantizer(z, None, return_indices=True)
        wav = model.decoder(q)
        wav2, nr2, loss2 = model(x.clone(), None)
        assert torch.equal(wav, wav2)
        qn, _, lossn, idxn = model.quantizer(z, partial_n, return_indices=True)
        wavn = model.decoder(qn)
        # a non-multiple-of-320 length exercises the "extra padding" branch (conv.py:61-68)
        xr = x[:1, :, :5000].clone()
        zr = model.encoder(xr.clone())
        qr, _, _, idxr = model.quantizer(zr, None, return_indices=True)
        wavr = model.decoder(qr)
    out.update(z=t2n(z), indices=t2n(idx).astype(np.int16), wav=t2n(wav), loss=t2n(loss),
               num_replaces=np.asarray(num_replaces),
               q_probe=t2n(q[:, :, ::15]),
               partial_n=np.int64(partial_n), indices_n=t2n(idxn).astype(np.int16),
               wav_n_probe=t2n(wavn[:, :, ::16]), loss_n=t2n(lossn),
               ragged_len=np.int64(5000), z_ragged=t2n(zr), indices_ragged=t2n(idxr).astype(np.int16),
               wav_ragged=t2n(wavr),
               weight_seed=np.int64(WEIGHT_SEED), clip_seed=np.int64(CLIP_SEED))
    np.savez_compressed(os.path.join(OUT, f"offline_{name}.npz"), **out)
    print(name, "offline: z", z.shape, "idx", idx.shape, "wav", wav.shape, "ragged z", zr.shape, "wav", wavr.shape)
    return model, mk, sd


def streaming_golden(ref, model, mk, sd, name: str):
    sm = R.build_streaming(ref, mk, model)
    hops = 10
    x = synth.synth_clips(1, 320 * hops, seed=CLIP_SEED + 500)
    ce, cd = sm.initialize_cache(x)
    zs, idxs, wavs = [], [], []
    snap = {}
    n = mk["vq_kwargs"]["num_quantizers"]
    with torch.no_grad():
        for h in range(hops):
            xin = x[:, :, 320 * h: 320 * (h + 1)]
            z, ce = sm.encoder(xin, *ce)
            idx = sm.quantizer(z, n)
            q = sm.dequantizer(idx, n)
            w, cd = sm.decoder(q, *cd)
            zs.append(z); idxs.append(idx); wavs.append(w)
            if h in (0, hops - 1):
                snap[h] = ([c.clone() for c in ce], [c.clone() for c in cd])
        # chunked call (3 frames at once) must equal frame-by-frame
        ce2, cd2 = sm.initialize_cache(x)
        z3, ce2 = sm.encoder(x[:, :, :960], *ce2)
    out = dict(z=t2n(torch.cat(zs, 1)), indices=t2n(torch.cat(idxs, 2)).astype(np.int16),
               wav=t2n(torch.cat(wavs, 2)), hops=np.int64(hops), clip_seed=np.int64(CLIP_SEED + 500),
               weight_seed=np.int64(WEIGHT_SEED), z_chunk3=t2n(z3))
    for i, c in enumerate(snap[hops - 1][0]):
        out[f"e_out{i}"] = t2n(c)
    for i, c in enumerate(snap[hops - 1][1]):
        out[f"d_out{i}"] = t2n(c)
    out["e_first_sums"] = np.array([c.double().sum().item() for c in snap[0][0]])
    out["d_first_sums"] = np.array([c.double().sum().item() for c in snap[0][1]])
    np.savez_compressed(os.path.join(OUT, f"stream_{name}.npz"), **out)
    print(name, "stream: z", out["z"].shape, "idx", out["indices"].shape, "wav", out["wav"].shape)


def ops_golden(ref):
    """One tiny known-answer vector per kernel kind, from the reference's own layer classes."""
    saved = list(sys.path)
    sys.path.insert(0, R.REFERENCE_ROOT)
    try:
        from models.hilcodec.modules import SConv1d, SConvTranspose1d, CausalSTFT
        from models.hilcodec.modules.seanet import SEANetResnetBlock, SpecBlock, L2Norm
        from models.hilcodec import causal_layers as CL
    finally:
        sys.path[:] = saved
    out = {}

    def fill(mod, seed):
        with torch.no_grad():
            for i, (k, p) in enumerate(sorted(mod.state_dict().items())):
                if k.endswith("spec.weight") or k == "weight" and isinstance(mod, CausalSTFT):
                    continue
                n = p.numel()
                if k.endswith("weight_g"):
                    v = synth.uniform(seed + i, n, 0.8, 1.2)
                elif k.endswith("scale_param"):
                    v = synth.uniform(seed + i, n, 0.5, 1.0)
                elif k.endswith("bias"):
                    v = synth.uniform(seed + i, n, -0.2, 0.2)
                else:
                    v = synth.uniform(seed + i, n, -1.0, 1.0)
                p.copy_(torch.from_numpy(v).view(p.shape))

    def dump(tag, mod):
        for k, p in mod.state_dict().items():
            out[f"{tag}.{k}"] = t2n(p)

    def inp(seed, *shape):
        return torch.from_numpy(synth.normalish(seed, int(np.prod(shape)))).view(*shape)

    with torch.no_grad():
        # pointwise conv after ELU, with bias (decoder up-pointwise style), odd Cin like the spec convs
        m = SConv1d(33, 40, 1, norm="weight_norm", bias=True); fill(m, 11)
        x = inp(1, 2, 33, 50)
        out["pw.x"] = t2n(x); dump("pw", m); out["pw.y"] = t2n(m(torch.nn.functional.elu(x)))
        # depthwise causal k5 (residual conv)
        m = SConv1d(24, 24, 5, groups=24, causal=True, norm="weight_norm", bias=True); fill(m, 21)
        x = inp(2, 2, 24, 37)
        out["dw5.x"] = t2n(x); dump("dw5", m); out["dw5.y"] = t2n(m(x))
        # strided depthwise (downsample), every ratio, ragged length
        for r in (2, 4, 5, 8):
            m = SConv1d(16, 16, 2 * r, stride=r, groups=16, causal=True, norm="weight_norm", bias=True)
            fill(m, 30 + r)
            x = inp(3 + r, 2, 16, 8 * r + 3)
            out[f"dws{r}.x"] = t2n(x); dump(f"dws{r}", m); out[f"dws{r}.y"] = t2n(m(x))
            mt = SConvTranspose1d(16, 16, 2 * r, stride=r, groups=16, causal=True, norm="weight_norm", bias=False)
            fill(mt, 40 + r)
            x = inp(13 + r, 2, 16, 9)
            out[f"dwt{r}.x"] = t2n(x); dump(f"dwt{r}", mt); out[f"dwt{r}.y"] = t2n(mt(x))
        # conv_pre (1 -> C, k5) and conv_post (C -> 1, k5)
        m = SConv1d(1, 16, 5, causal=True, norm="weight_norm", bias=True); fill(m, 51)
        x = inp(51, 2, 1, 100)
        out["pre.x"] = t2n(x); dump("pre", m); out["pre.y"] = t2n(m(x))
        m = SConv1d(12, 1, 5, causal=True, norm="weight_norm", bias=True); fill(m, 52)
        x = inp(52, 2, 12, 64)
        out["post.x"] = t2n(x); dump("post", m); out["post.y"] = t2n(m(x))
        # SpecBlock for a small n_fft (hop 1 and hop>1)
        for n_fft, hop in ((16, 1), (32, 4)):
            T = 96
            m = SpecBlock("stft", "log", n_fft, 8, hop, "weight_norm", {}, bias=False, pad_mode="constant",
                          learnable=False, causal=True, mean=-4.0, std=2.8, res_scale=0.5773502691896258,
                          zero_init=True, inout_norm=True)
            fill(m, 60 + hop)
            wav = inp(60 + hop, 2, 1, T) * 0.1
            xin = inp(61 + hop, 2, 8, (T - 1) // hop + 1)
            tag = f"spec{n_fft}"
            out[f"{tag}.wav"] = t2n(wav); out[f"{tag}.x"] = t2n(xin); dump(tag, m)
            out[f"{tag}.mag"] = t2n(m.spec(wav))
            out[f"{tag}.y"] = t2n(m(xin.clone(), wav))
        # residual block, idx 0/1/2
        for idx in (0, 1, 2):
            m = SEANetResnetBlock(16, kernel_size=5, dilations=[1, 1], norm="weight_norm", causal=True,
                                  skip="identity", res_scale=0.5773502691896258, idx=idx, zero_init=True)
            fill(m, 70 + idx)
            x = inp(70 + idx, 2, 16, 45)
            out[f"res{idx}.x"] = t2n(x); dump(f"res{idx}", m); out[f"res{idx}.y"] = t2n(m(x.clone()))
        # L2Norm
        x = inp(80, 2, 128, 9)
        x[0, :, 3] = 0.0
        out["l2.x"] = t2n(x); out["l2.y"] = t2n(L2Norm(128)(x))
        # weight-standardisation fold (available norm option, conv.py:36-37)
        conv = torch.nn.Conv1d(6, 10, 3)
        with torch.no_grad():
            conv.weight.copy_(inp(90, 10, 6, 3))
        out["ws.v"] = t2n(conv.weight)
        wsconv = ref.ws.weight_standardization(conv, scale=1.7)
        with torch.no_grad():
            wsconv.weight_g.copy_(torch.from_numpy(synth.uniform(91, 10, 0.5, 1.5)).view(10, 1, 1))
        wsconv(torch.zeros(1, 6, 8))   # pre-hook recomputes .weight
        out["ws.g"] = t2n(wsconv.weight_g); out["ws.scale"] = np.float32(1.7); out["ws.w"] = t2n(wsconv.weight)
        # streaming cache-carrying layers (causal_layers.py)
        c = CL.CausalConv1d(8, 8, 10, 5, groups=8, bias=True)
        x = inp(95, 2, 8, 15); cache = inp(96, 2, 8, c.causal_padding)
        y, nc = c(x, cache)
        out["cconv.x"] = t2n(x); out["cconv.cache"] = t2n(cache); out["cconv.w"] = t2n(c.weight)
        out["cconv.b"] = t2n(c.bias); out["cconv.y"] = t2n(y); out["cconv.cache_out"] = t2n(nc)
        ct = CL.CausalConvTranspose1d(8, 8, 10, 5, groups=8, bias=False)
        x = inp(97, 2, 8, 3); cache = inp(98, 2, 8, ct.causal_padding)
        y, nc = ct(x, cache)
        out["cconvtr.x"] = t2n(x); out["cconvtr.cache"] = t2n(cache); out["cconvtr.w"] = t2n(ct.weight)
        out["cconvtr.y"] = t2n(y); out["cconvtr.cache_out"] = t2n(nc)
    np.savez_compressed(os.path.join(OUT, "ops.npz"), **out)
    print("ops:", len(out), "arrays")


def rvq_golden(ref):
    """RVQ known-answer test: both distance forms (SURVEY §8 a8 vs a9/a16), n < Nq, indices + q."""
    nq, K, D = 12, 1024, 128
    z = torch.from_numpy(synth.normalish(4242, 2 * D * 75)).view(2, D, 75)
    z = torch.nn.functional.normalize(z, dim=1) * D ** 0.5
    new = ref.vq_new.ResidualVQ(num_quantizers=nq, dropout=False, channel_last=False, dim=D,
                                codebook_size=K, kmeans_init=False).eval()
    old = ref.vq_old.ResidualVQ(num_quantizers=nq, dropout=False, dim=D, codebook_size=K,
                                kmeans_init=False).eval()
    for i in range(nq):
        e = torch.from_numpy(synth.normalish(synth.key_seed(99, f"rvq{i}"), K * D) * np.float32(0.3 * 0.95 ** i)).view(K, D)
        new.layers[i].embed.copy_(e)
        old.layers[i]._codebook.embed.copy_(e)
    out = dict(codebook_seed=np.int64(99), z_seed=np.int64(4242))
    with torch.no_grad():
        q, nr, loss, idx = new(z, None, return_indices=True)
        out.update(indices=t2n(idx).astype(np.int16), q=t2n(q), loss=t2n(loss))
        q5, _, loss5, idx5 = new(z, 5, return_indices=True)
        out.update(indices_n5=t2n(idx5).astype(np.int16), q_n5_probe=t2n(q5[:, :, ::5]), loss_n5=t2n(loss5))
        qo, nro, losso = old(z, None)
        out.update(q_legacy=t2n(qo), loss_legacy=t2n(losso), num_replaces=np.asarray(nro))
    np.savez_compressed(os.path.join(OUT, "rvq.npz"), **out)
    print("rvq: idx", idx.shape, "legacy q diff", (q - qo).abs().max().item())


def rvq_train_golden(ref):
    """Training-branch known answer: two EMA steps of the reference `ResidualVQ` in train mode
    (dead-code expiry off so that no random replacement enters), from hash-generated codebooks."""
    nq, K, D, B, Tn, decay, init = 4, 1024, 128, 4, 75, 0.99, 0.5
    rvq = ref.vq_new.ResidualVQ(num_quantizers=nq, dropout=False, channel_last=False, dim=D, codebook_size=K,
                                kmeans_init=False, decay=decay, ema_num_threshold=0.0, ema_num_initial=init).train()
    for i in range(nq):
        e = torch.from_numpy(synth.normalish(synth.key_seed(77, f"rvq{i}"), K * D) * np.float32(0.3 * 0.95 ** i)).view(K, D)
        rvq.layers[i].embed.copy_(e)
        rvq.layers[i].ema_embed.copy_(e * init)
    out = dict(codebook_seed=np.int64(77), decay=np.float64(decay), ema_num_initial=np.float64(init))
    for step in range(2):
        z = torch.from_numpy(synth.normalish(600 + step, B * D * Tn)).view(B, D, Tn)
        z = torch.nn.functional.normalize(z, dim=1) * D ** 0.5
        q, nr, loss, idx = rvq(z, None, return_indices=True)
        out[f"z_seed{step}"] = np.int64(600 + step)
        out[f"indices{step}"] = t2n(idx).astype(np.int16)
        out[f"loss{step}"] = t2n(loss)
        out[f"q_probe{step}"] = t2n(q[:, :, ::5])
    out["ema_num"] = np.stack([t2n(l.ema_num) for l in rvq.layers])
    out["embed_rows"] = np.stack([t2n(l.embed[::16]) for l in rvq.layers])
    out["ema_embed_rows"] = np.stack([t2n(l.ema_embed[::16]) for l in rvq.layers])
    out["embed_sum"] = np.array([float(l.embed.double().sum()) for l in rvq.layers])
    np.savez_compressed(os.path.join(OUT, "rvq_train.npz"), **out)
    print("rvq_train: loss", float(loss), "ema_num range", out["ema_num"].min(), out["ema_num"].max())


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = R.load_reference()
    ops_golden(ref)
    rvq_golden(ref)
    model, mk, sd = offline_golden(ref, "hil_speech", n_clips=2, partial_n=4)
    streaming_golden(ref, model, mk, sd, "hil_speech")
    offline_golden(ref, "hil_music", n_clips=1, partial_n=2)
    trained_codebook_golden(ref)
    rvq_train_golden(ref)
    realistic_golden(ref)
    shard_golden(ref)
    for fname, scale in WS_GOLDENS:
        ws_golden(ref, fname, scale)
    vs_reference_golden(ref)
    onnx_files_golden()
    tot = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("golden bytes:", tot)




def realistic_golden(ref):
    """Realistic and adversarial INPUTS through the REAL reference (offline `HILCodec`): the reference's own 30.6 s speech
    recording (`onnx/input_speech.wav`) and its SHIPPED trained codebooks (`onnx/hil_speech_deq{i}.onnx`) — the only
    trained tensors in the tree; the conv weights stay the seeded synthetic ones (`.MISSING_LARGE_BLOBS`).  Stored: the
    waveform (int16 PCM as shipped), the 8 codebooks, and the reference's outputs for (a) the first 10 s, (b) the six
    adversarial clips, (c) RVQ encode of vectors 1e-6-close to sums of trained code words."""
    import wave
    from hilcodec_amd import wire
    onnx_dir = os.path.join(R.REFERENCE_ROOT, "onnx")
    with wave.open(os.path.join(onnx_dir, "input_speech.wav"), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2 and w.getframerate() == 24000
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy()
    assert pcm.shape == (734760,)          # 30.6 s; the reference encodes len // 320 * 320 = 734720 of them (test_onnx.py:53)
    cbs = np.stack([wire.read_onnx_codebook(os.path.join(onnx_dir, f"hil_speech_deq{i}.onnx")).numpy() for i in range(8)])
    assert cbs.shape == (8, 1024, 128) and cbs.dtype == np.float32
    mk = synth.model_kwargs("hil_speech")
    sd = synth.synth_state_dict("hil_speech", seed=WEIGHT_SEED)
    for i in range(8):
        sd[f"quantizer.layers.{i}.embed"] = torch.from_numpy(cbs[i]).clone()
    model = R.build_offline(ref, mk, sd)
    out = dict(pcm=pcm, codebooks=cbs, weight_seed=np.int64(WEIGHT_SEED))
    with torch.no_grad():
        x10 = torch.from_numpy(pcm[:240000].astype(np.float32) / 32768.0).view(1, 1, -1)
        z = model.encoder(x10.clone())
        q, _, loss, idx = model.quantizer(z, None, return_indices=True)
        wav = model.decoder(q)
        out.update(speech10_indices=t2n(idx).astype(np.int16), speech10_z_probe=t2n(z[:, :, ::25]),
                   speech10_wav_probe=t2n(wav[:, :, ::97]), speech10_loss=t2n(loss))
        xa = synth.adversarial_clips()
        za = model.encoder(xa.clone())
        qa, _, lossa, idxa = model.quantizer(za, None, return_indices=True)
        wava = model.decoder(qa)
        out.update(adv_indices=t2n(idxa).astype(np.int16), adv_z_probe=t2n(za[:, :, ::5]), adv_wav_probe=t2n(wava[:, :, ::31]),
                   adv_loss=t2n(lossa))
        # (c) near-tie stress on real tables: z = sum of the trained code words the reference's own bitstream selects
        # (onnx/hil_speech_quantized.npy) + 1e-6-scale noise, then the reference's RVQ encode
        idx_all = np.load(os.path.join(onnx_dir, "hil_speech_quantized.npy")).astype(np.int64)          # [8,1,2296]
        F = 600
        sel = torch.from_numpy(idx_all[:, 0, 200:200 + F])
        zq = sum(torch.from_numpy(cbs[i])[sel[i]] for i in range(8)).t().contiguous().view(1, 128, F)
        zq = zq + torch.from_numpy(synth.normalish(515, 128 * F)).view(1, 128, F) * 1e-6
        qn, _, lossn, idxn = model.quantizer(zq, None, return_indices=True)
        out.update(near_z=t2n(zq), near_indices=t2n(idxn).astype(np.int16), near_q_probe=t2n(qn[:, :, ::7]))
    np.savez_compressed(os.path.join(OUT, "realistic.npz"), **out)
    same = float((torch.from_numpy(t2n(idxn))[0] == sel).float().mean())
    print("realistic: speech10 idx", idx.shape, "adv idx", idxa.shape, "near-tie: fraction equal to the bitstream's own indices", same,
          "bytes", os.path.getsize(os.path.join(OUT, "realistic.npz")))


def shard_golden(ref):
    """BASELINE configs[4] (hil_music, 2048 clips over 8 GPUs = 256 per rank) has no reference-side multi-GPU inference to
    compare with (`train.py:51-61` is the reference's only NCCL setup); what CAN be pinned is that the clips a rank != 0
    owns — other seeds than any other golden — come out of the real reference's offline model as they do out of the HIP path
    when they sit inside that rank's full 256-clip shard.  Here: the first 8 clips of rank 7's shard (clips 1792..1799 of
    `synth_clips(first=1792)`, 1 s each) through the REAL reference; stored: all indices, z / wav probes."""
    name, first, n_clips = "hil_music", 1792, 8
    mk = synth.model_kwargs(name)
    sd = synth.synth_state_dict(name, seed=WEIGHT_SEED)
    model = R.build_offline(ref, mk, sd)
    x = synth.synth_clips(n_clips, 24000, seed=CLIP_SEED, first=first)
    zs, ids, ws = [], [], []
    with torch.no_grad():
        for i in range(0, n_clips, 4):
            z = model.encoder(x[i:i + 4].clone())
            q, _, _, idx = model.quantizer(z, None, return_indices=True)
            zs.append(z); ids.append(idx); ws.append(model.decoder(q))
    z, idx, wav = torch.cat(zs), torch.cat(ids), torch.cat(ws)
    np.savez_compressed(os.path.join(OUT, "shard_rank7_hil_music.npz"),
                        indices=t2n(idx).astype(np.int16), z_probe=t2n(z[:, :, ::5]), wav_probe=t2n(wav[:, :, ::25]),
                        z_abs_sum=np.float64(z.double().abs().sum()), wav_abs_sum=np.float64(wav.double().abs().sum()),
                        first=np.int64(first), rank=np.int64(7), world=np.int64(8), shard_clips=np.int64(256),
                        weight_seed=np.int64(WEIGHT_SEED), clip_seed=np.int64(CLIP_SEED))
    print("shard rank 7: idx", idx.shape, "checksum of the 8 clips", int(idx.sum()))


WS_KWARGS = {"eps": 1e-7, "scale": 0.8}      # (1.25 until round 4: the decoder caches reached |x| = 30 and the cache test needed a relative bar; at 0.8 they are O(1) and every bar is absolute)
# round 6 (advisor): BOTH scales are pinned — `ws_hil_speech.npz` at 0.8 (absolute bars) and `ws125_hil_speech.npz` at 1.25, the one model-level case with
# large activations (|x| ~ 30 through the fused stage kernels and the caches; its cache bar is relative)
WS_GOLDENS = (("ws_hil_speech.npz", 0.8), ("ws125_hil_speech.npz", 1.25))


def ws_golden(ref, fname="ws_hil_speech.npz", scale=None):
    """Whole-model weight standardisation (`conv.py:36-37`, `modules/weight_standardization.py:30-41`): the reference's
    offline `HILCodec(norm="weight_standardization", norm_kwargs=...)` on the seeded state dict (same keys as weight_norm:
    `weight_g/_v`; `weight_scale` is a buffer the constructor fills from `norm_kwargs['scale']`), 2 clips x 0.2 s.

    Streaming: the reference's streaming classes accept weight_norm only (`causal_layers.py:200-204` raises ValueError for
    anything else), so the only streaming flow a weight-standardised checkpoint has is fold -> plain weights -> streaming
    model (what `remove_weight_reparameterizations` + the notebook's mapping do for weight_norm).  The golden is the
    REFERENCE streaming model (built with weight_norm, hooks removed) carrying the plain weights that the reference's own
    `WeightStandardization.compute_weight` produced, 1 stream x 5 hops with every cache."""
    import copy
    name = "hil_speech"
    ws_kwargs = dict(WS_KWARGS, scale=WS_KWARGS["scale"] if scale is None else scale)
    mk = dict(synth.model_kwargs(name), norm="weight_standardization", norm_kwargs=dict(ws_kwargs))
    sd = synth.synth_state_dict(name, seed=WEIGHT_SEED)
    model = R.build_offline(ref, mk, sd)
    x = synth.synth_clips(2, 4800, seed=CLIP_SEED + 900)
    out = dict(weight_seed=np.int64(WEIGHT_SEED), clip_seed=np.int64(CLIP_SEED + 900), samples=np.int64(4800),
               ws_eps=np.float64(ws_kwargs["eps"]), ws_scale=np.float64(ws_kwargs["scale"]))
    with torch.no_grad():
        z = model.encoder(x.clone())
        q, _, loss, idx = model.quantizer(z, None, return_indices=True)
        wav = model.decoder(q)
    out.update(z=t2n(z), indices=t2n(idx).astype(np.int16), wav=t2n(wav), loss=t2n(loss))
    # one folded weight as a known answer of the fold itself (transposed conv: dim 0 = in_channels)
    out["fold_probe_convtr"] = t2n(model.decoder.model[4].convtr.convtr.weight)
    out["fold_probe_pw"] = t2n(model.encoder.blocks[1][0].block[1].conv.conv.weight)

    # streaming: plain (folded) weights into the reference's streaming model
    mk_wn = synth.model_kwargs(name)
    plain = R.build_offline(ref, mk_wn, sd)            # weight_norm twin: only its structure is used
    model(x[:1, :, :640].clone(), None)                # make sure every pre-hook has produced .weight
    src = dict(model.named_modules())
    with torch.no_grad():
        for mod_name, mod in plain.named_modules():
            if isinstance(mod, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)) and hasattr(mod, "weight_g"):
                torch.nn.utils.remove_weight_norm(mod)
                mod.weight.copy_(src[mod_name].weight)          # the reference's own compute_weight output
    sm = R.build_streaming(ref, mk_wn, plain, plain_weights=True)
    hops = 5
    xs = synth.synth_clips(1, 320 * hops, seed=CLIP_SEED + 901)
    ce, cd = sm.initialize_cache(xs)
    zs, idxs, wavs = [], [], []
    with torch.no_grad():
        for h in range(hops):
            zz, ce = sm.encoder(xs[:, :, 320 * h: 320 * (h + 1)], *ce)
            ii = sm.quantizer(zz, 8)
            w, cd = sm.decoder(sm.dequantizer(ii, 8), *cd)
            zs.append(zz); idxs.append(ii); wavs.append(w)
    out.update(s_z=t2n(torch.cat(zs, 1)), s_indices=t2n(torch.cat(idxs, 2)).astype(np.int16), s_wav=t2n(torch.cat(wavs, 2)),
               s_hops=np.int64(hops), s_clip_seed=np.int64(CLIP_SEED + 901))
    for i, c in enumerate(ce):
        out[f"e_out{i}"] = t2n(c)
    for i, c in enumerate(cd):
        out[f"d_out{i}"] = t2n(c)
    np.savez_compressed(os.path.join(OUT, fname), **out)
    print("ws", ws_kwargs["scale"], ": offline z", z.shape, "idx", idx.shape, "stream z", out["s_z"].shape, "largest cache value",
          max(float(np.abs(out[k]).max()) for k in out if k.startswith(("e_out", "d_out"))), "bytes", os.path.getsize(os.path.join(OUT, fname)))


def trained_codebook_golden(ref):
    """Dequantizer known-answer test on the reference's SHIPPED data: trained codebooks
    (`onnx/hil_speech_deq{i}.onnx`) + the first frames of `onnx/hil_speech_quantized.npy`, run through the
    reference's own `Dequantizer`.  Only the 8 x F referenced code vectors are stored, not the 4 MB tables."""
    from hilcodec_amd import wire
    onnx_dir = os.path.join(R.REFERENCE_ROOT, "onnx")
    idx_all = np.load(os.path.join(onnx_dir, "hil_speech_quantized.npy"))
    assert idx_all.dtype == np.int16 and idx_all.shape == (8, 1, 2296)
    F = 16
    idx = torch.from_numpy(idx_all[:, :, 100:100 + F].astype(np.int64))
    mk = synth.model_kwargs("hil_speech")
    deq = ref.StreamingHILCodec(24000, **{k: v for k, v in mk.items() if k not in ("spec_learnable", "causal", "pad_mode")}).dequantizer.eval()
    rows = np.zeros((8, F, 128), dtype=np.float32)
    for i in range(8):
        cb = wire.read_onnx_codebook(os.path.join(onnx_dir, f"hil_speech_deq{i}.onnx"))
        assert cb.shape == (1024, 128)
        deq.layers[i].embed.copy_(cb)
        rows[i] = cb[idx[i, 0]].numpy()
    with torch.no_grad():
        q = deq(idx, 8)
    np.savez_compressed(os.path.join(OUT, "trained_deq.npz"), indices=idx.numpy().astype(np.int16), rows=rows, q=t2n(q),
                        quantized_shape=np.array(idx_all.shape), quantized_sum=np.int64(idx_all.astype(np.int64).sum()))
    print("trained dequantizer KAT:", q.shape, float(q.abs().mean()))


def sha(t) -> str:
    """sha256 of a tensor's bytes: a bit-exact fingerprint of the tensors too large to store (codebooks, caches)."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(t2n(t)).tobytes()).hexdigest()


def vs_reference_golden(ref):
    """The reference's side of tests/test_oracle_vs_reference.py (its seeds and shapes, not those of the other goldens) and
    the reference's constructor signatures for tests/test_api_cpu.py.  Small outputs are stored whole, codebooks and
    streaming caches as sha256 fingerprints."""
    import inspect
    import json
    import yaml
    out = {}
    meta = {"state_dict_shapes": {}, "n_params": {}, "yaml_model_kwargs": {}}
    for name, f in (("hil_speech", "hilcodec_speech.yaml"), ("hil_music", "hilcodec_music.yaml")):
        mk = synth.model_kwargs(name)
        model = ref.OfflineHILCodec(sample_rate=24000, channels_audio=1, **copy.deepcopy(mk))
        meta["state_dict_shapes"][name] = [[k, list(v.shape)] for k, v in model.state_dict().items() if hasattr(v, "shape")]
        meta["n_params"][name] = sum(p.numel() for p in model.parameters())
        with open(os.path.join(R.REFERENCE_ROOT, "configs", f)) as fh:
            meta["yaml_model_kwargs"][name] = yaml.safe_load(fh)["model_kwargs"]
    # tests/test_api_cpu.py::test_legacy_rvq_matches_reference_constructor_and_state_dict
    sig = {}
    for cls in ("EuclideanCodebook", "VectorQuantize", "ResidualVQ"):
        ps = inspect.signature(getattr(ref.vq_old, cls).__init__).parameters
        sig[cls] = [[k, v.default is not inspect.Parameter.empty, None if v.default is inspect.Parameter.empty else v.default]
                    for k, v in ps.items()]
    sig["VectorQuantize.forward"] = list(inspect.signature(ref.vq_old.VectorQuantize.forward).parameters)
    meta["legacy_vq_signatures"] = sig
    kw = dict(num_quantizers=3, dropout=True, dropout_index=[1, 3], dim=16, codebook_size=32, kmeans_init=False,
              kmeans_iters=20, decay=0.9, eps=1e-7, ema_num_threshold=0.5, ema_num_initial=2.0, commitment=0.25,
              channel_last=False)
    meta["legacy_vq_state_dict_shapes"] = [[k, list(v.shape)] for k, v in ref.vq_old.ResidualVQ(**kw).state_dict().items()]

    for name, seed, T in (("hil_speech", 3, 6400), ("hil_music", 5, 3333)):
        mk = synth.model_kwargs(name)
        model = R.build_offline(ref, mk, synth.synth_state_dict(name, seed=seed))
        x = synth.synth_clips(2, T, seed=seed * 11)
        with torch.no_grad():
            z = model.encoder(x.clone())
            q, nr, loss, idx = model.quantizer(z, None, return_indices=True)
            wav = model.decoder(q)
        p = f"offline_{name}_"
        out.update({p + "z": t2n(z), p + "indices": t2n(idx).astype(np.int16), p + "wav": t2n(wav), p + "loss": t2n(loss),
                    p + "num_replaces": np.asarray(nr)})

    mk = synth.model_kwargs("hil_speech")
    model = R.build_offline(ref, mk, synth.synth_state_dict("hil_speech", seed=13))
    sm = R.build_streaming(ref, mk, model)
    x = synth.synth_clips(2, 1600, seed=77)
    ce, cd = sm.initialize_cache(x)
    meta["stream_cache_shapes"] = {"enc": [list(c.shape) for c in ce], "dec": [list(c.shape) for c in cd]}
    meta["stream_cache_sha"] = []
    zs, idxs, wavs = [], [], []
    with torch.no_grad():
        for h in range(0, 1600, 320):
            zr, ce = sm.encoder(x[:, :, h:h + 320], *ce)
            ir = sm.quantizer(zr, 8)
            wr, cd = sm.decoder(sm.dequantizer(ir, 8), *cd)
            zs.append(t2n(zr))
            idxs.append(t2n(ir).astype(np.int16))
            wavs.append(t2n(wr))
            meta["stream_cache_sha"].append({"enc": [sha(c) for c in ce], "dec": [sha(c) for c in cd]})
    out.update(stream_z=np.stack(zs), stream_indices=np.stack(idxs), stream_wav=np.stack(wavs))

    D, K, nq = 128, 1024, 4
    old = ref.vq_old.ResidualVQ(num_quantizers=nq, dropout=False, dim=D, codebook_size=K, kmeans_init=False).eval()
    for i in range(nq):
        old.layers[i]._codebook.embed.copy_(torch.from_numpy(synth.normalish(500 + i, K * D) * np.float32(0.3)).view(K, D))
    z = torch.from_numpy(synth.normalish(9, 3 * D * 20)).view(3, D, 20)
    with torch.no_grad():
        q, nr, loss = old(z, 3)
    out.update(legacy_q=t2n(q), legacy_num_replaces=np.asarray(nr), legacy_loss=t2n(loss))

    def train_trace(key, rvq, codebook, seed0, with_indices):
        """three train-mode steps: outputs per step, ema_num whole, embed / ema_embed as fingerprints"""
        meta[key + "_sha"] = []
        qs, losses, idxs, ema_nums = [], [], [], []
        for step in range(3):
            z = torch.from_numpy(synth.normalish(seed0 + step, 2 * D * 40)).view(2, D, 40)
            if with_indices:
                q, _, loss, idx = rvq(z, 2, return_indices=True)
                idxs.append(t2n(idx).astype(np.int16))
            else:
                q, _, loss = rvq(z, 2)
            qs.append(t2n(q))
            losses.append(t2n(loss))
            cbs = [codebook(rvq, i) for i in range(3)]
            ema_nums.append(np.stack([t2n(c.ema_num) for c in cbs]))
            meta[key + "_sha"].append({"embed": [sha(c.embed) for c in cbs], "ema_embed": [sha(c.ema_embed) for c in cbs]})
        out.update({key + "_q": np.stack(qs), key + "_loss": np.stack(losses), key + "_ema_num": np.stack(ema_nums)})
        if with_indices:
            out[key + "_indices"] = np.stack(idxs)

    decay, init = 0.9, 0.5
    rvq = ref.vq_new.ResidualVQ(num_quantizers=3, dropout=False, channel_last=False, dim=D, codebook_size=K,
                                kmeans_init=False, decay=decay, ema_num_threshold=0.0, ema_num_initial=init).train()
    for i in range(3):
        e = torch.from_numpy(synth.normalish(800 + i, K * D) * np.float32(0.3)).view(K, D)
        rvq.layers[i].embed.copy_(e)
        rvq.layers[i].ema_embed.copy_(e * init)
    train_trace("train", rvq, lambda m, i: m.layers[i], 70, True)
    rvq = ref.vq_old.ResidualVQ(num_quantizers=3, dropout=False, dim=D, codebook_size=K, kmeans_init=False,
                                decay=decay, ema_num_threshold=0.0, ema_num_initial=init).train()
    for i in range(3):
        e = torch.from_numpy(synth.normalish(820 + i, K * D) * np.float32(0.3)).view(K, D)
        rvq.layers[i]._codebook.embed.copy_(e)
        rvq.layers[i]._codebook.ema_embed.copy_(e * init)
    train_trace("legacy_train", rvq, lambda m, i: m.layers[i]._codebook, 75, False)

    out["meta_json"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "vs_reference.npz"), **out)
    print("vs_reference:", {k: v.shape for k, v in out.items()})


def onnx_files_golden():
    """The reference's shipped streaming-driver files (`onnx/`), rebuildable byte for byte from a few KB: every ONNX
    codebook file is a small frame around its `embed` table (and, in the `vq` graphs, the same table transposed).  The
    frame is stored with the offsets of the tables taken out; hil_speech's tables are realistic.npz's `codebooks`,
    hil_music's first and last are stored here.  sha256 of every original file is kept to prove the rebuild exact."""
    import hashlib
    from hilcodec_amd import wire
    onnx_dir = os.path.join(R.REFERENCE_ROOT, "onnx")
    out = {}
    for f in ("hil_speech_cache_enc.npz", "hil_speech_cache_dec.npz", "hil_speech_quantized.npy"):
        with open(os.path.join(onnx_dir, f), "rb") as fh:
            out["file:" + f] = np.frombuffer(fh.read(), dtype=np.uint8)
    for name, n in (("hil_speech", 8), ("hil_music", 12)):
        for i in (0, n - 1):
            for kind in ("deq", "vq"):
                fname = f"{name}_{kind}{i}.onnx"
                with open(os.path.join(onnx_dir, fname), "rb") as fh:
                    raw = fh.read()
                e = wire.read_onnx_codebook(os.path.join(onnx_dir, fname)).numpy()
                frame, spans, pos = b"", [], 0
                for table, code in ((e, 0), (np.ascontiguousarray(e.T), 1)):
                    at = raw.find(table.tobytes(), pos)
                    if at < 0:
                        continue
                    frame += raw[pos:at]
                    spans.append((len(frame), code))
                    pos = at + table.nbytes
                frame += raw[pos:]
                out["frame:" + fname] = np.frombuffer(frame, dtype=np.uint8)
                out["spans:" + fname] = np.array(spans, dtype=np.int64)
                out["sha256:" + fname] = np.array(hashlib.sha256(raw).hexdigest())
                if name == "hil_music" and kind == "deq":
                    out[f"codebook:{name}:{i}"] = e
    np.savez_compressed(os.path.join(OUT, "reference_files.npz"), **out)
    print("reference_files:", sorted(out))


if __name__ == "__main__":
    if "--trained" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        trained_codebook_golden(R.load_reference())
    elif "--realistic" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        realistic_golden(R.load_reference())
    elif "--shard" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        shard_golden(R.load_reference())
    elif "--ws" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        ref_ = R.load_reference()
        for fname_, scale_ in WS_GOLDENS:
            ws_golden(ref_, fname_, scale_)
    elif "--rvq-train" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        rvq_train_golden(R.load_reference())
    elif "--vs-reference" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        vs_reference_golden(R.load_reference())
    elif "--reference-files" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        onnx_files_golden()
    else:
        main()
