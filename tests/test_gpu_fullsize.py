"""GPU, BASELINE.json full sizes (batch = 256 x 1 s, hil_speech Nq=8 and hil_music Nq=12): the oracle cannot
run this in seconds, so parity is carried by size-independent properties —
  * the first clips of the big batch ARE the golden clips: z / indices / wav must match the real reference's
    golden vectors inside the batch of 256;
  * batch invariance: a clip's result does not depend on what else is in the batch (bit-exact);
  * shard invariance: two half batches == the full batch (what the multi-GPU layout relies on);
  * causality: changing the future of a clip leaves its past outputs bit-identical;
  * Dequantizer(indices) reproduces the quantiser's q bit for bit; index checksums are reproducible."""
import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from tests.models import build, run_bench

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.asarray(a))


def run(model, x):
    with torch.no_grad():
        z = model.encoder(x)
        q, _, loss, idx = model.quantizer(z, None, return_indices=True)
        wav = model.decoder(q)
    return z, q, idx, wav, loss


@pytest.mark.parametrize("name", ["hil_speech", "hil_music"])
def test_full_batch_properties(golden, name):
    from hilcodec_amd import ops
    dev = torch.device("cuda:0")
    g = golden(f"offline_{name}")
    model, mk, _ = build(name)
    nq = mk["vq_kwargs"]["num_quantizers"]
    B = 256
    x = synth.synth_clips(B, 24000, seed=int(g["clip_seed"])).to(dev)
    z, q, idx, wav, loss = run(model, x)
    assert z.shape == (B, 128, 75) and idx.shape == (B, nq, 75) and wav.shape == (B, 1, 24000)
    assert torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    # (1) the golden clips, embedded in the full batch
    n = g["z"].shape[0]
    assert (z[:n].cpu() - T(g["z"])).abs().max() < 1e-5
    assert torch.equal(idx[:n].cpu(), T(g["indices"]).long())
    assert (wav[:n].cpu() - T(g["wav"])).abs().max() < 1e-4
    # (2) batch invariance (bit-exact): clips 0, 100, 255 alone
    pick = [0, 100, 255]
    z1, q1, idx1, wav1, _ = run(model, x[pick].contiguous())
    assert torch.equal(z1, z[pick]) and torch.equal(idx1, idx[pick]) and torch.equal(wav1, wav[pick])
    # (3) shard invariance: two halves == whole (the multi-GPU layout)
    za, _, ia, wa, _ = run(model, x[:128].contiguous())
    zb, _, ib, wb, _ = run(model, x[128:].contiguous())
    assert torch.equal(torch.cat([ia, ib]), idx) and torch.equal(torch.cat([wa, wb]), wav)
    assert int(ia.sum()) + int(ib.sum()) == int(idx.sum())
    # (4) causality: perturb the last 0.5 s of three clips; everything before stays bit-identical
    x2 = x[pick].clone()
    x2[:, :, 12000:] = -x2[:, :, 12000:]
    z2, _, idx2, wav2, _ = run(model, x2)
    f = 12000 // 320          # frames that end before the perturbation (frame f covers samples <= 320 f)
    assert torch.equal(z2[:, :, :f], z[pick][:, :, :f]) and torch.equal(idx2[:, :, :f], idx[pick][:, :, :f])
    assert torch.equal(wav2[:, :, : 320 * f], wav[pick][:, :, : 320 * f])
    assert not torch.equal(wav2[:, :, 12320:], wav[pick][:, :, 12320:])
    # (5) Dequantizer(indices) == quantiser's q, bit for bit; partial n is a prefix of the index table
    cb = model.quantizer.spec(dev).codebooks
    dq = ops.rvq_decode(idx, cb, nq, channel_last=False, stage_major=False)
    assert torch.equal(dq, q)
    with torch.no_grad():
        _, _, _, idx4 = model.quantizer(z, 4, return_indices=True)
    assert torch.equal(idx4, idx[:, :4].contiguous())
    # (6) run-to-run determinism of the whole step
    _, _, idx_again, wav_again, loss_again = run(model, x)
    assert torch.equal(idx_again, idx) and torch.equal(wav_again, wav) and float(loss_again) == float(loss)


def test_streaming_equals_offline_encoder_on_zero_caches():
    """A single full-length streaming call on zero caches is the offline causal encoder."""
    dev = torch.device("cuda:0")
    model, mk, _ = build("hil_speech")
    sm = synth.streaming_model()
    x = synth.synth_clips(4, 9600, seed=77).to(dev)
    ce, _ = sm.initialize_cache(x)
    with torch.no_grad():
        zs, _ = sm.encoder(x, *ce)
        zo = model.encoder(x)
    assert (zs.transpose(1, 2) - zo).abs().max() < 1e-5


def test_rank7_shard_of_configs4_full_size(golden):
    """BASELINE configs[4] (hil_music, 2048 clips over 8 GPUs = 256 per rank) at its REAL per-GPU size for a rank != 0:
    rank 7's full 256-clip shard (clips 1792..2047 of the global batch — other seeds than any other golden) through the
    HIP path exactly as `bench.py` builds it; the shard's first 8 clips are pinned by the REAL reference
    (tests/golden/shard_rank7_hil_music.npz), three picks are batch-invariant bit for bit, and `bench.py --emulate-rank 7
    --emulate-world 8` at full size prints the same index checksum.  (The reference has no multi-GPU inference to compare
    with: `/root/reference/train.py:51-61` is its only NCCL setup.)"""
    import bench
    from hilcodec_amd import distributed as D
    g = golden("shard_rank7_hil_music")
    dev = torch.device("cuda:0")
    lo, hi = D.shard_range(256 * 8, 7, 8)
    assert (lo, hi) == (int(g["first"]), int(g["first"]) + int(g["shard_clips"])) == (1792, 2048)
    step, audio_s, ctx = bench.offline_workload("hil_music", hi - lo, lo, 24000, dev)
    assert audio_s == 256.0
    with torch.no_grad():
        idx, wav = step(0)
    z = ctx["last"]["z"]
    assert idx.shape == (256, 12, 75) and wav.shape == (256, 1, 24000) and torch.isfinite(wav).all()
    n = g["indices"].shape[0]
    flips = int((idx[:n].cpu() != T(g["indices"]).long()).sum())
    print(f"rank-7 shard: {n * 12 * 75} argmins against the real reference, flips = {flips}")
    assert flips == 0
    assert (z[:n, :, ::5].cpu() - T(g["z_probe"])).abs().max() < 1e-5
    assert (wav[:n, :, ::25].cpu() - T(g["wav_probe"])).abs().max() < 1e-4
    # batch invariance inside the shard, bit for bit
    model = ctx["model"]
    pick = [5, 131, 255]
    x = synth.synth_clips(256, 24000, seed=1234, first=lo)[pick].to(dev)
    z1, _, idx1, wav1, _ = run(model, x)
    assert torch.equal(z1, z[pick]) and torch.equal(idx1, idx[pick]) and torch.equal(wav1, wav[pick])
    # the bench line of the emulated rank at FULL size carries the same checksum
    d = run_bench("--emulate-rank", "7", "--emulate-world", "8", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                  "--no-clock-probe", "--no-launch-timing")
    assert d["config"]["shard"] == [1792, 2048] and d["config"]["global_batch"] == 2048
    assert "configs[4]" in d["config"]["workload"] and "hil_music" in d["config"]["workload"]
    assert d["index_checksum"] == int(idx.sum().item())


def test_batch_beyond_4gib_activations_keeps_the_fast_kernels():
    """B = 512 x 1 s: the decoder's [512, 96, 24000] activations are 4.7 GB, beyond the 32-bit byte offsets of the linear GEMM
    cores and the fused block (csrc/gemm_epilogues.h: lin_ok, csrc/resblock.hip) — the engine runs equal clip chunks instead
    of letting every launch fall back to the generic core: bit-identical to two B = 256 runs, and as fast as those."""
    import time
    from hilcodec_amd import engine
    dev = torch.device("cuda:0")
    model, mk, _ = build("hil_speech")
    x = synth.synth_clips(512, 24000, seed=4000).to(dev)
    assert len(engine._clip_chunks(512, 96 * 24000)) == 2 and len(engine._clip_chunks(256, 96 * 24000)) == 1

    def timed(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, sorted(ts)[reps // 2]

    run(model, x[:256].contiguous())                      # warm-up (folds, tables)
    (z, q, idx, wav, _), t512 = timed(lambda: run(model, x))
    halves, t256 = timed(lambda: [run(model, x[:256].contiguous()), run(model, x[256:].contiguous())])
    (za, _, ia, wa, _), (zb, _, ib, wb, _) = halves
    assert torch.equal(torch.cat([za, zb]), z) and torch.equal(torch.cat([ia, ib]), idx) and torch.equal(torch.cat([wa, wb]), wav)
    print(f"B=512: {t512 * 1e3:.1f} ms, two B=256 runs: {t256 * 1e3:.1f} ms")
    assert t512 < 1.05 * t256
