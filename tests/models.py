"""Whole-model helpers shared by test modules (no tests here): the offline model from the synthetic weights, its comparison with
reference outputs at the project's bars, the realistic weights, and one run of bench.py."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from hilcodec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def build(name, seed=7):
    """-> (the offline model with the seeded synthetic weights, its keyword arguments, the state dict)"""
    import hilcodec_amd
    mk = synth.model_kwargs(name)
    sd = synth.synth_state_dict(name, seed=seed)
    model = hilcodec_amd.HILCodec(24000, 1, **mk).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("_extra_state") for k in missing)
    for l in model.quantizer.layers:
        l.initted = True
    return model, mk, sd


def compare(model, mk, sd, x, z_ref, idx_ref, wav_ref, n=None, fixture=False):
    """`fixture`: the expected values are a committed golden from the real reference — every fp64 gap of those frames is
    data, no flip has ever been measured on them, so none is allowed (a regression that flips one index must not pass)."""
    from oracle import hilcodec_oracle as O
    dev = torch.device("cuda:0")
    with torch.no_grad():
        z = model.encoder(x.to(dev))
        q, nr, loss, idx = model.quantizer(z, n, return_indices=True)
        wav = model.decoder(q)
    dz = (z.cpu() - z_ref).abs().max().item()
    assert dz < 1e-5, f"encoder output differs by {dz:.3e}"        # measured 3 - 6e-6 (profiles/r05_parity_census_final.json): a 2 x drift fails
    same = idx.cpu() == idx_ref
    flips = 0
    if not same.all():
        gaps = O.rvq_gaps_fp64(sd, z_ref, idx_ref)
        for b, t in {(b, t) for b, s, t in (~same).nonzero().tolist()}:
            s0 = int((~same[b, :, t]).nonzero()[0])
            assert gaps[b, s0, t] < 1e-4, f"genuine index mismatch b={b} s={s0} t={t} gap={gaps[b, s0, t]:.3e}"
            flips += 1
    assert flips <= (0 if fixture else 1), f"{flips} near-tie flips"
    # decoder parity on the SAME codes as the reference: feed the reference indices' q
    cb = model.quantizer.spec(dev).codebooks
    from hilcodec_amd import ops
    q_ref = ops.rvq_decode(idx_ref.to(dev), cb, idx_ref.shape[1], channel_last=False, stage_major=False)
    with torch.no_grad():
        wav2 = model.decoder(q_ref)
    dw = (wav2.cpu() - wav_ref).abs().max().item()
    assert dw < 1e-4, f"decoded waveform differs by {dw:.3e}"
    if flips == 0:
        assert (wav.cpu() - wav_ref).abs().max().item() < 1e-4
    return dz, dw, flips


def realistic_state_dict(g):
    """seeded synthetic conv weights + the reference's SHIPPED trained codebooks (tests/golden/realistic.npz)"""
    sd = synth.synth_state_dict("hil_speech", seed=int(g["weight_seed"]))
    for i in range(8):
        sd[f"quantizer.layers.{i}.embed"] = T(g["codebooks"][i]).clone()
    return sd


def run_bench(*args, launcher=()):
    out = subprocess.run([sys.executable, *launcher, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # exactly one JSON line
    return json.loads(lines[0])
