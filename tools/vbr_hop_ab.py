#!/usr/bin/env python
"""What variable bitrate costs the graphed sender: same-box alternating A/B at 1 024 streams (hil_speech, n = 8, frames = 1), timed with
device events around `--hops` replays per leg and alternation.  Every hop here has sessions=True.
   (s) GraphedEncodeHop, vbr=None                                   — the sender graph of the parent commit
   (v) GraphedEncodeHop, vbr=VbrConfig(target_db)                   — one more launch, hilc_vbr_select, no cap
   (w) GraphedEncodeHop, vbr=VbrConfig(target_db, cap_kbps=4.5)     — the same launch with the token bucket
   python tools/vbr_hop_ab.py [--hops 200] [--alternations 5] [--legs svw] > profiles/vbr_hops.txt
The synthetic model's plain randn codebooks never let the rule fire, so the quantiser and the dequantiser get falling per-stage
codebooks randn g 0.95^s (g = 0.05 of the latents' norm) and target_db is the median of D[:, n / 2] / D[:, 0] over the first hop: about
half the slots stop at or before stage 4.  (The decision changes what the packer writes, not how long any launch takes: the kernel
measures every stage of every slot whatever it then decides.)
The kernel's own time comes from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/vbr_hop_ab.py --hops 50 --alternations 1 --legs vw"""
import math

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, vbr

args = hop_ab.parse_args(legs="svw", alternations=5)

dev = torch.device("cuda:0")
B, n = args.streams, 8
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]

with torch.no_grad():
    caches = model.initialize_cache(chunks[0])[0]
    z, _ = model.encoder(chunks[0], *caches)
    g = 0.05 * float(z.float().norm(dim=-1).median())
    gen = torch.Generator().manual_seed(11)
    for s, (ql, dl) in enumerate(zip(model.quantizer.layers, model.dequantizer.layers)):
        e = torch.randn(1024, 128, generator=gen) * g * 0.95 ** s
        ql.embed.copy_(e)
        dl.embed.copy_(e)
    idx = model.quantizer(z, n)
D = vbr.distortions(z.cpu(), idx.cpu(), model.quantizer._tables(dev).codebooks.cpu())
target_db = -10.0 * math.log10(float(np.median(D[:, n // 2] / D[:, 0])))

LEGS = {  # leg: (config, name)
    "s": (None, "(s) sender, vbr=None (parent graph)"),
    "v": (vbr.VbrConfig(target_db), "(v) sender, VBR, no cap"),
    "w": (vbr.VbrConfig(target_db, cap_kbps=4.5), "(w) sender, VBR, cap 4.5 kbit/s"),
}
hoppers = {leg: graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, vbr=LEGS[leg][0]) for leg in args.legs}


def run(leg, hops):
    h = hoppers[leg]
    for i in range(12):
        h.step(chunks[i % 8])
    return hop_ab.timed(hops, lambda i: h.step(chunks[i % 8]))


print(f"# vbr_hop_ab: {B} streams, hil_speech, frames 1, n {n}, target_db {target_db:.3f}, sessions=True, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][1], 40)
for leg in args.legs:
    if leg != "s":
        n_eff = hoppers[leg].n_eff.cpu()
        nbytes = hoppers[leg].outs[hoppers[leg].parity ^ 1][2].cpu()
        print(f"# {LEGS[leg][1]}: n_eff after the run: {np.bincount(n_eff.numpy(), minlength=n + 1).tolist()} slots at 0..{n} stages, "
              f"{float(nbytes.float().mean()):.2f} bytes per packet")
hop_ab.report(res, "# median over alternations; difference against the sender without VBR", lambda leg: LEGS[leg][1], 40,
              base=lambda leg: "s")
