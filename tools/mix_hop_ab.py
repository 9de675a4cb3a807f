#!/usr/bin/env python
"""What the room mixer costs the graphed receiver: same-box alternating A/B at 1 024 streams (hil_speech, n = 8, frames = 1), timed
with device events around `--hops` replays per leg and alternation.  Receivers: sessions=True, conceal=True, fec_stages=2, cng_order=8,
step() with packets on the host (random codes, every slot decoded on every hop).
   (p) GraphedDecodeHop, mix=None                         — the receiver graph of the parent commit
   (a) mix=MixConfig(3), every slot in no room             — the level kernel, and the room kernel's zero rows
   (b) mix=MixConfig(3), 128 rooms of 8
   (c) mix=MixConfig(3), one room of 1 024
The three mixer legs share one receiver; its membership is set before each leg's run (one upload of the room row on the first hop).
   python tools/mix_hop_ab.py [--hops 200] [--alternations 7] [--legs pabc] > profiles/mix_hops.txt
The two kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/mix_hop_ab.py --hops 50 --alternations 1 --legs bc"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire
from hilcodec_amd.mixer import MixConfig

args = hop_ab.parse_args(legs="pabc", alternations=7)

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
model = synth.streaming_model()
rng = np.random.default_rng(5)
stride = wire.packet_bytes(n + m, T)
packets = [torch.from_numpy(rng.integers(0, 256, (B, stride)).astype(np.uint8)) for _ in range(8)]
n_list = [n] * B

LEGS = {  # leg: (name, room of slot b or None for the receiver without the mixer)
    "p": ("(p) mix=None (parent graph)", None),
    "a": ("(a) MixConfig(3), no rooms", lambda b: -1),
    "b": ("(b) MixConfig(3), 128 rooms of 8", lambda b: b // 8 if B >= 8 else 0),
    "c": ("(c) MixConfig(3), one room of all", lambda b: 0),
}
kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K)
plain = graph_step.GraphedDecodeHop(model, B, T, n, dev, **kw) if "p" in args.legs else None
mixer = graph_step.GraphedDecodeHop(model, B, T, n, dev, mix=MixConfig(3), **kw) if set(args.legs) - {"p"} else None


def run(leg, hops):
    rooms = LEGS[leg][1]
    h = plain if rooms is None else mixer
    if rooms is not None:
        for b in range(B):
            r = rooms(b)
            h.leave(b) if r < 0 else h.join(b, r)
    return hop_ab.timed(hops, lambda i: h.step(packets[i % 8], n_list))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# mix_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, host packets, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][0], 36)
hop_ab.report(res, "# median over alternations; each mixer leg against (p) of the same run", lambda leg: LEGS[leg][0], 36,
              base=lambda leg: "p")
if mixer is not None:
    sp = int(mixer.speakers.sum())
    print(f"# after the last mixer leg: {sp} speakers, {int(mixer.mixed.any(dim=2).sum())} non-zero mixes", flush=True)
