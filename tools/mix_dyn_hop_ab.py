#!/usr/bin/env python
"""What per-speaker levelling and the limiter cost the room mixer of the graphed receiver: same-box alternating A/B at 1 024 streams
(hil_speech, n = 8, frames = 1), timed with device events around `--hops` replays per leg and alternation.  Receivers as in
tools/mix_hop_ab.py: sessions=True, conceal=True, fec_stages=2, cng_order=8, step() with packets on the host (random codes, every slot
decoded on every hop).  Four receivers, each at 128 rooms of 8 (b) and at one room of all (c):
   (p)  mix=MixConfig(3)                                       — the mixer graph of the parent commit: mix_levels, mix_rooms
   (v)  MixConfig(3, level=LevelConfig())                      — + mix_gains, mix_rooms_dyn with levelled terms in place of mix_rooms
   (m)  MixConfig(3, limit=LimitConfig())                      — mix_rooms_dyn with the limiter in place of mix_rooms
   (d)  MixConfig(3, level=LevelConfig(), limit=LimitConfig()) — both
A leg is a receiver letter and a layout, e.g. "pb"; every leg is reported against the (p) leg of its layout in the same run.
   python tools/mix_dyn_hop_ab.py [--hops 200] [--alternations 7] [--legs pb,vb,mb,db,pc,vc,mc,dc] > profiles/mix_dyn_hops.txt
The kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/mix_dyn_hop_ab.py --hops 50 --alternations 1"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire
from hilcodec_amd.mixer import LevelConfig, LimitConfig, MixConfig

ALL = "pb,vb,mb,db,pc,vc,mc,dc"
args = hop_ab.parse_args(legs=ALL, alternations=7)
legs = [leg for leg in args.legs.split(",") if leg]

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
model = synth.streaming_model()
rng = np.random.default_rng(5)
stride = wire.packet_bytes(n + m, T)
packets = [torch.from_numpy(rng.integers(0, 256, (B, stride)).astype(np.uint8)) for _ in range(8)]
n_list = [n] * B

CONFIGS = {  # receiver letter: (name, its MixConfig)
    "p": ("MixConfig(3) (parent graph)", MixConfig(3)),
    "v": ("+ level", MixConfig(3, level=LevelConfig())),
    "m": ("+ limit", MixConfig(3, limit=LimitConfig())),
    "d": ("+ level + limit", MixConfig(3, level=LevelConfig(), limit=LimitConfig())),
}
LAYOUTS = {  # layout letter: (name, room of slot b)
    "b": ("128 rooms of 8", lambda b: b // 8 if B >= 8 else 0),
    "c": ("one room of all", lambda b: 0),
}
kw = dict(sessions=True, conceal=True, fec_stages=m, cng_order=K)
receivers = {c: graph_step.GraphedDecodeHop(model, B, T, n, dev, mix=CONFIGS[c][1], **kw) for c in CONFIGS if any(leg[0] == c for leg in legs)}


def name(leg):
    return f"({leg}) {CONFIGS[leg[0]][0]}, {LAYOUTS[leg[1]][0]}"


def run(leg, hops):
    h, rooms = receivers[leg[0]], LAYOUTS[leg[1]][1]
    for b in range(B):
        h.join(b, rooms(b))
    return hop_ab.timed(hops, lambda i: h.step(packets[i % 8], n_list))


for leg in legs:                         # warm
    run(leg, min(5, args.hops))
print(f"# mix_dyn_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, host packets, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(legs, args, run, name, 46)
hop_ab.report(res, "# median over alternations; each leg against the (p) leg of its layout in the same run", name, 46,
              base=lambda leg: ["p" + leg[1]])
for c, h in receivers.items():
    tail = ""
    if h.mix.level is not None:
        tail += f", gains {float(h.gains[:, 1].min()):.3f} .. {float(h.gains[:, 1].max()):.3f}"
    if h.mix.limit is not None:
        tail += f", limiter gain {float(h.limiter_state[:, 1].min()):.3f} .. {float(h.limiter_state[:, 1].max()):.3f}"
    print(f"# ({c}) after its last leg: {int(h.speakers.sum())} speakers, peak |mixed| {float(h.mixed.abs().max()):.6f}{tail}", flush=True)
