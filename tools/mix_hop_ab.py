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
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire
from hilcodec_amd.mixer import MixConfig
from hilcodec_amd.models.hilcodec.streaming import HILCodec as StreamingHILCodec

ap = argparse.ArgumentParser()
ap.add_argument("--hops", type=int, default=200)
ap.add_argument("--alternations", type=int, default=7)
ap.add_argument("--legs", default="pabc")
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mix_hop_ab.py needs a GPU")

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
mk = synth.model_kwargs("hil_speech")
smk = {k: v for k, v in mk.items() if k not in ("spec_learnable", "causal", "pad_mode")}
model = StreamingHILCodec(24000, **smk).eval()
model.load_offline_state_dict(synth.synth_state_dict("hil_speech", 7))
model.remove_weight_reparameterizations()
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(hops):
        h.step(packets[i % 8], n_list)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / hops


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
res = {leg: [] for leg in args.legs}
print(f"# mix_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, host packets, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
for a in range(args.alternations):
    order = args.legs if a % 2 == 0 else args.legs[::-1]
    for leg in order:
        ms = run(leg, args.hops)
        res[leg].append(ms)
        print(f"alt {a} {LEGS[leg][0]:36s} {ms:.4f} ms/hop", flush=True)
print("# median over alternations; each mixer leg against (p) of the same run")
for leg in args.legs:
    med = statistics.median(res[leg])
    rel = ""
    if leg != "p" and "p" in res:
        b = statistics.median(res["p"])
        rel = f"  {1e3 * (med - b):+.1f} us ({100.0 * (med - b) / b:+.2f} %) vs (p)"
    print(f"{LEGS[leg][0]:36s} {med:.4f} ms/hop  (min {min(res[leg]):.4f}, max {max(res[leg]):.4f}){rel}", flush=True)
if mixer is not None:
    sp = int(mixer.speakers.sum())
    print(f"# after the last mixer leg: {sp} speakers, {int(mixer.mixed.any(dim=2).sum())} non-zero mixes", flush=True)
