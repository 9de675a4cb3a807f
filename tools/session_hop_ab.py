#!/usr/bin/env python
"""What per-stream sessions cost a graphed hop: same-box alternating A/B at 1 024 streams (hil_speech, hop 320, n = 8), timed
with device events around `--hops` replays per leg and alternation.
   (a) GraphedHop(sessions=False)                       — the graph of earlier rounds
   (b) GraphedHop(sessions=True), no actions            — one idle hilc_state_slots_apply per chain
   (c) GraphedHop(sessions=True), per hop 8 fresh starts, 2 resumes (host caches: the pinned upload) and 8 bitrate changes
   python tools/session_hop_ab.py [--hops 200] [--alternations 3] [--legs abc] [--groups 1] > profiles/sessions_hop_ab.txt
The slot kernel's own time comes from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/session_hop_ab.py --hops 50 --alternations 1 --legs bc"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hilcodec_amd import graph_step, synth
from hilcodec_amd.models.hilcodec.streaming import HILCodec as StreamingHILCodec

ap = argparse.ArgumentParser()
ap.add_argument("--hops", type=int, default=200)
ap.add_argument("--alternations", type=int, default=3)
ap.add_argument("--legs", default="abc")
ap.add_argument("--groups", type=int, default=1)
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("session_hop_ab.py needs a GPU")

dev = torch.device("cuda:0")
B = args.streams
mk = synth.model_kwargs("hil_speech")
smk = {k: v for k, v in mk.items() if k not in ("spec_learnable", "causal", "pad_mode")}
model = StreamingHILCodec(24000, **smk).eval()
model.load_offline_state_dict(synth.synth_state_dict("hil_speech", 7))
model.remove_weight_reparameterizations()
xs = [synth.synth_clips(B, 320, seed=4321 + 7 * j).to(dev) for j in range(8)]
rng = np.random.default_rng(5)

hoppers = {}
for leg in args.legs:
    hoppers[leg] = graph_step.GraphedHop(model, B, 320, 8, dev, groups=args.groups, sessions=leg in "bc")
if "c" in hoppers:                     # two resumable streams, held on the host as a server would after wire.load_cache_npz
    h = hoppers["c"]
    for i in range(4):
        h.step(xs[i % 8])
    saved = [tuple([c.cpu() for c in part] for part in h.export(s)) for s in (3, 5)]


def actions(h):
    slots = rng.permutation(B)[:18].tolist()
    for s in slots[:8]:
        h.start(s)
    for s, (enc, dec) in zip(slots[8:10], saved):
        h.start(s, enc, dec)
    for s in slots[10:18]:
        h.set_bitrate(s, int(rng.choice([1, 2, 4, 8])))


def run(leg, hops):
    h = hoppers[leg]
    for i in range(5):                 # warm
        if leg == "c":
            actions(h)
        h.step(xs[i % 8])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(hops):
        if leg == "c":
            actions(h)
        h.step(xs[i % 8])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / hops


names = {"a": "(a) sessions=False", "b": "(b) sessions=True, idle", "c": "(c) sessions=True, 8 starts + 2 resumes + 8 bitrates / hop"}
res = {leg: [] for leg in args.legs}
print(f"# session_hop_ab: {B} streams, hil_speech, hop 320, n 8, groups {args.groups}, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
for a in range(args.alternations):
    order = args.legs if a % 2 == 0 else args.legs[::-1]
    for leg in order:
        ms = run(leg, args.hops)
        res[leg].append(ms)
        print(f"alt {a} {names[leg]:62s} {ms:.4f} ms/hop", flush=True)
print("# median over alternations")
base = statistics.median(res["a"]) if "a" in res else None
for leg in args.legs:
    m = statistics.median(res[leg])
    rel = f"  {100.0 * (m - base) / base:+.2f} % vs (a) ({1e3 * (m - base):+.1f} us)" if base is not None and leg != "a" else ""
    print(f"{names[leg]:62s} {m:.4f} ms/hop  (min {min(res[leg]):.4f}, max {max(res[leg]):.4f}){rel}", flush=True)
