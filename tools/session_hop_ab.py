#!/usr/bin/env python
"""What per-stream sessions cost a graphed hop: same-box alternating A/B at 1 024 streams (hil_speech, hop 320, n = 8), timed
with device events around `--hops` replays per leg and alternation.
   (a) GraphedHop(sessions=False)                       — the graph of earlier rounds
   (b) GraphedHop(sessions=True), no actions            — one idle hilc_state_slots_apply per chain
   (c) GraphedHop(sessions=True), per hop 8 fresh starts, 2 resumes (host caches: the pinned upload) and 8 bitrate changes
   python tools/session_hop_ab.py [--hops 200] [--alternations 3] [--legs abc] [--groups 1] > profiles/sessions_hop_ab.txt
The slot kernel's own time comes from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/session_hop_ab.py --hops 50 --alternations 1 --legs bc"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth

args = hop_ab.parse_args(legs="abc", add=lambda ap: ap.add_argument("--groups", type=int, default=1))

dev = torch.device("cuda:0")
B = args.streams
model = synth.streaming_model()
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


def one(leg, i):
    h = hoppers[leg]
    if leg == "c":
        actions(h)
    h.step(xs[i % 8])


def run(leg, hops):
    for i in range(5):                 # warm
        one(leg, i)
    return hop_ab.timed(hops, lambda i: one(leg, i))


names = {"a": "(a) sessions=False", "b": "(b) sessions=True, idle", "c": "(c) sessions=True, 8 starts + 2 resumes + 8 bitrates / hop"}
print(f"# session_hop_ab: {B} streams, hil_speech, hop 320, n 8, groups {args.groups}, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, names.get, 62)
hop_ab.report(res, "# median over alternations", names.get, 62, base=lambda leg: "a")
