#!/usr/bin/env python
"""What loss concealment costs the graphed receiver: same-box alternating A/B at 1 024 streams (hil_speech, n = 8, frames = 1),
timed with device events around `--hops` replays per leg and alternation.  Every receiver here has sessions=True.
   (a) GraphedDecodeHop(conceal=False)                   — the receiver graph of the parent commit
   (b) conceal=True, nothing lost
   (c) conceal=True, 16 lost per hop (a new seeded random set every hop)
   (d) conceal=True, 128 lost per hop
   (e) conceal=True, a burst longer than F: the same 128 slots lost for 2 F hops, then 2 F hops received, and so on (half of
       the burst hops are device-decided holds of faded-out slots)
   (f) conceal=False, 128 held per hop (step(hold=)): what a receiver without concealment does with the same losses
   python tools/conceal_hop_ab.py [--hops 200] [--alternations 3] [--legs abcdef] > profiles/conceal_hops.txt
The two kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/conceal_hop_ab.py --hops 50 --alternations 1 --legs bd"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire

args = hop_ab.parse_args(legs="abcdef", add=lambda ap: ap.add_argument("--fade-hops", type=int, default=4))

dev = torch.device("cuda:0")
B, F = args.streams, args.fade_hops
model = synth.streaming_model()
stride = wire.packet_bytes(8, 1)
gen = torch.Generator(device=dev).manual_seed(9)
packets = [torch.randint(0, 256, (B, stride), device=dev, generator=gen, dtype=torch.uint8) for _ in range(8)]
n_list = [8] * B
rng = np.random.default_rng(5)
burst = sorted(rng.permutation(B)[:128].tolist())

LEGS = {  # leg: (conceal, lost (or held, leg f) per hop, name)
    "a": (False, 0, "(a) receiver, conceal=False (parent graph)"),
    "b": (True, 0, "(b) conceal, nothing lost"),
    "c": (True, 16, "(c) conceal, 16 lost / hop"),
    "d": (True, 128, "(d) conceal, 128 lost / hop"),
    "e": (True, -1, f"(e) conceal, 128 in bursts of {2 * F} > F hops"),
    "f": (False, 128, "(f) conceal=False, 128 held / hop"),
}


def make(leg):
    conceal = LEGS[leg][0]
    return graph_step.GraphedDecodeHop(model, B, 1, 8, dev, sessions=True, conceal=conceal, fade_hops=F)


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    conceal, nlost, _ = LEGS[leg]
    if not conceal:
        held = rng.permutation(B)[:nlost].tolist() if nlost else None
        hoppers[leg].step(packets[i % 8], n_list, hold=held)
        return
    if nlost > 0:
        lost = rng.permutation(B)[:nlost].tolist()
    elif nlost < 0:
        lost = burst if (i // (2 * F)) % 2 == 0 else None
    else:
        lost = None
    hoppers[leg].step(packets[i % 8], n_list, lost=lost)


def run(leg, hops):
    for i in range(5):                 # warm
        one(leg, i)
    return hop_ab.timed(hops, lambda i: one(leg, i))


print(f"# conceal_hop_ab: {B} streams, hil_speech, frames 1, n 8, fade_hops {F}, sessions=True, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][2], 48)
hop_ab.report(res, "# median over alternations; difference against the conceal=False receiver",
              lambda leg: LEGS[leg][2], 48, base=lambda leg: "a")
