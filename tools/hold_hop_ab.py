#!/usr/bin/env python
"""What held streams cost a graphed hop: same-box alternating A/B at 1 024 streams (hil_speech, hop 320, n = 8), timed with
device events around `--hops` replays per leg and alternation.  Every hop graph here has sessions=True.
   (a) loopback GraphedHop without the tail kernel      — the graph of the parent commit (hilc_state_slots_hold left out of
                                                          the capture)
   (b) loopback, tail kernel, nothing held
   (c) loopback, 16 held streams per hop (a new seeded random set every hop)
   (d) loopback, 128 held streams per hop
   (e) sender GraphedEncodeHop without the tail kernel  (f) sender, nothing held     (g) sender, 128 held per hop
   (h) receiver GraphedDecodeHop without the tail kernel (i) receiver, nothing held  (j) receiver, 128 held per hop
   python tools/hold_hop_ab.py [--hops 200] [--alternations 3] [--legs abcdefghij] > profiles/hold_hops.txt
The tail kernel's own time comes from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/hold_hop_ab.py --hops 50 --alternations 1 --legs bd"""
import contextlib

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire

args = hop_ab.parse_args(legs="abcdefghij")

dev = torch.device("cuda:0")
B = args.streams
model = synth.streaming_model()
xs = [synth.synth_clips(B, 320, seed=4321 + 7 * j).to(dev) for j in range(8)]
stride = wire.packet_bytes(8, 1)
gen = torch.Generator(device=dev).manual_seed(9)
packets = [torch.randint(0, 256, (B, stride), device=dev, generator=gen, dtype=torch.uint8) for _ in range(8)]
n_list = [8] * B
rng = np.random.default_rng(5)

LEGS = {  # leg: (kind, tail kernel captured, held streams per hop, name)
    "a": ("loop", False, 0, "(a) loopback, no tail kernel (parent graph)"),
    "b": ("loop", True, 0, "(b) loopback, tail, idle"),
    "c": ("loop", True, 16, "(c) loopback, tail, 16 held / hop"),
    "d": ("loop", True, 128, "(d) loopback, tail, 128 held / hop"),
    "e": ("send", False, 0, "(e) sender, no tail kernel (parent graph)"),
    "f": ("send", True, 0, "(f) sender, tail, idle"),
    "g": ("send", True, 128, "(g) sender, tail, 128 held / hop"),
    "h": ("recv", False, 0, "(h) receiver, no tail kernel (parent graph)"),
    "i": ("recv", True, 0, "(i) receiver, tail, idle"),
    "j": ("recv", True, 128, "(j) receiver, tail, 128 held / hop"),
}
BASE = {"loop": "a", "send": "e", "recv": "h"}


@contextlib.contextmanager
def no_tail():
    """capture without hilc_state_slots_hold: the sessions graph of the parent commit"""
    real = graph_step.ops.state_slots_hold
    graph_step.ops.state_slots_hold = lambda *a, **k: None
    try:
        yield
    finally:
        graph_step.ops.state_slots_hold = real


def make(leg):
    kind, tail, _, _ = LEGS[leg]
    with (contextlib.nullcontext() if tail else no_tail()):
        if kind == "loop":
            return graph_step.GraphedHop(model, B, 320, 8, dev, sessions=True)
        if kind == "send":
            return graph_step.GraphedEncodeHop(model, B, 320, 8, dev, sessions=True)
        return graph_step.GraphedDecodeHop(model, B, 1, 8, dev, sessions=True)


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    kind, _, nheld, _ = LEGS[leg]
    h = hoppers[leg]
    held = rng.permutation(B)[:nheld].tolist() if nheld else None
    if kind == "recv":
        h.step(packets[i % 8], n_list, hold=held)
    else:
        h.step(xs[i % 8], hold=held)


def run(leg, hops):
    for i in range(5):                 # warm
        one(leg, i)
    return hop_ab.timed(hops, lambda i: one(leg, i))


print(f"# hold_hop_ab: {B} streams, hil_speech, hop 320, n 8, sessions=True, {args.hops} hops per leg x {args.alternations} "
      f"alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][3], 48)
hop_ab.report(res, "# median over alternations; difference against the same side's graph without the tail kernel",
              lambda leg: LEGS[leg][3], 48, base=lambda leg: BASE[LEGS[leg][0]])
