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
import argparse
import contextlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire
from hilcodec_amd.models.hilcodec.streaming import HILCodec as StreamingHILCodec

ap = argparse.ArgumentParser()
ap.add_argument("--hops", type=int, default=200)
ap.add_argument("--alternations", type=int, default=3)
ap.add_argument("--legs", default="abcdefghij")
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("hold_hop_ab.py needs a GPU")

dev = torch.device("cuda:0")
B = args.streams
mk = synth.model_kwargs("hil_speech")
smk = {k: v for k, v in mk.items() if k not in ("spec_learnable", "causal", "pad_mode")}
model = StreamingHILCodec(24000, **smk).eval()
model.load_offline_state_dict(synth.synth_state_dict("hil_speech", 7))
model.remove_weight_reparameterizations()
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(hops):
        one(leg, i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / hops


res = {leg: [] for leg in args.legs}
print(f"# hold_hop_ab: {B} streams, hil_speech, hop 320, n 8, sessions=True, {args.hops} hops per leg x {args.alternations} "
      f"alternations; {torch.cuda.get_device_name(dev)}", flush=True)
for a in range(args.alternations):
    order = args.legs if a % 2 == 0 else args.legs[::-1]
    for leg in order:
        ms = run(leg, args.hops)
        res[leg].append(ms)
        print(f"alt {a} {LEGS[leg][3]:48s} {ms:.4f} ms/hop", flush=True)
print("# median over alternations; difference against the same side's graph without the tail kernel")
for leg in args.legs:
    m = statistics.median(res[leg])
    base = BASE[LEGS[leg][0]]
    rel = ""
    if base in res and leg != base:
        b = statistics.median(res[base])
        rel = f"  {1e3 * (m - b):+.1f} us ({100.0 * (m - b) / b:+.2f} %) vs {LEGS[base][3][:3]}"
    print(f"{LEGS[leg][3]:48s} {m:.4f} ms/hop  (min {min(res[leg]):.4f}, max {max(res[leg]):.4f}){rel}", flush=True)
