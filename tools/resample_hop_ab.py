#!/usr/bin/env python
"""What the sample-rate converter costs the graphed sender and receiver: same-box alternating A/B at 1 024 streams (hil_speech,
n = 8), timed with device events around `--hops` replays per leg and alternation.  No sessions (the converter adds one launch either
way).  Legs come in pairs with the same frames per hop, each against the 24 kHz graph of the parent commit:
   sender  F = 1: (a) 24 kHz          (b) 48 kHz input    (c) 44.1 kHz input
   sender  F = 3: (d) 24 kHz          (e) 16 kHz input
   receiver F = 1: (f) 24 kHz         (g) 48 kHz output
   receiver F = 3: (h) 24 kHz         (i) 16 kHz output
and one offline line: `hilcodec_amd.resample` of 256 clips x 1 s at 48 -> 24 kHz.
   python tools/resample_hop_ab.py [--hops 200] [--alternations 5] [--legs abcdefghi] > profiles/resample_hops.txt
The kernel's own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/resample_hop_ab.py --hops 50 --alternations 1"""
import statistics

import hop_ab  # first: it puts the repository root on sys.path
import torch

import hilcodec_amd
from hilcodec_amd import graph_step, ops, synth
from hilcodec_amd.resample import hop_samples

args = hop_ab.parse_args(legs="abcdefghi", alternations=5, add=lambda ap: ap.add_argument("--offline-reps", type=int, default=20))

dev = torch.device("cuda:0")
B = args.streams
model = synth.streaming_model()

LEGS = {  # leg: (side, frames, rate, baseline leg, name)
    "a": ("enc", 1, 24000, None, "(a) sender F=1, 24 kHz (parent graph)"),
    "b": ("enc", 1, 48000, "a", "(b) sender F=1, 48 kHz input"),
    "c": ("enc", 1, 44100, "a", "(c) sender F=1, 44.1 kHz input"),
    "d": ("enc", 3, 24000, None, "(d) sender F=3, 24 kHz (parent graph)"),
    "e": ("enc", 3, 16000, "d", "(e) sender F=3, 16 kHz input"),
    "f": ("dec", 1, 24000, None, "(f) receiver F=1, 24 kHz (parent graph)"),
    "g": ("dec", 1, 48000, "f", "(g) receiver F=1, 48 kHz output"),
    "h": ("dec", 3, 24000, None, "(h) receiver F=3, 24 kHz (parent graph)"),
    "i": ("dec", 3, 16000, "h", "(i) receiver F=3, 16 kHz output"),
}
gen = torch.Generator(device=dev).manual_seed(9)
inputs, hoppers = {}, {}
for leg in args.legs:
    side, frames, rate, _, _ = LEGS[leg]
    if side == "enc":
        hoppers[leg] = graph_step.GraphedEncodeHop(model, B, 320 * frames, 8, dev, input_rate=rate)
        n = hop_samples(frames, rate)
        inputs[leg] = [(torch.rand(B, 1, n, device=dev, generator=gen) * 2 - 1,) for _ in range(4)]
    else:
        hoppers[leg] = graph_step.GraphedDecodeHop(model, B, frames, 8, dev, output_rate=rate)
        idx = [torch.randint(0, 1024, (8, B, frames), device=dev, generator=gen) for _ in range(4)]
        inputs[leg] = [(ops.pack_codes_10bit(i)[0], [8] * B) for i in idx]


def run(leg, hops):
    h, ins = hoppers[leg], inputs[leg]
    for i in range(5):                 # warm
        h.step(*ins[i % 4])
    return hop_ab.timed(hops, lambda i: h.step(*ins[i % 4]))


print(f"# resample_hop_ab: {B} streams, hil_speech, n 8, sessions=False, {args.hops} hops per leg x {args.alternations} alternations; "
      f"{torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][4], 42)
hop_ab.report(res, "# median over alternations; difference against the 24 kHz graph with the same frames per hop",
              lambda leg: LEGS[leg][4], 42, base=lambda leg: LEGS[leg][3])

# offline: 256 clips x 1 s at 48 kHz -> 24 kHz, one launch per call
x = torch.rand(256, 1, 48000, device=dev, generator=gen) * 2 - 1
for _ in range(3):
    hilcodec_amd.resample(x, 48000, 24000)
times = []
for _ in range(args.offline_reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hilcodec_amd.resample(x, 48000, 24000)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
m = statistics.median(times)
print(f"offline resample 256 x 1 s, 48 -> 24 kHz: median {m:.4f} ms per call (min {min(times):.4f}, max {max(times):.4f}, "
      f"{args.offline_reps} calls) = {256.0 / (m * 1e-3):.0f} s of audio per s", flush=True)
