#!/usr/bin/env python
"""What report-driven rate control costs the graphed sender: same-box alternating A/B at 1 024 streams (hil_speech, n = 8, frames = 1),
timed with device events around `--hops` replays per leg and alternation (tools/hop_ab.py).
   (s) GraphedEncodeHop, sessions, header=True                          — the sender graph of the parent commit
   (R) the same + rate=RateConfig(2.625, 9.0), no report ever            — two more launches, hilc_rate_ceiling and hilc_rate_charge
   (r) the same + rate, a report for 1/16 of the slots every hop        — and the report row in the hop's one upload
   (A) the same + rate, a report for every slot on every hop            — 1 024 blobs checked on the host per hop
The baseline leg (s) is the parent commit's graph: `rate=None` captures exactly that.  Every report carries a fresh sequence number
and no loss, and 9 kbps pays for the full packet, so every leg sends the same packets: the legs differ in launches and uploads only.
   python tools/rate_hop_ab.py [--hops 200] [--alternations 5] [--legs sRrA] > profiles/rate_hops.txt"""
import hop_ab  # first: it puts the repository root on sys.path
import torch

from hilcodec_amd import graph_step, rate, synth, wire
from hilcodec_amd.rate import RateConfig

args = hop_ab.parse_args(legs="sRrA", alternations=5)

dev = torch.device("cuda:0")
B, n = args.streams, 8
cfg = RateConfig(2.625, 9.0)
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]

LEGS = {
    "s": "(s) sender, header (parent graph)",
    "R": "(R) sender + rate, no reports",
    "r": "(r) sender + rate, B/16 reports/hop",
    "A": "(A) sender + rate, B reports/hop",
}
report_slots = {"r": [list(range(r, B, 16)) for r in range(16)], "A": [list(range(B))]}
hoppers = {leg: graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, header=True, rate=cfg if leg != "s" else None)
           for leg in args.legs}
calls = {leg: 0 for leg in args.legs}


def one(leg, i):
    h = hoppers[leg]
    if leg in "rA":
        c = calls[leg]                               # the call counter runs on across runs: a slot's sequence numbers keep rising
        slots = report_slots[leg][c % len(report_slots[leg])]
        h.step(chunks[i % 8], reports=(slots, [wire.pack_report((c // len(report_slots[leg]) + 1) & 255, 0, 0)] * len(slots)))
        calls[leg] += 1
    else:
        h.step(chunks[i % 8])


def run(leg, hops):
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# rate_hop_ab: {B} streams, hil_speech, frames 1, n {n}, header, {cfg}, {args.hops} hops per leg x {args.alternations} "
      f"alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, LEGS.get, 38)
hop_ab.report(res, "# median over alternations; (R), (r) and (A) against (s)", LEGS.get, 38, base={"R": "s", "r": "s", "A": "s"}.get)
for leg in args.legs:
    if leg != "s":
        h = hoppers[leg]
        st = h.rate_state[:, rate.RC_REPORTS:].sum(0).tolist()
        print(f"{LEGS[leg]:38s} " + ", ".join(f"{name} {v}" for name, v in zip(rate.RC_NAMES, st)) +
              f"; n_ceil {int(h.n_ceil.min())}..{int(h.n_ceil.max())}, {float(rate.kbps(h.rate_state, 1).min()):.3f} kbps at least", flush=True)
