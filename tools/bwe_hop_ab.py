#!/usr/bin/env python
"""What the delay-based bandwidth estimate costs the graphed hops: same-box alternating legs at 1 024 slots (hil_speech, n = 8, frames =
1), timed with device events around `--hops` calls per leg and alternation (tools/hop_ab.py).
   (r) GraphedDecodeHop(sessions, conceal, jitter, report, nack).play    — the receiver graph of the parent commit, one arrival per slot
   (R) the same + bwe=BweConfig(2.625, 9.0), a tick per arrival          — one more launch, hilc_rx_bwe, and 1 024 more words uploaded
   (s) GraphedEncodeHop(sessions, header, rate).step                     — the sender graph of the parent commit
   (C) the same + cap=CapConfig(), no cap ever                           — one more launch, hilc_rate_cap, one more row
   (c) the same + cap, a cap for every slot on every hop                 — and 1 024 blobs checked on the host per hop
The base legs (r) and (s) are the parent commit's graphs: `bwe=None` / `cap=None` capture exactly those.  Every packet arrives one hop
after the last and every cap is the full rate, so the legs of a side send, play and emit the same: they differ in launches and uploads.
   python tools/bwe_hop_ab.py [--hops 200] [--alternations 9] [--legs rRsCc] > profiles/bwe_hops.txt
   python tools/bwe_hop_ab.py --loop > profiles/bwe_loop.txt
`--loop` needs no GPU: the closed loop of tests/bwe_loop.py on the host models (hilcodec_amd/bwe.py, rate.py, report.py, jitter.py) at
bottlenecks of 60, 80 and 200 bits per hop and over a 200 -> 60 -> 200 step, with and without the estimate: the figures that
tests/test_bwe_cpu.py holds conditions on."""
import sys

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import bwe, graph_step, rate, synth, wire
from hilcodec_amd.bwe import BweConfig, CapConfig
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.rate import RateConfig
from hilcodec_amd.report import ReportConfig
from hilcodec_amd.rtx import NackConfig


def loop():
    from tests.bwe_loop import LOOP_BWE, LOOP_CAP, run_models
    from tests.rate_loop import LOOP_JITTER, LOOP_RATE, LOOP_REPORT
    print(f"# bwe_hop_ab --loop: host models only, 3 000 hops, figures over hops [1000, 3000); {LOOP_RATE}, {LOOP_BWE}, {LOOP_CAP}, "
          f"{LOOP_REPORT}, {LOOP_JITTER}; a drop-tail queue of 4 hops, reports and caps 4 hops under way")
    print("# bottleneck (bits per hop)      estimate  loss    delay ms: mean  p95    bits sent: mean  / bottleneck   decreases: rate rule  estimate")
    for caps in (60, 80, 200, [(0, 200), (1000, 60), (2000, 200)]):
        for est in (False, True):
            o = run_models(caps, estimate=est)
            lo, hi = 1000, 3000
            name = str(caps) if isinstance(caps, int) else "200 -> 60 at 1000 -> 200 at 2000"
            mean_cap = caps if isinstance(caps, int) else 130
            bits = o.trace.mean_bits(lo, hi)
            print(f"{name:32s} {'with' if est else 'without':8s}  {o.trace.loss(lo, hi):.4f}  {o.mean_delay_ms(lo, hi):14.1f}  "
                  f"{o.p95_delay_ms(lo, hi):5.1f}  {bits:15.1f}  {bits / mean_cap:12.3f}  {int(o.rm.state[0, rate.RC_DECREASED]):20d}  "
                  f"{int(o.bm.state[0, bwe.BW_DECREASED]):8d}")
    print("# (the step's bottleneck column divides by the mean of the three stretches, 130)")


if "--loop" in sys.argv:
    loop()
    sys.exit(0)

args = hop_ab.parse_args(legs="rRsCc", alternations=9)

dev = torch.device("cuda:0")
B, n, T = args.streams, 8, 1
bcfg, ccfg, rcfg = BweConfig(2.625, 9.0), CapConfig(), RateConfig(2.625, 9.0)
model = synth.streaming_model()
tb = wire.transport_bytes(n, 0, T)
slots = list(range(B))
rows = np.random.default_rng(5).integers(0, 256, (B, tb), dtype=np.uint8)
rows[:, 2] = n
packets, nbytes = torch.from_numpy(rows), [tb] * B
spread = np.arange(B, dtype=np.int64) % 7                  # the arrivals of a hop a few ticks apart
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]

LEGS = {"r": "(r) receiver, jitter + report + nack", "R": "(R) receiver + bwe, a tick per arrival", "s": "(s) sender, header + rate",
        "C": "(C) sender + cap, no caps", "c": "(c) sender + cap, B caps/hop"}
W = 40


def make(leg):
    if leg in "rR":
        return graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, jitter=JitterConfig(2, 8), max_arrivals=B,
                                           report=ReportConfig(), nack=NackConfig(), bwe=bcfg if leg == "R" else None)
    return graph_step.GraphedEncodeHop(model, B, 320 * T, n, dev, sessions=True, header=True, rate=rcfg, cap=ccfg if leg in "Cc" else None)


hoppers = {leg: make(leg) for leg in args.legs}
calls = {leg: 0 for leg in args.legs}


def one(leg, i):
    h, c = hoppers[leg], calls[leg]                  # the call counter runs on across runs: hop indices and sequence numbers keep rising
    calls[leg] += 1
    if leg in "rR":
        rows[:, 0], rows[:, 1] = (c >> 8) & 0xFF, c & 0xFF
        if leg == "R":
            h.play(slots, packets, nbytes, times=spread + 320 * T * c)
        else:
            h.play(slots, packets, nbytes)
    elif leg == "c":
        h.step(chunks[i % 8], caps=(slots, [wire.pack_cap((c + 1) & 255, 120)] * B))
    else:
        h.step(chunks[i % 8])


def run(leg, hops):
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# bwe_hop_ab: {B} slots, hil_speech, frames {T}, n {n}, {bcfg}, {ccfg}, {rcfg}; host packets, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], W)
hop_ab.report(res, "# median over alternations; (R) against (r); (C), (c) against (s)", lambda leg: LEGS[leg], W,
              base={"R": "r", "C": "s", "c": "sC"}.get)
for leg in args.legs:
    h = hoppers[leg]
    if leg == "R":
        st = h.bwe_state[:, bwe.BW_SAMPLES:bwe.BW_TREND].sum(0).tolist()
        print(f"{LEGS[leg]:{W}s} " + ", ".join(f"{name} {v}" for name, v in zip(bwe.BW_NAMES, st)) +
              f"; estimate {float(bwe.kbps(h.bwe_state, T).min()):.3f} kbps at least", flush=True)
    elif leg in "Cc":
        st = h.cap_state[:, bwe.CP_CAPS:].sum(0).tolist()
        print(f"{LEGS[leg]:{W}s} " + ", ".join(f"{name} {v}" for name, v in zip(bwe.CP_NAMES, st)) +
              f"; n_ceil {int(h.n_ceil.min())}..{int(h.n_ceil.max())}", flush=True)
