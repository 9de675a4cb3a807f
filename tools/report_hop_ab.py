#!/usr/bin/env python
"""What receiver reports and loss-adaptive FEC cost the graphed sender and receiver: same-box alternating A/B at 1 024 streams
(hil_speech, n = 8, frames = 1, m = 2), timed with device events around `--hops` replays per leg and alternation (tools/hop_ab.py).
   (s) GraphedEncodeHop, sessions, fec_stages=2, header=True           — the sender graph of the parent commit
   (S) the same + fec_adapt=FecAdaptConfig(), no report ever            — one more launch, hilc_fec_adapt; the same packets as (s)
   (R) the same + fec_adapt, a report for 1/16 of the slots every hop  — and the report row in the hop's one upload (loss 20/256: on)
   (a) GraphedDecodeHop, sessions, conceal, fec_stages=2, cng_order=8, jitter=JitterConfig(2, 8), play() of in-order traffic
   (A) the same + report=ReportConfig()                                 — one more launch, hilc_rx_report
   (b) / (B) the same pair on 5 % loss, reordering up to D hops, 1 % duplicates
The baseline legs (s), (a), (b) are the parent commit's graphs: `fec_adapt=None` / `report=None` capture exactly those.  A traffic
trace of `--hops` hops is generated once per mix; every receiver leg replays it from a start of all slots.
   python tools/report_hop_ab.py [--hops 200] [--alternations 7] [--legs sSRaAbB] > profiles/report_hops.txt"""
import time

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, report, synth, wire
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.report import FecAdaptConfig, ReportConfig

args = hop_ab.parse_args(legs="sSRaAbB", alternations=7)

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
cfg = JitterConfig(depth=2, capacity=8)
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]
tb = wire.transport_bytes(n, m, T)


def trace(mix, hops, seed=5):
    """[(slots, packets uint8 [A, tb], nbytes)] of `hops` hops of one traffic mix"""
    rng = np.random.default_rng(seed)
    flight, out = [], []
    plain, wide = wire.packet_bytes(n, T), wire.fec_packet_bytes(n, m, T)
    for k in range(hops):
        for b in range(B):
            fec = k > 0
            body = rng.integers(0, 256, wide if fec else plain)
            if mix == "b" and rng.random() < 0.05:
                continue
            row = np.zeros(tb, dtype=np.uint8)
            row[:3], row[3:3 + len(body)] = [k >> 8, k & 0xFF, (0x40 if fec else 0) | n], body
            for _ in range(2 if mix == "b" and rng.random() < 0.01 else 1):
                flight.append((k + (int(rng.integers(0, cfg.depth + 1)) if mix == "b" else 0), b, row, 3 + len(body)))
        now = [f for f in flight if f[0] <= k]
        flight = [f for f in flight if f[0] > k]
        if mix == "b":
            now = [now[i] for i in rng.permutation(len(now))]
        packets = np.stack([f[2] for f in now]) if now else np.zeros((0, tb), dtype=np.uint8)
        out.append(([f[1] for f in now], torch.from_numpy(packets), [f[3] for f in now]))
    return out


LEGS = {  # leg: (kind, mix, name)
    "s": ("enc", None, "(s) sender, FEC + header (parent graph)"),
    "S": ("enc", None, "(S) sender + fec_adapt, no reports"),
    "R": ("enc", None, "(R) sender + fec_adapt, B/16 reports/hop"),
    "a": ("dec", "a", "(a) in-order, play() (parent graph)"),
    "A": ("dec", "a", "(A) in-order, play() + report"),
    "b": ("dec", "b", "(b) 5 % loss + reorder + dup, play()"),
    "B": ("dec", "b", "(B) 5 % loss + reorder + dup, + report"),
}
t0 = time.time()
traces = {mix: trace(mix, args.hops) for mix in sorted({LEGS[leg][1] for leg in args.legs if LEGS[leg][1]})}
print(f"# traces generated in {time.time() - t0:.0f} s", flush=True)
report_slots = [list(range(r, B, 16)) for r in range(16)]


def make(leg):
    kind = LEGS[leg][0]
    if kind == "enc":
        return graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, fec_stages=m, header=True,
                                           fec_adapt=FecAdaptConfig() if leg in "SR" else None)
    return graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=cfg,
                                       report=ReportConfig() if leg in "AB" else None)


hoppers = {leg: make(leg) for leg in args.legs}
calls = {leg: 0 for leg in args.legs}


def one(leg, i):
    kind, mix, _ = LEGS[leg]
    h = hoppers[leg]
    if kind == "dec":
        h.play(*traces[mix][i])
    elif leg == "R":
        slots = report_slots[calls[leg] % 16]       # the call counter runs on across runs: every slot's seq goes up by one each time
        h.step(chunks[i % 8], reports=(slots, [wire.pack_report(calls[leg] // 16 & 255, 20, 0)] * len(slots)))
        calls[leg] += 1
    else:
        h.step(chunks[i % 8])


def run(leg, hops):
    if LEGS[leg][0] == "dec":
        for b in range(B):               # every leg replays its trace from fresh slots
            hoppers[leg].start(b)
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# report_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, {cfg}, {ReportConfig()}, {FecAdaptConfig()}, host "
      f"packets, {args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][2], 42)
hop_ab.report(res, "# median over alternations; (S) and (R) against (s), (A) against (a), (B) against (b)", lambda leg: LEGS[leg][2], 42,
              base={"S": "s", "R": "s", "A": "a", "B": "b"}.get)
for leg in args.legs:
    h = hoppers[leg]
    if leg in "SR":
        st = h.fec_adapt_state
        print(f"{LEGS[leg][2]:42s} fec_on {int(h.fec_on.sum())} of {B}, reports accepted {int(st[:, report.FA_REPORTS].sum())}, "
              f"stale {int(st[:, report.FA_STALE].sum())}", flush=True)
    if leg in "AB":
        st = h.report_state.float()
        print(f"{LEGS[leg][2]:42s} reports emitted {int(st[:, report.RP_REPORTS].sum())}, mean loss_q8 "
              f"{float(st[:, report.RP_LOSS].mean()):.1f}, mean residual_q8 {float(st[:, report.RP_RESIDUAL].mean()):.1f}", flush=True)
