#!/usr/bin/env python
"""What NACK and retransmission cost the graphed sender and receiver: same-box alternating A/B at 1 024 streams (hil_speech, n = 8,
frames = 1, m = 2), timed with device events around `--hops` replays per leg and alternation (tools/hop_ab.py).
   (s) GraphedEncodeHop, sessions, fec_stages=2, header=True           — the sender graph of the parent commit
   (S) the same + rtx=RtxConfig(), no NACK ever                         — one more launch, hilc_rtx_step; the same packets as (s)
   (n) the same + rtx, a NACK for 1/16 of the slots every hop          — and the two NACK rows in the hop's one upload
   (N) the same + rtx, a NACK for every slot on every hop              — 1 024 blobs checked on the host per hop, two retransmissions each
   (b) GraphedDecodeHop, sessions, conceal, fec_stages=2, cng_order=8, jitter=JitterConfig(4, 8), play() of 5 % loss, reordering up
       to 2 hops, 1 % duplicates
   (B) the same + nack=NackConfig()                                     — one more launch, hilc_nack_build
The baseline legs (s) and (b) are the parent commit's graphs: `rtx=None` / `nack=None` capture exactly those.  A NACK asks for the
slot's previous two hops, which are in the history.  The traffic trace of `--hops` hops is generated once; every receiver leg replays
it from a start of all slots (nothing is retransmitted into it: the cost of a retransmission at the receiver is an arrival's).
   python tools/rtx_hop_ab.py [--hops 200] [--alternations 5] [--legs sSnNbB] > profiles/rtx_hops.txt"""
import time

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, jitter, rtx, synth, wire
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.rtx import NackConfig, RtxConfig

args = hop_ab.parse_args(legs="sSnNbB", alternations=5)

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
cfg = JitterConfig(depth=4, capacity=8)
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]
tb = wire.transport_bytes(n, m, T)


def trace(hops, seed=5):
    """[(slots, packets uint8 [A, tb], nbytes)] of `hops` hops: 5 % loss, a delay of 0..2 hops, 1 % duplicates"""
    rng = np.random.default_rng(seed)
    flight, out = [], []
    plain, wide = wire.packet_bytes(n, T), wire.fec_packet_bytes(n, m, T)
    for k in range(hops):
        for b in range(B):
            fec = k > 0
            body = rng.integers(0, 256, wide if fec else plain)
            if rng.random() < 0.05:
                continue
            row = np.zeros(tb, dtype=np.uint8)
            row[:3], row[3:3 + len(body)] = [k >> 8, k & 0xFF, (0x40 if fec else 0) | n], body
            for _ in range(2 if rng.random() < 0.01 else 1):
                flight.append((k + int(rng.integers(0, 3)), b, row, 3 + len(body)))
        now = [f for f in flight if f[0] <= k]
        flight = [f for f in flight if f[0] > k]
        now = [now[i] for i in rng.permutation(len(now))]
        packets = np.stack([f[2] for f in now]) if now else np.zeros((0, tb), dtype=np.uint8)
        out.append(([f[1] for f in now], torch.from_numpy(packets), [f[3] for f in now]))
    return out


LEGS = {  # leg: (kind, name)
    "s": ("enc", "(s) sender, FEC + header (parent graph)"),
    "S": ("enc", "(S) sender + rtx, no NACKs"),
    "n": ("enc", "(n) sender + rtx, B/16 NACKs/hop"),
    "N": ("enc", "(N) sender + rtx, B NACKs/hop"),
    "b": ("dec", "(b) 5 % loss + reorder + dup, play()"),
    "B": ("dec", "(B) 5 % loss + reorder + dup, + nack"),
}
t0 = time.time()
lossy = trace(args.hops) if any(LEGS[leg][0] == "dec" for leg in args.legs) else None
print(f"# trace generated in {time.time() - t0:.0f} s", flush=True)
nack_slots = {"n": [list(range(r, B, 16)) for r in range(16)], "N": [list(range(B))]}


def make(leg):
    if LEGS[leg][0] == "enc":
        return graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, fec_stages=m, header=True,
                                           rtx=RtxConfig() if leg in "SnN" else None)
    return graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, fec_stages=m, cng_order=K, jitter=cfg,
                                       max_arrivals=4 * B, nack=NackConfig() if leg == "B" else None)


hoppers = {leg: make(leg) for leg in args.legs}
calls = {leg: 0 for leg in args.legs}


def one(leg, i):
    kind, _ = LEGS[leg]
    h = hoppers[leg]
    if kind == "dec":
        h.play(*lossy[i])
    elif leg in "nN":
        c = calls[leg]                               # the call counter runs on across runs, as every slot's hop counter does
        slots = nack_slots[leg][c % len(nack_slots[leg])]
        h.step(chunks[i % 8], nacks=(slots, [wire.pack_nack((c - 2) & 0xFFFF, 1)] * len(slots)))
        calls[leg] += 1
    else:
        h.step(chunks[i % 8])


def run(leg, hops):
    if LEGS[leg][0] == "dec":
        for b in range(B):               # every leg replays the trace from fresh slots
            hoppers[leg].start(b)
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# rtx_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, {cfg}, {NackConfig()}, {RtxConfig()}, host packets, "
      f"{args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][1], 42)
hop_ab.report(res, "# median over alternations; (S), (n) and (N) against (s), (B) against (b)", lambda leg: LEGS[leg][1], 42,
              base={"S": "s", "n": "s", "N": "s", "B": "b"}.get)
for leg in args.legs:
    h = hoppers[leg]
    if leg in "SnN":
        st = h.rtx_state.sum(0).tolist()
        print(f"{LEGS[leg][1]:42s} " + ", ".join(f"{name} {v}" for name, v in zip(rtx.RX_NAMES, st)), flush=True)
    if leg == "B":
        st = h.nack_state[:, :rtx.NK_RING].sum(0).tolist()
        print(f"{LEGS[leg][1]:42s} " + ", ".join(f"{name} {v}" for name, v in zip(rtx.NK_NAMES, st)) +
              f"; lost {int(h.jitter_state[:, jitter.STAT_LOST].sum())}, repaired {int(h.jitter_state[:, jitter.STAT_FEC].sum())} (nothing is retransmitted here)", flush=True)
