#!/usr/bin/env python
"""What a conference hop costs with selective forwarding, beside the decode-mix-encode bridge: same-box alternating legs at 1 024
slots in rooms of 8 (hil_speech, n = 8, frames = 1, m = 2, fanout 3), one headed FEC packet per slot and hop from the host, timed
with device events around `--hops` calls per leg and alternation (tools/hop_ab.py).
   (f) GraphedForwardHop.forward, every listener at 8 layers            — one upload, two launches; nothing is cut
   (F) the same after set_layers(slot, 4) on every slot                 — every packet is cut to 4 stages, the redundant section moves up
   (b) the bridge of today, for context: GraphedDecodeHop(jitter=, mix=MixConfig(3)).play of the same packets, then
       GraphedEncodeHop(fec_stages=2, header=True).step of the mixes     — a full decode and a full encode per slot and hop
Every slot sends on every hop (no DTX), so every listener's three routes carry a packet: 3 072 forwarded packets per hop.  The trace
of `--hops` hops is generated once; the bridge's receiver replays it from a start of all slots.
   python tools/forward_hop_ab.py [--hops 200] [--alternations 5] [--legs fFb] > profiles/forward_hops.txt"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import forward, graph_step, synth, wire
from hilcodec_amd.forward import ForwardConfig
from hilcodec_amd.jitter import JitterConfig
from hilcodec_amd.mixer import MixConfig

args = hop_ab.parse_args(legs="fFb", alternations=5, add=lambda ap: ap.add_argument("--room", type=int, default=8))

dev = torch.device("cuda:0")
B, n, m, T, ROOM = args.streams, 8, 2, 1, args.room
cfg, jcfg = ForwardConfig(fanout=3), JitterConfig(depth=2, capacity=8)
tb = wire.transport_bytes(n, m, T)
slots = list(range(B))


def trace(hops, seed=5):
    """[(packets uint8 [B, tb], nbytes)] of `hops` hops: slot b's packet of hop k, random codes, a redundant section from hop 1 on"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(hops):
        length = tb if k else wire.TRANSPORT_HEADER + wire.packet_bytes(n, T)
        rows = rng.integers(0, 256, (B, tb), dtype=np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2] = k >> 8, k & 0xFF, (wire.FEC_BIT if k else 0) | n
        rows[:, length:] = 0
        out.append((torch.from_numpy(rows), [length] * B))
    return out


LEGS = {"f": "(f) forward, 8 layers (untrimmed)", "F": "(F) forward, 4 layers (all trimmed)", "b": "(b) bridge: decode + mix + encode"}
sent = trace(args.hops)


def make(leg):
    if leg in "fF":
        h = graph_step.GraphedForwardHop(B, T, n, dev, fec_stages=m, cfg=cfg, max_arrivals=B)
        for b in range(B):
            h.join(b, b // ROOM)
            if leg == "F":
                h.set_layers(b, 4)
        return h
    model = synth.streaming_model()
    rx = graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, fec_stages=m, jitter=jcfg, max_arrivals=B,
                                     mix=MixConfig(cfg.fanout))
    for b in range(B):
        rx.join(b, b // ROOM)
    return rx, graph_step.GraphedEncodeHop(model, B, 320 * T, n, dev, sessions=True, fec_stages=m, header=True)


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    packets, nbytes = sent[i]
    if leg in "fF":
        hoppers[leg].forward(slots, packets, nbytes)
    else:
        rx, tx = hoppers[leg]
        rx.play(slots, packets, nbytes)
        tx.step(rx.mixed)


def run(leg, hops):
    if leg == "b":
        for b in range(B):               # the receiver replays the trace from fresh slots
            hoppers[leg][0].start(b)
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# forward_hop_ab: {B} slots in rooms of {ROOM}, hil_speech, frames 1, n {n}, m {m}, {cfg}, bridge: {jcfg}, MixConfig({cfg.fanout}); "
      f"host packets, {args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], 38)
hop_ab.report(res, "# median over alternations; (F) against (f), both beside (b)", lambda leg: LEGS[leg], 38, base={"F": "f", "f": "b"}.get,
              tail=lambda leg, med: f"  = {100.0 * med / np.median(res['b']):.1f} % of (b)" if leg in "fF" and "b" in res else "")
for leg in args.legs:
    if leg in "fF":
        h = hoppers[leg]
        st, sd = h.listener_state.sum(0).tolist(), h.sender_state[:, forward.SD_CODES:].sum(0).tolist()
        print(f"{LEGS[leg]:38s} " + ", ".join(f"{name} {v}" for name, v in zip(forward.LR_NAMES, st)) + "; senders: " +
              ", ".join(f"{name} {v}" for name, v in zip(forward.SD_NAMES[forward.SD_CODES:], sd)), flush=True)
