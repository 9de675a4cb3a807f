#!/usr/bin/env python
"""What in-band FEC costs the graphed sender and receiver: same-box alternating A/B at 1 024 streams (hil_speech, n = 8,
frames = 1, m = 2), timed with device events around `--hops` replays per leg and alternation.  Every hop here has sessions=True;
the receivers also have conceal=True (the receiver FEC pairs with: what FEC cannot recover is concealed).
   (s) GraphedEncodeHop, fec_stages=0                    — the sender graph of the parent commit
   (t) GraphedEncodeHop, fec_stages=2
   (a) GraphedDecodeHop, fec_stages=0, nothing lost      — the receiver graph of the parent commit
   (b) fec_stages=2, nothing lost (every row carries a redundant section)
   (c) fec_stages=2, 16 FEC slots per hop (a new seeded random set every hop)
   (d) fec_stages=2, 128 FEC slots per hop
   (z) a second fec_stages=0 receiver, nothing lost: a control — two instances of the same graph differ by where their buffers
       landed, and (z) - (a) shows how much of a difference that alone makes
   python tools/fec_hop_ab.py [--hops 200] [--alternations 5] [--legs stabcdz] [--host-packets] > profiles/fec_hops.txt
`--host-packets`: the receivers' packets are host tensors (one upload copy of control rows and packets per hop, as from a
socket) instead of device tensors (a control-row upload plus a device copy of the packets).
The two kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/fec_hop_ab.py --hops 50 --alternations 1 --legs tbd"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth, wire

def options(ap):
    ap.add_argument("--fec-stages", type=int, default=2)
    ap.add_argument("--host-packets", action="store_true")


args = hop_ab.parse_args(legs="stabcdz", alternations=5, add=options)

dev = torch.device("cuda:0")
B, m, n = args.streams, args.fec_stages, 8
model = synth.streaming_model()
gen = torch.Generator(device=dev).manual_seed(9)
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]
packets = {w: [torch.randint(0, 256, (B, wire.packet_bytes(n + w, 1)), device=dev, generator=gen, dtype=torch.uint8)
               for _ in range(8)] for w in (0, m)}
if args.host_packets:
    packets = {w: [p.cpu() for p in rows] for w, rows in packets.items()}
n_list = [n] * B
rng = np.random.default_rng(5)

LEGS = {  # leg: (side, fec_stages, FEC slots per hop, name)
    "s": ("enc", 0, 0, "(s) sender, fec_stages=0 (parent graph)"),
    "t": ("enc", m, 0, f"(t) sender, fec_stages={m}"),
    "a": ("dec", 0, 0, "(a) receiver, fec_stages=0 (parent graph)"),
    "b": ("dec", m, 0, f"(b) receiver, fec_stages={m}, no FEC slot"),
    "c": ("dec", m, 16, f"(c) receiver, fec_stages={m}, 16 FEC / hop"),
    "d": ("dec", m, 128, f"(d) receiver, fec_stages={m}, 128 FEC / hop"),
    "z": ("dec", 0, 0, "(z) receiver, fec_stages=0, control instance"),
}


def make(leg):
    side, stages, _, _ = LEGS[leg]
    if side == "enc":
        return graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, fec_stages=stages)
    return graph_step.GraphedDecodeHop(model, B, 1, n, dev, sessions=True, conceal=True, fec_stages=stages)


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    side, stages, nfec, _ = LEGS[leg]
    if side == "enc":
        hoppers[leg].step(chunks[i % 8])
        return
    fec = rng.permutation(B)[:nfec].tolist() if nfec else None
    hoppers[leg].step(packets[stages][i % 8], n_list, fec=fec)


def run(leg, hops):
    for i in range(5):                 # warm
        one(leg, i)
    return hop_ab.timed(hops, lambda i: one(leg, i))


print(f"# fec_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, sessions=True (receivers: conceal=True), packets on the "
      f"{'host' if args.host_packets else 'device'}, {args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][3], 44)
hop_ab.report(res, "# median over alternations; difference against the same side with fec_stages=0",
              lambda leg: LEGS[leg][3], 44, base=lambda leg: "s" if LEGS[leg][0] == "enc" else "a")
