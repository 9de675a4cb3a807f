#!/usr/bin/env python
"""What DTX and comfort noise cost the graphed sender and receiver: same-box alternating A/B at 1 024 streams (hil_speech, n = 8,
frames = 1, K = 8), timed with device events around `--hops` replays per leg and alternation.  Every hop here has sessions=True.
   (s) GraphedEncodeHop, dtx=None                        — the sender graph of the parent commit
   (t) GraphedEncodeHop, dtx=DtxConfig(), every stream active (loud input: every hop is SPEECH)
   (u) GraphedEncodeHop, dtx=DtxConfig(), every stream silent (digital silence: SID / SILENT hops after the hangover)
   (a) GraphedDecodeHop, cng_order=None                  — the receiver graph of the parent commit
   (b) cng_order=8, no CN slot
   (c) cng_order=8, 128 CN slots per hop (SID rows)
   (d) cng_order=8, all 1 024 slots CN (SID rows)
   (h) cng_order=None, the 128 slots of (c) held      — what the parent graph does with those slots (a held slot's caches are copied
   (i) cng_order=None, all 1 024 slots held             back, as a CN slot's are): the baseline of (c) / (d)
   python tools/dtx_hop_ab.py [--hops 200] [--alternations 5] [--legs stuabcdhi] > profiles/dtx_hops.txt
The receivers' packets are host tensors (one upload of control rows and packets per hop, as from a socket).
The two kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/dtx_hop_ab.py --hops 50 --alternations 1 --legs tud"""
import hop_ab  # first: it puts the repository root on sys.path
import torch

from hilcodec_amd import dtx, graph_step, synth, wire

args = hop_ab.parse_args(legs="stuabcdhi", alternations=5)

dev = torch.device("cuda:0")
B, n, K = args.streams, 8, 8
cfg = dtx.DtxConfig(order=K)
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
loud = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]
quiet = [torch.zeros_like(c) for c in loud]
gen = torch.Generator().manual_seed(9)
packets = [torch.randint(0, 256, (B, wire.packet_bytes(n, 1)), generator=gen, dtype=torch.uint8) for _ in range(8)]
sid_rows = []
for p in packets:
    s = p.clone()
    s[:, 0] = torch.randint(40, 90, (B,), generator=gen, dtype=torch.uint8)
    s[:, 1:1 + K] = torch.randint(-60, 60, (B, K), generator=gen).to(torch.int8).view(torch.uint8)
    sid_rows.append(s)
n_list = [n] * B

LEGS = {  # leg: (side, dtx on, input / CN slots, name)
    "s": ("enc", False, "loud", "(s) sender, dtx=None (parent graph)"),
    "t": ("enc", True, "loud", "(t) sender, DTX, all active"),
    "u": ("enc", True, "quiet", "(u) sender, DTX, all silent"),
    "a": ("dec", False, 0, "(a) receiver, cng_order=None (parent graph)"),
    "b": ("dec", True, 0, "(b) receiver, cng_order=8, no CN slot"),
    "c": ("dec", True, 128, "(c) receiver, cng_order=8, 128 CN / hop"),
    "d": ("dec", True, B, f"(d) receiver, cng_order=8, {B} CN / hop"),
    "h": ("dec", False, 128, "(h) receiver, cng_order=None, 128 held / hop"),
    "i": ("dec", False, B, f"(i) receiver, cng_order=None, {B} held / hop"),
}


def make(leg):
    side, on, _, _ = LEGS[leg]
    if side == "enc":
        return graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, dtx=cfg if on else None)
    return graph_step.GraphedDecodeHop(model, B, 1, n, dev, sessions=True, cng_order=K if on else None)


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    side, on, what, _ = LEGS[leg]
    if side == "enc":
        hoppers[leg].step((loud if what == "loud" else quiet)[i % 8])
        return
    if what and not on:
        hoppers[leg].step(packets[i % 8], n_list, hold=list(range(what)))
    elif what:
        hoppers[leg].step(sid_rows[i % 8], n_list, sid=list(range(what)))
    else:
        hoppers[leg].step(packets[i % 8], n_list)


def run(leg, hops):
    for i in range(12):                # warm (past the hangover for the silent sender)
        one(leg, i)
    return hop_ab.timed(hops, lambda i: one(leg, i))


print(f"# dtx_hop_ab: {B} streams, hil_speech, frames 1, n {n}, K {K}, {cfg}, sessions=True, packets on the host, {args.hops} hops "
      f"per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][3], 44)
if "u" in hoppers:
    kinds = hoppers["u"].kind.cpu()
    print(f"# (u) kinds after the run: {[(k, int((kinds == k).sum())) for k in (dtx.SPEECH, dtx.SID, dtx.SILENT)]}")


def bases(leg):
    """the same side without DTX / CN traffic, then the same side's parent graph"""
    if LEGS[leg][0] == "enc":
        return "s"
    return {"c": "h", "d": "i"}.get(leg, "a") + "a"


hop_ab.report(res, "# median over alternations; difference against the same side without DTX / CN",
              lambda leg: LEGS[leg][3], 44, base=bases)
