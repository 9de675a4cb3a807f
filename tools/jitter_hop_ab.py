#!/usr/bin/env python
"""What the transport header and the jitter buffer cost the graphed sender and receiver: same-box alternating A/B at 1 024 streams
(hil_speech, n = 8, frames = 1), timed with device events around `--hops` replays per leg and alternation.  Senders: sessions=True,
fec_stages=2.  Receivers: sessions=True, conceal=True, fec_stages=2, cng_order=8, packets on the host.
   (s) GraphedEncodeHop, header=False                     — the sender graph of the parent commit
   (t) GraphedEncodeHop, header=True
   (a) / (A) in-order traffic:  step() fed jitter.JitterModel's decisions (the parent graph) / play() of the arrivals
   (b) / (B) 5 % loss, reordering up to D hops, 1 % duplicates
   (c) / (C) DTX-heavy: per slot 10 speech hops, then SIDs every 8 hops and silence in between, 32-hop cycle
   (X) (Y) (Z) the play() of (A) (B) (C) on a receiver with an adaptive playout clock, JitterConfig(..., adapt=AdaptConfig())
A traffic trace of `--hops` hops is generated once per mix (JitterConfig(depth=2, capacity=8)); every leg replays it from a start
of all slots.  Also printed: the per-hop upload bytes and the host time of a play() / step() call.
   python tools/jitter_hop_ab.py [--hops 200] [--alternations 7] [--legs stabcABC] > profiles/jitter_hops.txt
   python tools/jitter_hop_ab.py --legs ABCXYZ > profiles/jitter_adapt_hops.txt
The two kernels' own times come from a separate kernel-trace run of this script (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/jitter_hop_ab.py --hops 50 --alternations 1 --legs tB"""
import statistics
import time

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import dtx, graph_step, synth, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel

args = hop_ab.parse_args(legs="stabcABC", alternations=7)

dev = torch.device("cuda:0")
B, n, m, K, T = args.streams, 8, 2, 8, 1
cfg = JitterConfig(depth=2, capacity=8)
cfg_adapt = JitterConfig(depth=2, capacity=8, adapt=AdaptConfig())
model = synth.streaming_model()
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]
tb = wire.transport_bytes(n, m, T)


def trace(mix, hops, seed=5):
    """[(slots, packets uint8 [A, tb], nbytes, model rows)] of `hops` hops of one traffic mix, from a start of every slot"""
    rng = np.random.default_rng(seed)
    jm = JitterModel(B, cfg, n, m, T, K, True)
    flight, out = [], []
    plain, wide = wire.packet_bytes(n, T), wire.fec_packet_bytes(n, m, T)
    for k in range(hops):
        for b in range(B):
            phase = (k + b) % 32
            if mix == "c" and phase >= 10:
                if (phase - 10) % 8:
                    continue                                    # silent: nothing sent
                body, hdr = rng.integers(0, 256, dtx.sid_bytes(K)), [k >> 8, k & 0xFF, 0x80]
            else:
                fec = k > 0
                body = rng.integers(0, 256, wide if fec else plain)
                hdr = [k >> 8, k & 0xFF, (0x40 if fec else 0) | n]
            if mix == "b" and rng.random() < 0.05:
                continue
            row = np.zeros(tb, dtype=np.uint8)
            row[:3], row[3:3 + len(body)] = hdr, body
            for _ in range(2 if mix == "b" and rng.random() < 0.01 else 1):
                flight.append((k + (int(rng.integers(0, cfg.depth + 1)) if mix == "b" else 0), b, row, 3 + len(body)))
        now = [f for f in flight if f[0] <= k]
        flight = [f for f in flight if f[0] > k]
        if mix == "b":
            now = [now[i] for i in rng.permutation(len(now))]
        slots = [f[1] for f in now]
        packets = np.stack([f[2] for f in now]) if now else np.zeros((0, tb), dtype=np.uint8)
        nbytes = [f[3] for f in now]
        rows = jm.step(np.full(B, int(k == 0)), np.zeros(B, dtype=np.int32), slots, packets, nbytes)
        hv = rows["hold"]
        kw = dict(hold=np.nonzero(hv == 1)[0].tolist(), lost=np.nonzero(rows["lost"])[0].tolist(),
                  fec=np.nonzero(rows["fec"])[0].tolist(), sid=np.nonzero(hv == 2)[0].tolist(), silent=np.nonzero(hv == 3)[0].tolist())
        out.append((slots, torch.from_numpy(packets), nbytes, torch.from_numpy(rows["packets"]), rows["n"].tolist(), kw))
    return out


LEGS = {  # leg: (kind, mix, name)
    "s": ("enc", None, "(s) sender, header=False (parent graph)"),
    "t": ("enc", None, "(t) sender, header=True"),
    "a": ("step", "a", "(a) in-order, step() (parent graph)"),
    "A": ("play", "a", "(A) in-order, play()"),
    "b": ("step", "b", "(b) 5 % loss + reorder + dup, step()"),
    "B": ("play", "b", "(B) 5 % loss + reorder + dup, play()"),
    "c": ("step", "c", "(c) DTX-heavy, step()"),
    "C": ("play", "c", "(C) DTX-heavy, play()"),
    "X": ("adapt", "a", "(X) in-order, adaptive play()"),
    "Y": ("adapt", "b", "(Y) 5 % loss + reorder + dup, adaptive"),
    "Z": ("adapt", "c", "(Z) DTX-heavy, adaptive play()"),
}
t0 = time.time()
traces = {mix: trace(mix, args.hops) for mix in sorted({LEGS[leg][1] for leg in args.legs if LEGS[leg][1]})}
print(f"# traces generated in {time.time() - t0:.0f} s", flush=True)


def make(leg):
    kind, _, _ = LEGS[leg]
    if kind == "enc":
        return graph_step.GraphedEncodeHop(model, B, 320, n, dev, sessions=True, fec_stages=m, header=leg == "t")
    return graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, fec_stages=m, cng_order=K,
                                       jitter={"play": cfg, "adapt": cfg_adapt}.get(kind))


hoppers = {leg: make(leg) for leg in args.legs}
host_s = {leg: [] for leg in args.legs}
sent = {leg: [] for leg in args.legs}      # bytes of each call's pinned copy (ControlStage.sent_words)


def one(leg, i):
    kind, mix, _ = LEGS[leg]
    h = hoppers[leg]
    if kind == "enc":
        h.step(chunks[i % 8])
        return
    slots, packets, nbytes, rows, n_list, kw = traces[mix][i]
    c0 = time.perf_counter()
    if kind in ("play", "adapt"):
        h.play(slots, packets, nbytes)
    else:
        h.step(rows, n_list, **kw)
    host_s[leg].append(time.perf_counter() - c0)
    sent[leg].append(4 * h.stage.sent_words)


def run(leg, hops):
    if LEGS[leg][0] != "enc":
        for b in range(B):               # every leg replays its trace from fresh slots (the trace starts with a start of all)
            hoppers[leg].start(b)
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
    host_s[leg].clear()
    sent[leg].clear()
print(f"# jitter_hop_ab: {B} streams, hil_speech, frames 1, n {n}, m {m}, K {K}, {cfg}, host packets, {args.hops} hops per leg x "
      f"{args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg][2], 40)
hop_ab.report(res, "# median over alternations; (t) against (s), each play() leg against the step() leg of its mix, each adaptive leg "
              "against the play() leg of its mix", lambda leg: LEGS[leg][2], 40,
              base={"t": "s", "A": "a", "B": "b", "C": "c", "X": "A", "Y": "B", "Z": "C"}.get)
print("# per-hop upload (bytes, one pinned copy) and host time of a call (median, us; includes waiting for the previous upload)")
for leg in args.legs:
    kind, mix, name = LEGS[leg]
    if kind == "enc":
        continue
    sizes = sent[leg]
    print(f"{name:40s} upload median {int(statistics.median(sizes))} B (min {min(sizes)}, max {max(sizes)}), host "
          f"{1e6 * statistics.median(host_s[leg]):.1f} us/call", flush=True)
