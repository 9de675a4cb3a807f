#!/usr/bin/env python
"""What SRTP packet protection costs the graphed hops: same-box alternating legs at 1 024 slots (hil_speech, n = 8, frames = 1), timed
with device events around `--hops` calls per leg and alternation (tools/hop_ab.py).
   (s) GraphedEncodeHop(sessions, header).step                           — the sender graph of the parent commit
   (S) the same + srtp=SrtpConfig(), a key on every slot                 — one more launch, hilc_srtp_protect, rows 10 bytes wider
   (r) GraphedDecodeHop(sessions, conceal, jitter).play                  — the receiver graph of the parent commit, one arrival per slot
   (R) the same + srtp=SrtpConfig(), every arrival authentic             — one more launch, hilc_srtp_unprotect, 3 more words per arrival
   (p) hilc_srtp_protect alone, outside a graph, on the rows of one hop
   (u) hilc_srtp_unprotect alone, on the arrivals of one hop
The base legs (s) and (r) are the parent commit's graphs: `srtp=None` captures exactly those.  The receiver's packets are protected once
per call counter outside the timed legs, so every arrival authenticates and is new (a replay or a forgery ends earlier and costs less).
   python tools/srtp_hop_ab.py [--hops 200] [--alternations 9] [--legs sSrRpu] > profiles/srtp_hops.txt
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/srtp_hop_ab.py --hops 50 --alternations 1 --legs pu"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import forward, graph_step, ops, srtp, synth, wire
from hilcodec_amd.jitter import JitterConfig

args = hop_ab.parse_args(legs="sSrRpu", alternations=9)

dev = torch.device("cuda:0")
B, n, T = args.streams, 8, 1
cfg = srtp.SrtpConfig()
model = synth.streaming_model()
tb = wire.transport_bytes(n, 0, T)
slots = list(range(B))
rng = np.random.default_rng(5)
rows = rng.integers(0, 256, (B, tb), dtype=np.uint8)
rows[:, 2] = n
key_rows = np.stack([srtp.key_row(bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 14, dtype=np.uint8)), b)
                     for b in range(B)])
x = synth.synth_clips(B, 320 * 8, seed=11).to(dev)
chunks = [x[:, :, 320 * i:320 * (i + 1)].contiguous() for i in range(8)]

LEGS = {"s": "(s) sender, header", "S": "(S) sender + srtp", "r": "(r) receiver, jitter", "R": "(R) receiver + srtp",
        "p": "(p) hilc_srtp_protect alone", "u": "(u) hilc_srtp_unprotect alone"}
W = 32


def keyed(hop):
    hop._keys.rows[:] = key_rows          # the rows set_key builds, without deriving 1 024 keys twice
    hop._keys.dirty = True
    return hop


def make(leg):
    if leg in "sS":
        hop = graph_step.GraphedEncodeHop(model, B, 320 * T, n, dev, sessions=True, header=True, srtp=cfg if leg == "S" else None)
    elif leg in "rR":
        hop = graph_step.GraphedDecodeHop(model, B, T, n, dev, sessions=True, conceal=True, jitter=JitterConfig(2, 8), max_arrivals=B,
                                          srtp=cfg if leg == "R" else None)
    else:
        return None
    return keyed(hop) if leg in "SR" else hop


hoppers = {leg: make(leg) for leg in args.legs}
calls = {leg: 0 for leg in args.legs}
protected = {}                             # call counter -> the hop's protected rows on the host (made outside the timed legs)
d_keys = torch.from_numpy(key_rows).to(dev)
d_nb = torch.full((B,), tb, dtype=torch.int32, device=dev)
d_gen_tx = torch.zeros(B, srtp.TX_WORDS, dtype=torch.int32, device=dev)


def wire_rows(c):
    """the protected rows of call c of leg (R), by the stand-alone launch (tests/test_gpu_srtp.py holds it equal to the host model)"""
    if c not in protected:
        rows[:, 0], rows[:, 1] = (c >> 8) & 0xFF, c & 0xFF
        protected[c] = ops.srtp_protect(torch.from_numpy(rows).to(dev), d_nb, d_keys, d_gen_tx)[0].cpu()
    return protected[c]


# the stand-alone launches: one hop's rows and records on the device
d_rows = torch.from_numpy(rows).to(dev)
d_out, d_out_nb = torch.zeros(B, tb + 10, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
d_tx = torch.zeros(B, srtp.TX_WORDS, dtype=torch.int32, device=dev)
rec, offs = forward.arrival_records(slots, wire_rows(0).numpy(), [tb + 10] * B, tb + 10, B, B)
d_rec, d_offs = torch.from_numpy(rec).to(dev), torch.from_numpy(offs).to(dev)
d_plain = torch.zeros(B, 1 + (tb + 3) // 4, dtype=torch.int32, device=dev)
d_rx = torch.zeros(B, srtp.RX_WORDS, dtype=torch.int32, device=dev)
d_start = torch.ones(B, dtype=torch.int32, device=dev)      # (u): every call starts its slots, so the one record is new every time


def one(leg, i):
    h, c = hoppers[leg], calls[leg]
    calls[leg] += 1
    if leg in "sS":
        h.step(chunks[i % 8])
    elif leg == "r":
        rows[:, 0], rows[:, 1] = (c >> 8) & 0xFF, c & 0xFF
        h.play(slots, torch.from_numpy(rows), [tb] * B)
    elif leg == "R":
        h.play(slots, wire_rows(c), [tb + 10] * B)
    elif leg == "p":
        ops.srtp_protect(d_rows, d_nb, d_keys, d_tx, out=d_out, out_nbytes=d_out_nb)
    else:
        ops.srtp_unprotect(d_rec, d_offs, d_keys, d_rx, tb, plain=d_plain, action=d_start)


def run(leg, hops):
    if leg == "R":
        for c in range(calls[leg], calls[leg] + hops):
            wire_rows(c)
        for c in [c for c in protected if c < calls[leg]]:
            del protected[c]
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# srtp_hop_ab: {B} slots, hil_speech, frames {T}, n {n}, {cfg}; rows of {tb} bytes, protected {tb + 10}; host packets, "
      f"{args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], W)
hop_ab.report(res, "# median over alternations; (S) against (s); (R) against (r); (p), (u): the launch alone, host call included",
              lambda leg: LEGS[leg], W, base={"S": "s", "R": "r"}.get)
for leg in args.legs:
    h = hoppers[leg]
    if leg in "SR":
        names, first = (srtp.TX_NAMES, srtp.TX_PROTECTED) if leg == "S" else (srtp.RX_NAMES, srtp.RX_OK)
        print(f"{LEGS[leg]:{W}s} " + ", ".join(f"{name} {v}" for name, v in zip(names, h.srtp_state[:, first:].sum(0).tolist())), flush=True)
print(f"# mean / min / max per leg: " + "; ".join(f"({leg}) {sum(v) / len(v):.4f} / {min(v):.4f} / {max(v):.4f}" for leg, v in res.items()))
