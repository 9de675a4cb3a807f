#!/usr/bin/env python
"""What SRTP costs the forwarding hop: same-box alternating legs at 1 024 slots in rooms of 8 (frames = 1, n = 8, m = 2, fanout 3, burst
2), one headed FEC packet per slot and hop from the host, timed with device events around `--hops` calls per leg and alternation
(tools/hop_ab.py).
   (f) GraphedForwardHop.forward                                         — the graph of the parent commit: `srtp=None` captures exactly it
   (S) the same + srtp=SrtpConfig(), both keys on every slot              — two more launches, arrivals and rows 10 bytes wider
   (u) hilc_srtp_unprotect alone, outside a graph, on the arrivals of one hop
   (e) hilc_srtp_protect_routes alone on one hop's rows, burst 1          — 3 072 rows, one per route
   (E) the same at burst 4, every row filled                              — 12 288 rows: one thread per row, so the chain is no longer
Every slot sends on every hop, so every listener's three routes carry a packet: 3 072 packets protected per hop of (S).  The protected
arrivals of (S) are made once per call counter outside the timed legs (hilc_srtp_protect), so every arrival authenticates and is new;
(u) starts its slots and (e) / (E) restart their routes on every call for the same reason.
   python tools/forward_srtp_ab.py [--hops 200] [--alternations 9] [--legs fSueE] > profiles/forward_srtp_hops.txt"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import forward, forward_srtp, graph_step, ops, srtp, wire
from hilcodec_amd.forward import ForwardConfig

args = hop_ab.parse_args(legs="fSueE", alternations=9, add=lambda ap: ap.add_argument("--room", type=int, default=8))

dev = torch.device("cuda:0")
B, n, m, T, ROOM = args.streams, 8, 2, 1, args.room
cfg = ForwardConfig(fanout=3, burst=2)
F = cfg.fanout
tb = wire.transport_bytes(n, m, T)
slots = list(range(B))
rng = np.random.default_rng(5)
rows = rng.integers(0, 256, (B, tb), dtype=np.uint8)
rows[:, 2] = wire.FEC_BIT | n


def key_rows(seed):
    r = np.random.default_rng(seed)
    return np.stack([srtp.key_row(bytes(r.integers(0, 256, 16, dtype=np.uint8)), bytes(r.integers(0, 256, 14, dtype=np.uint8)), 8 * b)
                     for b in range(B)])


up_rows, down_rows = key_rows(1), key_rows(2)
LEGS = {"f": "(f) forward", "S": "(S) forward + srtp", "u": "(u) hilc_srtp_unprotect alone", "e": "(e) hilc_srtp_protect_routes, burst 1",
        "E": "(E) hilc_srtp_protect_routes, burst 4"}
W = 40


def make(leg):
    if leg not in "fS":
        return None
    h = graph_step.GraphedForwardHop(B, T, n, dev, fec_stages=m, cfg=cfg, max_arrivals=B, srtp=srtp.SrtpConfig() if leg == "S" else None)
    for b in range(B):
        h.join(b, b // ROOM)
    if leg == "S":                             # the rows the key methods build, without deriving 2 048 keys through them
        h._keys.up.rows[:], h._keys.down.rows[:] = up_rows, down_rows
        h._keys.up.dirty = h._keys.down.dirty = True
    return h


hoppers = {leg: make(leg) for leg in args.legs}
calls = {leg: 0 for leg in args.legs}
protected = {}                                 # call counter -> the hop's protected arrivals on the host
d_up, d_down = torch.from_numpy(up_rows).to(dev), torch.from_numpy(down_rows).to(dev)
d_nb = torch.full((B,), tb, dtype=torch.int32, device=dev)
d_gen_tx = torch.zeros(B, srtp.TX_WORDS, dtype=torch.int32, device=dev)


def wire_rows(c):
    """the protected arrivals of call c of leg (S), by the senders' stand-alone launch"""
    if c not in protected:
        rows[:, 0], rows[:, 1] = (c >> 8) & 0xFF, c & 0xFF
        protected[c] = ops.srtp_protect(torch.from_numpy(rows).to(dev), d_nb, d_up, d_gen_tx)[0].cpu()
    return protected[c]


# the stand-alone launches: one hop's records and rows on the device
rec, offs = forward.arrival_records(slots, wire_rows(0).numpy(), [tb + 10] * B, tb + 10, B, B)
d_rec, d_offs = torch.from_numpy(rec).to(dev), torch.from_numpy(offs).to(dev)
d_plain = torch.zeros(B, 1 + (tb + 3) // 4, dtype=torch.int32, device=dev)
d_rx = torch.zeros(B, srtp.RX_WORDS, dtype=torch.int32, device=dev)
d_ones = torch.ones(B, dtype=torch.int32, device=dev)
egress = {}
for leg, P in (("e", 1), ("E", 4)):
    data = rng.integers(0, 256, (B, F, P, tb), dtype=np.uint8)
    data[..., 0], data[..., 1], data[..., 2] = 0, np.arange(P, dtype=np.uint8), wire.FEC_BIT | n
    owners = np.array([[(b // ROOM) * ROOM + (b % ROOM + 1 + j) % ROOM for j in range(F)] for b in range(B)], dtype=np.int32)
    egress[leg] = dict(rows=torch.from_numpy(data).to(dev), nbytes=torch.full((B, F, P), tb, dtype=torch.int32, device=dev),
                       routes=torch.from_numpy(owners).to(dev), new_routes=torch.ones(B, F, dtype=torch.int32, device=dev), keys=d_down,
                       route_rows=torch.zeros(B, F, forward_srtp.RT_WORDS, dtype=torch.int32, device=dev),
                       out=torch.zeros(B, F, P, tb + 10, dtype=torch.uint8, device=dev),
                       out_nbytes=torch.zeros(B, F, P, dtype=torch.int32, device=dev))


def one(leg, i):
    c = calls[leg]
    calls[leg] += 1
    if leg == "f":
        rows[:, 0], rows[:, 1] = (c >> 8) & 0xFF, c & 0xFF
        hoppers[leg].forward(slots, torch.from_numpy(rows), [tb] * B)
    elif leg == "S":
        hoppers[leg].forward(slots, wire_rows(c), [tb + 10] * B)
    elif leg == "u":
        ops.srtp_unprotect(d_rec, d_offs, d_up, d_rx, tb, plain=d_plain, action=d_ones)
    else:
        ops.srtp_protect_routes(**egress[leg])


def run(leg, hops):
    if leg == "S":
        for c in range(calls[leg], calls[leg] + hops):
            wire_rows(c)
        for c in [c for c in protected if c < calls[leg]]:
            del protected[c]
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                          # warm
    run(leg, min(5, args.hops))
print(f"# forward_srtp_ab: {B} slots in rooms of {ROOM}, frames {T}, n {n}, m {m}, {cfg}; rows of {tb} bytes, protected {tb + 10}; host "
      f"packets, {args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], W)
hop_ab.report(res, "# median over alternations; (S) against (f); (E) against (e); (u), (e), (E): the launch alone, host call included",
              lambda leg: LEGS[leg], W, base={"S": "f", "E": "e"}.get)
if "S" in hoppers:
    h = hoppers["S"]
    print(f"{LEGS['S']:{W}s} egress: " + ", ".join(f"{name} {v}" for name, v in zip(
        forward_srtp.RT_NAMES, h.egress_state[:, :, forward_srtp.RT_PROTECTED:].sum((0, 1)).tolist())) + "; ingress: " + ", ".join(
        f"{name} {v}" for name, v in zip(srtp.RX_NAMES, h.ingress_state[:, srtp.RX_OK:].sum(0).tolist())), flush=True)
for leg in "eE":
    if leg in args.legs:
        st = egress[leg]["route_rows"][:, :, forward_srtp.RT_PROTECTED:].sum((0, 1)).tolist()
        print(f"{LEGS[leg]:{W}s} " + ", ".join(f"{name} {v}" for name, v in zip(forward_srtp.RT_NAMES, st)), flush=True)
print("# mean / min / max per leg: " + "; ".join(f"({leg}) {sum(v) / len(v):.4f} / {min(v):.4f} / {max(v):.4f}" for leg, v in res.items()))
