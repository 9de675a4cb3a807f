#!/usr/bin/env python
"""What the forwarding hop's downlink control costs: same-box alternating legs at 1 024 slots in rooms of 8 (n = 8, frames = 1, m = 2,
fanout 3), one headed FEC packet per slot and hop from the host, timed with device events around `--hops` calls per leg and alternation
(tools/hop_ab.py).
   (f) GraphedForwardHop.forward without downlink=                      — one upload, two launches: the hop as it was
   (d) with downlink=DownlinkConfig(rate=, history=16), no feedback     — the same upload with the feedback rows in it, four launches
   (D) the same with a report and a NACK for every listener route on every hop: 3 072 of each, checked and staged on the host,
       every NACK answered from the owner's history
Every slot sends on every hop (no DTX), so every listener's three routes carry a packet.  Behind the legs, the four launches of (D)'s
last hop are timed one by one, eagerly, on that hop's staged inputs: which launch a difference between the legs belongs to.
   python tools/downlink_hop_ab.py [--hops 200] [--alternations 5] [--legs fdD] > profiles/downlink_hops.txt"""
import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import downlink, graph_step, ops, wire
from hilcodec_amd.downlink import DownlinkConfig
from hilcodec_amd.forward import ForwardConfig
from hilcodec_amd.rate import RateConfig

args = hop_ab.parse_args(legs="fdD", alternations=5, add=lambda ap: ap.add_argument("--room", type=int, default=8))

dev = torch.device("cuda:0")
B, n, m, T, ROOM = args.streams, 8, 2, 1, args.room
cfg = ForwardConfig(fanout=3)
dcfg = DownlinkConfig(rate=RateConfig(min_kbps=9.0, max_kbps=36.0), history=16, per_hop=2)
tb = wire.transport_bytes(n, m, T)
slots = list(range(B))
F = cfg.fanout


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


def feedback(hops):
    """per hop (reports, nacks) for every listener route: a report whose seq advances with no loss, a NACK for the hop two back"""
    listeners, routes = np.repeat(np.arange(B), F), np.tile(np.arange(F), B)
    out = []
    for k in range(hops):
        rep = torch.tensor([k & 255, 0, 0], dtype=torch.uint8).repeat(B * F, 1)
        base = max(k - 2, 0)
        nack = torch.tensor([base >> 8, base & 255, 0, 0], dtype=torch.uint8).repeat(B * F, 1)
        out.append(((listeners, routes, rep), (listeners, routes, nack)))
    return out


LEGS = {"f": "(f) forward, no downlink=", "d": "(d) downlink=, no feedback", "D": "(D) downlink=, 3 072 reports + NACKs"}
sent, fed = trace(args.hops), feedback(args.hops)


def make(leg):
    h = graph_step.GraphedForwardHop(B, T, n, dev, fec_stages=m, cfg=cfg, max_arrivals=B, downlink=None if leg == "f" else dcfg)
    for b in range(B):
        h.join(b, b // ROOM)
    return h


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    packets, nbytes = sent[i]
    if leg == "D":
        hoppers[leg].forward(slots, packets, nbytes, reports=fed[i][0], nacks=fed[i][1])
    else:
        hoppers[leg].forward(slots, packets, nbytes)


def run(leg, hops):
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# downlink_hop_ab: {B} slots in rooms of {ROOM}, frames 1, n {n}, m {m}, {cfg}, {dcfg}; host packets and feedback, "
      f"{args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], 40)
hop_ab.report(res, "# median over alternations; (d) and (D) against (f), (D) against (d)", lambda leg: LEGS[leg], 40,
              base={"d": "f", "D": "fd"}.get)
for leg in args.legs:
    if leg != "f":
        h = hoppers[leg]
        st, ds = h.downlink_state[:, downlink.DL_REPORTS:].sum(0).tolist(), h.history_state.sum(0).tolist()
        print(f"{LEGS[leg]:40s} " + ", ".join(f"{name} {v}" for name, v in zip(downlink.DL_NAMES, st)) + "; histories: " +
              ", ".join(f"{name} {v}" for name, v in zip(downlink.DS_NAMES, ds)) + f"; layers {int(h.eff_layers.min())}..{int(h.eff_layers.max())}",
              flush=True)

if "D" in args.legs:                     # the four launches of (D)'s last hop, eagerly, on its staged inputs and copies of its state
    h = hoppers["D"]
    st, a = h.stage, (cfg, n, T, m, None)
    c = lambda t: t.clone()
    sd, lr, pick, count, routes, new = c(h._sd), c(h._lr), c(h._pick), c(h._pick_count), c(h._routes), c(h._new_routes)
    out, nb, tags, ring, dsr = c(h._out[0]), c(h._out_nbytes[0]), *(c(t) for t in h._hist)
    dl, mem, eff, out2, nb2 = c(h._dl), c(h._dl_mem), c(h._eff[0]), c(h._dl_out[0]), c(h._dl_nbytes[0])
    rtx = dict(zip(("rtx_out", "rtx_nbytes", "rtx_routes"), (c(t) for t in h._rtx[0])))
    launches = {
        "hilc_forward_classify": lambda i: ops.forward_classify(h.arrivals, h.offsets, sd, pick, count, *a, action=st.row["action"]),
        "hilc_forward_route": lambda i: ops.forward_route(h.arrivals, st.row["room"], st.row["layers"], sd, pick, count, routes, new, lr,
                                                          out, nb, *a, action=st.row["action"]),
        "hilc_downlink_store": lambda i: ops.downlink_store(h.arrivals, pick, count, tags, ring, dsr, n, T, m, action=st.row["action"]),
        "hilc_downlink_step": lambda i: ops.downlink_step(routes, new, out, nb, st.row["layers"], dl, mem, eff, out2, nb2, dcfg, cfg, n, T,
                                                          m, action=st.row["action"], tags=tags, ring=ring, **h._fb, **rtx),
    }
    print("# the launches of (D)'s last hop, one by one (eager, 200 calls each, launch overhead included)")
    for name, fn in launches.items():
        fn(0)
        print(f"{name:24s} {1e3 * hop_ab.timed(200, fn):.1f} us/call", flush=True)
