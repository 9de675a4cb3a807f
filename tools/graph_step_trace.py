#!/usr/bin/env python
"""Which kernels and which host-to-device copies the graphed hops issue: every hop class of hilcodec_amd/graph_step.py is built in
a fixed list of option combinations (COMBOS: each feature on and off) and replays a fixed, seeded schedule of `HOPS` hops with
session actions.  Two commits issue the same graphs and the same copies when their tables are equal.
   rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d <dir> -o t -- python tools/graph_step_trace.py --log <dir>/host.json
   python tools/graph_step_trace.py --summarize <dir>          (no GPU needed)  > table
The run separates the combinations in the trace by one marker launch (an erfinv_ on a [1] tensor, used nowhere else); the copies the
host code issues are also counted in the process itself (every Tensor.copy_ from the host to the device: count and bytes), since
the trace's copy records carry no sizes.  No counters in that run."""
import argparse
import collections
import csv
import glob
import json
import os
import re
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HOP, N, M, K, HOPS = 16, 320, 8, 2, 8, 6
COMBOS = ["hop_g1", "hop_g2", "hop_sessions", "hop_sessions_g2", "pipelined_g1", "pipelined_g2",
          "send_plain", "send_sessions", "send_all", "recv_plain", "recv_sessions", "recv_all_but_jitter", "recv_jitter_only",
          "recv_jitter_all", "send_feedback", "recv_jitter_feedback", "forward"]
MARK = "erfinv"


def short(name):
    """a kernel's name for the table: the project's kernels with their template arguments; any other (ATen's long functor names)
    cut to 70 characters plus a checksum of the whole name, so that different kernels stay different"""
    name = name.replace("(anonymous namespace)::", "")
    m = re.search(r"hilc::(\w+)(<[^(]*>)?\(", name)
    if m:
        return (m.group(1) + (m.group(2) or "")).replace(", ", ",")
    return f"{name.replace('void ', '')[:70]} #{zlib.crc32(name.encode()) & 0xFFFF:04x}"


def summarize(d):
    host = json.load(open(os.path.join(d, "host.json")))
    kfile = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(kfile)))
    marks = [t for t, k in rows if MARK in k]
    if len(marks) != len(COMBOS) + 1:
        sys.exit(f"{len(marks)} marker launches in the trace, {len(COMBOS) + 1} expected")
    copies = []
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        copies += [(int(r["Start_Timestamp"]), r["Direction"]) for r in csv.DictReader(open(f))]
    for i, name in enumerate(COMBOS):
        lo, hi = marks[i], marks[i + 1]
        per = collections.Counter(short(k) for t, k in rows if lo < t < hi)
        h2d = sum(1 for t, dr in copies if lo < t < hi and "HOST_TO_DEVICE" in dr.upper())
        hc = host[name]
        print(f"## {name}: {sum(per.values())} kernel launches; host-to-device copies: {h2d} in the trace; issued by Tensor.copy_: "
              f"{hc['h2d_copies']} copies, {hc['h2d_bytes']} bytes ({hc['h2d_nonblocking']} non_blocking)")
        for k, c in sorted(per.items()):
            print(f"{c:6d}  {k}")


if "--summarize" in sys.argv:
    summarize(sys.argv[sys.argv.index("--summarize") + 1])
    sys.exit(0)

import numpy as np
import torch

from hilcodec_amd import dtx, graph_step, synth, wire
from hilcodec_amd.forward import ForwardConfig
from hilcodec_amd.jitter import AdaptConfig, JitterConfig
from hilcodec_amd.mixer import MixConfig
from hilcodec_amd.rate import RateConfig
from hilcodec_amd.report import FecAdaptConfig, ReportConfig
from hilcodec_amd.rtx import NackConfig, RtxConfig
from hilcodec_amd.vbr import VbrConfig

ap = argparse.ArgumentParser()
ap.add_argument("--log", required=True)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("graph_step_trace.py needs a GPU")

dev = torch.device("cuda:0")
model = synth.streaming_model()
xs = [synth.synth_clips(B, HOP, seed=4321 + 7 * j).to(dev) for j in range(HOPS)]
xs48 = [synth.synth_clips(B, HOP * 2, seed=99 + j).to(dev) for j in range(HOPS)]                 # a hop at 48 kHz
marker = torch.full((1,), 0.5, device=dev)

count = {"h2d_copies": 0, "h2d_bytes": 0, "h2d_nonblocking": 0}
_copy = torch.Tensor.copy_


def counted_copy(self, src, non_blocking=False):
    if self.is_cuda and isinstance(src, torch.Tensor) and src.device.type == "cpu":
        count["h2d_copies"] += 1
        count["h2d_bytes"] += self.numel() * self.element_size()
        count["h2d_nonblocking"] += bool(non_blocking)
    return _copy(self, src, non_blocking)


torch.Tensor.copy_ = counted_copy


def cpu(caches):
    return [c.cpu() for c in caches]


def run_hop(groups, sessions):
    h = graph_step.GraphedHop(model, B, HOP, N, dev, groups=groups, sessions=sessions)
    saved = None
    for k in range(HOPS):
        if sessions:
            if k == 1:
                h.start(2)
                h.set_bitrate(5, 3)
                saved = h.export(9)                              # device caches
            if k == 2:
                h.start(3, *saved)                               # a device record
                h.start(11, cpu(saved[0]), cpu(saved[1]), n=4)    # a host record
                h.stop(7)
            if k == 4:
                h.start(7)
            h.step(xs[k], hold=[1, 12] if k == 3 else None)
        else:
            h.step(xs[k])
    h.reset()
    h.step(xs[0])


def run_pipelined(groups):
    h = graph_step.PipelinedHop(model, B, HOP, N, dev, groups=groups)
    for k in range(HOPS):
        h.step(xs[k])
    h.flush()
    h.reset(h.cache_enc, h.cache_dec)
    h.step(xs[0])
    h.step(xs[1])
    h.flush()


def run_send(sessions, everything):
    kw = dict(input_rate=48000, fec_stages=M, dtx=dtx.DtxConfig(), header=True) if everything else {}
    h = graph_step.GraphedEncodeHop(model, B, HOP, N, dev, sessions=sessions, **kw)
    x = xs48 if everything else xs
    saved = None
    for k in range(HOPS):
        if sessions:
            if k == 1:
                h.start(2)
                h.set_bitrate(5, 3)
                saved = h.export(9)
            if k == 2:
                h.start(3, saved)
                h.start(11, cpu(saved), n=4)
                h.stop(7)
            if k == 4:
                h.start(7)
            h.step(x[k], hold=[1, 12] if k == 3 else None)
        else:
            h.step(x[k])
    h.reset()
    h.step(x[0])


def run_recv(sessions, everything):
    kw = dict(conceal=True, output_rate=48000, fec_stages=M, cng_order=K) if everything else {}
    h = graph_step.GraphedDecodeHop(model, B, 1, N, dev, sessions=sessions, **kw)
    rng = np.random.default_rng(3)
    saved = None
    for k in range(HOPS):
        pk = torch.from_numpy(rng.integers(0, 256, (B, h.stride), dtype=np.uint8))
        if k % 2:
            pk = pk.to(dev)                                      # packets already on the device: the other copy path
        n_list = [N] * B
        opt = {}
        if sessions:
            if k == 1:
                h.start(2)
                saved = h.export(9)
            if k == 2:
                h.start(3, saved)
                h.start(11, cpu(saved))
                h.stop(7)
            if k == 4:
                h.start(7)
            if k == 3:
                opt["hold"] = [1, 12]
        if everything and k >= 2:
            opt.update(lost=[4], fec=[6], sid=[8] if k == 2 else [], silent=[8] if k > 2 else [])
        h.step(pk, n_list, **opt)


def run_send_feedback():
    """the sender with vbr (cap), fec_adapt, rtx and rate: reports and NACKs on hops 2 and 3, then two hops that only clear them"""
    h = graph_step.GraphedEncodeHop(model, B, HOP, N, dev, sessions=True, fec_stages=M, header=True,
                                    vbr=VbrConfig(12.0, cap_kbps=4.5, burst_hops=2), fec_adapt=FecAdaptConfig(), rtx=RtxConfig(),
                                    rate=RateConfig(min_kbps=6.0, max_kbps=12.0))
    for k in range(HOPS):
        if k == 1:
            h.start(2)
            h.stop(7)
        opt = {}
        if k in (2, 3):
            opt["reports"] = ([0, 5, 9], [wire.pack_report(k, 40 * (k - 1), 0)] * 3)
            opt["nacks"] = ([4, 5], torch.tensor([list(wire.pack_nack(k - 2, 1))] * 2, dtype=torch.uint8))
        h.step(xs[k], hold=[1, 12] if k == 3 else None, **opt)
    h.reset()
    h.step(xs[0])


def run_forward():
    """the forwarding hop: a join, a leave and a set_layers between hops, host packets on even hops and device packets on odd hops"""
    h = graph_step.GraphedForwardHop(B, 1, N, dev, fec_stages=M, cfg=ForwardConfig(fanout=3))
    rng = np.random.default_rng(6)
    for b in range(B):
        h.join(b, b // 8)
    for k in range(HOPS):
        order = rng.permutation(B).tolist() if k < 4 else list(range(B))           # in slot order: no gather on the device path
        slots = [b for b in order if (k + b) % 5]
        rows = rng.integers(0, 256, (len(slots), h.tstride), dtype=np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2] = k >> 8, k & 0xFF, (wire.FEC_BIT if k else 0) | N
        pk = torch.from_numpy(rows)
        if k % 2:
            pk = pk.to(dev)
        if k == 2:
            h.join(3, 1)
            h.leave(12)
        if k == 3:
            h.set_layers(5, 4)
        h.forward(slots, pk, [h.tstride] * len(slots))


def run_jitter(everything, feedback=False):
    kw = dict(conceal=True, output_rate=48000, fec_stages=M, cng_order=K) if everything else {}
    jcfg = JitterConfig(depth=2, capacity=8, adapt=AdaptConfig() if feedback else None)
    if feedback:
        kw.update(mix=MixConfig(2), report=ReportConfig(8, 4), nack=NackConfig())
    h = graph_step.GraphedDecodeHop(model, B, 1, N, dev, sessions=True, jitter=jcfg, **kw)
    m = M if everything else 0
    rng = np.random.default_rng(4)
    plain, wide = wire.packet_bytes(N, 1), wire.fec_packet_bytes(N, m, 1) if m else wire.packet_bytes(N, 1)
    for b in range(B):
        h.start(b)
    saved = None
    for k in range(HOPS):
        slots, rows, nbytes = [], [], []
        for b in rng.permutation(B).tolist():
            if (k + b) % 5 == 0:
                continue                                         # not arrived
            fec = bool(m) and k > 0
            body = rng.integers(0, 256, wide if fec else plain)
            row = np.zeros(h.tstride, dtype=np.uint8)
            row[:3], row[3:3 + len(body)] = [k >> 8, k & 0xFF, (0x40 if fec else 0) | N], body
            slots.append(b)
            rows.append(row)
            nbytes.append(3 + len(body))
        pk = torch.from_numpy(np.stack(rows))
        if k % 2:
            pk = pk.to(dev)
        if k == 1:
            saved = h.export(9)
        if k == 2:
            h.start(3, saved)
            h.start(11, cpu(saved))
            h.stop(7)
        if k == 4:
            h.start(7)
        if feedback and k == 2:
            h.join(5, 3)
        if feedback and k == 4:
            h.leave(6)
        h.play(slots, pk, nbytes, hold=[1, 12] if k == 3 else None)


RUN = {"hop_g1": lambda: run_hop(1, False), "hop_g2": lambda: run_hop(2, False), "hop_sessions": lambda: run_hop(1, True),
       "hop_sessions_g2": lambda: run_hop(2, True), "pipelined_g1": lambda: run_pipelined(1), "pipelined_g2": lambda: run_pipelined(2),
       "send_plain": lambda: run_send(False, False), "send_sessions": lambda: run_send(True, False),
       "send_all": lambda: run_send(True, True), "recv_plain": lambda: run_recv(False, False),
       "recv_sessions": lambda: run_recv(True, False), "recv_all_but_jitter": lambda: run_recv(True, True),
       "recv_jitter_only": lambda: run_jitter(False), "recv_jitter_all": lambda: run_jitter(True),
       "send_feedback": run_send_feedback, "recv_jitter_feedback": lambda: run_jitter(True, True), "forward": run_forward}

host = {}
torch.cuda.synchronize()
marker.erfinv_()
torch.cuda.synchronize()
for name in COMBOS:
    for key in count:
        count[key] = 0
    with torch.no_grad():
        RUN[name]()
    torch.cuda.synchronize()
    host[name] = dict(count)
    marker.erfinv_()
    torch.cuda.synchronize()
    print(f"{name}: {host[name]}", flush=True)
with open(args.log, "w") as f:
    json.dump(host, f, indent=1)
