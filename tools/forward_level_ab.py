#!/usr/bin/env python
"""What level-based speaker selection costs: same-box alternating legs at 1 024 slots in rooms of 8 (hil_speech, n = 8, frames = 1, m =
2, fanout 3), one headed FEC packet per slot and hop from the host, timed with device events around `--hops` calls per leg and
alternation (tools/hop_ab.py; the traffic is tools/forward_hop_ab.py's).
   (p) GraphedForwardHop.forward without speakers                        — the graph of forward_hop_ab's leg (f): compare the two lines
   (u) GraphedForwardHop(speakers=SpeakerConfig()).forward, no levels    — one more launch, one more row; every arrival unknown
   (l) the same with a level on every arrival                           — and the host's reduction of 1 024 levels
   (e) GraphedEncodeHop(sessions, fec_stages=2, header).step             — the sender hop at 1 024 streams
   (E) the same with audio_level=True                                    — one more launch
   python tools/forward_level_ab.py [--hops 200] [--alternations 9] [--legs pulEe] > profiles/forward_level_hops.txt
   python tools/forward_level_ab.py --loop > profiles/forward_level_loop.txt
Then, unless `--alone`, tools/forward_hop_ab.py runs in a child process of the same session with the same --hops and --alternations: its
leg (f) is the graph of leg (p), so the two lines should lie within each other's spread.
`--loop` needs no GPU: the two host scenarios of tests/test_audio_level_cpu.py (a room of six senders without DTX; two talkers 1 dB
apart) with the models of hilcodec_amd/audio_level.py, the counts that the tests hold conditions on."""
import os
import subprocess
import sys

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import audio_level, forward, graph_step, synth, wire
from hilcodec_amd.audio_level import SpeakerConfig, SpeakerForwardModel
from hilcodec_amd.forward import LR_SWITCHES, ForwardConfig, ForwardModel


def loop():
    from tests.level_loop import ROOM_SCRIPT, ScriptedRoom, heard_of_wanted
    B, n, T = 6, 8, 1
    cfg, sp = ForwardConfig(fanout=2, burst=1, hang_hops=8), SpeakerConfig()
    room, layers = np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32)
    join = lambda h, B=B: np.full(B, int(h == 0), dtype=np.int32)
    print(f"# forward_level_ab --loop: host models only (forward.ForwardModel, audio_level.SpeakerForwardModel), {sp}")
    print(f"# room: {B} senders without DTX in one room, {cfg}, 400 hops, script (slot, from, to, level) {ROOM_SCRIPT}; listener 0")
    plain, ruled = ForwardModel(B, cfg, n, T), SpeakerForwardModel(B, cfg, sp, n, T)
    for name, model, step in (("plain", plain, lambda h, s, p, nb, lv: plain.step(s, p, nb, room, layers, join(h))["routes"]),
                              ("with the rule", ruled, lambda h, s, p, nb, lv: ruled.step(s, p, nb, lv, room, layers, join(h))["routes"])):
        heard, wanted = heard_of_wanted(ScriptedRoom(B, n, T, ROOM_SCRIPT, seed=1), step, 400)
        print(f"{name:14s} heard {heard} of {wanted} scripted talker-hops ({100.0 * heard / wanted:.1f} %), "
              f"{int(model.listener.state[0, LR_SWITCHES])} route switches, final routes {model.listener.routes[0].tolist()}")
    B, cfg = 4, ForwardConfig(fanout=1, burst=1, hang_hops=8)
    print(f"# duel: {B} senders, slots 1 and 2 at levels 20 and 21 + U{{-4..4}}, the others at 70, {cfg}, 300 hops; listener 0")
    for margin in (0, 3, 6):
        model = SpeakerForwardModel(B, cfg, SpeakerConfig(margin_db=margin), n, T)
        net = ScriptedRoom(B, n, T, ((1, 0, 300, 20), (2, 0, 300, 21)), seed=2, background_jitter=0, spike_p=0.0)
        for h in range(300):
            s, p, nb, lv = net.hop(h)
            model.step(s, p, nb, lv, np.zeros(B, dtype=np.int32), np.full(B, n, dtype=np.int32), join(h, B))
        print(f"margin_db {margin}: {int(model.listener.state[0, LR_SWITCHES])} route switches")


if "--loop" in sys.argv:
    loop()
    sys.exit(0)

def _more_args(ap):
    ap.add_argument("--room", type=int, default=8)
    ap.add_argument("--alone", action="store_true", help="do not run tools/forward_hop_ab.py afterwards")


args = hop_ab.parse_args(legs="pulEe", alternations=9, add=_more_args)

dev = torch.device("cuda:0")
B, n, m, T, ROOM = args.streams, 8, 2, 1, args.room
cfg, sp = ForwardConfig(fanout=3), SpeakerConfig()
tb = wire.transport_bytes(n, m, T)
slots = list(range(B))


def trace(hops, seed=5):
    """[(packets uint8 [B, tb], nbytes, levels)] of `hops` hops: forward_hop_ab's packets, and a level per slot that wanders between
    loud and murmur so that the stage changes"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(hops):
        length = tb if k else wire.TRANSPORT_HEADER + wire.packet_bytes(n, T)
        rows = rng.integers(0, 256, (B, tb), dtype=np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2] = k >> 8, k & 0xFF, (wire.FEC_BIT if k else 0) | n
        rows[:, length:] = 0
        talking = (np.arange(B) // 3 + k // 25) % 3 == 0
        levels = np.where(talking, 22, 72) + rng.integers(-4, 5, B)
        out.append((torch.from_numpy(rows), [length] * B, levels.tolist()))
    return out


LEGS = {"p": "(p) forward, no speakers", "u": "(u) forward, speakers, levels unknown", "l": "(l) forward, speakers, a level each",
        "e": "(e) sender hop", "E": "(E) sender hop, audio_level=True"}
W = 40
sent = trace(args.hops)
x = synth.synth_clips(B, 320 * 8, seed=3).to(dev) if set(args.legs) & set("eE") else None


def make(leg):
    if leg in "pul":
        h = graph_step.GraphedForwardHop(B, T, n, dev, fec_stages=m, cfg=cfg, max_arrivals=B, speakers=None if leg == "p" else sp)
        for b in range(B):
            h.join(b, b // ROOM)
        return h
    return graph_step.GraphedEncodeHop(synth.streaming_model(), B, 320 * T, n, dev, sessions=True, fec_stages=m, header=True,
                                       audio_level=leg == "E")


hoppers = {leg: make(leg) for leg in args.legs}


def one(leg, i):
    if leg in "eE":
        hoppers[leg].step(x[:, :, 320 * (i % 8):320 * (i % 8 + 1)])
        return
    packets, nbytes, levels = sent[i]
    if leg == "l":
        hoppers[leg].forward(slots, packets, nbytes, levels)
    else:
        hoppers[leg].forward(slots, packets, nbytes)


def run(leg, hops):
    return hop_ab.timed(hops, lambda i: one(leg, i))


for leg in args.legs:                    # warm
    run(leg, min(5, args.hops))
print(f"# forward_level_ab: {B} slots in rooms of {ROOM}, hil_speech, frames 1, n {n}, m {m}, {cfg}, {sp}; host packets, "
      f"{args.hops} hops per leg x {args.alternations} alternations; {torch.cuda.get_device_name(dev)}", flush=True)
res = hop_ab.alternate(args.legs, args, run, lambda leg: LEGS[leg], W)
hop_ab.report(res, "# median over alternations; (u), (l) against (p); (E) against (e)", lambda leg: LEGS[leg], W,
              base={"u": "p", "l": "pu", "E": "e"}.get)
for leg in args.legs:
    if leg in "ul":
        h = hoppers[leg]
        st, spk = h.listener_state.sum(0).tolist(), h.speaker_state[:, audio_level.SP_LEVELLED:].sum(0).tolist()
        print(f"{LEGS[leg]:{W}s} " + ", ".join(f"{name} {v}" for name, v in zip(forward.LR_NAMES, st)) + "; speakers: " +
              ", ".join(f"{name} {v}" for name, v in zip(audio_level.SP_NAMES[audio_level.SP_LEVELLED:], spk)), flush=True)
    elif leg == "E":
        print(f"{LEGS[leg]:{W}s} levels of the last hop: min {int(hoppers[leg].audio_level.min())}, max {int(hoppers[leg].audio_level.max())}",
              flush=True)
if not args.alone:
    hoppers.clear()                      # a fresh child process measures the same graph by the earlier tool
    torch.cuda.empty_cache()
    print("# tools/forward_hop_ab.py in the same session: its leg (f) is the graph of leg (p)", flush=True)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "forward_hop_ab.py"), "--hops", str(args.hops),
                    "--alternations", str(args.alternations), "--streams", str(B), "--room", str(ROOM)], check=True)
