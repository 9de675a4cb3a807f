#!/usr/bin/env python
"""What the sender / receiver split of the graphed hop costs per side: same-box, alternating legs, device events around `--hops`
replays per leg and alternation (hil_speech, hop 320 = 13.33 ms at 24 kHz, n = 8).
   loop  GraphedHop (encoder -> RVQ -> dequantiser -> decoder, the loopback)
   send  GraphedEncodeHop alone (packets out)
   recv  GraphedDecodeHop alone (device packets and host n in, one frame per hop)
   s+r   sender then receiver back to back, the sender's packets passed on the device
then the sender and the receiver alone at 1, 8, 64, 256 and 1 024 streams (ms per hop and x real time = streams x 13.33 ms / ms
per hop), and the reference's protocol: ONE stream, the first 5 s of the speech recording of tests/golden/realistic.npz (its
trained codebooks), encoder side and decoder side real-time factors (audio seconds / processing seconds).
   python tools/split_hop_ab.py [--hops 200] [--alternations 3] [--streams 1024] > profiles/split_hops.txt
The kernels' own times come from a separate kernel-trace run (no counters in that run):
   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/split_hop_ab.py --hops 50 --alternations 1 --no-sweep --no-ref"""
import os
import statistics

import hop_ab  # first: it puts the repository root on sys.path
import numpy as np
import torch

from hilcodec_amd import graph_step, synth

def options(ap):
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-ref", action="store_true")


args = hop_ab.parse_args(add=options)

dev = torch.device("cuda:0")
HOP, N, SR = 320, 8, 24000
HOP_MS = 1e3 * HOP / SR
model = synth.streaming_model()


def legs_for(B, which):
    xs = [synth.synth_clips(B, HOP, seed=4321 + 7 * j).to(dev) for j in range(8)]
    n_list = [N] * B
    out = {}
    if "send" in which or "s+r" in which:
        s = graph_step.GraphedEncodeHop(model, B, HOP, N, dev)
        packets = [s.step(xs[j])[0].clone() for j in range(8)]
        if "send" in which:
            out["send"] = lambda i: s.step(xs[i % 8])
    if "recv" in which or "s+r" in which:
        r = graph_step.GraphedDecodeHop(model, B, 1, N, dev)
        if "recv" in which:
            out["recv"] = lambda i: r.step(packets[i % 8], n_list)
    if "s+r" in which:
        out["s+r"] = lambda i: r.step(s.step(xs[i % 8])[0], n_list)
    if "loop" in which:
        g = graph_step.GraphedHop(model, B, HOP, N, dev)
        out["loop"] = lambda i: g.step(xs[i % 8])
    for fn in out.values():             # warm
        for i in range(5):
            fn(i)
    return out


names = {"loop": "loopback GraphedHop", "send": "sender GraphedEncodeHop", "recv": "receiver GraphedDecodeHop",
         "s+r": "sender + receiver back to back"}
B = args.streams
print(f"# split_hop_ab: hil_speech, hop {HOP} ({HOP_MS:.2f} ms), n {N}, {args.hops} hops per leg x {args.alternations} "
      f"alternations; {torch.cuda.get_device_name(dev)}", flush=True)
legs = legs_for(B, ("loop", "send", "recv", "s+r"))
res = hop_ab.alternate(list(legs), args, lambda leg, hops: hop_ab.timed(hops, legs[leg]), lambda leg: f"{B:5d} streams {names[leg]}", 48)
med = hop_ab.report(res, f"# {B} streams, median over alternations", names.get, 34,
                    tail=lambda leg, ms: f"  x{B * HOP_MS / ms:.0f} real time")
print(f"sender + receiver - loopback: {1e3 * (med['s+r'] - med['loop']):+.1f} us/hop; sender + receiver measured alone: "
      f"{med['send'] + med['recv']:.4f} ms/hop", flush=True)
del legs

if not args.no_sweep:
    print("# per side alone: streams, ms/hop (median over alternations), x real time")
    for b in (1, 8, 64, 256, 1024):
        legs = legs_for(b, ("send", "recv"))
        r = hop_ab.alternate(list(legs), args, lambda leg, hops: hop_ab.timed(hops, legs[leg]))
        ms = {k: statistics.median(v) for k, v in r.items()}
        print(f"sweep {b:5d} streams  sender {ms['send']:.4f} ms/hop x{b * HOP_MS / ms['send']:.1f} RT   "
              f"receiver {ms['recv']:.4f} ms/hop x{b * HOP_MS / ms['recv']:.1f} RT", flush=True)
        del legs

if not args.no_ref:
    from tests.models import realistic_state_dict
    g = dict(np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "realistic.npz")))
    real = synth.streaming_model(state_dict=realistic_state_dict(g))
    hops = 5 * SR // HOP                                     # 375 hops: the first 5 s
    x = torch.from_numpy(g["pcm"][:hops * HOP].astype(np.float32) / 32768.0).view(1, 1, -1).to(dev)
    chunks = [x[:, :, HOP * h:HOP * (h + 1)].contiguous() for h in range(hops)]
    s = graph_step.GraphedEncodeHop(real, 1, HOP, N, dev)
    packets = [s.step(c)[0].clone() for c in chunks]
    s.reset()
    enc_ms = hop_ab.timed(hops, lambda i: s.step(chunks[i])) * hops
    r = graph_step.GraphedDecodeHop(real, 1, 1, N, dev)
    dec_ms = hop_ab.timed(hops, lambda i: r.step(packets[i], [N])) * hops
    sec = hops * HOP / SR
    print(f"# reference protocol: 1 stream, hop {HOP}, n {N}, the first {sec:.1f} s of realistic.npz's speech, one replay per hop "
          f"per side (device events around all {hops} hops)")
    print(f"reference-protocol encoder rtf {sec / (enc_ms * 1e-3):.2f}  decoder rtf {sec / (dec_ms * 1e-3):.2f}  total rtf "
          f"{sec / ((enc_ms + dec_ms) * 1e-3):.2f}   (encoder {enc_ms / hops:.4f} ms/hop, decoder {dec_ms / hops:.4f} ms/hop)")
    print("reference's published (scripts/HILCodec Onnx.ipynb: ONNX Runtime on a CPU, not a GPU): encoder rtf 1.565  decoder rtf "
          "0.555  total rtf 0.410", flush=True)
