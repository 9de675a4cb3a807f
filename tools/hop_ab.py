"""The method every tools/*_hop_ab.py measures by, stated once (DESIGN.md §3.3 records their numbers): same-box legs, each timed
with one pair of device events around `--hops` calls, run `--alternations` times in an order that reverses on odd rounds, and
reported as the median with min and max and the difference against a base leg.  A tool keeps what is its own: its legs and
traffic, its `run(leg, hops)` with its own warm-up (once up front or before every timed run: part of how its numbers were
taken), its heading lines and any extra report.  Import this module first: it puts the repository root on sys.path."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def parse_args(legs=None, alternations=3, add=None):
    """--hops --alternations [--legs] --streams and what `add(parser)` adds; exits without a GPU"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=alternations)
    if legs is not None:
        ap.add_argument("--legs", default=legs)
    ap.add_argument("--streams", type=int, default=1024)
    if add is not None:
        add(ap)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit(f"{os.path.basename(sys.argv[0])} needs a GPU")
    return args


def timed(hops, fn):
    """ms per call of fn(0) .. fn(hops - 1), between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(hops):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / hops


def alternate(legs, args, run, name=None, width=0):
    """{leg: [run(leg, args.hops) per alternation]}, the legs in reverse order on odd alternations; with `name(leg)`, one
    `alt k <name> <ms> ms/hop` line per run"""
    res = {leg: [] for leg in legs}
    for a in range(args.alternations):
        for leg in (legs if a % 2 == 0 else legs[::-1]):
            ms = run(leg, args.hops)
            res[leg].append(ms)
            if name is not None:
                print(f"alt {a} {name(leg):{width}s} {ms:.4f} ms/hop", flush=True)
    return res


def report(res, heading, name, width, base=None, tail=None):
    """the heading, then per leg its median, min and max, the difference against each of the legs `base(leg)` names (a string of
    leg letters or None; a leg that did not run, or the leg itself, is passed over) and `tail(leg, median)`; returns the medians"""
    print(heading)
    med = {leg: statistics.median(v) for leg, v in res.items()}
    for leg, v in res.items():
        line = f"{name(leg):{width}s} {med[leg]:.4f} ms/hop  (min {min(v):.4f}, max {max(v):.4f})"
        for b in dict.fromkeys(base(leg) or "" if base else ""):
            if b in res and b != leg:
                line += f"  {1e3 * (med[leg] - med[b]):+.1f} us ({100.0 * (med[leg] - med[b]) / med[b]:+.2f} %) vs ({b})"
        print(line + (tail(leg, med[leg]) if tail else ""), flush=True)
    return med
