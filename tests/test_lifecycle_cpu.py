"""CPU: the random session traffic of tests/lifecycle.py is what tests/test_gpu_lifecycle.py needs it to be.  The GPU tests only
compare two objects; that the inputs reach the paths worth comparing is proven here, for exactly the configurations, seeds and
lengths used there: scripts are deterministic and private to their stream, every script set runs through the host side of a hop
(sessions.SessionQueue with the argument checks of step() / play()) without an error, and the coverage conditions hold."""
import numpy as np
import pytest

from hilcodec_amd import jitter
from tests import lifecycle as L

TABLE = ["loop1", "loop2", "tx-plain", "tx-all", "rx-step", "rx-play"]
SOLO = ["loop2", "tx-all", "rx-play-bare"]                   # test_row_equals_solo_hop: B = 6, 30 hops, three streams per class
SOLO_HOPS, SOLO_SIZE = 30, 3


def dry_run(cfg, scripts, slot_of, arrivals=None, records_from=None, batch=None):
    """every hop of `scripts` through a DryHop; returns (the hop, the driver)"""
    hop = L.DryHop(cfg, len(slot_of) if batch is None else batch)
    drv = L.Driver(cfg, hop, scripts, slot_of, "cpu", arrivals=arrivals, records_from=records_from)
    for _ in range(drv.hops):
        drv.step()
    return hop, drv


def object_sets(name, hops=40, size=4):
    """the two objects of the neighbour tests: (scripts, arrivals or None) each"""
    cfg = L.CONFIGS[name]
    probe, first, second = L.SEEDS[name]
    slot_of = L.slot_map(size)
    out = []
    for other in (first, second):
        arrivals = L.arrivals_for(cfg, probe, other, slot_of, hops, size) if cfg.kind == "rx_play" else None
        out.append((L.make_scripts(cfg, probe, other, hops, size), arrivals))
    return cfg, slot_of, out


def solo_set(name):
    """the big object of the solo test: (configuration, slots, scripts, arrivals or None)"""
    cfg = L.CONFIGS[name]
    probe, other = L.SOLO_SEEDS[name]
    slot_of = L.slot_map(SOLO_SIZE)
    arrivals = L.arrivals_for(cfg, probe, other, slot_of, SOLO_HOPS, SOLO_SIZE) if cfg.kind == "rx_play" else None
    return cfg, slot_of, L.make_scripts(cfg, probe, other, SOLO_HOPS, SOLO_SIZE), arrivals


@pytest.mark.parametrize("name", sorted(L.CONFIGS))
def test_scripts_are_deterministic_and_private(name):
    cfg = L.CONFIGS[name]
    for hops, size in ((40, 4), (SOLO_HOPS, SOLO_SIZE)):
        for s in list(range(size)) + list(range(L.NEIGHBOUR, L.NEIGHBOUR + size)):
            assert L.make_script(5, s, cfg, hops, size).digest() == L.make_script(5, s, cfg, hops, size).digest()
            assert L.make_script(5, s, cfg, hops, size).digest() != L.make_script(6, s, cfg, hops, size).digest()
        a, b = L.make_scripts(cfg, 5, 6, hops, size), L.make_scripts(cfg, 5, 7, hops, size)
        for s in range(size):
            assert a[s].digest() == b[s].digest()            # a probe's script under two neighbour seeds: byte-identical
            assert a[L.NEIGHBOUR + s].digest() != b[L.NEIGHBOUR + s].digest()
    if cfg.kind == "rx_play":
        # the probes' arrivals are the same bytes whatever the neighbours' network does
        slot_of = L.slot_map()
        probes = {slot for s, slot in slot_of.items() if s < L.NEIGHBOUR}
        a, b = L.arrivals_for(cfg, 5, 6, slot_of, 40), L.arrivals_for(cfg, 5, 7, slot_of, 40)
        for (sa, pa, na), (sb, pb, nb) in zip(a, b):
            ia, ib = [i for i, s in enumerate(sa) if s in probes], [i for i, s in enumerate(sb) if s in probes]
            assert [sa[i] for i in ia] == [sb[i] for i in ib] and [na[i] for i in ia] == [nb[i] for i in ib]
            assert np.array_equal(pa[ia], pb[ib])
        assert any(sa != sb for (sa, _p, _n), (sb, _q, _m) in zip(a, b))


def test_scripted_places():
    """the quiet window: at least 6 hops without an event of any stream, with a stream stopped"""
    for name in sorted(L.CONFIGS):
        for hops, size in ((40, 4), (SOLO_HOPS, SOLO_SIZE)):
            scripts = L.make_scripts(L.CONFIGS[name], 5, 6, hops, size)
            P = L.plan(hops)
            assert P["quiet1"] - P["quiet0"] >= 6 and P["quiet1"] < hops
            held = L.held_sets(scripts)
            for k in range(P["quiet0"], P["quiet1"]):
                assert all(not sc.events[k].kinds() for sc in scripts.values()), (name, k)
                assert held[k] and not any(scripts[s].events[k].hold for s in held[k]), (name, k)


@pytest.mark.parametrize("name", sorted(L.CONFIGS))
def test_every_script_set_is_valid(name):
    """no call raises and no hop queues more than max_loads_per_hop resumes: the 40-hop objects of the neighbour, poison and twin
    tests (a forced upload included), and the 30-hop objects of the solo test with each probe alone"""
    cfg, slot_of, objects = object_sets(name)
    for scripts, arrivals in objects:
        hop, _ = dry_run(cfg, scripts, slot_of, arrivals)
        assert max(h + d for h, d in hop.loads) <= L.MAX_LOADS
        if cfg.has_n:
            twin = L.Driver(cfg, L.DryHop(cfg, len(slot_of)), scripts, slot_of, "cpu", force_upload=True)
            for _ in range(twin.hops):
                twin.step()
    if name in SOLO:
        cfg, slot_of, scripts, arrivals = solo_set(name)
        probe, first = L.SOLO_SEEDS[name]
        big = L.Driver(cfg, L.DryHop(cfg, len(slot_of)), scripts, slot_of, "cpu", arrivals=arrivals)
        solos = []
        for s in range(SOLO_SIZE):
            alone = L.arrivals_for(cfg, probe, first, {s: 0}, SOLO_HOPS, SOLO_SIZE) if cfg.kind == "rx_play" else None
            solos.append(L.Driver(cfg, L.DryHop(cfg, 1), {s: scripts[s]}, {s: 0}, "cpu", arrivals=alone, records_from=big))
        for _ in range(SOLO_HOPS):                           # hop by hop: a solo object resumes from what the big one just exported
            big.step()
            for solo in solos:
                solo.step()


def coverage(name):
    """the coverage counts of a configuration's first and second object"""
    cfg, slot_of, objects = object_sets(name)
    probes, others = list(range(4)), list(range(L.NEIGHBOUR, L.NEIGHBOUR + 4))
    out = []
    for scripts, arrivals in objects:
        hop, _ = dry_run(cfg, scripts, slot_of, arrivals)
        c = dict(probe_kinds=L.kind_counts(scripts, probes), neighbour_kinds=L.kind_counts(scripts, others),
                 mixed_record_hops=sum(h > 0 and d > 0 for h, d in hop.loads),
                 full_load_hops=sum(h + d == L.MAX_LOADS for h, d in hop.loads), resumes_into_held=hop.resumes_into_held,
                 held_again_quietly=len(L.held_again_quietly(scripts)), skipped_uploads=len(L.skipped_uploads(scripts)))
        if cfg.reports:
            c["probe_fec_switches"] = L.fec_switch_changes(scripts, probes)
        if cfg.kind == "rx_play":
            even = sorted(slot_of[s] for s in probes)
            c["probe_stats"] = dict(zip(jitter.STAT_NAMES, hop.stat_seen[even, jitter.STAT_ACCEPTED:].max(axis=0).tolist()))
            c["probe_adapt"] = dict(zip(jitter.AD_NAMES, hop.adapt_seen[even, jitter.AD_GROWN:].max(axis=0).tolist()))
            c["probe_reports_due"] = int(hop.due[even].sum())
        out.append(c)
    return out


@pytest.mark.parametrize("name", TABLE)
def test_coverage(name):
    cfg = L.CONFIGS[name]
    for c in coverage(name):
        print(name, L.SEEDS[name], c)
        for kind in cfg.kinds():
            assert c["probe_kinds"].get(kind, 0) >= 2, (kind, "probes")
            assert c["neighbour_kinds"].get(kind, 0) >= 2, (kind, "neighbours")
        assert c["mixed_record_hops"] >= 1 and c["full_load_hops"] >= 1 and c["resumes_into_held"] >= 1
        if cfg.kind in ("loop", "tx"):
            # GraphedHop._upload's early return; a receiver uploads its packets on every hop and has none
            assert c["held_again_quietly"] >= 1
            assert c["skipped_uploads"] >= 5
        if cfg.reports:
            assert c["probe_fec_switches"] >= 1
        if cfg.kind == "rx_play":
            # every counter a 40-hop run can move.  With AdaptConfig()'s window of 50 hops no window completes in 40 hops: the
            # windowed estimate (AD_PENDING, AD_STALE, AD_MARGIN) never acts and AD_FORCED, which needs force_windows = 4 windows
            # that wanted the same direction (200 hops), cannot move.  These runs cover the urgent-debt and resync half of the
            # adaptive playout only; grown and shrunk come from urgent debts (tests/test_gpu_jitter_adapt.py covers the rest)
            assert all(v > 0 for v in c["probe_stats"].values()), c["probe_stats"]
            assert all(v > 0 for k, v in c["probe_adapt"].items() if k != "forced"), c["probe_adapt"]
            assert c["probe_reports_due"] >= 1


@pytest.mark.parametrize("name", SOLO)
def test_solo_coverage(name):
    """the objects of test_row_equals_solo_hop: on the three compared probes every event kind occurs, a probe resumes from
    ANOTHER stream's record (the one path that test alone has: the solo object takes the record the big one exported) as host and
    as device tensors, and the sender with every option moves a compared probe's FEC switch"""
    cfg, slot_of, scripts, arrivals = solo_set(name)
    probes = list(range(SOLO_SIZE))
    hop, _ = dry_run(cfg, scripts, slot_of, arrivals)
    kinds, cross = L.kind_counts(scripts, probes), L.cross_resumes(scripts, probes)
    print(name, L.SOLO_SEEDS[name], kinds, cross)
    for kind in cfg.kinds():
        assert kinds.get(kind, 0) >= 1, kind
    assert cross["host"] >= 1 and cross["dev"] >= 1, cross
    assert any(h > 0 and d > 0 for h, d in hop.loads)
    if cfg.reports:
        assert L.fec_switch_changes(scripts, probes) >= 1
    if cfg.kind == "rx_play":
        even = sorted(slot_of[s] for s in probes)
        assert all(hop.stat_seen[even, jitter.STAT_ACCEPTED + i].max() > 0 for i, n in enumerate(jitter.STAT_NAMES) if n != "noise")
        assert hop.due[even].sum() >= 1
