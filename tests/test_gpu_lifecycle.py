"""GPU: the session machinery of the graphed hops under random traffic (tests/lifecycle.py): random start / resume / stop / hold /
set_bitrate / reports / losses / rooms per stream, quiet stretches in which _upload returns early with stops and holds live on the
device, resumes from host and device records on one hop up to max_loads_per_hop, a resume into a held slot.  Nothing is compared
with a model here — every kernel has its own test for that — but one object with another: what a slot produces must not depend
on what the other slots do (other traffic, non-finite audio, poisoned records), must equal the same stream alone in a B = 1
object, and must not depend on whether a hop uploaded its control stage.  Every comparison is bit for bit, of everything the
object shows of a slot (tests/hops.observe).  That the scripts reach the paths named above is proven in tests/test_lifecycle_cpu.py
for exactly the seeds used here."""
import pytest

from hilcodec_amd import dtx, synth
from tests import lifecycle as L
from tests.hops import DEV, HOP, first_difference, first_non_finite, observe, slot_views, target_from_reference, vbr_speech_model

pytestmark = pytest.mark.gpu

HOPS, SIZE = 40, 4
# the per-slot views each configuration must show beside its outputs, indices and exported record (tests/hops.observe)
VIEWS = {"loop1": set(), "loop2": set(), "tx-plain": set(),
         "tx-all": {"n_eff", "distortion", "credit", "kind", "fec_on", "fec_adapt_state", "hop_index"},
         "rx-step": {"concealed", "cng_state"},
         "rx-play": {"concealed", "cng_state", "jitter_state", "jitter_adapt", "reports", "report_due", "report_state", "mixed", "speakers",
                     "levels"}}
SOLO_HOPS, SOLO_SIZE = 30, 3


@pytest.fixture(scope="module")
def plain():
    return synth.streaming_model()


@pytest.fixture(scope="module")
def vbr_speech():
    """falling per-stage codebooks, so that VBR decides"""
    return vbr_speech_model()


@pytest.fixture(scope="module")
def models(plain, vbr_speech):
    """{configuration: (model, VBR target or None)}: the sender with every option takes test_gpu_vbr's model and the target of its
    reference at hop 0, every other configuration the plain streaming model"""
    target = target_from_reference(vbr_speech, 8, 1, L.N, synth.synth_clips(8, HOP, seed=1).to(DEV))
    return {name: (vbr_speech, target) if cfg.full else (plain, None) for name, cfg in L.CONFIGS.items()}


def drivers_for(name, models, seeds, hops=HOPS, size=SIZE, **second):
    """two objects of a configuration with their drivers: probes from seeds[0] in both, neighbours from seeds[1] in the first and
    seeds[2] in the second; `second`: what only the second driver gets"""
    cfg = L.CONFIGS[name]
    model, target = models[name]
    slot_of = L.slot_map(size)
    out = []
    for i, other in enumerate(seeds[1:]):
        hop = L.make_hop(cfg, model, 2 * size, DEV, target)
        arrivals = L.arrivals_for(cfg, seeds[0], other, slot_of, hops, size) if cfg.kind == "rx_play" else None
        out.append(L.Driver(cfg, hop, L.make_scripts(cfg, seeds[0], other, hops, size), slot_of, DEV, arrivals=arrivals,
                            **(second if i else {})))
    return cfg, slot_of, out


def compare_probes(what, cfg, seeds, slot_of, a, b, finite=False, every_option=False):
    """run two drivers side by side; after every hop every probe slot shows the same in both objects"""
    probes = [s for s in slot_of if s < L.NEIGHBOUR]
    n_eff, kinds, switch = set(), set(), set()
    held = L.held_sets(a.scripts)
    others, differ, poisoned = [slot_of[s] for s in slot_of if s >= L.NEIGHBOUR], False, False
    for k in range(a.hops):
        a.step()
        b.step()
        for s in probes:
            slot = slot_of[s]
            seen, other = observe(a.hop, slot), observe(b.hop, slot)
            diff = first_difference(seen, other)
            assert diff is None, L.explain(what, cfg, seeds, k, slot, diff, a, b)
            if finite:
                bad = first_non_finite(other)
                assert bad is None, L.explain(what, cfg, seeds, k, slot, bad, b)
            if every_option:
                if s not in held[k] and a.cur_n[s] == L.N:
                    n_eff.add(int(seen["n_eff"]))            # what the rule and the cap chose, not a ceiling or a hold
                kinds.add(int(seen["kind"]))
                switch.add((s, int(seen["fec_on"])))
        # the comparison is not empty: the neighbours do differ between the objects, and poison does pass through the kernels
        if not differ:
            differ = any(first_difference(observe(a.hop, slot), observe(b.hop, slot)) is not None for slot in others)
        if finite and not poisoned:
            poisoned = any(first_non_finite(observe(b.hop, slot)) is not None for slot in others)
    assert differ and (poisoned or not finite), (differ, poisoned)
    return n_eff, kinds, switch


@pytest.mark.parametrize("name", ["loop1", "loop2", "tx-plain", "tx-all", "rx-step", "rx-play"])
def test_neighbours_cannot_be_seen(models, name):
    """the probe streams (even slots) get the same scripts in two objects, the neighbours (odd slots) other audio or packets, other
    events and other resumes: every probe slot shows the same after every hop"""
    seeds = L.SEEDS[name]
    cfg, slot_of, (a, b) = drivers_for(name, models, seeds)
    assert set(slot_views(a.hop)) == VIEWS[name]
    n_eff, kinds, switch = compare_probes("neighbours", cfg, seeds, slot_of, a, b, every_option=cfg.full)
    if cfg.full:
        # the sender with every option did decide something on the probes (as tests/test_gpu_vbr.py asks of its reference)
        assert len(n_eff) >= 3, f"n_eff takes {sorted(n_eff)} only"
        assert dtx.SID in kinds and dtx.SPEECH in kinds, sorted(kinds)
        assert any((s, 0) in switch and (s, 1) in switch for s in range(SIZE)), sorted(switch)


@pytest.mark.parametrize("name", ["loop1", "tx-plain", "tx-all", "rx-step"])
def test_poisoned_neighbours(models, name):
    """as above, and the second object's neighbours are hostile: +Inf, -Inf and NaN samples on every third hop (loopback and
    senders), resumes from records with NaN and Inf in every cache (loopback and receiver).  The probes stay equal, and finite"""
    seeds = L.SEEDS[name]
    cfg = L.CONFIGS[name]
    others = range(L.NEIGHBOUR, L.NEIGHBOUR + SIZE)
    hostile = dict(poison_audio=others if cfg.kind in ("loop", "tx") else (), poison_records=others if name in ("loop1", "rx-step") else ())
    cfg, slot_of, (a, b) = drivers_for(name, models, seeds, **hostile)
    compare_probes("poisoned neighbours", cfg, seeds, slot_of, a, b, finite=True)


@pytest.mark.parametrize("name", ["loop2", "tx-all", "rx-play-bare"])
def test_row_equals_solo_hop(models, name):
    """row b of a B = 6 object equals the same stream alone in a B = 1 object of the same configuration, exported records
    included; a resume from another stream's record takes the record the big object exported.  (The jitter receiver without
    comfort noise and rooms: the noise seed depends on the slot index, and a room couples slots by design.)"""
    seeds = L.SOLO_SEEDS[name]
    cfg = L.CONFIGS[name]
    model, target = models[name]
    slot_of = L.slot_map(SOLO_SIZE)
    scripts = L.make_scripts(cfg, seeds[0], seeds[1], SOLO_HOPS, SOLO_SIZE)
    trace = lambda where: L.arrivals_for(cfg, seeds[0], seeds[1], where, SOLO_HOPS, SOLO_SIZE) if cfg.kind == "rx_play" else None
    big = L.Driver(cfg, L.make_hop(cfg, model, 2 * SOLO_SIZE, DEV, target), scripts, slot_of, DEV, arrivals=trace(slot_of))
    solos = {s: L.Driver(cfg, L.make_hop(cfg, model, 1, DEV, target), {s: scripts[s]}, {s: 0}, DEV, arrivals=trace({s: 0}),
                         records_from=big) for s in range(SOLO_SIZE)}
    for k in range(SOLO_HOPS):
        big.step()
        for s, solo in solos.items():
            solo.step()
            diff = first_difference(observe(big.hop, slot_of[s]), observe(solo.hop, 0))
            assert diff is None, L.explain("row against solo", cfg, seeds, k, slot_of[s], diff, big)


@pytest.mark.parametrize("name", ["loop1", "tx-plain", "tx-all"])
def test_forced_upload_twin(models, name):
    """one object and a twin with the same scripts; on every hop the twin also queues set_bitrate(slot, its current n) for one slot,
    which uploads the control stage and changes nothing.  All 8 slots stay equal, and the first object skipped its upload on
    exactly the hops the scripts predict (tests/test_lifecycle_cpu.py asserts there are at least 5)"""
    seeds = L.SEEDS[name]
    seeds = (seeds[0], seeds[1], seeds[1])
    cfg, slot_of, (a, b) = drivers_for(name, models, seeds, force_upload=True)
    sent = []
    send = a.hop.stage.send

    def counted(words):
        sent.append(a.k)
        send(words)
    a.hop.stage.send = counted
    for k in range(HOPS):
        a.step()
        b.step()
        for slot in range(2 * SIZE):
            diff = first_difference(observe(a.hop, slot), observe(b.hop, slot))
            assert diff is None, L.explain("forced-upload twin", cfg, seeds, k, slot, diff, a)
    del a.hop.stage.send                                     # the wrapper refers to the driver: a cycle that would keep the hop alive
    skipped = [k for k in range(HOPS) if k not in sent]
    print(f"{name}: uploads skipped on hops {skipped}, predicted {L.skipped_uploads(a.scripts)}")
    assert skipped == L.skipped_uploads(a.scripts)


def test_reset_restores_every_per_slot_state(models):
    """a sender with every option: after 6 hops with a start, a stop, a hold, reports and NACKs, reset() puts every per-slot tensor
    the allocator registered (_slot_state) back to what it held right after construction, bit for bit — the DTX run counter and the
    header's hop counter among them — and the same 6 hops then give the first run's packets, byte counts, indices and views"""
    import torch
    from hilcodec_amd import wire
    from hilcodec_amd.graph_step import GraphedEncodeHop
    from hilcodec_amd.rate import RateConfig
    from hilcodec_amd.rtx import RtxConfig
    model, target = models["tx-all"]
    B, hops = 4, 6
    hop = GraphedEncodeHop(model, B, HOP, L.N, DEV, sessions=True, input_rate=L.INPUT_RATE, fec_stages=L.M, header=True, dtx=L.DTX,
                           vbr=L.vbr_config(target), fec_adapt=L.FEC_ADAPT, rtx=RtxConfig(history=4, per_hop=2),
                           rate=RateConfig(min_kbps=6.0, max_kbps=12.0, start_kbps=6.0, burst_hops=1))
    # every feature's state went through the allocator: previous codes, DTX run, hop counter, credit, adapt row and switch, the
    # three history tensors with the two retransmission outputs, rate row and ceiling
    assert len(hop._scratch) == 13
    fresh = [t.clone() for t, *_ in hop._scratch]
    xs = [synth.synth_clips(B, HOP * L.INPUT_RATE // 24000, seed=50 + k).to(DEV) for k in range(hops)]
    xs[4][0], xs[5][0] = 0.0, 0.0                            # slot 0 ends in silence: its DTX run counter is not 0 at the reset
    views = slot_views(hop) + ["rtx_packets", "rtx_nbytes", "rtx_state", "n_ceil", "rate_state"]

    def run():
        seen = []
        for k in range(hops):
            if k == 1:
                hop.start(2)
            if k == 2:
                hop.stop(1)
            opt = {}
            if k in (2, 4):
                opt["reports"] = ([0, 3], [wire.pack_report(k, 0, 0)] * 2)    # two calm reports: slots 0 and 3 switch FEC off
            if k in (3, 5):
                opt["nacks"] = ([0, 2], [wire.pack_nack(k - 2, 1), wire.pack_nack(0, 3)])
            packets, nbytes = hop.step(xs[k], hold=[3] if k == 3 else None, **opt)
            seen.append([packets.clone(), nbytes.clone(), hop.indices.clone()] + [getattr(hop, name).clone() for name in views])
        return seen

    first = run()
    moved = [not torch.equal(t, f) for (t, *_), f in zip(hop._scratch, fresh)]
    assert all(moved), moved                                 # the comparison below is not empty: every tensor did change
    hop.reset()
    for i, ((t, cleared, _), f) in enumerate(zip(hop._scratch, fresh)):
        assert torch.equal(t, f), f"registered tensor {i} {tuple(t.shape)} {t.dtype} (cleared = {cleared}) differs after reset()"
    assert hop.stopped == ()
    for k, (a, b) in enumerate(zip(first, run())):
        for name, x, y in zip(["packets", "nbytes", "indices"] + views, a, b):
            assert torch.equal(x, y), f"hop {k}: {name} differs on the second run"
