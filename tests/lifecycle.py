"""Random session traffic for the graphed hops (GraphedHop / GraphedEncodeHop / GraphedDecodeHop with sessions=True): per-stream
scripts, the driver that applies them to a hop object, a host-only stand-in for a hop (the dry run of the CPU test) and what the
assertions print.  A plain module like tests/hops.py: no fixtures, nothing runs at import.

A run has `size` probe streams (ids 0 .. size - 1) and `size` neighbour streams (ids 4 .. 4 + size - 1).  Stream s draws its audio
(or packet rows) and its events from np.random.default_rng([seed, s]) alone, so its script is a pure function of (seed, s, config,
hops, size) and does not move when another stream's seed does.  Besides the random stretches every script has three scripted places
(`plan`), by the stream's role r = s % 4, so that what the CPU test demands does not hang on luck:
  * hold window (3 hops): role 2 is held, nobody else has an event — a slot held on hops in a row with nothing else to upload;
  * burst hop: role 0 resumes from its own record (host tensors), role 3 from role 0's (device tensors) and is held on that hop —
    with both classes that is max_loads_per_hop = 4 resumes on one hop, host and device records together, one into a held slot;
  * stop hop, then the quiet window (7 hops): role 1 stops, nobody has an event until the window is over, role 1 starts again
    0-3 hops after it.  That pair is 8-11 hops apart, so it counts as "stop_scripted" / "restart_scripted", apart from the
    random stops, which a start follows 1-4 hops later."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from hilcodec_amd import dtx, jitter, report, synth, wire
from hilcodec_amd.jitter import AdaptConfig, JitterConfig, JitterModel
from hilcodec_amd.mixer import MixConfig
from hilcodec_amd.report import FecAdaptConfig, FecAdaptModel, ReportConfig, ReportModel
from hilcodec_amd.sessions import SessionQueue

N, M, K = 8, 2, 8                     # stages, redundant stages, comfort-noise order
NEIGHBOUR = 4                         # the first neighbour stream's id
MAX_LOADS = 4                         # max_loads_per_hop of every object (the constructor's default)
DTX = dtx.DtxConfig(threshold_db=-50.0, hangover=1, sid_interval=2)
FEC_ADAPT = FecAdaptConfig(on_q8=8, off_q8=3, calm_reports=2, timeout_hops=12)
JITTER = JitterConfig(2, 8, adapt=AdaptConfig())
REPORT = ReportConfig(8, 4)
INPUT_RATE = OUTPUT_RATE = 48000


@dataclass(frozen=True)
class Config:
    """one row of the configuration table: `kind` "loop" (GraphedHop), "tx" (GraphedEncodeHop), "rx_step" / "rx_play"
    (GraphedDecodeHop through step() / play()); `full`: every option of a sender; `cng` / `mix`: a jitter receiver's"""
    name: str
    kind: str
    groups: int = 1
    full: bool = False
    cng: bool = True
    mix: bool = True

    @property
    def has_n(self) -> bool:          # start(n=) and set_bitrate exist
        return self.kind in ("loop", "tx")

    @property
    def n_min(self) -> int:
        return M if self.full else 1

    @property
    def reports(self) -> bool:
        return self.kind == "tx" and self.full

    @property
    def rooms(self) -> bool:
        return self.kind == "rx_play" and self.mix

    @property
    def samples(self) -> int:         # a hop's input samples per stream (the 48 kHz sender: 640)
        return 640 if self.kind == "tx" and self.full else 320

    def kinds(self) -> Tuple[str, ...]:
        """the event kinds a script of this configuration can hold"""
        k = ["fresh", "resume_host", "resume_dev", "hold", "stop", "restart"]
        if self.has_n:
            k += ["fresh_n", "bitrate"]
        if self.reports:
            k += ["report_calm", "report_lossy"]
        if self.kind == "rx_step":
            k += ["lost", "fec", "sid", "silent"]
        if self.rooms:
            k += ["join", "leave"]
        return tuple(k)


CONFIGS = {c.name: c for c in (
    Config("loop1", "loop"), Config("loop2", "loop", groups=2), Config("tx-plain", "tx"), Config("tx-all", "tx", full=True),
    Config("rx-step", "rx_step"), Config("rx-play", "rx_play"), Config("rx-play-bare", "rx_play", cng=False, mix=False))}

# per configuration: the probes' seed and the neighbours' seed in the first and in the second object.  Chosen so that the coverage
# conditions of tests/test_lifecycle_cpu.py hold (they are conditions, asserted there for exactly these seeds)
SEEDS = {"loop1": (2, 9, 10), "loop2": (2, 9, 10), "tx-plain": (2, 9, 10), "tx-all": (2, 3, 4), "rx-step": (1, 2, 3),
         "rx-play": (4, 5, 6), "rx-play-bare": (4, 5, 6)}
# the same for test_row_equals_solo_hop's objects (30 hops, three streams per class): the probes' seed and the neighbours'
SOLO_SEEDS = {"loop2": (1, 2), "tx-all": (8, 9), "rx-play-bare": (1, 2)}
# the jitter receiver's networks (tests/test_gpu_jitter_adapt.Network, one per class, four senders each): rates at which a 40-hop
# run moves every counter on a probe slot.  Slot 2 of a class is the fast sender (b % 3 == 2) and the stream the hold window holds
NETWORK = dict(loss=0.12, delay=5, dup=0.08, bad=0.06, sid=0.08, restart=0.03, every=5, mild=False)


def plan(hops: int) -> Dict[str, int]:
    """the scripted places of a run of `hops` hops (module docstring)"""
    hold0, quiet0 = (35 * hops) // 100, (6 * hops) // 10
    return dict(hold0=hold0, hold1=hold0 + 3, burst=hops // 2, stop=quiet0 - 1, quiet0=quiet0, quiet1=quiet0 + 7)


@dataclass
class Ev:
    """what one stream does on one hop"""
    start: Optional[tuple] = None     # ("fresh", n or None) / ("resume", source stream, age in hops, "host" / "dev", n or None)
    restart: bool = False             # that start ends a stop
    scripted: bool = False            # the stop in front of the quiet window or the start behind it: 8-11 hops apart, not 1-4
    stop: bool = False
    hold: bool = False
    bitrate: Optional[int] = None
    report: Optional[Tuple[int, int, int]] = None
    rx: Optional[str] = None          # "lost" / "fec" / "sid" / "silent"
    room: Optional[tuple] = None      # ("join", room) / ("leave",)

    def kinds(self) -> List[str]:
        out = []
        if self.start is not None:
            if self.restart:
                out.append("restart_scripted" if self.scripted else "restart")
            elif self.start[0] == "fresh":
                out.append("fresh" if self.start[1] is None else "fresh_n")
            else:
                out.append("resume_" + self.start[3])
        out += ["stop_scripted" if self.scripted else "stop"] * self.stop + ["hold"] * self.hold + ["bitrate"] * (self.bitrate is not None)
        if self.report is not None:
            out.append("report_lossy" if self.report[1] >= FEC_ADAPT.on_q8 else "report_calm" if self.report[1] <= FEC_ADAPT.off_q8
                       else "report_between")
        if self.rx is not None:
            out.append(self.rx)
        if self.room is not None:
            out.append(self.room[0])
        return out

    def __str__(self) -> str:
        parts = [f"{k}={v}" for k, v in vars(self).items() if v not in (None, False)]
        return " ".join(parts) or "-"


@dataclass
class Script:
    stream: int
    events: List[Ev]
    data: Dict[str, np.ndarray] = field(default_factory=dict)     # "audio" [hops, samples] fp32, or "rows" [hops, stride] u8 and "n" [hops]

    def digest(self) -> bytes:
        """everything the script holds, as bytes: two scripts are the same script iff their digests are equal"""
        return (repr(self.events) + "".join(f"{k}{v.dtype}{v.shape}" for k, v in sorted(self.data.items()))).encode() + \
            b"".join(np.ascontiguousarray(v).tobytes() for _k, v in sorted(self.data.items()))


def class_base(stream: int) -> int:
    return NEIGHBOUR if stream >= NEIGHBOUR else 0


def make_script(seed: int, stream: int, cfg: Config, hops: int = 40, size: int = 4) -> Script:
    rng = np.random.default_rng([seed, stream])
    base, role = class_base(stream), stream % 4
    P = plan(hops)
    fixed = sorted((P["hold0"], P["burst"], P["stop"]))
    rooms = [base // NEIGHBOUR, base // NEIGHBOUR + 2]       # probes share rooms 0 and 2, neighbours 1 and 3
    n_of = lambda: int(rng.integers(cfg.n_min, N + 1))
    events = [Ev() for _ in range(hops)]
    stopped, restart_at, held, seq, where = False, -1, False, int(rng.integers(0, 256)), stream % 2
    in_dtx = long_stop = False
    for k, e in enumerate(events):
        if P["hold0"] <= k < P["hold1"]:
            e.hold = held = role == 2
            continue
        if P["quiet0"] <= k < P["quiet1"]:
            held = False
            continue
        if k == P["burst"]:
            held = False
            if role == 0:
                e.start = ("resume", stream, 2, "host", None)
            elif role == 3:
                e.start = ("resume", base, 1, "dev", None)
                e.hold = held = True
            continue
        if k == P["stop"]:
            held = False
            if role == 1:
                e.stop, e.scripted, stopped, restart_at, long_stop = True, True, True, P["quiet1"] + int(rng.integers(0, 4)), True
            continue
        if stopped:
            if k == restart_at:
                e.start, e.restart, stopped = ("fresh", n_of() if cfg.has_n and rng.random() < 0.5 else None), True, False
                e.scripted, long_stop = long_stop, False
            continue
        e.hold = held = bool(rng.random() < (0.5 if held else 0.08))
        u = float(rng.random())
        ahead = [f for f in fixed if f > k]
        if u < 0.05:
            e.start = ("fresh", None)
        elif u < 0.10 and cfg.has_n:
            e.start = ("fresh", n_of())
        elif u < 0.20 and k >= 5:
            own = size == 1 or rng.random() < 0.5
            src = stream if own else base + (stream - base + 1 + int(rng.integers(0, size - 1))) % size
            age = int(rng.integers(2, 5)) if own else 1
            e.start = ("resume", src, age, ("host", "dev")[where], n_of() if cfg.has_n and rng.random() < 0.5 else None)
            where ^= 1
        elif u < 0.25 and (not ahead or k + 4 < ahead[0]):
            e.stop, stopped, restart_at = True, True, k + int(rng.integers(1, 5))
        elif u < 0.33 and cfg.has_n:
            e.bitrate = n_of()
        if cfg.reports and rng.random() < 0.2:
            seq = (seq + 1) & 255
            loss = int(rng.choice([0, FEC_ADAPT.off_q8, FEC_ADAPT.off_q8 + 1, FEC_ADAPT.on_q8 - 1, FEC_ADAPT.on_q8, 40]))
            e.report = (seq, loss, int(rng.integers(0, loss + 1)))
        if cfg.kind == "rx_step" and not e.hold and not e.stop:
            v = float(rng.random())
            e.rx = "lost" if v < 0.08 else "fec" if v < 0.16 else "sid" if v < 0.22 else "silent" if v < (0.55 if in_dtx else 0.26) else None
            in_dtx = e.rx in ("sid", "silent")
        if cfg.rooms:
            v = float(rng.random())
            if v < 0.10:
                e.room = ("join", rooms[int(rng.integers(0, 2))])
            elif v < 0.16:
                e.room = ("leave",)
    data = {}
    if cfg.kind in ("loop", "tx"):
        S = cfg.samples
        if cfg.full:
            # speech-like clips with silent stretches, so that VBR and DTX have something to decide
            x = synth.synth_clips(1, S * hops, seed=int(rng.integers(0, 1 << 30)))[0, 0].numpy().reshape(hops, S).copy()
            gain, left = np.ones(hops, dtype=np.float32), 0
            for k in range(hops):
                if left == 0 and rng.random() < 0.12:
                    left = int(rng.integers(3, 5))
                if left:
                    gain[k], left = 3e-5, left - 1
            data["audio"] = x * gain[:, None]
        else:
            data["audio"] = (0.1 * rng.standard_normal((hops, S))).astype(np.float32)
    elif cfg.kind == "rx_step":
        stride = wire.packet_bytes(N + M, 1)
        rows, ns = np.zeros((hops, stride), dtype=np.uint8), np.zeros(hops, dtype=np.int64)
        for k, e in enumerate(events):
            ns[k] = int(rng.integers(M, N + 1))
            if e.rx == "sid":
                blob = rng.integers(0, 256, dtx.sid_bytes(K)).astype(np.uint8).tobytes()
            else:
                blob = wire.pack_stream_packet(torch.from_numpy(rng.integers(0, 1024, (int(ns[k]) + M, 1))))
            rows[k, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        data["rows"], data["n"] = rows, ns
    return Script(stream, events, data)


def make_scripts(cfg: Config, probe_seed: int, neighbour_seed: int, hops: int = 40, size: int = 4) -> Dict[int, Script]:
    """the scripts of one object: probes 0 .. size - 1 from `probe_seed`, neighbours 4 .. 4 + size - 1 from `neighbour_seed`"""
    out = {s: make_script(probe_seed, s, cfg, hops, size) for s in range(size)}
    out.update({s: make_script(neighbour_seed, s, cfg, hops, size) for s in range(NEIGHBOUR, NEIGHBOUR + size)})
    return out


def slot_map(size: int = 4) -> Dict[int, int]:
    """probes on the even slots, neighbours on the odd ones"""
    m = {s: 2 * s for s in range(size)}
    m.update({NEIGHBOUR + j: 2 * j + 1 for j in range(size)})
    return m


# ---------------------------------------------------------------- the jitter receiver's arrivals
def network_trace(seed: int, hops: int, size: int = 4):
    """per hop (network slots, packets uint8 [A, tbytes], byte counts) of one class's senders: one Network, events left to the scripts"""
    from tests.hops import Network
    net = Network(size, N, M, K, 1, seed=seed, **NETWORK)
    return [net.hop()[:3] for _ in range(hops)]


def merge_traces(parts, hops: int):
    """`parts`: (trace, {network slot: hop slot}) pairs -> per hop (slots, packets, byte counts) of the hop object; arrivals of
    network slots that are not mapped are dropped"""
    out = []
    for k in range(hops):
        slots, rows, nbytes = [], [], []
        for trace, where in parts:
            sl, pk, nb = trace[k]
            for a, b in enumerate(sl):
                if int(b) in where:
                    slots.append(where[int(b)])
                    rows.append(pk[a])
                    nbytes.append(int(nb[a]))
        width = parts[0][0][0][1].shape[1]
        out.append((slots, np.stack(rows) if rows else np.zeros((0, width), dtype=np.uint8), nbytes))
    return out


def arrivals_for(cfg: Config, probe_seed: int, neighbour_seed: int, slot_of: Dict[int, int], hops: int, size: int = 4):
    """the merged arrival trace of an object whose streams sit at `slot_of` (streams missing from it: dropped)"""
    parts = []
    for seed, base in ((probe_seed, 0), (neighbour_seed, NEIGHBOUR)):
        where = {s - base: slot for s, slot in slot_of.items() if class_base(s) == base}
        if where:
            parts.append((network_trace(seed, hops, size), where))
    return merge_traces(parts, hops)


# ---------------------------------------------------------------- the objects
def vbr_config(target_db: float):
    from hilcodec_amd.vbr import VbrConfig
    return VbrConfig(target_db, cap_kbps=0.75 * ((3 * N) // 4), burst_hops=2)


def max_arrivals(batch: int) -> int:
    """room for a hop's arrivals (the default, 2 B, is 2 for a stream alone: one delayed packet beside a duplicated one is 3); it
    sizes the staging buffer and nothing else"""
    return 4 * batch + 8


def make_hop(cfg: Config, model, batch: int, device, target_db: Optional[float] = None):
    """the hop object of a configuration (`target_db`: the VBR target of the sender with every option)"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop, GraphedHop
    if cfg.kind == "loop":
        return GraphedHop(model, batch, 320, N, device, sessions=True, groups=cfg.groups)
    if cfg.kind == "tx" and not cfg.full:
        return GraphedEncodeHop(model, batch, 320, N, device, sessions=True)
    if cfg.kind == "tx":
        return GraphedEncodeHop(model, batch, 320, N, device, sessions=True, input_rate=INPUT_RATE, fec_stages=M, header=True, dtx=DTX,
                                vbr=vbr_config(target_db), fec_adapt=FEC_ADAPT)
    rx = dict(sessions=True, conceal=True, fec_stages=M, output_rate=OUTPUT_RATE)
    if cfg.kind == "rx_step":
        return GraphedDecodeHop(model, batch, 1, N, device, cng_order=K, **rx)
    return GraphedDecodeHop(model, batch, 1, N, device, jitter=JITTER, report=REPORT, cng_order=K if cfg.cng else None,
                            mix=MixConfig(2) if cfg.mix else None, max_arrivals=max_arrivals(batch), **rx)


# ---------------------------------------------------------------- the driver
def _poisoned(t):
    t = t.clone()
    flat = t.view(-1)
    flat[0], flat[flat.numel() // 2], flat[-1] = float("nan"), float("-inf"), float("inf")
    return t


class Driver:
    """applies hop k of `scripts` ({stream: Script}) to `hop` with `slot_of` ({stream: slot}); keeps every stream's export() of the
    last hops (`history[stream][k]`: after hop k) for the resumes.  `records_from`: the driver whose history serves the resumes
    from ANOTHER stream's record (a solo object has no other stream).  `arrivals`: the jitter receiver's merged trace.
    `poison_audio` / `poison_records`: streams whose audio carries +Inf, -Inf and NaN on every third hop / whose resumes load
    records with NaN and Inf written into every cache.  `force_upload`: on every hop also queue set_bitrate(slot, its current n)
    for slot k mod B, which uploads and changes nothing."""

    def __init__(self, cfg: Config, hop, scripts: Dict[int, Script], slot_of: Dict[int, int], device, records_from=None,
                 arrivals=None, poison_audio=(), poison_records=(), force_upload=False):
        self.cfg, self.hop, self.scripts, self.slot_of, self.device = cfg, hop, scripts, slot_of, device
        self.records_from, self.arrivals, self.force_upload = records_from, arrivals, force_upload
        self.poison_records = set(poison_records)
        self.batch = hop.queue.batch
        self.hops = len(next(iter(scripts.values())).events)
        self.stream_at = {slot: s for s, slot in slot_of.items()}
        self.history = {s: {} for s in scripts}
        self.cur_n = {s: N for s in scripts}
        self.k = 0
        B = self.batch
        if cfg.kind in ("loop", "tx"):
            x = np.zeros((self.hops, B, 1, cfg.samples), dtype=np.float32)
            for s, sc in scripts.items():
                x[:, slot_of[s], 0] = sc.data["audio"]
                if s in poison_audio:
                    for k in range(1, self.hops, 3):
                        x[k, slot_of[s], 0, [5, 77, 200]] = [np.inf, -np.inf, np.nan]
            self.x = torch.from_numpy(x).to(device)
        elif cfg.kind == "rx_step":
            stride = wire.packet_bytes(N + M, 1)
            self.rows, self.n_rows = np.zeros((self.hops, B, stride), dtype=np.uint8), np.full((self.hops, B), N, dtype=np.int64)
            for s, sc in scripts.items():
                self.rows[:, slot_of[s]], self.n_rows[:, slot_of[s]] = sc.data["rows"], sc.data["n"]

    def events(self, k: int) -> str:
        """hop k's events of every slot, for a failing assertion"""
        return "; ".join(f"slot {slot} (stream {s}): {self.scripts[s].events[k]}" for slot, s in sorted(self.stream_at.items()))

    def _record(self, stream: int, src: int, k: int, age: int, where: str):
        source = self if src == stream or self.records_from is None else self.records_from
        rec = source.history[src][k - age]
        lists = rec if self.cfg.kind == "loop" else (rec,)
        if stream in self.poison_records:
            lists = tuple([_poisoned(t) for t in lst] for lst in lists)
        if where == "host":
            lists = tuple([t.cpu() for t in lst] for lst in lists)
        return lists

    def _start(self, stream: int, slot: int, ev: Ev, k: int) -> None:
        st = ev.start
        n = st[-1]
        kw = {"n": n} if self.cfg.has_n and n is not None else {}
        if st[0] == "fresh":
            self.hop.start(slot, **kw)
        else:
            self.hop.start(slot, *self._record(stream, st[1], k, st[2], st[3]), **kw)
        self.cur_n[stream] = N if n is None else n

    def step(self) -> None:
        k, hop, cfg = self.k, self.hop, self.cfg
        holds, rep_slots, blobs = [], [], []
        rx = {"lost": [], "fec": [], "sid": [], "silent": []}
        for s, sc in self.scripts.items():
            ev, slot = sc.events[k], self.slot_of[s]
            if ev.stop:
                hop.stop(slot)
            if ev.start is not None:
                self._start(s, slot, ev, k)
            if ev.bitrate is not None:
                hop.set_bitrate(slot, ev.bitrate)
                self.cur_n[s] = ev.bitrate
            if ev.hold:
                holds.append(slot)
            if ev.report is not None:
                rep_slots.append(slot)
                blobs.append(wire.pack_report(*ev.report))
            if ev.rx is not None:
                rx[ev.rx].append(slot)
            if ev.room is not None:
                hop.join(slot, ev.room[1]) if ev.room[0] == "join" else hop.leave(slot)
        if self.force_upload and k % self.batch in self.stream_at:
            hop.set_bitrate(k % self.batch, self.cur_n[self.stream_at[k % self.batch]])
        if cfg.kind == "loop" or (cfg.kind == "tx" and not cfg.reports):
            hop.step(self.x[k], hold=holds)
        elif cfg.kind == "tx":
            hop.step(self.x[k], hold=holds, reports=(rep_slots, blobs) if rep_slots else None)
        elif cfg.kind == "rx_step":
            hop.step(torch.from_numpy(self.rows[k]), self.n_rows[k].tolist(), hold=holds, **rx)
        else:
            slots, packets, nbytes = self.arrivals[k]
            hop.play(slots, torch.from_numpy(packets), nbytes, hold=holds)
        for s, slot in self.slot_of.items():
            h = self.history[s]
            h[k] = hop.export(slot)
            h.pop(k - 6, None)
        self.k += 1


# ---------------------------------------------------------------- what the scripts predict (host only)
def held_sets(scripts: Dict[int, Script]) -> List[frozenset]:
    """per hop the streams that are held: this hop's holds and everything stopped"""
    hops = len(next(iter(scripts.values())).events)
    out, stopped = [], set()
    for k in range(hops):
        for s, sc in scripts.items():
            if sc.events[k].stop:
                stopped.add(s)
            if sc.events[k].start is not None:
                stopped.discard(s)
        out.append(frozenset(stopped | {s for s, sc in scripts.items() if sc.events[k].hold}))
    return out


def skipped_uploads(scripts: Dict[int, Script]) -> List[int]:
    """the hops on which GraphedHop._upload takes its early return: no start or bitrate now, no start on the previous hop (its
    action row is still live), the held set as on the previous hop, no report now or on the previous hop"""
    held = held_sets(scripts)
    any_of = lambda k, what: k >= 0 and any(what(sc.events[k]) for sc in scripts.values())
    start = lambda e: e.start is not None
    out = []
    for k in range(len(held)):
        if any_of(k, start) or any_of(k, lambda e: e.bitrate is not None) or any_of(k - 1, start):
            continue
        if held[k] != (held[k - 1] if k else frozenset()):
            continue
        if any_of(k, lambda e: e.report is not None) or any_of(k - 1, lambda e: e.report is not None):
            continue
        out.append(k)
    return out


def held_again_quietly(scripts: Dict[int, Script]) -> List[int]:
    """the hops of skipped_uploads on which a stream is held by `hold` as on the hop before: the device's hold row must still mark it"""
    return [k for k in skipped_uploads(scripts)
            if k and any(sc.events[k].hold and sc.events[k - 1].hold for sc in scripts.values())]


def kind_counts(scripts: Dict[int, Script], streams) -> Dict[str, int]:
    out: Dict[str, int] = {}
    for s in streams:
        for e in scripts[s].events:
            for kind in e.kinds():
                out[kind] = out.get(kind, 0) + 1
    return out


def cross_resumes(scripts: Dict[int, Script], streams) -> Dict[str, int]:
    """{"host" / "dev": resumes of `streams` from ANOTHER stream's record, handed over that way}"""
    out = {"host": 0, "dev": 0}
    for s in streams:
        for e in scripts[s].events:
            if e.start is not None and e.start[0] == "resume" and e.start[1] != s:
                out[e.start[3]] += 1
    return out


def fec_switch_changes(scripts: Dict[int, Script], streams) -> int:
    """how often report.FecAdaptModel moves the switch of one of `streams` under the scripts' reports, starts and holds"""
    order = sorted(scripts)
    model = FecAdaptModel(len(order), FEC_ADAPT, M, 1)
    held = held_sets(scripts)
    before, changes = model.state[:, report.FA_ON].copy(), 0
    for k in range(len(held)):
        ev = [scripts[s].events[k] for s in order]
        words = [0 if e.report is None else report.report_word(*e.report) for e in ev]
        on = model.step(words, [int(e.start is not None) for e in ev], [int(s in held[k]) for s in order])
        changes += sum(int(on[i] != before[i]) for i, s in enumerate(order) if s in streams)
        before = on
    return changes


# ---------------------------------------------------------------- the dry run: a hop object without a device
class _FakeCache:
    """stands for a cache tensor in a dry run: only where it lives matters"""

    def __init__(self, is_cuda: bool):
        self.is_cuda = is_cuda

    def cpu(self):
        return _FakeCache(False)


class _FakeLayout:
    def record(self, cache_enc, cache_dec):
        return (list(cache_enc) + list(cache_dec))[0]


class DryHop:
    """the host side of a hop object and nothing else: a sessions.SessionQueue behind the methods the Driver calls, with the
    argument checks of the real step() / play() in the same order, so that a script set that passes here raises nothing there.
    Counts what the coverage conditions ask for; a jitter receiver also runs jitter.JitterModel and report.ReportModel."""

    def __init__(self, cfg: Config, batch: int):
        self.cfg, self.batch = cfg, batch
        self.queue = SessionQueue(batch, N, MAX_LOADS, _FakeLayout(), one_sided=cfg.kind != "loop")
        self.queue.n_min = cfg.n_min
        self.loads: List[Tuple[int, int]] = []               # per hop (host records, device records)
        self.resumes_into_held = 0
        self.rooms = [-1] * batch
        if cfg.kind == "rx_play":
            self.max_arrivals = max_arrivals(batch)
            self.jitter = JitterModel(batch, JITTER, N, M, 1, K if cfg.cng else None, True)
            self.report = ReportModel(batch, REPORT)
            self.due = np.zeros(batch, dtype=np.int64)
            self.stat_seen = np.zeros((batch, jitter.ST_WORDS), dtype=np.int64)        # the most every counter reached
            self.adapt_seen = np.zeros((batch, jitter.AD_WORDS), dtype=np.int64)

    def start(self, slot, a=None, b=None, n=None):
        if self.cfg.kind == "loop":
            self.queue.start(slot, a, b, n)
        elif self.cfg.kind == "tx":
            self.queue.start(slot, a, None, n)
        else:
            assert b is None and n is None
            self.queue.start(slot, None, a)

    def stop(self, slot):
        self.queue.stop(slot)

    def set_bitrate(self, slot, n):
        assert self.cfg.has_n
        self.queue.set_bitrate(slot, n)

    def join(self, slot, room):
        assert self.cfg.rooms and 0 <= int(room) < self.batch
        self.rooms[self.queue.slot(slot)] = int(room)

    def leave(self, slot):
        assert self.cfg.rooms
        self.rooms[self.queue.slot(slot)] = -1

    def export(self, slot):
        self.queue.slot(slot)
        return ([_FakeCache(True)], [_FakeCache(True)]) if self.cfg.kind == "loop" else [_FakeCache(True)]

    def _taken(self, held) -> np.ndarray:
        """the queue as the upload takes it: counts, then the action row (1: a start of any kind)"""
        q = self.queue
        recs = [r for r in q.starts.values() if r is not None]
        assert len(recs) <= MAX_LOADS
        self.loads.append((sum(not r.is_cuda for r in recs), sum(r.is_cuda for r in recs)))
        self.resumes_into_held += sum(r is not None and s in held for s, r in q.starts.items())
        action = np.zeros(self.batch, dtype=np.int32)
        action[list(q.starts)] = 1
        q.clear()
        return action

    def step(self, x, n_per_stream=None, hold=None, reports=None, lost=None, fec=None, sid=None, silent=None):
        q, B = self.queue, self.batch
        held = [q.slot(s) for s in SessionQueue.host_slots(hold)]
        if self.cfg.kind in ("loop", "tx"):
            assert tuple(x.shape) == (B, 1, self.cfg.samples) and n_per_stream is None
            if reports is not None:
                assert self.cfg.reports
                slots, blobs = reports
                assert len(slots) == len(blobs) and all(0 <= s < B for s in slots)
                for blob in blobs:
                    report.report_word(*wire.parse_report(blob))
            q.hold(held)
            self._taken(q.held)
            return
        gone = q.lost_slots(SessionQueue.host_slots(lost), held)
        red = q.fec_slots(SessionQueue.host_slots(fec), held, gone)
        sids, quiet = q.cn_slots(SessionQueue.host_slots(sid), SessionQueue.host_slots(silent), held, gone, red)
        all_held = set(held) | q.stops
        unread = all_held | set(gone) | set(sids) | set(quiet)
        assert len(n_per_stream) == B and all(1 <= v <= N for b, v in enumerate(n_per_stream) if b not in unread)
        assert all(n_per_stream[b] >= M for b in red)
        assert x.dtype == torch.uint8 and tuple(x.shape) == (B, wire.packet_bytes(N + M, 1))
        self._taken(all_held)

    def play(self, slots, packets, nbytes, hold=None):
        q, B = self.queue, self.batch
        held = {q.slot(s) for s in SessionQueue.host_slots(hold)} | q.stops
        A = len(slots)
        assert A <= self.max_arrivals and len(nbytes) == A and all(0 <= s < B for s in slots)
        assert packets.dtype == torch.uint8 and tuple(packets.shape) == (A, wire.transport_bytes(N, M, 1))
        action = self._taken(held)
        hold_row = np.zeros(B, dtype=np.int32)
        hold_row[sorted(held)] = 1
        self.jitter.step(action, hold_row, slots, packets.numpy(), nbytes)
        self.due += self.report.step(self.jitter.state, action)["due"]
        self.stat_seen = np.maximum(self.stat_seen, self.jitter.state)
        self.adapt_seen = np.maximum(self.adapt_seen, self.jitter.adapt)


# ---------------------------------------------------------------- what a failing assertion prints
def explain(what: str, cfg: Config, seeds, k: int, slot: int, diff: str, driver: Driver, other: Optional[Driver] = None) -> str:
    text = f"{what} [{cfg.name}, seeds {seeds}] hop {k}, slot {slot}: {diff}\n  events: {driver.events(k)}"
    if other is not None:
        text += f"\n  other object's events: {other.events(k)}"
    return text
