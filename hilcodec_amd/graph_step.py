"""HIP-graph replay of one streaming hop (encoder -> RVQ -> dequantiser -> decoder with all 52 caches) over a
persistent, ping-pong state block in HBM.

A hop for 1024 streams is ~60 kernel launches of 30-400 us each; the hop is shape-static, so it is captured once into
a graph whose inputs (the hop's samples, the caches) and outputs live at fixed addresses, and a replay is one launch.

State: every cache exists twice, as views into two contiguous HBM blocks A and B (22 + 30 caches per stream, 313 MB
per block at 1024 streams).  The reference returns the new caches as fresh tensors (`streaming.py:482-517,619-648`);
here the kernels of an even hop read A and write B, those of an odd hop read B and write A (`cache_out=` of the
streaming Encoder / Decoder), so a hop moves no cache bytes beyond what its kernels read and write — no allocation, no
copy-back.  Two graphs are captured (A->B and B->A) and replayed alternately.

The captured kernels are the same launches the eager path issues (same custom ops on the capture stream), so a
replayed hop is bit-identical to an eager hop (tests/test_gpu_streaming.py).  The graph is not a pure chain: the
log-magnitude spectra of the un-fused SpecBlocks (n_fft 256 / 512 / 1024 at one hop: small launches that depend on the
waveform only) sit on a second branch beside the first encoder stages (`engine._early_spectra`)."""
from __future__ import annotations

import gc
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import dtx as dtx_def
from . import audio_level as level_def
from . import bwe as bwe_def
from . import srtp as srtp_def
from . import engine, ops, wire
from . import downlink as downlink_def
from . import forward as forward_def
from . import forward_srtp as fsrtp_def
from . import rate as rate_def
from . import report as report_def
from . import rtx as rtx_def
from . import vbr as vbr_def
from .jitter import AD_WORDS, ST_WORDS, JitterConfig
from .mixer import MixConfig
from .resample import BASE_RATE, HOP, design, device_taps, hop_samples
from .sessions import (HOLD_SID, HOLD_SILENT, ONE_HOP_ROWS, Arrivals, SessionQueue, arrival_bytes, arrival_region_words, arrival_width,
                       check_arrivals, put_arrivals, stage_layout, stage_starts)


def state_layout(model, batch: int, side: str = "both", history: int = 0) -> ops.StateLayout:
    """the layout of a state block of `batch` streams of `model` (host-only: the cache shapes come from a CPU probe); `side`
    "enc" / "dec": a one-sided block of the 22 encoder or the 30 decoder caches only (its records hold that side only).
    `history` > 0 (one-sided only): one more cache `[batch, 1, history]` after that side's last, the resampler's input history
    (GraphedEncodeHop(input_rate=), GraphedDecodeHop(output_rate=))"""
    if side not in ("both", "enc", "dec"):
        raise ValueError(f"side must be 'both', 'enc' or 'dec', got {side!r}")
    if history and side == "both":
        raise ValueError("state_layout: a resampler history belongs to a one-sided block")
    ce, cd = model.initialize_cache(torch.zeros(1, 1, 1))
    shapes = [tuple(c.shape[1:]) for c in (ce if side != "dec" else [])]
    shapes_dec = [tuple(c.shape[1:]) for c in (cd if side != "enc" else [])]
    if history:
        (shapes if side == "enc" else shapes_dec).append((1, int(history)))
    return ops.StateLayout([(batch,) + sh for sh in shapes + shapes_dec], len(shapes))


def _int_arg(name: str, value, lo: int, hi: Optional[int] = None) -> int:
    """an argument that must be an int (not a bool) in [lo, hi], or >= lo without `hi`: ValueError otherwise"""
    if isinstance(value, bool) or int(value) != value or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} must be an int {f'>= {lo}' if hi is None else f'in [{lo}, {hi}]'}, got {value!r}")
    return int(value)


def _whole_frames(who: str, hop: int) -> int:
    """the frames of a hop of `hop` samples at 24 kHz, for an option `who` that works on whole 320-sample frames"""
    if hop % HOP:
        raise ValueError(f"{who}: hop must be a multiple of {HOP}, got {hop}")
    return hop // HOP


def _fec_stages(fec_stages, n: int) -> int:
    """the `fec_stages` argument of the sender and the receiver checked: 0 (no FEC) or an int m in [1, n] with n + m <= 32 (the
    most stages one packet holds, as hilc_rvq_decode_packed)"""
    m = _int_arg("fec_stages", fec_stages, 0, int(n))
    if int(n) + m > wire.MAX_STAGES:
        raise ValueError(f"fec_stages = {m}: a packet holds at most {wire.MAX_STAGES} stages, n + m = {int(n) + m}")
    return m


def _config_arg(name: str, value, cls):
    """an option that must be None or an instance of the config class `cls`: ValueError otherwise"""
    if value is not None and not isinstance(value, cls):
        raise ValueError(f"{name} must be a {cls.__module__.rsplit('.', 1)[-1]}.{cls.__name__} or None, got {value!r}")
    return value


def _needs(who: str, have, what: str) -> None:
    """the option `who` (as a constructor call shows it) works only with `what`: ValueError unless `have`"""
    if not have:
        raise ValueError(f"{who} needs {what}")


def _mark(row: Tensor, slots) -> None:
    """a pinned int32 control row that is not a one-hop row (hold, lost, fec): 1 at `slots`, 0 elsewhere"""
    row.zero_()
    if slots:
        row[torch.tensor(sorted(slots), dtype=torch.long)] = 1


class StateBlock:
    """The 22 + 30 caches of `batch` streams as views into ONE contiguous fp32 buffer (16-B aligned slices); `side` "enc" /
    "dec": one side's caches only (the other list is empty).  `history` > 0: that side's list ends with the resampler's history
    `[batch, 1, history]` (`hist`); `codec_enc` / `codec_dec` are the model's caches alone."""

    def __init__(self, model, batch: int, device: torch.device, side: str = "both", history: int = 0):
        self.layout = state_layout(model, batch, side, history)
        self.buffer = torch.zeros(self.layout.total, device=device, dtype=torch.float32)
        views = [self.buffer[o:o + s[0] * n].view(s) for s, o, n in zip(self.layout.shapes, self.layout.off, self.layout.lens)]
        self.enc: List[Tensor] = views[:self.layout.n_enc]
        self.dec: List[Tensor] = views[self.layout.n_enc:]
        self.hist: Optional[Tensor] = None
        self.codec_enc, self.codec_dec = self.enc, self.dec
        if history:
            self.hist = views[-1] if side == "dec" else self.enc[-1]
            if side == "dec":
                self.codec_dec = self.dec[:-1]
            else:
                self.codec_enc = self.enc[:-1]

    def zero_(self) -> None:
        self.buffer.zero_()

    def load_(self, cache_enc: Optional[Sequence[Tensor]], cache_dec: Optional[Sequence[Tensor]]) -> None:
        for dst, src in ((self.enc, cache_enc), (self.dec, cache_dec)):
            for i, c in enumerate(dst):
                c.zero_() if src is None else c.copy_(src[i])

    @property
    def nbytes(self) -> int:
        return self.buffer.numel() * 4


class ControlStage:
    """A hop's control data: ONE device buffer, captured by address, and its pinned host mirror, laid out as int32 rows per slot |
    payload | staged records (sessions.stage_layout), so that what a hop needs goes up in one copy.  `row[name]` / `h_row[name]` are
    the `[B]` int32 rows on the device / in the mirror, `payload` / `h_payload` and `records` / `h_records` the two regions.
    A hop's upload is: `wait()`, write the mirror (`put_starts` for the queued starts), `send(words)`, `finish(...)`.
    `sent_words` / `sent_record_words`: the words of the last upload's pinned copy / of its host records' own copy.
    The rows among sessions.ONE_HOP_ROWS apply to exactly one hop: they are written with `put_one_hop`, and `one_hop_live` says
    whether one of them still holds entries on the device, so that the next upload has to clear it.
    `arrivals` = (max_arrivals, row_bytes): the payload is an arrival region (sessions.arrival_region_words) — `offsets` /
    `h_offsets` int32 `[B + 1]` and `arrivals` / `h_arrivals` int32 `[max_arrivals, arrival_width]` — which `send_arrivals` sends;
    `times=True`: the region also carries `times` / `h_times` int32 `[max_arrivals]`, the arrival ticks parallel to the records."""

    def __init__(self, batch: int, rows: Sequence[str], payload_words: int, loads: int, record_len: int, device: torch.device,
                 arrivals: Optional[Tuple[int, int]] = None, times: bool = False):
        if times and arrivals is None:
            raise ValueError("ControlStage: arrival times belong to an arrival region")
        n_times = arrivals[0] if times else 0
        if arrivals is not None:
            if payload_words:
                raise ValueError("ControlStage: the arrival region is the whole payload, payload_words must be 0 with arrivals")
            payload_words = arrival_region_words(batch, *arrivals) + n_times
        self.row_off, self.payload_off, self.rec_off, total = stage_layout(batch, rows, payload_words, loads, record_len)
        self.device = device
        self.dev = torch.zeros(total, device=device)
        self.host = torch.zeros(total).pin_memory()
        self.row = {k: self.dev[o:o + batch].view(torch.int32) for k, o in self.row_off.items()}
        self.h_row = {k: self.host[o:o + batch].view(torch.int32) for k, o in self.row_off.items()}
        self.payload, self.h_payload = self.dev[self.payload_off:self.rec_off], self.host[self.payload_off:self.rec_off]
        self.records, self.h_records = self.dev[self.rec_off:].view(loads, record_len), self.host[self.rec_off:].view(loads, record_len)
        self.uploaded = torch.cuda.Event()
        self.sent_words = self.sent_record_words = 0
        self._n_host, self._dev_records = 0, []
        self._live = {name: False for name in ONE_HOP_ROWS if name in self.row_off}    # the row was last written with entries
        if arrivals is not None:
            # uploaded up to the last arrival used: the CSR offsets of the arrivals [B + 1], the arrival records grouped by slot
            # `times`: the arrival ticks int32 [max_arrivals], parallel to the records, between the offsets and the records (they go up
            # whole: a few words per slot); without them the region is offsets | records
            max_arrivals, self.row_bytes = arrivals
            first = batch + 1 + n_times
            self.arr_off = self.payload_off + first           # the words in front of the arrival records
            self.offsets, self.h_offsets = self.payload[:batch + 1].view(torch.int32), self.h_payload[:batch + 1].view(torch.int32)
            self.times = self.payload[batch + 1:first].view(torch.int32) if times else None
            self.h_times = self.h_payload[batch + 1:first].view(torch.int32) if times else None
            self.arrivals = self.payload[first:].view(torch.int32).view(max_arrivals, arrival_width(self.row_bytes))
            self.h_arrivals = self.h_payload[first:].view(torch.int32).view(max_arrivals, arrival_width(self.row_bytes))

    def wait(self) -> None:
        """before the mirror is written: the previous upload's copy has left the pinned buffer"""
        self.uploaded.synchronize()

    def put_one_hop(self, name: str, slots=(), values=()) -> None:
        """the one-hop row `name` of the mirror: `values` at `slots` (host arrays or lists), 0 elsewhere; one indexed write: a full
        batch of NACKs is a thousand slots"""
        self.h_row[name].zero_()
        self._live[name] = len(slots) > 0
        if self._live[name]:
            self.h_row[name].numpy()[slots] = values

    @property
    def one_hop_live(self) -> bool:
        """whether a one-hop row holds entries as it was last written — after the `send` that follows every write: on the device"""
        return any(self._live.values())

    def put_starts(self, starts) -> int:
        """the queued starts -> the mirror's action row and records (sessions.stage_starts); returns the number of host records"""
        self.h_row["action"].zero_()          # the one-hop rule of put_one_hop, the entries written by stage_starts
        self._n_host, self._dev_records = stage_starts(starts, self.h_row["action"], self.h_records)
        self._live["action"] = bool(starts)
        return self._n_host

    def send(self, words: int) -> None:
        """the first `words` words of the mirror -> the device, on the current stream"""
        self.dev[:words].copy_(self.host[:words], non_blocking=True)
        self.sent_words = words

    def send_arrivals(self, arr: Arrivals, packets: Tensor, times: Optional[np.ndarray] = None) -> None:
        """checked arrivals (sessions.check_arrivals) -> the mirror's arrival region, then `send` up to the last arrival used; packets
        that are on the device go into the device records behind that copy, gathered first unless they came grouped by slot.  `times`
        (a stage with arrival times only): their ticks int32 [A] in the records' slot-grouped order, in the same copy"""
        put_arrivals(arr, packets, self.h_offsets, self.h_arrivals, self.row_bytes)
        if self.h_times is not None and arr.count:
            self.h_times.numpy()[:arr.count] = times
        self.send(self.arr_off + arr.count * self.arrivals.shape[1])
        if arr.count and packets.is_cuda:
            grouped = np.array_equal(arr.order, np.arange(arr.count))
            rows = packets if grouped else packets[torch.from_numpy(arr.order).to(self.device)]
            arrival_bytes(self.arrivals[:arr.count], self.row_bytes).copy_(rows)

    def finish(self, host_records_apart: bool = False) -> None:
        """after `send`: the host records in a copy of their own (`host_records_apart`: `send` stopped short of them), the device
        records one by one behind them, and the event that `wait` waits for"""
        stream = torch.cuda.current_stream(self.device)
        n_host, rec_len = self._n_host, self.records.shape[1]
        self.sent_record_words = n_host * rec_len if host_records_apart else 0
        if self.sent_record_words:
            end = self.rec_off + self.sent_record_words
            self.dev[self.rec_off:end].copy_(self.host[self.rec_off:end], non_blocking=True)
        for r, rec in enumerate(self._dev_records, start=n_host):
            rec.record_stream(stream)
            self.records[r].copy_(rec, non_blocking=True)
        self._n_host, self._dev_records = 0, []
        self.uploaded.record(stream)


class _GraphPair:
    """A ping-pong pair of captured graphs over `batch` slots: `parity`, warm-up and capture, replay-and-flip, and the per-slot
    device state the graphs update in place, allocated with its cleared value (`_slot_state`) and cleared by `_zero`."""

    def __init__(self, batch: int, device: torch.device):
        self.batch, self.device = int(batch), device
        self.parity = 0                       # the graph the next replay takes
        self._scratch: List[Tuple[Tensor, object, bool]] = []  # every _slot_state tensor with its cleared value and rezero

    def _slot_state(self, *shape: int, dtype: torch.dtype = torch.int32, cleared=0, pingpong: bool = False,
                    rezero: bool = False) -> Tensor:
        """per-slot device state `[B, *shape]` (`pingpong`: `[2, B, *shape]`, a row per parity), as cleared: `cleared` everywhere, or,
        for a dict {column: value}, zero but for those columns of the last dimension.  `_clear_scratch` clears it again, so a
        feature's state cannot be allocated without being reset with the rest (`rezero`: it zeroes the tensor before it fills it)"""
        t = torch.empty((2,) * pingpong + (self.batch,) + shape, dtype=dtype, device=self.device)
        self._scratch.append((t, cleared, rezero))
        self._clear(t, cleared)
        return t

    @staticmethod
    def _clear(t: Tensor, cleared, rezero: bool = False) -> None:
        if rezero or isinstance(cleared, dict):
            t.zero_()
        if not isinstance(cleared, dict):
            t.fill_(cleared)
            return
        for column, value in cleared.items():
            t[..., column].fill_(value)

    def _clear_scratch(self) -> None:
        for t, cleared, rezero in self._scratch:
            self._clear(t, cleared, rezero)

    def _zero(self) -> None:
        """everything the graphs update in place, as constructed (a subclass: with what else it owns)"""
        self._clear_scratch()

    def _capture_pair(self, hop, warmup: int):
        """warm `hop(0)` / `hop(1)` up on a side stream (builds every lazily cached table: folded weights, codebooks), zero the
        state, then capture one graph per parity; returns (graphs, their static outputs)"""
        device = self.device
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                hop(0)
                hop(1)
            self._zero()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        graphs, outs = [], []
        # no pass of the cyclic collector while a capture is open: it would finalize whatever dead cycle owns device objects (the
        # graphs of an earlier hop whose stage.send a caller wrapped, say) in the middle of the capture, and a pass that fell into
        # a capture has aborted the process.  Such garbage waits for the first pass after the captures
        collecting = gc.isenabled()
        gc.disable()
        try:
            for p in (0, 1):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g), torch.no_grad():
                    out = hop(p)
                graphs.append(g)
                outs.append(out)
        finally:
            if collecting:
                gc.enable()
        self._zero()
        return graphs, outs

    def _replay(self):
        """replay the current parity's graph and flip; returns that graph's static outputs"""
        p = self.parity
        self.graphs[p].replay()
        self.parity ^= 1
        return self.outs[p]

    def _need(self, have, what: str, how: str) -> None:
        """a method, argument or view `what` of an option this object was constructed without (`how` to get it): RuntimeError"""
        if not have:
            raise RuntimeError(f"{type(self).__name__}.{what}: construct with {how}")


class _Hop(_GraphPair):
    """What the graphed codec hops share on top of the graph pair: the groups' bounds and ping-pong state blocks (`parity`: the block
    holding the CURRENT caches), the per-group concatenation of the caches, and the session front end (the queue is host-only and
    always exists; `sessions` gates the public methods and the graph's session kernels)."""

    srtp = None                               # GraphedEncodeHop / GraphedDecodeHop(srtp=): the SrtpConfig

    def __init__(self, model, batch: int, n: int, device: torch.device, groups: int = 1, sessions: bool = False,
                 max_loads_per_hop: int = 4):
        super().__init__(batch, device)
        self.model, self.n = model, n
        groups = max(1, min(int(groups), batch))
        self.bounds = [(batch * g // groups, batch * (g + 1) // groups) for g in range(groups)]
        # per group: a ping-pong pair of state blocks (a cache tensor is [streams, C, pad]: a group's slice must be contiguous)
        self.gstate = [(self._block(hi - lo), self._block(hi - lo)) for lo, hi in self.bounds]
        self.sessions = bool(sessions)
        if self.sessions and max_loads_per_hop < 1:
            raise ValueError("max_loads_per_hop must be >= 1")
        layout = self.gstate[0][0].layout
        self.queue = SessionQueue(batch, n, int(max_loads_per_hop) if self.sessions else 0, layout,
                                  one_sided=layout.n_enc in (0, len(layout.shapes)))
        if self.sessions:
            for a, b in self.gstate:          # the kernels' layout tables, built before the capture
                a.layout.tables(device)
                b.layout.tables(device)

    def _block(self, streams: int) -> StateBlock:
        """a state block of `streams` streams (the sender and the receiver: one side's caches only)"""
        return StateBlock(self.model, streams, self.device)

    def _new_stage(self, rows: Sequence[str], payload_words: int = 0, arrivals: Optional[Tuple[int, int]] = None,
                   times: bool = False) -> ControlStage:
        """the control stage of a hop with these rows and payload (`arrivals`: an arrival region, `times`: with arrival ticks), and the
        device views every session graph reads"""
        q = self.queue
        stage = ControlStage(q.batch, rows, payload_words, q.max_loads, q.layout.record_len, self.device, arrivals, times)
        self.action, self.hold, self.records = stage.row["action"], stage.row["hold"], stage.records
        return stage

    @property
    def state(self):
        """(block A, block B) of a single-group schedule (the form tests and callers of earlier rounds use)"""
        if len(self.gstate) != 1:
            raise RuntimeError(f"{type(self).__name__}.state: the streams are split into groups — use .gstate[g]")
        return self.gstate[0]

    def _zero(self) -> None:
        for a, b in self.gstate:
            a.zero_()
            b.zero_()
        super()._zero()

    def _load(self, cache_enc: Optional[Sequence[Tensor]], cache_dec: Optional[Sequence[Tensor]]) -> None:
        """reset's state part: parity 0, block A zero or the given caches, the scratch buffers zero"""
        self.parity = 0
        for (lo, hi), (a, _b) in zip(self.bounds, self.gstate):
            a.load_(None if cache_enc is None else [c[lo:hi] for c in cache_enc],
                    None if cache_dec is None else [c[lo:hi] for c in cache_dec])
        self._clear_scratch()

    def _current(self, which: str) -> List[Tensor]:
        per_group = [getattr(blocks[self.parity], which) for blocks in self.gstate]
        if len(per_group) == 1:
            return per_group[0]                                        # views of the state block itself
        return [torch.cat(cs, dim=0) for cs in zip(*per_group)]      # groups are contiguous stream ranges: copies, full batch

    # ---------------------------------------------------------------- sessions
    def _need_sessions(self, what: str) -> None:
        self._need(self.sessions, what, "sessions=True")

    def _hold_slots(self, hold) -> List[int]:
        """step's `hold` checked before anything is launched"""
        slots = SessionQueue.host_slots(hold)
        if slots:
            self._need_sessions("step(hold=...)")
            slots = [self.queue.slot(s) for s in slots]
        return slots

    def _where(self, slot: int) -> Tuple[int, int]:
        for g, (lo, hi) in enumerate(self.bounds):
            if lo <= slot < hi:
                return g, slot - lo
        raise IndexError(slot)

    def start(self, slot: int, cache_enc: Optional[Sequence[Tensor]] = None, cache_dec: Optional[Sequence[Tensor]] = None,
              n: Optional[int] = None) -> None:
        """At the next step, slot `slot` begins a fresh stream (zero caches) or, given one stream's 22 + 30 caches (B = 1
        tensors, as `export` / `wire.load_cache_npz(..., batch=1)` give them, on the host or the device), resumes that stream.
        `n`: its number of quantiser stages (default: the graph's n).  At most `max_loads_per_hop` resumes per hop."""
        self._need_sessions("start")
        self.queue.start(slot, cache_enc, cache_dec, n)

    # ---------------------------------------------------------------- SRTP keys (GraphedEncodeHop / GraphedDecodeHop with srtp=)
    def _init_keys(self) -> None:
        """per slot: the key rows the SRTP launch reads (srtp.KEY_*; device, captured by address) and their host table"""
        self._keys = srtp_def.KeyTable(self.batch)
        self._keys_dev = self._slot_state(srtp_def.KEY_WORDS)

    def _send_keys(self) -> None:
        """before a replay, on its stream: the key table, when it has changed since the last hop"""
        if self.srtp is not None and self._keys.dirty:
            self._keys_dev.copy_(torch.from_numpy(self._keys.rows))
            self._keys.dirty = False

    def _start_keyed(self, slot: int, queue_start) -> None:
        """a start on an srtp hop: the header restarts SEQ at 0, so the slot needs a key set since its previous start (ValueError);
        the key counts as used once the start is queued"""
        if self.srtp is None:
            return queue_start()
        s = self.queue.slot(slot)
        if not self._keys.fresh[s]:
            self._keys.started(s)             # raises
        queue_start()
        self._keys.started(s)

    def set_key(self, slot: int, master_key, master_salt, ssrc: Optional[int] = None, roc: int = 0) -> None:
        """from the next hop on, slot `slot` protects / unprotects under the session keys derived (RFC 3711 4.3.1) from `master_key`
        (16 bytes) and `master_salt` (14 bytes), with `ssrc` (default: the slot) in the counter blocks; a start of the slot begins
        at rollover counter `roc` (a late joiner's receiver).  The key row is built on the host and goes up before the next replay.
        ValueError: wrong lengths, a slot, ssrc or roc out of range, or a key the slot had before (its previous one, or one it was
        started under since the last reset).  Keys never appear in a repr or an error message."""
        self._need(self.srtp is not None, "set_key", "srtp=SrtpConfig()")
        self._keys.set_key(self.queue.slot(slot), master_key, master_salt, ssrc, roc)

    def clear_key(self, slot: int) -> None:
        """from the next hop on, slot `slot` has no key: a sender slot sends nothing, a receiver slot rejects every arrival"""
        self._need(self.srtp is not None, "clear_key", "srtp=SrtpConfig()")
        self._keys.clear_key(self.queue.slot(slot))

    def stop(self, slot: int) -> None:
        """from the next step on, slot `slot` is held (does not advance) on every step until the next `start(slot, ...)`"""
        self._need_sessions("stop")
        self.queue.stop(slot)

    @property
    def stopped(self) -> Tuple[int, ...]:
        """the stopped slots, sorted"""
        return self.queue.stopped

    def export(self, slot: int) -> Tuple[List[Tensor], List[Tensor]]:
        """the current 22 + 30 caches of slot `slot` as B = 1 device tensors (one gather launch) — the state after the last
        step, without actions queued since (a stopped slot: its caches when it stopped)"""
        self._need_sessions("export")
        g, local = self._where(self.queue.slot(slot))
        blk = self.gstate[g][self.parity]
        slots = torch.tensor([local], dtype=torch.int32, device=self.device)
        with torch.no_grad():
            rec = ops.state_slots_gather(blk.buffer, blk.layout, slots)
        return blk.layout.split(rec[0])


class GraphedHop(_Hop):
    """model: `hilcodec_amd.models.hilcodec.streaming.HILCodec` (eval, reparameterisations removed).
    `step(x)` consumes `[B,1,hop]` samples (copied into the static input) and returns (indices `[n,B,T]`, wav `[B,1,hop]`)
    as views of static buffers that a later `step` overwrites (each parity has its own pair).

    `groups` > 1: the streams are split into that many contiguous groups, each with its own state blocks, and the graph
    runs the groups' chains (encoder -> RVQ -> dequantiser -> decoder) side by side on separate HIP streams.  Streams are
    independent, so this is the same arithmetic on the same data — outputs bit-identical to `groups=1`, NO added latency
    (unlike PipelinedHop) — but every launch of a hop covers the chip only 1.3-4 times at 1024 streams, and two or more
    independent chains fill each other's partly-filled last rounds.

    `sessions=True`: every slot is an independent stream session.  `start(slot, ...)` begins a fresh stream (zero caches)
    or resumes one from its 22 + 30 caches, `set_bitrate(slot, n)` changes its number of quantiser stages (`n` of the
    constructor is the maximum and the default), `export(slot)` returns its current caches; each takes effect at the next
    `step()`.  The graph then starts each group's chain with one hilc_state_slots_apply on the block the hop reads, and the
    quantiser and dequantiser take their per-stream n from a device buffer (rows >= a stream's n of the indices hold -1).
    Pending actions travel from pinned host buffers on the replay stream, only when something changed.
    Held streams: `step(x, hold=slots)` leaves the slots `slots` (host ints) exactly as they are for that hop (caches
    bit-identical afterwards, a `start` queued for the hop included; their `x` rows are not read for anything that matters; their
    wav rows are 0 and indices -1); `stop(slot)` holds a slot on every step until its next `start`, `stopped` lists those slots.
    Each group's chain ends with one hilc_state_slots_hold, which copies held streams back from the block the hop read.
    `sessions=False` captures exactly the graph of earlier rounds."""

    def __init__(self, model, batch: int, hop: int, n: int, device: torch.device, warmup: int = 2, groups: int = 1,
                 sessions: bool = False, max_loads_per_hop: int = 4):
        super().__init__(model, batch, n, device, groups, sessions, max_loads_per_hop)
        self.x = torch.zeros(batch, 1, hop, device=device)
        if self.sessions:
            # ONE buffer so that a hop's upload is one copy: action per slot (0 keep, -1 zero, r >= 1 load record r-1), n per
            # slot, 1 where the slot is held, (a subclass's _extra_rows) then the staged records
            self.stage = self._new_stage(("action", "n_slot", "hold") + self._extra_rows())
            self.n_slot = self.stage.row["n_slot"]
            self.n_slot.fill_(self.n)
            self.stage.h_row["n_slot"].fill_(self.n)
            self._held_live = frozenset()     # the slots the device hold row marks
        self._init_state()
        # the STFT side branch (engine._early_spectra) only for a single chain: with several chains the launches of the other
        # groups already fill the idle CUs, and a fork of a forked stream inside one capture crashes hipStreamEndCapture (ROCm 7.2)
        self.spec_side = [torch.cuda.Stream(device) if len(self.bounds) == 1 else None for _ in self.bounds]
        self.chain = [None] + [torch.cuda.Stream(device) for _ in self.bounds[1:]]      # group 0 runs on the capture stream
        self.sched = [ops.SchedWorkspace(device) for _ in self.bounds]    # ticket words: one workspace per concurrent chain
        self.graphs, self.outs = self._capture_pair(self._hop, warmup)

    def _chain(self, g: int, p: int) -> Tuple[Tensor, Tensor]:
        m = self.model
        lo, hi = self.bounds[g]
        src, dst = self.gstate[g][p], self.gstate[g][p ^ 1]
        x = self.x[lo:hi]
        n_clip = self.n_slot[lo:hi] if self.sessions else None
        if self.sessions:
            # before the encoder: it forks the STFT side branch, which reads this block's waveform histories
            ops.state_slots_apply(src.buffer, src.layout, self.action[lo:hi], self.records)
        with ops.sched_workspace(self.sched[g]):
            # while this thread warms up or captures: the STFT front halves of the un-fused SpecBlocks go to the side stream
            # (context-local, nothing is written into the model)
            with engine.spectra_side_stream(self.spec_side[g]):
                z, _ = m.encoder(x, *src.enc, cache_out=dst.enc)
            idx = m.quantizer(z, self.n, n_clip=n_clip)
            q = m.dequantizer(idx, self.n, n_clip=n_clip)
            wav, _ = m.decoder(q, *src.dec, cache_out=dst.dec)
        if self.sessions:
            # after the last write to dst and to this group's outputs
            ops.state_slots_hold(src.buffer, dst.buffer, src.layout, self.hold[lo:hi], wav=wav, indices=idx)
        return idx, wav

    def _hop(self, p: int) -> Tuple[Tensor, Tensor]:
        if len(self.bounds) == 1:
            return self._chain(0, p)
        main = torch.cuda.current_stream(self.device)
        outs = [None] * len(self.bounds)
        for g in range(1, len(self.bounds)):              # fork
            self.chain[g].wait_stream(main)
            with torch.cuda.stream(self.chain[g]):
                outs[g] = self._chain(g, p)
        outs[0] = self._chain(0, p)
        for g in range(1, len(self.bounds)):              # join
            main.wait_stream(self.chain[g])
        return torch.cat([o[0] for o in outs], dim=1), torch.cat([o[1] for o in outs], dim=0)

    @property
    def cache_enc(self) -> List[Tensor]:
        """the CURRENT encoder caches of all streams, in the reference's order (`streaming.py:458-470`) — what
        `wire.save_cache` / `reset(...)` take; with groups > 1 concatenated over the groups (copies)"""
        return self._current("enc")

    @property
    def cache_dec(self) -> List[Tensor]:
        return self._current("dec")

    def reset(self, cache_enc: Optional[Sequence[Tensor]] = None, cache_dec: Optional[Sequence[Tensor]] = None) -> None:
        """zero history, or resume from caches saved earlier (`wire.save_cache` / `e_in*`, `d_in*`); with sessions also drops
        every queued action, clears every stop and puts every slot back to the default n.  (GraphedEncodeHop: with FEC, no stream
        has a previous hop afterwards; with DTX, every run counter is 0; with the header, every hop counter is 0; with a VBR
        cap, every bucket is full; with `rate`, every slot is back at its start rate with a full bucket)"""
        with torch.no_grad():
            self._load(cache_enc, cache_dec)
            if self.sessions:
                self.queue.reset()
                st = self.stage
                st.wait()
                st.put_starts({})
                st.h_row["n_slot"].fill_(self.n)
                st.h_row["hold"].zero_()
                self._put_extra(st)
                st.send(st.rec_off)
                st.finish()
                self._held_live = frozenset()

    def step(self, x: Tensor, hold=None) -> Tuple[Tensor, Tensor]:
        """`hold`: slots (host ints) that do not advance on this hop (sessions=True only; None or empty: every slot advances)"""
        held = self._hold_slots(hold)
        self.x.copy_(x)
        if self.sessions:
            self.queue.hold(held)
            self._upload()
        return self._replay()

    def _upload(self) -> None:
        """queued actions, bitrates and holds (and a subclass's extra rows) -> the graph's device buffers, on the replay stream (an
        action applies to exactly one hop: the upload after a hop with actions clears them; the hold row goes up when it changes)"""
        q, st = self.queue, self.stage
        held = q.held
        if not q.pending and not st.one_hop_live and held == self._held_live and not self._extra_pending():
            q.clear()                         # this hop's holds are spent (the device row already marks them)
            return
        st.wait()
        n_host = st.put_starts(q.starts)      # host records first: they go up in the one copy
        for slot, n in q.n.items():
            st.h_row["n_slot"][slot] = n
        _mark(st.h_row["hold"], held)
        self._put_extra(st)
        st.send(st.rec_off + n_host * st.records.shape[1])
        st.finish()
        self._held_live = held
        q.clear()

    def _init_state(self) -> None:
        """a subclass's per-slot device state (_slot_state), allocated before the capture that reads it"""

    # a subclass's own rows of the control stage (GraphedEncodeHop(fec_adapt=): the report row)
    def _extra_rows(self) -> Tuple[str, ...]:
        return ()

    def _extra_pending(self) -> bool:
        """whether an extra row must go up on this hop although nothing else changed"""
        return False

    def _put_extra(self, st: ControlStage) -> None:
        """write the extra rows of the mirror, before an upload's copy"""

    def set_bitrate(self, slot: int, n: int) -> None:
        """from the next step on, slot `slot` uses the first `n` quantiser stages (1 <= n <= the graph's n)"""
        self._need_sessions("set_bitrate")
        self.queue.set_bitrate(slot, n)


class PipelinedHop(_Hop):
    """Throughput schedule for a node that runs BOTH halves of the codec on the same streams (transcoding, evaluation,
    the benchmark): a two-stage software pipeline over hops.  One graph replay runs, side by side on two HIP streams,
    the encoder + RVQ of hop i and the dequantiser + decoder of hop i-1 — two independent chains (the only edge between
    them, the indices of hop i-1, was produced by the previous replay), so the tails of one chain's small launches are
    filled with workgroups of the other instead of idle CUs.  The arithmetic is the GraphedHop's — same kernels' products in the
    same order; the decoder is captured with `ExecOptions.decoder_stage_narrow = False` (its narrow stages as up-sampling launch +
    chain instead of one launch: another launch structure, the same bits) —
    outputs are bit-identical, the decoded audio just arrives one replay later (`step` returns the indices of the hop it
    was given and the wav of the previous one; `flush` decodes the last hop).  Cost: one hop (320 samples, 13.3 ms) of
    extra latency on the decoded output — a schedule for aggregate throughput, not for the lowest-latency single call,
    which stays `GraphedHop`.

    State blocks as in GraphedHop; the encoder and decoder halves of a block flip on opposite parities (the decoder is
    one hop behind), the indices travel through two fixed `[n,B,T]` buffers."""

    def __init__(self, model, batch: int, hop: int, n: int, device: torch.device, warmup: int = 2, groups: int = 1,
                 sessions: bool = False):
        """`groups` > 1: additionally split the streams into contiguous groups, each with its own encoder and decoder chain
        (2 * groups HIP streams inside the graph), as in GraphedHop.  `sessions` (GraphedHop's per-stream sessions) is not
        available on this schedule."""
        if sessions:
            raise NotImplementedError("PipelinedHop(sessions=True): per-stream sessions exist on GraphedHop only (the encoder and "
                                      "decoder halves of a block flip on opposite parities here)")
        super().__init__(model, batch, n, device, groups)
        self.x = torch.zeros(batch, 1, hop, device=device)
        # `parity` is the encoder's: the block holding the encoder caches of the next hop
        self.pending = False                  # a hop is encoded but not decoded yet
        # chains: encoder of group 0 on the capture stream, every other chain on its own stream (all forked from the capture
        # stream; a fork of a fork crashes hipStreamEndCapture on ROCm 7.2, so the STFT side branch exists for groups == 1 only)
        self.enc_stream = [None] + [torch.cuda.Stream(device) for _ in self.bounds[1:]]
        self.dec_stream = [torch.cuda.Stream(device) for _ in self.bounds]
        self.spec_side = torch.cuda.Stream(device) if len(self.bounds) == 1 else None
        # concurrent chains never share ticket words
        self.sched_enc = [ops.SchedWorkspace(device) for _ in self.bounds]
        self.sched_dec = [ops.SchedWorkspace(device) for _ in self.bounds]
        with torch.no_grad():                 # one eager encode gives the shape of the two index buffers
            idx = torch.cat([self._encode(g, 0) for g in range(len(self.bounds))], dim=1)
        self.idx = (torch.zeros_like(idx), torch.zeros_like(idx))
        self.graphs, self.outs = self._capture_pair(self._both, warmup)        # outs: the wav of each parity

    def _encode(self, g: int, p: int) -> Tensor:
        m = self.model
        lo, hi = self.bounds[g]
        st = self.gstate[g]
        with ops.sched_workspace(self.sched_enc[g]), engine.spectra_side_stream(self.spec_side):
            z, _ = m.encoder(self.x[lo:hi], *st[p].enc, cache_out=st[p ^ 1].enc)
        return m.quantizer(z, self.n)

    def _decode(self, g: int, p: int) -> Tensor:
        """decode the hop whose encoder ran with parity p^1 (its indices sit in idx[p^1]); decoder parity = p^1"""
        m = self.model
        lo, hi = self.bounds[g]
        st = self.gstate[g]
        # captured with the model's own ExecOptions: an override for this chain alone measured slower (tools/ab_pipelined_overrides.py)
        with ops.sched_workspace(self.sched_dec[g]):
            wav, _ = m.decoder(m.dequantizer(self.idx[p ^ 1][:, lo:hi].contiguous(), self.n), *st[p ^ 1].dec,
                               cache_out=st[p].dec)
        return wav

    def _both(self, p: int) -> Tensor:
        main = torch.cuda.current_stream(self.device)
        G = len(self.bounds)
        wavs, idxs = [None] * G, [None] * G
        for g in range(G):                                # fork: every decoder chain, and the encoder chains of groups > 0
            self.dec_stream[g].wait_stream(main)
            with torch.cuda.stream(self.dec_stream[g]):
                wavs[g] = self._decode(g, p)
            if g > 0:
                self.enc_stream[g].wait_stream(main)
                with torch.cuda.stream(self.enc_stream[g]):
                    idxs[g] = self._encode(g, p)
        idxs[0] = self._encode(0, p)
        for g in range(G):                                # join
            main.wait_stream(self.dec_stream[g])
            if g > 0:
                main.wait_stream(self.enc_stream[g])
        self.idx[p].copy_(idxs[0] if G == 1 else torch.cat(idxs, dim=1))
        return wavs[0] if G == 1 else torch.cat(wavs, dim=0)

    @property
    def cache_enc(self) -> List[Tensor]:
        """CURRENT encoder caches of all streams, concatenated over the groups.  Only after `flush()`: while a hop is pending the
        decoder is one hop behind the encoder, and a (cache_enc, cache_dec) pair taken then would resume with the decoder out of
        step — refused instead of silently wrong."""
        self._no_pending("cache_enc")
        return self.cache_enc_unsynced

    @property
    def cache_enc_unsynced(self) -> List[Tensor]:
        """The encoder caches as of the LAST ENCODED hop, also while a hop is pending (then the decoder's caches are one hop older: this
        list alone is a valid encoder snapshot, a (cache_enc_unsynced, cache_dec) pair is not a resumable state — `flush()` first for
        that).  For callers that checkpoint the encoder side only; rounds 2-4's `cache_enc` behaved like this."""
        return self._current("enc")

    @property
    def cache_dec(self) -> List[Tensor]:
        """CURRENT decoder caches (only after `flush()`, see `cache_enc`: then both cache lists describe the same instant)"""
        self._no_pending("cache_dec")
        return self._current("dec")

    def _no_pending(self, what: str) -> None:
        if self.pending:
            raise RuntimeError(f"PipelinedHop.{what}: a hop is encoded but not decoded yet — call flush() first (the decoder's caches "
                               "are one hop behind the encoder's until then)")

    def reset(self, cache_enc: Optional[Sequence[Tensor]] = None, cache_dec: Optional[Sequence[Tensor]] = None) -> None:
        """zero history, or resume from caches exported earlier (`cache_enc` / `cache_dec`, which can only be read after a `flush()`)"""
        with torch.no_grad():
            self.pending = False
            self._load(cache_enc, cache_dec)

    def step(self, x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        """x `[B,1,hop]` -> (indices of THIS hop `[n,B,T]`, wav `[B,1,hop]` of the PREVIOUS hop or None on the first
        call); both are views of static buffers that the next-but-one `step` overwrites."""
        p = self.parity
        self.x.copy_(x)
        if self.pending:
            wav = self._replay()
        else:                                              # first hop: nothing to decode yet
            with torch.no_grad():
                self.idx[p].copy_(torch.cat([self._encode(g, p) for g in range(len(self.bounds))], dim=1))
            wav = None
            self.parity ^= 1
        self.pending = True
        return self.idx[p], wav

    def flush(self) -> Optional[Tensor]:
        """decode the last encoded hop (end of the streams)"""
        if not self.pending:
            return None
        with torch.no_grad():
            wav = torch.cat([self._decode(g, self.parity) for g in range(len(self.bounds))], dim=0)
        self.pending = False
        return wav


class GraphedEncodeHop(GraphedHop):
    """The sender: one graph replay per hop turns `[B,1,hop]` samples into per-stream 10-bit packets (`wire.packet_bytes`).
    A hop is GraphedHop's chain cut after the quantiser — (hilc_state_slots_apply if `sessions`) -> streaming encoder with its
    STFT side branch -> RVQ (per-stream n if `sessions`) -> hilc_pack_codes_10bit — on a ping-pong pair of ENCODER-ONLY state
    blocks (the 22 encoder caches; `state_bytes`).  `step(x)` returns (packets uint8 `[B, packet_bytes(n, T)]`, nbytes int32
    `[B]`), `.indices` the same hop's `[n,B,T]`: static views that the next-but-one `step` overwrites.
    Sessions as in GraphedHop, on the encoder side: `start(slot, cache_enc=None, n=None)`, `set_bitrate(slot, n)`,
    `export(slot) -> cache_enc`, `step(x, hold=slots)`, `stop(slot)`; a held row's packet is all zero with nbytes 0 and its
    `.indices` are -1.
    `input_rate` (resample.RATES; default 24 000 = no resampler): `step(x)` takes `[B,1,resample.hop_samples(hop // 320,
    input_rate)]` samples at that rate, and the graph converts them to the encoder's 24 kHz hop with one hilc_resample_poly launch
    after hilc_state_slots_apply.  Its per-stream input history is one more cache, the LAST of the encoder list: `export`,
    `start` and `cache_enc` then hold 23 caches, `start(slot)` zeroes it and a held or stopped slot keeps it.
    `fec_stages` = m >= 1 (in-band FEC, at most n; `hop` a multiple of 320): each packet also carries the first m stages of the
    stream's previous encoded hop, `wire.pack_fec_packet(idx[:n_b], prev)`, so packets are uint8 `[B, wire.fec_packet_bytes(n, m,
    T)]`; `.indices` are unchanged.  A stream without a previous encoded hop (the first hop after construction, `reset`, a `start`
    or a resume) sends the plain n_b-stage packet; a held or stopped slot keeps its previous codes; `export` and a resume carry no
    FEC state.  Per-stream n (`start(n=)`, `set_bitrate`) must be >= m.  The graph runs hilc_pack_codes_10bit_fec in place of
    hilc_pack_codes_10bit on a ping-pong pair of int32 rows `[B, 1 + m T]` (valid, codes) indexed by parity, like the state blocks.
    `fec_stages=0` captures exactly the graph without FEC.
    `dtx` = dtx.DtxConfig(threshold_db, hangover, sid_interval, order) (`hop` a multiple of 320; a SID of 1 + order bytes must fit
    `wire.packet_bytes(n, T)`): discontinuous transmission.  After the packer, one hilc_dtx_encode analyses each stream's 24 kHz hop
    (after the input resampler) and advances its run counter; `.kind` (int32 `[B]` device view, like `.indices`) is each stream's
    dtx.HELD / SPEECH / SID / SILENT.  SPEECH rows are what the sender without DTX sends; a SID row holds `dtx.pack_sid(L, q)` then
    zeros with nbytes 1 + order, a SILENT row is zero with nbytes 0, and both have `.indices` -1 (with FEC, the next speech hop is a
    plain packet).  A held slot keeps its run; `start` clears it; `export` and a resume carry no DTX state.  `dtx=None` captures
    exactly the graph without DTX.
    `header=True` (`hop` a multiple of 320): every packet carries the 3-byte transport header of `wire.pack_transport` — the slot's hop
    index (the hops its encoder advanced since its last start, mod 2^16), the SID and FEC flags and n — so rows are uint8 `[B,
    wire.transport_bytes(n, m, T)]` and byte counts include the header (0: nothing to send).  One hilc_packet_header runs last, on a
    ping-pong pair of int32 counter rows indexed by parity.  A start or a resume restarts a slot's counter at 0 (that hop's packet
    carries h = 0); a held or stopped slot sends nothing and keeps it; a DTX SILENT hop sends nothing but advances it.  `.hop_index`
    (int32 `[B]` device view) is each slot's counter for the next hop; `export` and a resume carry none.  `header=False` captures
    exactly the graph without the header.
    `vbr` = vbr.VbrConfig(target_db, n_min, cap_kbps, burst_hops) (`hop` a multiple of 320; with `fec_stages` it needs `header=True`:
    without the header a receiver cannot tell an n-stage packet with a redundant section from a longer plain one): quality-targeted
    variable bitrate (vbr.py).  Right after the quantiser one hilc_vbr_select measures, per slot, the float64 quantisation error after
    every stage, picks the fewest stages n_eff in [max(n_min, fec_stages, 1), n_b] whose error is target_db below the energy of the
    quantiser's input (n_b: the graph's n, or the slot's `start(n=)` / `set_bitrate` ceiling), caps it by the slot's token bucket when
    `cap_kbps` is given, and sets the rows >= n_eff of `.indices` to -1; the packer, the FEC packer and the header take n_eff in place
    of the per-stream n, so `nbytes` follows.  `.n_eff` (int32 `[B]`), `.distortion` (float64 `[B, n + 1]`) and, with a cap, `.credit`
    (int32 `[B]`, bits) are device views like `.indices`.  A `start` or a resume refills a slot's bucket; a held or stopped slot keeps
    it, reports n_eff = n_b and a zero distortion row; `reset` refills every bucket; `export` and a resume carry no VBR state.  DTX runs
    after the packer, unchanged: a SID or SILENT hop is still charged what VBR chose.  A receiver gets n from the header (`play()`), or
    from `wire.packet_n(nbytes, T)` for headerless packets without FEC.  `vbr=None` captures exactly the graph without VBR.
    `fec_adapt` = report.FecAdaptConfig(on_q8, off_q8, calm_reports, timeout_hops, initial_on) (needs `sessions` and `fec_stages` >= 1):
    loss-adaptive FEC (report.py).  `step(x, hold=None, reports=(slots, blobs))` takes this hop's receiver reports — A host ints, and a
    uint8 `[A, 3]` host tensor or a sequence of 3-byte `bytes` (`wire.pack_report`; a slot outside [0, B) or a wrong width: ValueError; a
    slot named twice keeps its last) — which go up as one more int32 row of the control stage's single copy and apply to exactly one hop,
    like an action.  One hilc_fec_adapt ahead of hilc_vbr_select and the packer moves each slot's switch (on at a reported loss >=
    on_q8, off after calm_reports reports <= off_q8 in a row, back to initial_on after timeout_hops hops without an accepted report) and
    clears word 0 of the previous-codes row the packer reads for the slots that are off and not held: their packets are the plain
    n_b-stage ones, the header's FEC flag follows the length, and since the packer still stores every hop's codes, switching on takes
    effect on the next packet.  `fec_on` (int32 `[B]`) and `fec_adapt_state` (int32 `[B, report.FA_WORDS]`) are device views; a `start`
    or a resume clears a slot's row inside the graph, `reset` every row; held and stopped slots take their reports but do not age and keep
    their previous codes; `export` and a resume carry none.  VBR, DTX and the header are untouched.  `fec_adapt=None` captures exactly
    the graph without it.
    `rtx` = rtx.RtxConfig(history, per_hop) (needs `sessions` and `header`): retransmission (rtx.py).  One hilc_rtx_step, the graph's last
    launch, keeps each slot's last `history` headed packets (what `step` returned for it, byte for byte; held, stopped and DTX SILENT hops
    store nothing) and answers this hop's NACKs: `step(x, hold=None, reports=None, nacks=(slots, blobs))` takes them like `reports` — A host
    ints, and a uint8 `[A, 4]` host tensor or a sequence of 4-byte `bytes` (`wire.pack_nack`; a slot outside [0, B) or a wrong width:
    ValueError; a slot named twice keeps its last) — as two more int32 rows of the control stage's single copy, for exactly one hop.  The
    hops asked for that are still in the history go to `rtx_packets` (uint8 `[B, per_hop, wire.transport_bytes(n, m, T)]`) with
    `rtx_nbytes` (int32 `[B, per_hop]`, 0: the row is unused), in request order; they are sent beside the hop's packet and reach the
    receiver as ordinary `play()` arrivals.  `rtx_state` (int32 `[B, rtx.RX_WORDS]`) counts; all three are device views, the first two
    overwritten by the next-but-one `step`.  A `start` or a resume empties a slot's history inside the graph (a NACK for its earlier hops
    is a miss), `stop` and a hold keep it and such a slot still answers; `reset` clears every history; `export` and a resume carry none.
    Every other option is untouched: a retransmission is not charged to VBR's bucket.  `rtx=None` captures exactly the graph without it.
    `rate` = rate.RateConfig(min_kbps, max_kbps, start_kbps, high_q8, low_q8, increase_q8, burst_hops, timeout_hops) (needs `sessions`;
    `hop` a multiple of 320; min_kbps must pay for the floor of a hop — the header, max(fec_stages, 1) stages and the redundant section:
    ValueError otherwise): report-driven rate control (rate.py).  Each slot has a rate that follows this hop's `reports` (taken as for
    `fec_adapt`; with both, one report feeds both launches): down by half the reported loss at loss_q8 >= high_q8, up by increase_q8 / 256
    of itself at loss_q8 <= low_q8, back to start_kbps after timeout_hops hops without an accepted report; and a token bucket filled at
    that rate and charged with every byte the slot sends.  Two launches: hilc_rate_ceiling in front of the quantiser (behind
    hilc_fec_adapt, which moves there) writes `n_ceil`, the most stages the bucket pays for behind the hop's header and live redundant
    section, never fewer than min(n_b, max(fec_stages, 1)); that row takes the place of the per-stream n for the quantiser, VBR (as its
    n_b), the packers and the header.  hilc_rate_charge, the graph's last launch, takes 8 x (`nbytes` + the hop's `rtx_nbytes`) out of
    the bucket: header, primary codes, redundant section, a SID, nothing for a DTX silent hop, what VBR saved, retransmissions.  `n_ceil`
    (int32 `[B]`) and `rate_state` (int32 `[B, rate.RC_WORDS]`; `rate.kbps(rate_state, frames)` on the host) are device views.  A `start`
    or a resume resets a slot's row inside the graph (start rate, full bucket, counters 0), `reset` every row; a held or stopped slot
    takes its reports but neither ages nor fills, reports n_ceil = its own n, and still pays for the NACKs it answers; `export` and a
    resume carry none.  `fec_adapt`, `rtx` and VBR's `cap_kbps` work as without it.  `rate=None` captures exactly the graph without it.
    `audio_level=True`: one hilc_audio_level launch measures each slot's 24 kHz hop (behind the input resampler where there is one) in
    front of the encoder: `.audio_level` (int32 `[B]` device view, valid until the next-but-one `step`, like `.indices`) is the hop's
    level, -dBov in 1 dB steps in [0, 127] (audio_level.py: the rule), 127 for a held or stopped slot.  It is what a forwarding hop
    takes as `forward(levels=)`; it travels beside the packet, and nothing else the hop returns changes.  `audio_level=False` captures
    exactly the graph without it.
    `cap` = bwe.CapConfig(timeout_hops) (needs `rate`): the receiver's delay-based bandwidth estimate as a ceiling of the rate (bwe.py).
    `step(x, hold=None, reports=None, nacks=None, caps=(slots, blobs))` takes this hop's rate caps like `reports` — A host ints, and a
    uint8 `[A, 3]` host tensor or a sequence of 3-byte `bytes` (`wire.pack_cap`, what GraphedDecodeHop(bwe=...) shows as
    `caps[cap_due]`; a slot outside [0, B) or a wrong width: ValueError; a slot named twice keeps its last) — as one more int32 row of
    the control stage's single copy, for exactly one hop.  One hilc_rate_cap directly in front of hilc_rate_ceiling accepts a cap by
    that kernel's sequence rule, keeps it (clamped to the rate's bounds) until the next one or until timeout_hops hops without one, and
    holds the slot's rate at or below it; hilc_rate_ceiling, unchanged, runs on the clamped rate.  The slot's rate is therefore the
    smaller of the loss-based rate and the receiver's estimate: the reports keep probing upward and handle the standing queue a delay
    gradient cannot see.  `cap_state` (int32 `[B, bwe.CP_WORDS]`) is a device view.  A `start` or a resume clears a slot's row inside
    the graph, `reset` every row; held and stopped slots take their caps but do not age; `export` and a resume carry none.  `cap=None`
    captures exactly the graph without it.
    `srtp` = srtp.SrtpConfig() (needs `sessions` and `header`): packet protection, RFC 3711's AES_CM_128_HMAC_SHA1_80 (srtp.py: the
    rules).  One hilc_srtp_protect behind hilc_packet_header, in front of hilc_rtx_step (the history holds ciphertext: a retransmission
    is the packet that was sent, byte for byte) and of hilc_rate_charge (the bucket pays for the tag; hilc_rate_ceiling does not
    anticipate the 10 bytes, the bucket absorbs them as it does retransmissions).  `step` returns rows `[B, wire.srtp_bytes(n, m,
    T)]`: the 3 header bytes clear, the rest encrypted, a 10-byte tag; `rtx_packets` widens the same way; `srtp_state` (int32 `[B,
    srtp.TX_WORDS]`) is a device view.  `set_key(slot, master_key, master_salt, ssrc=None, roc=0)` / `clear_key(slot)`: the key table is
    built on the host and goes up before the next replay, only when it changed; a slot without a key sends nothing.  `start(slot)`
    needs a `set_key(slot, ...)` since the slot's previous start (the header restarts at hop 0 and the same key would reuse its
    keystream): ValueError otherwise, as for a `set_key` equal to the slot's previous one or to a key the slot was started under since
    the last `reset`.  A `start` or a resume clears the slot's TX row inside the graph, `reset` every row and every key; `export` and a
    resume carry no key and no row.  `srtp=None` captures exactly the graph without it."""

    def __init__(self, model, batch: int, hop: int, n: int, device: torch.device, warmup: int = 2, sessions: bool = False,
                 max_loads_per_hop: int = 4, input_rate: int = BASE_RATE, fec_stages: int = 0,
                 dtx: Optional[dtx_def.DtxConfig] = None, header: bool = False, vbr: Optional[vbr_def.VbrConfig] = None,
                 fec_adapt: Optional[report_def.FecAdaptConfig] = None, rtx: Optional[rtx_def.RtxConfig] = None,
                 rate: Optional[rate_def.RateConfig] = None, audio_level: bool = False, cap: Optional[bwe_def.CapConfig] = None,
                 srtp: Optional[srtp_def.SrtpConfig] = None):
        # the options are checked and what they derive is set up first: GraphedHop's constructor allocates (_init_state) and captures
        self.fec_stages = _fec_stages(fec_stages, n)
        self.fec_adapt = _config_arg("fec_adapt", fec_adapt, report_def.FecAdaptConfig)
        _needs("GraphedEncodeHop(fec_adapt=...)", fec_adapt is None or (sessions and self.fec_stages),
               "sessions=True and fec_stages >= 1")
        self._reports = {}                    # slot -> report word for the next hop
        self.header = bool(header)
        if self.header:
            _whole_frames("GraphedEncodeHop(header=True)", hop)
        self.rtx = _config_arg("rtx", rtx, rtx_def.RtxConfig)
        _needs("GraphedEncodeHop(rtx=...)", rtx is None or (sessions and self.header), "sessions=True and header=True")
        self.rate = _config_arg("rate", rate, rate_def.RateConfig)
        if rate is not None:
            _needs("GraphedEncodeHop(rate=...)", sessions, "sessions=True")
            # ValueError: a min_kbps that does not pay for the floor of a hop, a max_kbps past the int32 rows
            self._rate_bits = rate_def.bucket(rate, _whole_frames("GraphedEncodeHop(rate=...)", hop), self.fec_stages, self.header)
        self._nacks = {}                      # slot -> (word, bitmap) for the next hop
        self.cap = _config_arg("cap", cap, bwe_def.CapConfig)
        _needs("GraphedEncodeHop(cap=...)", cap is None or rate is not None, "rate=RateConfig(...): a cap is a ceiling of the rate")
        self._caps = {}                       # slot -> cap word for the next hop
        self.srtp = _config_arg("srtp", srtp, srtp_def.SrtpConfig)
        _needs("GraphedEncodeHop(srtp=...)", srtp is None or (sessions and self.header), "sessions=True and header=True")
        self._measure_level = bool(audio_level)
        self.frames = hop // HOP
        self.dtx = _config_arg("dtx", dtx, dtx_def.DtxConfig)
        if dtx is not None:
            dtx_def.check_order(dtx.order, wire.packet_bytes(n, _whole_frames("GraphedEncodeHop(dtx=...)", hop)),
                                "GraphedEncodeHop(dtx=...)")
        if self.fec_stages:
            _whole_frames(f"GraphedEncodeHop(fec_stages={fec_stages})", hop)
        self.input_rate = int(input_rate)
        self.rs, self._history, hop_in = None, 0, hop
        if self.input_rate != BASE_RATE:
            hop_in = hop_samples(_whole_frames(f"GraphedEncodeHop(input_rate={input_rate})", hop), self.input_rate)
            self.rs = design(self.input_rate, BASE_RATE)
            self.rs_taps = device_taps(self.rs, device)
            self._history = self.rs.history
        self.vbr = _config_arg("vbr", vbr, vbr_def.VbrConfig)
        if vbr is not None:
            _needs("GraphedEncodeHop(vbr=..., fec_stages=m)", self.header or not self.fec_stages, "header=True: without the header a "
                   "receiver cannot tell an n-stage packet with a redundant section from a longer plain one")
            self._vbr_lo = min(int(n), vbr_def.floor_stages(vbr, self.fec_stages))
            self._vbr_bits = vbr_def.bucket_bits(vbr, _whole_frames("GraphedEncodeHop(vbr=...)", hop), self.fec_stages)
        super().__init__(model, batch, hop_in, n, device, warmup, 1, sessions, max_loads_per_hop)
        self.queue.n_min = max(1, self.fec_stages)
        self.indices = self.outs[0][0]
        self.kind = self.outs[0][3] if dtx is not None else None
        self.n_eff, self.distortion = self.outs[0][-2:] if vbr is not None else (None, None)

    def _init_state(self) -> None:
        n, m, T = self.n, self.fec_stages, self.frames
        self._prev = self._run = self._ctr = self._credit = self._fa = self._fec_on = self._rx = self._rc = self._n_ceil = self._level = None
        self._cp = self._tx = None
        # the bytes of a sent row: the headed packet, with srtp its tag behind it
        self._sent_bytes = wire.srtp_bytes(n, m, T) if self.srtp is not None else wire.transport_bytes(n, m, T)
        if m:
            # per parity, per slot: valid, then the first m stages x T frames of its last encoded hop (the hop of parity p reads
            # row p and writes row p ^ 1)
            self._prev = self._slot_state(1 + m * T, pingpong=True)
        if self.dtx is not None:
            # per slot: the DTX run counter (updated in place by hilc_dtx_encode once per hop)
            self._run = self._slot_state()
            self._level_thr = torch.from_numpy(dtx_def.level_table()).to(self.device)
        if self.header:
            # per parity, per slot: the hop counter (the hop of parity p reads row p and writes row p ^ 1)
            self._ctr = self._slot_state(pingpong=True)
        if self.vbr is not None and self.vbr.cap_kbps is not None:
            # per slot: the token bucket's credit in bits (updated in place by hilc_vbr_select once per hop); cleared = full
            # (a clearing zeroes it and then fills it, as it did before the allocator: its launches stay what they were)
            self._credit = self._slot_state(cleared=self._vbr_bits[2], rezero=True)
        if self.fec_adapt is not None:
            # per slot: the adapt row (report.FA_*, updated in place by hilc_fec_adapt once per hop) and its switch; cleared = the
            # row zero but for FA_ON = initial_on
            on0 = int(self.fec_adapt.initial_on)
            self._fa = self._slot_state(report_def.FA_WORDS, cleared={report_def.FA_ON: on0})
            self._fec_on = self._slot_state(cleared=on0)
        if self.rtx is not None:
            # per slot: the history (tags and rows of headed packets, updated in place by hilc_rtx_step once per hop) and its counter
            # row; per parity: the retransmission rows and their byte counts
            tb, history, per_hop = self._sent_bytes, self.rtx.history, self.rtx.per_hop
            self._rx = (self._slot_state(history), self._slot_state(history, (tb + 3) // 4), self._slot_state(rtx_def.RX_WORDS))
            self._rx_out = self._slot_state(per_hop, tb, dtype=torch.uint8, pingpong=True)
            self._rx_nbytes = self._slot_state(per_hop, pingpong=True)
        if self.rate is not None:
            # per slot: the rate row (rate.RC_*, updated in place by hilc_rate_ceiling and hilc_rate_charge once per hop) and its
            # ceiling; cleared = the row zero but for the start rate and a full bucket, the ceiling n
            start = self._rate_bits.start_bits
            self._rc = self._slot_state(rate_def.RC_WORDS, cleared={rate_def.RC_RATE_Q8: 256 * start,
                                                                     rate_def.RC_CREDIT: self.rate.burst_hops * start})
            self._n_ceil = self._slot_state(cleared=int(n))
        if self.cap is not None:
            # per slot: the cap row (bwe.CP_*, updated in place by hilc_rate_cap once per hop)
            self._cp = self._slot_state(bwe_def.CP_WORDS)
        if self.srtp is not None:
            # per slot: the key row (srtp.KEY_*, uploaded when set_key / clear_key changed it) and the TX row (srtp.TX_*, updated in
            # place by hilc_srtp_protect once per hop)
            self._init_keys()
            self._tx = self._slot_state(srtp_def.TX_WORDS)
        if self._measure_level:
            # per parity, per slot: the hop's level (the hop of parity p writes row p); cleared = silence
            self._level = self._slot_state(pingpong=True, cleared=level_def.MAX_LEVEL)
            self._level_thr = torch.from_numpy(dtx_def.level_table()).to(self.device)

    def _block(self, streams: int) -> StateBlock:
        return StateBlock(self.model, streams, self.device, "enc", self._history)

    @property
    def state_bytes(self) -> int:
        """bytes of the two encoder-only state blocks"""
        return sum(b.nbytes for b in self.gstate[0])

    def _chain(self, g: int, p: int) -> Tuple[Tensor, Tensor, Tensor]:
        m = self.model
        src, dst = self.gstate[0][p], self.gstate[0][p ^ 1]
        action, hold, n_clip = (self.action, self.hold, self.n_slot) if self.sessions else (None, None, None)
        if self.sessions:
            ops.state_slots_apply(src.buffer, src.layout, action, self.records)
        x = self.x
        if self.rs is not None:
            x = ops.resample_poly(x, self.rs_taps, self.rs.L, self.rs.M, hist=src.hist, hist_out=dst.hist)
        if self._level is not None:
            ops.audio_level(x, self._level_thr, self._level[p], hold)
        with ops.sched_workspace(self.sched[0]):
            with engine.spectra_side_stream(self.spec_side[0]):
                z, _ = m.encoder(x, *src.codec_enc, cache_out=dst.codec_enc)
            if self.rate is not None:
                # in front of the quantiser: hilc_fec_adapt (it reads nothing the quantiser writes) so that the ceiling sees this hop's
                # switch, then the ceiling, which stands in for the per-stream n from here on
                if self.fec_adapt is not None:
                    ops.fec_adapt(self._prev[p], self._fa, self._fec_on, self.fec_stages, self.frames, self.fec_adapt,
                                  self.stage.row["report"], action, hold)
                if self.cap is not None:
                    # directly in front of the ceiling: the rate it moves and fills the bucket with is at most the receiver's cap
                    ops.rate_cap(self._cp, self._rc, self.cap, self._rate_bits.min_bits, self._rate_bits.max_bits,
                                 self.stage.row["cap"], action, hold)
                ops.rate_ceiling(self._rc, self._n_ceil, self.n, self.frames, self.fec_stages, self.header, self.rate,
                                 self.stage.row["report"], action, hold, n_clip, self._prev[p] if self.fec_stages else None)
                n_clip = self._n_ceil
            idx = m.quantizer(z, self.n, n_clip=n_clip)
        if self.fec_adapt is not None and self.rate is None:
            # ahead of the packer (and of VBR): a slot whose switch is off loses the valid word of the row the packer reads
            ops.fec_adapt(self._prev[p], self._fa, self._fec_on, self.fec_stages, self.frames, self.fec_adapt, self.stage.row["report"],
                          action, hold)
        n_eff = distortion = None
        if self.vbr is not None:
            stage_bits, rate_bits, burst_bits = self._vbr_bits
            n_eff, distortion = ops.vbr_select(z.contiguous(), idx, m.quantizer._tables(z.device).codebooks, self._vbr_lo, self.vbr.rho,
                                               stage_bits, rate_bits, burst_bits, n_clip, action, hold, self._credit)
            n_clip = n_eff
        if self.fec_stages:
            packets, nbytes = ops.pack_codes_10bit_fec(idx, self._prev[p], self._prev[p ^ 1], self.fec_stages, n_clip, action, hold)
        else:
            packets, nbytes = ops.pack_codes_10bit(idx, n_clip)
        kind = None
        if self.dtx is not None:
            d = self.dtx
            kind = ops.dtx_encode(x, self._run, packets, nbytes, idx, self._level_thr, d.thr_vad, d.order, d.hangover, d.sid_interval,
                                  action, hold, self._prev[p ^ 1] if self.fec_stages else None)
        if self.sessions:
            ops.state_slots_hold(src.buffer, dst.buffer, src.layout, hold, indices=idx, packets=packets, nbytes=nbytes)
        if self.header:
            packets, nbytes = ops.packet_header(packets, nbytes, self._ctr[p], self._ctr[p ^ 1], self.n, self.fec_stages, self.frames,
                                                n_clip, kind, action, hold)
        if self.srtp is not None:
            # behind the header, in front of the history and the bill: the history holds ciphertext, so a retransmission is the packet
            # that was sent byte for byte, and the bucket pays for the tag
            packets, nbytes = ops.srtp_protect(packets, nbytes, self._keys_dev, self._tx, action=action)
        if self.rtx is not None:
            # the graph's last launch: this hop's headed packets enter the history, this hop's NACKs are answered from it
            ops.rtx_step(packets, nbytes, *self._rx, self._rx_out[p], self._rx_nbytes[p], self.stage.row["nack_base"],
                         self.stage.row["nack_bitmap"], action)
        if self.rate is not None:
            # the graph's last launch: what the slot really sent on this hop, retransmissions included, leaves its bucket
            ops.rate_charge(nbytes, self._rc, self.rate, self._rx_nbytes[p] if self.rtx is not None else None)
        out = (idx, packets, nbytes) if kind is None else (idx, packets, nbytes, kind)
        return out if n_eff is None else out + (n_eff, distortion)

    @property
    def audio_level(self) -> Tensor:
        """int32 `[B]` device view: the level of each slot's last hop, -dBov in 1 dB steps (audio_level=True only; a held slot: 127);
        overwritten by the next-but-one `step`.  Read-only: written by the graph."""
        self._need(self._level is not None, "audio_level", "audio_level=True")
        return self._level[self.parity ^ 1]

    @property
    def credit(self) -> Tensor:
        """int32 `[B]` device view: each slot's token-bucket credit in bits after the last hop (vbr with a cap only).  Read-only:
        written by the graph."""
        self._need(self._credit is not None, "credit", "vbr=VbrConfig(..., cap_kbps=...)")
        return self._credit

    @property
    def hop_index(self) -> Tensor:
        """int32 `[B]` device view: each slot's hop counter, the h its next sent packet carries unless a start intervenes (header=True
        only).  Read-only: written by the graph."""
        self._need(self.header, "hop_index", "header=True")
        return self._ctr[self.parity]

    @property
    def fec_on(self) -> Tensor:
        """int32 `[B]` device view: each slot's FEC switch after the last hop (fec_adapt only).  Read-only: written by the graph."""
        self._need(self._fec_on is not None, "fec_on", "fec_adapt=FecAdaptConfig(...)")
        return self._fec_on

    @property
    def fec_adapt_state(self) -> Tensor:
        """int32 `[B, report.FA_WORDS]` device view: each slot's adapt row after the last hop (report.FA_*; fec_adapt only).
        Read-only: written by the graph."""
        self._need(self._fa is not None, "fec_adapt_state", "fec_adapt=FecAdaptConfig(...)")
        return self._fa

    @property
    def n_ceil(self) -> Tensor:
        """int32 `[B]` device view: the most stages each slot's bucket paid for on the last hop (rate only; a held slot: its own n).
        Read-only: written by the graph."""
        self._need(self._n_ceil is not None, "n_ceil", "rate=RateConfig(...)")
        return self._n_ceil

    @property
    def rate_state(self) -> Tensor:
        """int32 `[B, rate.RC_WORDS]` device view: each slot's rate row after the last hop (rate.RC_*; rate only; `rate.kbps(row,
        frames)` gives RC_RATE_Q8 in kbps).  Read-only: written by the graph."""
        self._need(self._rc is not None, "rate_state", "rate=RateConfig(...)")
        return self._rc

    @property
    def cap_state(self) -> Tensor:
        """int32 `[B, bwe.CP_WORDS]` device view: each slot's cap row after the last hop (bwe.CP_*; cap only).  Read-only: written by
        the graph."""
        self._need(self._cp is not None, "cap_state", "cap=CapConfig(...)")
        return self._cp

    @property
    def srtp_state(self) -> Tensor:
        """int32 `[B, srtp.TX_WORDS]` device view: each slot's TX row after the last hop (srtp.TX_*; srtp only).  Read-only: written
        by the graph."""
        self._need(self._tx is not None, "srtp_state", "srtp=SrtpConfig()")
        return self._tx

    @property
    def rtx_packets(self) -> Tensor:
        """uint8 `[B, per_hop, wire.transport_bytes(n, m, T)]` (with srtp: `wire.srtp_bytes(n, m, T)`) device view: each slot's
        retransmissions of the last hop, in request order, zero past their lengths (rtx only); overwritten by the next-but-one
        `step`.  Read-only: written by the graph."""
        self._need(self.rtx is not None, "rtx_packets", "rtx=RtxConfig(...)")
        return self._rx_out[self.parity ^ 1]

    @property
    def rtx_nbytes(self) -> Tensor:
        """int32 `[B, per_hop]` device view: the byte counts of `rtx_packets` (0: the row is unused).  Read-only: written by the
        graph."""
        self._need(self.rtx is not None, "rtx_nbytes", "rtx=RtxConfig(...)")
        return self._rx_nbytes[self.parity ^ 1]

    @property
    def rtx_state(self) -> Tensor:
        """int32 `[B, rtx.RX_WORDS]` device view: each slot's counter row after the last hop (rtx.RX_*; rtx only).  Read-only:
        written by the graph."""
        self._need(self.rtx is not None, "rtx_state", "rtx=RtxConfig(...)")
        return self._rx[2]

    def _feedback(self, name: str, pair, width: int, word, enabled: bool, needs: str) -> dict:
        """step's `reports` / `nacks` = (slots, blobs) checked before anything is launched -> {slot: word(blob)}; a slot named
        twice keeps its last blob"""
        if pair is None:
            return {}
        self._need(enabled, f"step({name}=...)", needs)
        try:
            slots, blobs = pair
        except (TypeError, ValueError):
            raise ValueError(f"{name}: a pair (slots, blobs) expected") from None
        for what, v in (("slots", slots), ("blobs", blobs)):
            if isinstance(v, Tensor) and v.is_cuda:
                raise ValueError(f"{name}: {what} must be on the host, not a device tensor")
        slots = [int(s) for s in (slots.reshape(-1).tolist() if isinstance(slots, Tensor) else slots)]
        if isinstance(blobs, Tensor):
            if blobs.dtype != torch.uint8 or blobs.dim() != 2 or blobs.shape[1] != width:
                raise ValueError(f"{name}: blobs must be uint8 [A, {width}] or {width}-byte bytes objects")
            blobs = [bytes(row) for row in blobs.tolist()]
        else:
            blobs = list(blobs)
        if len(blobs) != len(slots):
            raise ValueError(f"{name}: {len(slots)} slots but {len(blobs)} {name}")
        words = {}
        for s, blob in zip(slots, blobs):
            if not 0 <= s < self.queue.batch:
                raise ValueError(f"{name}: slot {s} outside [0, {self.queue.batch})")
            words[s] = word(blob)                                           # ValueError: not `width` bytes
        return words

    def _report_words(self, reports) -> dict:
        return self._feedback("reports", reports, wire.REPORT_BYTES, lambda blob: report_def.report_word(*wire.parse_report(blob)),
                              self.fec_adapt is not None or self.rate is not None, "fec_adapt=FecAdaptConfig(...) or rate=RateConfig(...)")

    def _nack_words(self, nacks) -> dict:
        return self._feedback("nacks", nacks, wire.NACK_BYTES, lambda blob: rtx_def.nack_words(*wire.parse_nack(blob)),
                              self.rtx is not None, "rtx=RtxConfig(...)")

    def _cap_words(self, caps) -> dict:
        return self._feedback("caps", caps, wire.CAP_BYTES, lambda blob: bwe_def.cap_word(*wire.parse_cap(blob)),
                              self.cap is not None, "cap=CapConfig(...)")

    def _extra_rows(self) -> Tuple[str, ...]:
        return (("report",) * (self.fec_adapt is not None or self.rate is not None) + ("nack_base", "nack_bitmap") * (self.rtx is not None)
                + ("cap",) * (self.cap is not None))

    def _extra_pending(self) -> bool:
        return bool(self._reports or self._nacks or self._caps)

    def _put_extra(self, st: ControlStage) -> None:
        """the report row: this hop's reports, 0 elsewhere (a report applies to exactly one hop, like an action: the upload after a
        hop with reports clears them); with fec_adapt and rate, one report feeds both launches"""
        if "report" in st.h_row and not self._reports:
            st.put_one_hop("report")
        elif "report" in st.h_row:
            slots = np.fromiter(self._reports, dtype=np.int64, count=len(self._reports))
            st.put_one_hop("report", slots, np.fromiter(self._reports.values(), dtype=np.int32, count=len(slots)))
            self._reports = {}
        if self.rtx is not None and not self._nacks:
            st.put_one_hop("nack_base")
            st.put_one_hop("nack_bitmap")
        elif self.rtx is not None:
            # the NACK rows, likewise: this hop's NACKs, (0, 0) elsewhere; one indexed write per row: a full batch of NACKs is a
            # thousand slots
            slots = np.fromiter(self._nacks, dtype=np.int64, count=len(self._nacks))
            words = np.array(list(self._nacks.values()), dtype=np.int32)
            st.put_one_hop("nack_base", slots, words[:, 0])
            st.put_one_hop("nack_bitmap", slots, words[:, 1])
            self._nacks = {}
        if self.cap is not None and not self._caps:
            st.put_one_hop("cap")
        elif self.cap is not None:
            # the cap row, likewise: this hop's caps, 0 elsewhere
            slots = np.fromiter(self._caps, dtype=np.int64, count=len(self._caps))
            st.put_one_hop("cap", slots, np.fromiter(self._caps.values(), dtype=np.int32, count=len(slots)))
            self._caps = {}

    def reset(self, cache_enc: Optional[Sequence[Tensor]] = None, cache_dec: Optional[Sequence[Tensor]] = None) -> None:
        self._reports, self._nacks, self._caps = {}, {}, {}
        if self.srtp is not None:
            self._keys.reset()                # every key and, with the scratch rows, every TX row
        super().reset(cache_enc, cache_dec)

    def step(self, x: Tensor, hold=None, reports=None, nacks=None, caps=None) -> Tuple[Tensor, Tensor]:
        """`reports` (fec_adapt or rate only): (slots, blobs), this hop's receiver reports — A host ints, and a uint8 `[A, 3]` host tensor or a
        sequence of 3-byte `bytes` (wire.pack_report).  `nacks` (rtx only): (slots, blobs) likewise, this hop's NACKs, 4 bytes each
        (wire.pack_nack).  `caps` (cap only): (slots, blobs) likewise, this hop's rate caps, 3 bytes each (wire.pack_cap)"""
        self._reports = self._report_words(reports)
        self._nacks = self._nack_words(nacks)
        self._caps = self._cap_words(caps)
        self._send_keys()
        try:
            out = super().step(x, hold)
        finally:
            self._reports, self._nacks, self._caps = {}, {}, {}       # taken by the upload, or dropped with a step that raised before it
        self.indices, packets, nbytes = out[:3]
        if self.dtx is not None:
            self.kind = out[3]
        if self.vbr is not None:
            self.n_eff, self.distortion = out[-2:]
        return packets, nbytes

    def start(self, slot: int, cache_enc: Optional[Sequence[Tensor]] = None, n: Optional[int] = None) -> None:
        """At the next step, slot `slot` begins a fresh stream or resumes one from its 22 encoder caches (B = 1 tensors, host or
        device; 23 with `input_rate`, the resampler's history last); `n`: its number of quantiser stages (default: the graph's n).
        With `srtp`: ValueError unless `set_key(slot, ...)` was called since the slot's previous start"""
        self._start_keyed(slot, lambda: _Hop.start(self, slot, cache_enc, None, n))

    def export(self, slot: int) -> List[Tensor]:
        """the current 22 encoder caches of slot `slot` as B = 1 device tensors (23 with `input_rate`: the resampler's history last)"""
        return super().export(slot)[0]


class GraphedDecodeHop(_Hop):
    """The receiver: one graph replay per hop turns per-stream 10-bit packets (`wire.packet_bytes(n, frames)` bytes per row)
    into `[B,1,320 frames]` samples.  `step(packets, n_per_stream)`: `packets` uint8 `[B, packet_bytes(n, frames)]` on the host
    or the device, `n_per_stream` B host ints in [1, n] (checked here: ValueError).  Both go into one static device buffer (one
    copy from the host; packets already on the device take a device copy), then the graph runs (hilc_state_slots_apply if
    `sessions`) -> hilc_rvq_decode_packed -> streaming decoder on a ping-pong pair of DECODER-ONLY state blocks (the 30 decoder
    caches).  The returned waveform is a static view that the next-but-one `step` overwrites.
    `frames` may differ from the sender's T (the reference's `num_frames`): packets of consecutive sender hops are re-framed by
    the caller (`wire.unpack_stream_packet` / `pack_stream_packet`).  The per-stream n arrives with every hop, so there is no
    `set_bitrate`; sessions: `start(slot, cache_dec=None)`, `export(slot) -> cache_dec`, and held streams as in GraphedHop:
    `step(packets, n_per_stream, hold=slots)` (a late or lost packet: the slot does not advance, its packet row and its
    n_per_stream entry are not read or checked, its wav row is 0) and `stop(slot)`.
    `conceal=True` (needs `sessions`): `step(..., lost=slots)` conceals the slots whose packet did not arrive instead of holding
    them.  Each slot keeps the codes of the last frame of the last packet it received; a lost hop is decoded from those codes
    repeated over the hop (with that packet's n) and faded from G[k] to G[k+1] over the hop (k = hops lost in a row before it,
    G[k] = (F - k) / F, F = `fade_hops`); the first received hop after k >= 1 lost ones fades from G[k] back to 1.  A lost slot
    with nothing received since its start, or with k = F, is held by the graph itself (wav 0, caches unchanged).  Ramps and
    tables: `wire.conceal_tables`; substitute packets: `wire.conceal_packet`.  `concealed` is each slot's k after the last step.
    Graph: hilc_conceal_prepare after hilc_state_slots_apply (rewrites this hop's packet, n and hold rows of concealed slots),
    hilc_conceal_gain after the decoder.  `conceal=False` captures exactly the graph of earlier rounds.
    `output_rate` (resample.RATES; default 24 000 = no resampler): the graph converts the decoded (and, with `conceal`, faded) hop
    with one hilc_resample_poly launch before hilc_state_slots_hold, and `step` returns `[B,1,resample.hop_samples(frames,
    output_rate)]` samples at that rate (held rows 0).  Its per-stream history is one more cache, the LAST of the decoder list:
    `export`, `start` and `cache_dec` then hold 31 caches, `start(slot)` zeroes it and a held, stopped or faded-out slot keeps it.
    `fec_stages` = m >= 1 (in-band FEC, at most n; the sender's m, and `frames` must equal the sender's T: FEC packets are not
    re-framed): `packets` rows are `wire.fec_packet_bytes(n, m, frames)` wide, with or without a redundant section.
    `step(..., fec=slots)` names the slots whose packet for this hop was lost but whose NEXT packet has arrived: their rows hold
    that next packet and their n_per_stream entries its primary n_b, in [m, n].  Such a slot is decoded from the next packet's
    redundant section at n = m, bit for bit as if `wire.fec_redundant(next, n_b, m, frames)` had arrived with n = m (wav, caches
    and, with `conceal`, the concealment state: run 0, the fade-in after a loss, the stored frame).  Other slots are decoded from
    their primary section (`wire.fec_primary`).  Graph: one hilc_fec_select after hilc_state_slots_apply compacts the wide rows
    into the rows the unchanged concealment and dequantiser kernels read.  `fec_stages=0` captures exactly the graph without FEC.
    `cng_order` = K (needs `sessions`; a SID of 1 + K bytes must fit `wire.packet_bytes(n, frames)`): comfort noise for senders in DTX
    (dtx.py).  `step(..., sid=slots, silent=slots)`: a `sid` slot's row holds a SID packet (its n_per_stream entry is not read or
    checked), a `silent` slot received nothing because its stream is in DTX.  A `sid` slot stores the SID's level and coefficients and
    produces this hop's noise (filter memory from zero after a decoded hop, else carried over); a `silent` slot produces noise from
    the stored SID, or is held (wav 0) when it has none.  A slot producing noise leaves its decoder caches and, with `conceal`, its
    concealment state as they were; with `output_rate` the noise goes through the resampler, whose history advances.  Any decoded
    slot (received, concealed or FEC) forgets its SID; a held slot keeps it; `start` clears it; `export` and a resume carry none.
    Graph: the host marks `sid` / `silent` slots 2 / 3 in the hold row (so every existing kernel treats them as held); one
    hilc_cng_synth writes the noise — after the final hilc_state_slots_hold without `output_rate`; with it, before the resampler,
    followed by one hilc_state_slots_hold over the decoder caches (not the resampler history) of the slots that produced noise.
    `cng_order=None` captures exactly the graph without comfort noise.
    `jitter` = jitter.JitterConfig(depth=D, capacity=C) (needs `sessions`; `frames` must equal the sender's T): a device-side jitter
    buffer for packets with the transport header of GraphedEncodeHop(header=True).  `play(slots, packets, nbytes, hold=None)` takes
    this hop's arrivals in push order — `slots` and `nbytes` A host ints, `packets` uint8 `[A, wire.transport_bytes(n, m, frames)]` on
    the host or the device, 0 <= A <= `max_arrivals` (default 2 B) — and the graph's first launch, hilc_jitter_step, keeps them in a
    per-slot ring of C entries and decides what each slot plays (jitter.py): its packet D hops after the first one arrived, a SID or
    DTX silence as comfort noise, a gap from the next packet's redundant section, concealed (`conceal`) or held.  It writes the n,
    lost and fec rows and the packet matrix that `step` uploads, so the rest of the graph is unchanged and the output is a pure
    function of the arrival trace.  Host holds and stops pause a slot's playout (its arrivals are still buffered); `start` clears
    its jitter state; `export` and a resume carry none; `jitter_state` is the int32 `[B, jitter.ST_WORDS]` state rows.  With `jitter`,
    `step` raises RuntimeError; without it, `play` does.  `jitter=None` captures exactly the graph without the jitter buffer.
    `jitter=JitterConfig(..., adapt=jitter.AdaptConfig(...))`: an adaptive playout clock (jitter.py: a slot follows a sender whose
    clock drifts, a burst of delay or a sender restart by inserting a hop, skipping an entry or anchoring again).  The first launch
    is hilc_jitter_adapt_step in place of hilc_jitter_step, the launch count is the same; `jitter_adapt` is the int32 `[B,
    jitter.AD_WORDS]` adapt rows, cleared with the jitter state.  `adapt=None` captures exactly the graph of the fixed buffer.
    `mix` = mixer.MixConfig(top_k) (needs `sessions`): a conference bridge's room mixer at the tail of the graph (mixer.py).  `join(slot,
    room)` / `leave(slot)` put a slot into a room (an id in [0, B)) or into none, `rooms` is the host's membership tuple (-1: none;
    initially every slot; `stop` does not leave a room).  Membership is a pinned int32 row; when it has changed since the last hop, the
    whole row goes to a device row captured by address, on the replay stream before the replay (not through the control stage).
    `step` and `play` return what they return without `mix`; after them `mixed` (fp32 `[B,1,L]`, L the returned waveform's length, so at
    `output_rate`) holds every slot's mix of its room's `top_k` highest-scoring other members — a static view that the next-but-one call
    overwrites, like the waveform, and that a GraphedEncodeHop on the same device takes as its `step(x)`: a bridge is two replays per
    hop and no host copy.  `speakers` (int32 `[B]`) marks the slots among their room's top_k, `levels` (float64 `[B]`) is the peak-hold
    score of every slot; a `start` clears a slot's score inside the graph.  Graph: hilc_mix_levels and hilc_mix_rooms are the last two
    launches, after the final hilc_state_slots_hold and the hilc_cng_synth behind it: comfort noise is mixed as noise, a held slot as
    zeros, and a held listener still gets its mix.  `mix=None` captures exactly the graph without the mixer.
    `MixConfig(top_k, level=mixer.LevelConfig(...))`: per-speaker levelling, one more launch (hilc_mix_gains behind hilc_mix_levels):
    every slot's gain follows its smoothed power towards the target level, hops under the gate do not count, and the speakers' rows
    enter the sums with their gains; `gains` (float64 `[B, 2]`) is every slot's gain at the hop's start and end.
    `MixConfig(top_k, limit=mixer.LimitConfig(...))`: a per-listener limiter with state in place of the clamp; `limiter_state` (float64
    `[B, 2]`) is every listener's envelope and gain.  With either, hilc_mix_rooms_dyn is the last launch in place of hilc_mix_rooms; a
    `start` or a resume clears a slot's rows inside the graph; `export` and a resume carry none.  `MixConfig(top_k)` captures exactly the
    two launches above.
    `report` = report.ReportConfig(window, interval) (needs `jitter`: the rule reads the jitter state, the explicit `step()` has no
    report): receiver reports (report.py).  One hilc_rx_report directly after the jitter step classes each slot's hop from its jitter
    counters (decoded, repaired by FEC, lost, noise), keeps a sliding window of the last `window` decoded / repaired / lost hops and
    every `interval` classed hops emits a report (seq, loss_q8, residual_q8: `wire.pack_report`).  It only observes: wav, caches and
    every other state are those of the receiver without it.  `reports` (uint8 `[B, 3]`: each slot's latest report, unchanged between
    reports), `report_due` (int32 `[B]`: 1 on the hop a report was emitted) and `report_state` (int32 `[B, report.RP_WORDS]`) are device
    views; a `start` clears a slot's row, report and flag inside the graph; `export` and a resume carry none.  `report=None` captures
    exactly the graph without it.
    `nack` = rtx.NackConfig(rtt_hops, retry_hops, max_requests, skip_fecable) (needs `jitter`: the rule reads the ring): negative
    acknowledgements (rtx.py).  One hilc_nack_build directly after the jitter step, beside hilc_rx_report and independent of it, finds
    the holes of each slot's ring that a retransmission can still fill — not those that would come too late, lie in DTX silence or (with
    `skip_fecable`) are repaired by FEC — and asks for each at most `max_requests` times, `retry_hops` apart: `nacks` (uint8 `[B, 4]`:
    each slot's latest NACK, `wire.parse_nack`, unchanged between NACKs), `nack_due` (int32 `[B]`: 1 on the hop a NACK was emitted) and
    `nack_state` (int32 `[B, rtx.NK_WORDS]`) are device views.  It only observes: wav, caches and every other state are those of the
    receiver without it.  The sender's answers (GraphedEncodeHop(rtx=...)) are pushed with `play()` like any packet.  A `start` or a
    resume clears a slot's row, NACK and flag inside the graph; `export` and a resume carry none.  `nack=None` captures exactly the
    graph without it.
    `bwe` = bwe.BweConfig(min_kbps, max_kbps, window, rate_window, alpha_q8, beta_q8, increase_q16, interval, reset_ticks) (needs
    `jitter`: the rule reads `play()`'s arrivals; at most bwe.MAX_FRAMES frames and a cap of at most 65535 bits per hop: ValueError
    otherwise): the delay-based bandwidth estimate (bwe.py).  `play(slots, packets, nbytes, hold=None, times=...)` then takes each
    arrival's tick — A host ints in units of 1/24000 s, any origin, taken mod 2^32 — which travel in the control stage's single copy as
    an int32 array parallel to the arrival records.  One hilc_rx_bwe directly after the jitter step, beside hilc_rx_report and
    hilc_nack_build and independent of both, measures each slot's delay gradient (how much further apart its packets arrive than they
    were sent: exact from the header's hop index), runs the over-use detector and an AIMD controller on the incoming rate and emits the
    slot's cap (seq, bits per hop: `wire.pack_cap`) every `interval` hops and at once after a decrease: `caps` (uint8 `[B, 3]`: each
    slot's latest cap, unchanged between caps), `cap_due` (int32 `[B]`: 1 on the hop a cap was emitted) and `bwe_state` (int32 `[B,
    bwe.BW_WORDS]`; `bwe.kbps(bwe_state, frames)` on the host) are device views.  The caps go to the sender:
    GraphedEncodeHop(cap=...).step(caps=).  It only observes: wav, caches and every other state are those of the receiver without it.
    A `start` or a resume clears a slot's row, cap and flag inside the graph; `export` and a resume carry none.  `bwe=None` captures
    exactly the graph without it, with today's stage layout and upload.
    `srtp` = srtp.SrtpConfig() (needs `jitter`): packet protection, the receiving side (srtp.py: the rules).  `play()` takes protected
    rows of `wire.srtp_bytes(n, m, frames)` bytes and the stage's arrival region is sized for them; hilc_srtp_unprotect is the graph's
    first launch and writes the plain records (a device-only buffer of the plain width) that every later launch reads: the jitter step
    and hilc_rx_bwe are handed that buffer and are otherwise what they were.  An arrival that is too short, a replay (64-packet window)
    or fails its tag comes out as a record of 0 bytes, which the jitter step and `bwe` drop as malformed; `bwe` therefore measures the
    plain sizes, 80 bits per packet under the wire.  `srtp_state` (int32 `[B, srtp.RX_WORDS]`) is a device view.  `set_key`, `clear_key`
    and the fresh-key rule of `start` are the sender's; `roc` starts a late joiner at a known rollover counter.  `srtp=None` captures
    exactly the graph without it, with today's stage layout and upload."""

    def __init__(self, model, batch: int, frames: int, n: int, device: torch.device, warmup: int = 2, sessions: bool = False,
                 max_loads_per_hop: int = 4, conceal: bool = False, fade_hops: int = 4, output_rate: int = BASE_RATE,
                 fec_stages: int = 0, cng_order: Optional[int] = None, jitter: Optional[JitterConfig] = None,
                 max_arrivals: Optional[int] = None, mix: Optional[MixConfig] = None,
                 report: Optional[report_def.ReportConfig] = None, nack: Optional[rtx_def.NackConfig] = None,
                 bwe: Optional[bwe_def.BweConfig] = None, srtp: Optional[srtp_def.SrtpConfig] = None):
        self.batch, self.frames = int(batch), int(frames)
        self.output_rate = int(output_rate)
        self.rs, self._history = None, 0
        if self.output_rate != BASE_RATE:
            hop_samples(self.frames, self.output_rate)                  # ValueError: frames do not make whole samples at that rate
            self.rs = design(BASE_RATE, self.output_rate)
            self.rs_taps = device_taps(self.rs, device)
            self._history = self.rs.history
        if not 1 <= int(n) <= len(model.dequantizer.layers):
            raise ValueError(f"n = {n} outside [1, {len(model.dequantizer.layers)}]")
        self.conceal = bool(conceal)
        _needs("GraphedDecodeHop(conceal=True)", sessions or not self.conceal, "sessions=True")
        self.fade_hops = _int_arg("fade_hops", fade_hops, 1)
        self.fec_stages = _fec_stages(fec_stages, int(n))
        self.cng_order = None
        if cng_order is not None:
            self.cng_order = _int_arg("cng_order", cng_order, 0, dtx_def.MAX_ORDER)
            _needs("GraphedDecodeHop(cng_order=...)", sessions, "sessions=True")
            dtx_def.check_order(self.cng_order, wire.packet_bytes(int(n), self.frames), "GraphedDecodeHop(cng_order=...)")
        self.jitter = _config_arg("jitter", jitter, JitterConfig)
        _needs("GraphedDecodeHop(jitter=...)", sessions or jitter is None, "sessions=True")
        _needs("GraphedDecodeHop(max_arrivals=...)", jitter is not None or max_arrivals is None, "jitter=JitterConfig(...)")
        self.mix = _config_arg("mix", mix, MixConfig)
        _needs("GraphedDecodeHop(mix=...)", sessions or mix is None, "sessions=True")
        self.report = _config_arg("report", report, report_def.ReportConfig)
        _needs("GraphedDecodeHop(report=...)", jitter is not None or report is None,
               "jitter=JitterConfig(...): the reports are made from the jitter state")
        self.nack = _config_arg("nack", nack, rtx_def.NackConfig)
        _needs("GraphedDecodeHop(nack=...)", jitter is not None or nack is None,
               "jitter=JitterConfig(...): the NACKs are made from the jitter ring")
        self.bwe = _config_arg("bwe", bwe, bwe_def.BweConfig)
        _needs("GraphedDecodeHop(bwe=...)", jitter is not None or bwe is None,
               "jitter=JitterConfig(...): the estimate is made from play()'s arrivals")
        if bwe is not None:
            bwe_def.bits(bwe, self.frames)                              # ValueError: bounds past a uint16 cap, too many frames
            if wire.transport_bytes(int(n), self.fec_stages, self.frames) > bwe_def.MAX_ROW_BYTES:
                raise ValueError(f"GraphedDecodeHop(bwe=...): a headed packet of more than {bwe_def.MAX_ROW_BYTES} bytes")
        self.srtp = _config_arg("srtp", srtp, srtp_def.SrtpConfig)
        _needs("GraphedDecodeHop(srtp=...)", jitter is not None or srtp is None,
               "jitter=JitterConfig(...): play()'s arrivals are what is unprotected")
        if srtp is not None and wire.transport_bytes(int(n), self.fec_stages, self.frames) > srtp_def.MAX_ROW_BYTES:
            raise ValueError(f"GraphedDecodeHop(srtp=...): a headed packet of more than {srtp_def.MAX_ROW_BYTES} bytes")
        super().__init__(model, self.batch, int(n), device, 1, sessions, max_loads_per_hop)
        self.stride = wire.packet_bytes(self.n + self.fec_stages, self.frames)
        B = self.batch
        if jitter is not None:
            self._init_jitter(jitter, 2 * B if max_arrivals is None else max_arrivals)
        else:
            # ONE device buffer, captured by address: action per slot, n per slot, 1 where the slot is held, (conceal) 1 where its
            # packet was lost, (fec) 1 where it is decoded from the next packet's redundant section, the packets, the staged records
            rows = ["action", "n_slot", "hold"] + ["lost"] * self.conceal + ["fec"] * (self.fec_stages > 0)
            st = self.stage = self._new_stage(rows, (B * self.stride + 3) // 4)
            self.n_slot, self.lost, self.fec = st.row["n_slot"], st.row.get("lost"), st.row.get("fec")
            self.packets = st.payload.view(torch.uint8)[:B * self.stride].view(B, self.stride)
            self._h_packets = st.h_payload.view(torch.uint8)[:B * self.stride].view(B, self.stride)
        self.n_slot.fill_(self.n)
        if self.conceal:
            # per slot: run k, has-codes, stored n, the stored frame's n codes (updated in place by hilc_conceal_prepare once per hop)
            self._conceal = self._slot_state(self.n + wire.CONCEAL_CODES)
            gains, weights = wire.conceal_tables(self.fade_hops, HOP * self.frames)
            self._gains, self._weights = gains.to(device), weights.to(device)
        if self.cng_order is not None:
            # per slot: the CN state row (dtx.state_words, updated in place by hilc_cng_synth once per hop); device-only: the slots
            # that produced noise this hop (their decoder caches are copied back)
            self._cn = self._slot_state(dtx_def.state_words(self.cng_order))
            self._cn_gains = torch.from_numpy(dtx_def.gain_table()).to(device)
            self._restore = self._slot_state()
        if report is not None:
            # per slot: the report row (report.RP_*, updated in place by hilc_rx_report once per hop), its latest report, its due flag
            self._rp = self._slot_state(report_def.RP_WORDS)
            self._rp_bytes = self._slot_state(wire.REPORT_BYTES, dtype=torch.uint8)
            self._rp_due = self._slot_state()
        if nack is not None:
            # per slot: the NACK row (rtx.NK_*, updated in place by hilc_nack_build once per hop), its latest NACK, its due flag
            self._nk = self._slot_state(rtx_def.NK_WORDS)
            self._nk_bytes = self._slot_state(wire.NACK_BYTES, dtype=torch.uint8)
            self._nk_due = self._slot_state()
        if bwe is not None:
            # per slot: the estimate row (bwe.BW_*, updated in place by hilc_rx_bwe once per hop), its latest cap, its due flag; cleared
            # = the row zero but for the estimate at max_kbps and the detector's starting threshold
            self._bw = self._slot_state(bwe_def.BW_WORDS, cleared={bwe_def.BW_RATE_Q8: 256 * bwe_def.bits(bwe, self.frames).max_bits,
                                                                   bwe_def.BW_THR: bwe_def.THR_START})
            self._bw_bytes = self._slot_state(wire.CAP_BYTES, dtype=torch.uint8)
            self._bw_due = self._slot_state()
        if mix is not None:
            # per slot: the peak-hold score (updated in place by hilc_mix_levels once per hop); per parity: the mixes; the speaker
            # marks; the room row (device, captured by address) and its pinned host mirror
            L = hop_samples(self.frames, self.output_rate) if self.rs is not None else HOP * self.frames
            self._score = self._slot_state(dtype=torch.float64)
            # with levelling: the hop-start and hop-end gain and the smoothed power (hilc_mix_gains); with the limiter: its envelope
            # and gain (hilc_mix_rooms_dyn); cleared to (1, 1), 0 and (0, 1)
            self._mix_gains = self._slot_state(2, dtype=torch.float64, cleared=1) if mix.level is not None else None
            self._mix_power = self._slot_state(dtype=torch.float64) if mix.level is not None else None
            self._mix_limiter = self._slot_state(2, dtype=torch.float64, cleared={1: 1}) if mix.limit is not None else None
            self._mixed = torch.zeros(2, B, 1, L, device=device)
            self._speakers = torch.zeros(B, dtype=torch.int32, device=device)
            self._room = torch.full((B,), -1, dtype=torch.int32, device=device)
            self._h_room = torch.full((B,), -1, dtype=torch.int32).pin_memory()
            self._room_dirty, self._room_sent = False, torch.cuda.Event()
        self.sched = ops.SchedWorkspace(device)
        self.graphs, self.outs = self._capture_pair(self._hop, warmup)

    def _block(self, streams: int) -> StateBlock:
        return StateBlock(self.model, streams, self.device, "dec", self._history)

    @property
    def state_bytes(self) -> int:
        """bytes of the two decoder-only state blocks"""
        return sum(b.nbytes for b in self.state)

    @property
    def cache_dec(self) -> List[Tensor]:
        """the CURRENT 30 decoder caches of all streams (views of the state block; 31 with `output_rate`, the history last)"""
        return self._current("dec")

    @property
    def concealed(self) -> Tensor:
        """int32 `[B]` device view: each slot's run of lost hops after the last step (0: decoded from a received packet, or no
        run; k >= 1: k hops lost in a row, at most `fade_hops`).  Read-only: written by the graph."""
        self._need(self.conceal, "concealed", "conceal=True")
        return self._conceal[:, wire.CONCEAL_RUN]

    @property
    def cng_state(self) -> Tensor:
        """int32 `[B, dtx.state_words(cng_order)]` device view: each slot's CN state (has-SID, L, c, q, filter memory) after the last
        step.  Read-only: written by the graph."""
        self._need(self.cng_order is not None, "cng_state", "cng_order=K")
        return self._cn

    def _hop(self, p: int) -> Tensor:
        m = self.model
        src, dst = self.state[p], self.state[p ^ 1]
        if self.srtp is not None:
            # the graph's first launch: the protected arrivals become the plain records of the jitter step and the estimate
            ops.srtp_unprotect(self._wire_arrivals, self.offsets, self._keys_dev, self._rxs, self.tstride, plain=self.arrivals,
                               action=self.action)
        if self.jitter is not None and self.jitter.adapt is not None:
            ops.jitter_adapt_step(self.arrivals, self.offsets, self.hold, self.n_slot, self.packets, self._jstate, self._jmeta,
                                  self._jring, self._jadapt, self.n, self.fec_stages, self.frames, self.cng_order, self.jitter,
                                  self.action, self.lost, self.fec)
        elif self.jitter is not None:
            ops.jitter_step(self.arrivals, self.offsets, self.hold, self.n_slot, self.packets, self._jstate, self._jmeta, self._jring,
                            self.n, self.fec_stages, self.frames, self.cng_order, self.jitter.depth, self.action, self.lost, self.fec)
        if self.report is not None:
            ops.rx_report(self._jstate, self._rp, self._rp_bytes, self._rp_due, self.report, self.action)
        if self.nack is not None:
            ops.nack_build(self._jstate, self._jmeta, self._nk, self._nk_bytes, self._nk_due, self.nack, self.fec_stages, self.action)
        if self.bwe is not None:
            ops.rx_bwe(self.arrivals, self.offsets, self.stage.times, self._bw, self._bw_bytes, self._bw_due, self.bwe, self.n,
                       self.frames, self.fec_stages, self.cng_order, self.action)
        if self.sessions:
            ops.state_slots_apply(src.buffer, src.layout, self.action, self.records)
        packets = self.packets
        if self.fec_stages:
            packets = ops.fec_select(self.packets, self.fec, self.n_slot, self.n, self.fec_stages, self.frames)
        if self.conceal:
            ramp = ops.conceal_prepare(self._conceal, self.action, self.hold, self.lost, self.n_slot, packets, self.frames,
                                       self.fade_hops)
        with ops.sched_workspace(self.sched):
            q = m.dequantizer.decode_packed(packets, self.n_slot, self.n, self.frames)
            wav, _ = m.decoder(q, *src.codec_dec, cache_out=dst.codec_dec)
        if self.conceal:
            ops.conceal_gain(wav, ramp, self._gains, self._weights)
        cng = self.cng_order is not None
        if cng and self.rs is not None:
            # the noise goes through the resampler: written before it, and the decoder caches (not the history) of the slots that
            # produced it are copied back from the block the hop read
            wav = wav.contiguous()
            ops.cng_synth(self.packets, self.hold, self._cn, wav, self._cn_gains, self.cng_order, self.action, self._restore)
            ops.state_slots_hold(src.buffer, dst.buffer, src.layout, self._restore, slices=len(src.layout.shapes) - 1)
        if self.rs is not None:
            wav = ops.resample_poly(wav.contiguous(), self.rs_taps, self.rs.L, self.rs.M, hist=src.hist, hist_out=dst.hist)
        if self.sessions:
            ops.state_slots_hold(src.buffer, dst.buffer, src.layout, self.hold, wav=wav)
        if cng and self.rs is None:
            # the final hold treated the CN slots (hold 2 / 3) as held: their caches are as they were, the noise overwrites the zeros
            ops.cng_synth(self.packets, self.hold, self._cn, wav, self._cn_gains, self.cng_order, self.action)
        if self.mix is not None:
            # the graph's last two launches (three with levelling): the rows are final (noise written, held rows zero)
            ops.mix_levels(wav, self._score, self.action)
            if self.mix.level is not None:
                ops.mix_gains(wav, self._mix_gains, self._mix_power, self.mix.level, self.action)
            if self.mix.level is not None or self.mix.limit is not None:
                ops.mix_rooms_dyn(wav, self._room, self._score, self.mix.top_k, self._mixed[p], self._speakers, self._mix_gains,
                                  self._mix_limiter, self.mix.limit, self.action)
            else:
                ops.mix_rooms(wav, self._room, self._score, self.mix.top_k, self._mixed[p], self._speakers)
        return wav

    # ---------------------------------------------------------------- room mixing
    def join(self, slot: int, room: int) -> None:
        """from the next hop on, slot `slot` is a member of room `room` (an int in [0, B): ValueError), and of no other"""
        self._need(self.mix is not None, "join", "mix=MixConfig(...)")
        s = self.queue.slot(slot)
        self._set_room(s, _int_arg("room", room, 0, self.batch - 1))

    def leave(self, slot: int) -> None:
        """from the next hop on, slot `slot` is in no room (its mix is zero and nobody hears it)"""
        self._need(self.mix is not None, "leave", "mix=MixConfig(...)")
        self._set_room(self.queue.slot(slot), -1)

    def _set_room(self, slot: int, room: int) -> None:
        if int(self._h_room[slot]) != room:
            self._room_sent.synchronize()     # the previous upload's copy has left the pinned row
            self._h_room[slot] = room
            self._room_dirty = True

    def _send_rooms(self) -> None:
        """before a replay, on its stream: the membership row, when it has changed since the last hop"""
        if self.mix is not None and self._room_dirty:
            self._room.copy_(self._h_room, non_blocking=True)
            self._room_sent.record(torch.cuda.current_stream(self.device))
            self._room_dirty = False

    @property
    def rooms(self) -> Tuple[int, ...]:
        """each slot's room as the host has it (-1: none)"""
        self._need(self.mix is not None, "rooms", "mix=MixConfig(...)")
        return tuple(self._h_room.tolist())

    @property
    def mixed(self) -> Tensor:
        """fp32 `[B,1,L]` device view: every slot's mix after the last hop (zeros before the first); overwritten by the next-but-one
        call.  Read-only: written by the graph."""
        self._need(self.mix is not None, "mixed", "mix=MixConfig(...)")
        return self._mixed[self.parity ^ 1]

    @property
    def speakers(self) -> Tensor:
        """int32 `[B]` device view: 1 for the slots among their room's top_k after the last hop.  Read-only: written by the graph."""
        self._need(self.mix is not None, "speakers", "mix=MixConfig(...)")
        return self._speakers

    @property
    def levels(self) -> Tensor:
        """float64 `[B]` device view: every slot's peak-hold score after the last hop.  Read-only: written by the graph."""
        self._need(self.mix is not None, "levels", "mix=MixConfig(...)")
        return self._score

    @property
    def gains(self) -> Tensor:
        """float64 `[B, 2]` device view: every slot's levelling gain at the start and at the end of the last hop ((1, 1) as cleared).
        Read-only: written by the graph."""
        self._need(self.mix is not None and self.mix.level is not None, "gains", "mix=MixConfig(..., level=LevelConfig(...))")
        return self._mix_gains

    @property
    def limiter_state(self) -> Tensor:
        """float64 `[B, 2]` device view: every listener's limiter envelope and gain after the last hop ((0, 1) as cleared).
        Read-only: written by the graph."""
        self._need(self.mix is not None and self.mix.limit is not None, "limiter_state", "mix=MixConfig(..., limit=LimitConfig(...))")
        return self._mix_limiter

    def _check(self, packets: Tensor, n_per_stream, held=(), fec=()) -> Tensor:
        """n_per_stream as a tensor; the entries of `held` slots are not range-checked and become the graph's n, those of `fec`
        slots must lie in [fec_stages, n]"""
        if isinstance(n_per_stream, Tensor) and n_per_stream.is_cuda:
            raise ValueError("n_per_stream: host ints, not a device tensor")
        n = torch.as_tensor(n_per_stream).reshape(-1)
        if n.is_floating_point() or n.numel() != self.batch:
            raise ValueError(f"n_per_stream: {self.batch} ints expected")
        if held:
            n = n.clone()
            n[torch.tensor(sorted(held), dtype=torch.long)] = self.n
        if int(n.min()) < 1 or int(n.max()) > self.n:
            raise ValueError(f"n_per_stream: every entry must lie in [1, {self.n}]")
        if fec and int(n[torch.tensor(sorted(fec), dtype=torch.long)].min()) < self.fec_stages:
            raise ValueError(f"n_per_stream: the entries of fec slots (the next packet's n) must lie in [{self.fec_stages}, {self.n}]")
        if not isinstance(packets, Tensor) or packets.dtype != torch.uint8 or tuple(packets.shape) != (self.batch, self.stride):
            raise ValueError(f"packets: uint8 [{self.batch}, {self.stride}] expected")
        return n

    def step(self, packets: Tensor, n_per_stream, hold=None, lost=None, fec=None, sid=None, silent=None) -> Tensor:
        """`hold`: slots (host ints) that do not advance on this hop (sessions=True only; None or empty: every slot advances).
        `lost`: slots (host ints) whose packet for this hop did not arrive (conceal=True only): concealed; their packet rows and
        n_per_stream entries are not read or checked.  `fec`: slots (host ints) whose packet for this hop was lost but whose next
        packet is in their row (fec_stages >= 1 only): decoded from its redundant section.  `sid` / `silent`: slots (host ints) whose
        row holds a SID / that received nothing because their stream is in DTX (cng_order only): comfort noise"""
        if self.jitter is not None:
            raise RuntimeError("GraphedDecodeHop.step: a receiver with jitter=... takes play(slots, packets, nbytes)")
        held = self._hold_slots(hold)
        gone = SessionQueue.host_slots(lost)
        self._need(self.conceal or not gone, "step(lost=...)", "conceal=True")
        if self.conceal:
            gone = self.queue.lost_slots(gone, held)
        red = SessionQueue.host_slots(fec)
        self._need(self.fec_stages or not red, "step(fec=...)", "fec_stages >= 1")
        if self.fec_stages:
            red = self.queue.fec_slots(red, held, gone)
        sids, quiet = SessionQueue.host_slots(sid), SessionQueue.host_slots(silent)
        self._need(self.cng_order is not None or not (sids or quiet), "step(sid=..., silent=...)", "cng_order=K")
        if self.cng_order is not None:
            sids, quiet = self.queue.cn_slots(sids, quiet, held, gone, red)
        held = set(held) | self.queue.stops
        n = self._check(packets, n_per_stream, held | set(gone) | set(sids) | set(quiet), red)
        st, q = self.stage, self.queue
        st.wait()
        h = st.h_row
        h["n_slot"].copy_(n)
        _mark(h["hold"], held)
        if sids:
            h["hold"][torch.tensor(sids, dtype=torch.long)] = HOLD_SID
        if quiet:
            h["hold"][torch.tensor(quiet, dtype=torch.long)] = HOLD_SILENT
        if self.conceal:
            _mark(h["lost"], gone)
        if self.fec_stages:
            _mark(h["fec"], red)
        st.put_starts(q.starts)
        q.clear()
        if packets.is_cuda:
            st.send(st.payload_off)
            self.packets.copy_(packets)
        else:
            self._h_packets.copy_(packets)
            st.send(st.rec_off)
        st.finish(host_records_apart=True)
        self._send_rooms()
        return self._replay()

    # ---------------------------------------------------------------- jitter buffer
    def _init_jitter(self, cfg: JitterConfig, max_arrivals) -> None:
        B, dev = self.batch, self.device
        self.max_arrivals = _int_arg("max_arrivals", max_arrivals, 1)
        self.tstride = wire.transport_bytes(self.n, self.fec_stages, self.frames)
        # ONE device buffer, captured by address, uploaded up to the last arrival used: action per slot, the host's holds
        # (hilc_jitter_step adds its own), the arrival region (an arrival record: byte count, then the headed packet), the staged
        # records.  The n, lost and fec rows and the packet matrix are written by hilc_jitter_step and are never uploaded.
        # with srtp the arrivals are protected packets, 10 bytes wider; hilc_srtp_unprotect writes the plain records every later launch
        # reads into a device-only buffer of the width they check
        self.wstride = self.tstride + (wire.SRTP_TAG_BYTES if self.srtp is not None else 0)
        st = self.stage = self._new_stage(("action", "hold"), arrivals=(self.max_arrivals, self.wstride), times=self.bwe is not None)
        self.offsets, self.arrivals = st.offsets, st.arrivals
        self._wire_arrivals = None
        if self.srtp is not None:
            self._wire_arrivals = st.arrivals
            self.arrivals = torch.zeros(self.max_arrivals, 1 + (self.tstride + 3) // 4, dtype=torch.int32, device=dev)
            # per slot: the key row (srtp.KEY_*) and the RX row (srtp.RX_*, updated in place by hilc_srtp_unprotect once per hop)
            self._init_keys()
            self._rxs = self._slot_state(srtp_def.RX_WORDS)
        rows = torch.zeros(3, B, dtype=torch.int32, device=dev)
        self.n_slot = rows[0]
        self.lost = rows[1] if self.conceal else None
        self.fec = rows[2] if self.fec_stages else None
        self.packets = torch.zeros(B, self.stride, dtype=torch.uint8, device=dev)
        # per slot: the state row (jitter.ST_*, updated in place once per hop), the ring's meta words and bodies
        self._jstate = self._slot_state(ST_WORDS)
        self._jmeta = self._slot_state(cfg.capacity)
        self._jring = self._slot_state(cfg.capacity, (self.stride + 3) // 4)
        if cfg.adapt is not None:
            # per slot: the adapt row (jitter.AD_*, updated in place once per hop by hilc_jitter_adapt_step)
            self._jadapt = self._slot_state(AD_WORDS)

    @property
    def jitter_state(self) -> Tensor:
        """int32 `[B, jitter.ST_WORDS]` device view: each slot's jitter state row after the last play (jitter.ST_* / STAT_*).
        Read-only: written by the graph."""
        self._need(self.jitter is not None, "jitter_state", "jitter=JitterConfig(...)")
        return self._jstate

    @property
    def jitter_adapt(self) -> Tensor:
        """int32 `[B, jitter.AD_WORDS]` device view: each slot's adapt row after the last play (jitter.AD_*).  Read-only: written by
        the graph."""
        self._need(self.jitter is not None and self.jitter.adapt is not None, "jitter_adapt",
                   "jitter=JitterConfig(..., adapt=AdaptConfig(...))")
        return self._jadapt

    @property
    def reports(self) -> Tensor:
        """uint8 `[B, 3]` device view: each slot's latest report (wire.parse_report; zeros before its first), unchanged between
        reports.  Read-only: written by the graph."""
        self._need(self.report is not None, "reports", "report=ReportConfig(...)")
        return self._rp_bytes

    @property
    def report_due(self) -> Tensor:
        """int32 `[B]` device view: 1 for the slots whose report was emitted on the last play.  Read-only: written by the graph."""
        self._need(self.report is not None, "report_due", "report=ReportConfig(...)")
        return self._rp_due

    @property
    def report_state(self) -> Tensor:
        """int32 `[B, report.RP_WORDS]` device view: each slot's report row after the last play (report.RP_*).  Read-only: written
        by the graph."""
        self._need(self.report is not None, "report_state", "report=ReportConfig(...)")
        return self._rp

    @property
    def nacks(self) -> Tensor:
        """uint8 `[B, 4]` device view: each slot's latest NACK (wire.parse_nack; zeros before its first), unchanged between NACKs.
        Read-only: written by the graph."""
        self._need(self.nack is not None, "nacks", "nack=NackConfig(...)")
        return self._nk_bytes

    @property
    def nack_due(self) -> Tensor:
        """int32 `[B]` device view: 1 for the slots whose NACK was emitted on the last play.  Read-only: written by the graph."""
        self._need(self.nack is not None, "nack_due", "nack=NackConfig(...)")
        return self._nk_due

    @property
    def nack_state(self) -> Tensor:
        """int32 `[B, rtx.NK_WORDS]` device view: each slot's NACK row after the last play (rtx.NK_*).  Read-only: written by the
        graph."""
        self._need(self.nack is not None, "nack_state", "nack=NackConfig(...)")
        return self._nk

    @property
    def srtp_state(self) -> Tensor:
        """int32 `[B, srtp.RX_WORDS]` device view: each slot's RX row after the last play (srtp.RX_*; srtp only).  Read-only: written
        by the graph."""
        self._need(self.srtp is not None, "srtp_state", "srtp=SrtpConfig()")
        return self._rxs

    @property
    def caps(self) -> Tensor:
        """uint8 `[B, 3]` device view: each slot's latest rate cap (wire.parse_cap; zeros before its first), unchanged between caps.
        Read-only: written by the graph."""
        self._need(self.bwe is not None, "caps", "bwe=BweConfig(...)")
        return self._bw_bytes

    @property
    def cap_due(self) -> Tensor:
        """int32 `[B]` device view: 1 for the slots whose cap was emitted on the last play.  Read-only: written by the graph."""
        self._need(self.bwe is not None, "cap_due", "bwe=BweConfig(...)")
        return self._bw_due

    @property
    def bwe_state(self) -> Tensor:
        """int32 `[B, bwe.BW_WORDS]` device view: each slot's estimate row after the last play (bwe.BW_*; `bwe.kbps(row, frames)`
        gives BW_RATE_Q8 in kbps).  Read-only: written by the graph."""
        self._need(self.bwe is not None, "bwe_state", "bwe=BweConfig(...)")
        return self._bw

    def _arrival_times(self, times, arr: Arrivals) -> Optional[np.ndarray]:
        """play's `times` checked before anything is written -> the ticks int32 [A] in the records' slot-grouped order (None without
        `bwe`): A host ints, taken mod 2^32"""
        if self.bwe is None:
            self._need(times is None, "play(times=...)", "bwe=BweConfig(...)")
            return None
        if times is None:
            if arr.count:
                raise ValueError("play: a receiver with bwe= needs `times`, the arrival tick of every packet")
            return np.zeros(0, dtype=np.int32)
        if isinstance(times, Tensor):
            if times.is_cuda:
                raise ValueError("play: times must be host ints, not a device tensor")
            times = times.numpy()
        try:
            ticks = np.asarray(times)
            if ticks.dtype.kind not in "iu":
                ticks = np.array([int(t) & 0xFFFFFFFF for t in ticks.reshape(-1).tolist()], dtype=np.int64)
        except OverflowError:                                           # Python ints past 64 bits
            ticks = np.array([int(t) & 0xFFFFFFFF for t in times], dtype=np.int64)
        ticks = ticks.reshape(-1)
        if len(ticks) != arr.count:
            raise ValueError(f"play: {arr.count} slots but {len(ticks)} times")
        return (ticks.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)[arr.order]

    def play(self, slots, packets: Tensor, nbytes, hold=None, times=None) -> Tensor:
        """one hop of a jitter receiver: this hop's arrivals, in push order — `slots` and `nbytes` (A host ints), `packets` uint8
        `[A, wire.transport_bytes(n, m, frames)]` (with srtp: `wire.srtp_bytes(n, m, frames)`; host or device) — and `hold`: slots
        (host ints) held on this hop (playout pauses).  `times` (with `bwe` only, then required whenever A > 0): the arrivals'
        ticks, A host ints in units of 1/24000 s (ValueError for a device tensor or another length).  Returns the hop's waveform,
        a static view that the next-but-one call overwrites."""
        self._need(self.jitter is not None, "play", "jitter=JitterConfig(...)")
        held = set(self._hold_slots(hold)) | self.queue.stops
        arr = check_arrivals("play", slots, packets, nbytes, self.batch, self.max_arrivals, self.wstride)
        ticks = self._arrival_times(times, arr)
        st, q = self.stage, self.queue
        st.wait()
        _mark(st.h_row["hold"], held)
        st.put_starts(q.starts)
        q.clear()
        st.send_arrivals(arr, packets, ticks)
        st.finish(host_records_apart=True)
        self._send_rooms()
        self._send_keys()
        return self._replay()

    def start(self, slot: int, cache_dec: Optional[Sequence[Tensor]] = None) -> None:
        """At the next step, slot `slot` begins a fresh stream (zero caches) or resumes one from its 30 decoder caches (B = 1
        tensors, host or device; 31 with `output_rate`, the resampler's history last); at most `max_loads_per_hop` resumes per hop.
        With `jitter`, its jitter state (and its adapt row) is cleared on that hop.  With `srtp`: ValueError unless `set_key(slot,
        ...)` was called since the slot's previous start"""
        self._start_keyed(slot, lambda: _Hop.start(self, slot, None, cache_dec))

    def export(self, slot: int) -> List[Tensor]:
        """the current 30 decoder caches of slot `slot` as B = 1 device tensors (one gather launch; a stopped slot: its caches
        when it stopped; 31 with `output_rate`, the resampler's history last)"""
        return super().export(slot)[1]


class GraphedForwardHop(_GraphPair):
    """A selective forwarding hop (hilcodec_amd/forward.py: the rules, bit for bit): a conference server for `batch` participant slots
    that routes packets and cuts them to each listener's number of stages without decoding.  It holds no model and no codec state: each
    slot is a sender (its arrivals are checked and its activity kept) and a listener (it is sent the packets of its room's `cfg.fanout`
    most active other members, each cut to its `layers` stages).  The senders are GraphedEncodeHop(header=True) of `frames` frames and
    `n` stages, `fec_stages` = their m, `cng_order` = the K of their SIDs (None: a SID is malformed); a listener plays the rows of route
    j into slot j of a GraphedDecodeHop(jitter=, mix=), after `start(j)` where `new_routes` is set.
    A hop is one upload (the stage's rows — action, room, layers — the offsets and the arrival records, staged as
    GraphedDecodeHop.play stages them) and the replay of a graph of two launches (hilc_forward_classify, hilc_forward_route); two
    graphs are captured and replayed alternately, so what `forward` returns stays valid for one further call.
    `cfg`: the forward.ForwardConfig; `max_arrivals`: the most arrivals of one hop (default 2 B).
    `downlink` (a downlink.DownlinkConfig; hilcodec_amd/downlink.py: the rules): the listeners' receiver reports and NACKs come back with
    a hop (`forward(..., reports=, nacks=)`, one per listener and route), and two further launches follow the two above in the same
    graph, one behind the other (hilc_downlink_store, hilc_downlink_step): with `rate`, each listener's downlink gets a rate that
    follows its reports and a bucket, and the hop's rows are cut to the layers the bucket pays for (`eff_layers`; `set_layers` stays the
    cap); with `history`, every sender slot's arrivals are kept and the NACKs are answered from them (`rtx_packets`, `rtx_nbytes`,
    `rtx_routes`: a retransmission is played into the client's slot of that route like any arrival).  The feedback rows travel in the
    same upload, and apply to exactly one hop.  Without `downlink` nothing of this is allocated or launched.
    `speakers` (an audio_level.SpeakerConfig; hilcodec_amd/audio_level.py: the rules): level-based speaker selection, for senders without
    DTX.  `forward(..., levels=)` takes one level per arrival (what the sender's `audio_level` said: 0..127, -1: unknown); the host reduces
    them to the loudest per slot into one more one-hop row of the same upload, and one launch (hilc_forward_rank) between the two above
    keeps each sender's smoothed loudness and writes a ping-pong pair of shadow sender rows, which hilc_forward_route reads in place of
    the real ones: it then selects a room's loudest speakers, with a margin for those on stage.  `speaker_state` and `speaker_rank` show
    the result; `sender_state` stays the real rows, and the downlink launches follow unchanged.  `speakers=None` allocates nothing and
    captures exactly the graph without it.
    `srtp` (a srtp.SrtpConfig; hilcodec_amd/forward_srtp.py: the rules): SRTP hop by hop.  The arrivals are protected packets under each
    sender's uplink key (`set_uplink_key`), 10 bytes wider; hilc_srtp_unprotect runs as the graph's first launch and writes the plain
    records every launch above reads into a device-only buffer (a rejected arrival: a record of 0 bytes, which counts as malformed).
    hilc_srtp_protect_routes runs last, on the rows the hop would have returned, and `forward` returns its rows instead: each protected
    under its listener's downlink key (`set_downlink_key`) and the route's own SSRC, `forward_srtp.route_ssrc(base, j,
    route_epoch[b][j])`; the client re-keys and restarts route j whenever that epoch changes.  The slots given a key travel as two
    more one-hop rows of the same upload.  `speakers` and `downlink=DownlinkConfig(rate=...)` work unchanged under it; `downlink.history
    > 0` raises ValueError: a NACK answer is cut again at answer time, so it could put other plaintext under an index already used (a
    per-route history of ciphertext is the follow-up).  `srtp=None` allocates nothing and captures exactly the graphs without it."""

    def __init__(self, batch: int, frames: int, n: int, device: torch.device, fec_stages: int = 0, cng_order: Optional[int] = None,
                 cfg: forward_def.ForwardConfig = forward_def.ForwardConfig(), max_arrivals: Optional[int] = None, warmup: int = 2,
                 downlink: Optional[downlink_def.DownlinkConfig] = None, speakers: Optional[level_def.SpeakerConfig] = None,
                 srtp: Optional[srtp_def.SrtpConfig] = None):
        if not isinstance(cfg, forward_def.ForwardConfig):
            raise ValueError(f"GraphedForwardHop: cfg must be a forward.ForwardConfig, got {cfg!r}")
        self.downlink = _config_arg("downlink", downlink, downlink_def.DownlinkConfig)
        self.speakers = _config_arg("speakers", speakers, level_def.SpeakerConfig)
        self.srtp = _config_arg("srtp", srtp, srtp_def.SrtpConfig)
        if srtp is not None and downlink is not None and downlink.history > 0:
            raise ValueError("GraphedForwardHop(srtp=...) with downlink.history > 0: a NACK answer is cut again at answer time, so it "
                             "could put other plaintext under an index already used; answers under srtp need a per-route history of "
                             "ciphertext")
        super().__init__(_int_arg("batch", batch, 1), device)
        B = self.batch
        self.frames, self.n, self.cfg = _int_arg("frames", frames, 1), _int_arg("n", n, 1, 31), cfg
        self.fec_stages = _fec_stages(fec_stages, self.n)
        self.cng_order = None if cng_order is None else _int_arg("cng_order", cng_order, 0, dtx_def.MAX_ORDER)
        self.max_arrivals = _int_arg("max_arrivals", 2 * B if max_arrivals is None else max_arrivals, 1)
        self.tstride = wire.transport_bytes(self.n, self.fec_stages, self.frames)
        if self.cng_order is not None:
            dtx_def.check_order(self.cng_order, self.tstride - wire.TRANSPORT_HEADER, "GraphedForwardHop(cng_order=...)")
        # ONE device buffer, captured by address, uploaded up to the last arrival used: the action, room and layers rows, the
        # arrival region (an arrival record: byte count, then the headed packet)
        F, P = cfg.fanout, cfg.burst
        # with `srtp` the arrivals are protected packets, 10 bytes wider, and two more one-hop rows say which slots were given a key
        self.wstride = self.tstride + (wire.SRTP_TAG_BYTES if srtp is not None else 0)
        # with `downlink`: behind them the feedback rows in use, int32 [B, fanout] each (fanout stage rows laid end to end)
        self._fb_names = () if downlink is None else \
            ("report",) * (downlink.rate is not None) + ("nack_base", "nack_bitmap") * (downlink.history > 0)
        fb_rows = tuple(f"{name}{j}" for name in self._fb_names for j in range(F))
        # with `speakers`: the one-hop row loud (128 - the loudest level of the slot's arrivals, 0: none)
        key_rows = ("rekey_up", "rekey_down") * (srtp is not None)
        st = self.stage = ControlStage(B, ("action", "room", "layers") + ("loud",) * (speakers is not None) + fb_rows + key_rows, 0, 0, 0,
                                       device, arrivals=(self.max_arrivals, self.wstride))
        self.offsets, self.arrivals = st.offsets, st.arrivals
        self._fb = {name: st.dev[st.row_off[name + "0"]:st.row_off[name + "0"] + B * F].view(torch.int32).view(B, F)
                    for name in self._fb_names}
        self._h_fb = {name: st.host[st.row_off[name + "0"]:st.row_off[name + "0"] + B * F].view(torch.int32).view(B, F)
                      for name in self._fb_names}
        self._fb_live = False                 # the feedback rows hold entries on the device
        self._sd, self._lr = self._slot_state(forward_def.SD_WORDS), self._slot_state(forward_def.LR_WORDS)
        self._pick, self._pick_count = self._slot_state(P), self._slot_state()
        self._routes, self._new_routes = self._slot_state(F, cleared=-1), self._slot_state(F)
        self._out = [self._slot_state(F, P, self.tstride, dtype=torch.uint8) for _ in (0, 1)]
        self._out_nbytes = [self._slot_state(F, P) for _ in (0, 1)]
        self._joined = set()                  # the slots joined since the last hop
        self._shadow = self._sp = None
        if speakers is not None:
            # per parity, per slot: the shadow sender row (the hop of parity p reads row p and writes row p ^ 1); per slot: the speaker row
            self._shadow = self._slot_state(forward_def.SD_WORDS, pingpong=True)
            self._sp = self._slot_state(level_def.SP_WORDS)
        if downlink is not None:
            self._init_downlink(downlink)
        if srtp is not None:
            self._init_srtp()
        self.graphs, self.outs = self._capture_pair(self._hop, warmup)

    def _init_srtp(self) -> None:
        """the state of the two SRTP launches: the plain records hilc_srtp_unprotect writes for every later launch, the two key tables
        and their device rows, the ingress rows (srtp.RX_*), the route rows (forward_srtp.RT_*) and per parity the protected rows that
        `forward` returns"""
        F, P = self.cfg.fanout, self.cfg.burst
        self._wire_arrivals = self.arrivals
        self.arrivals = torch.zeros(self.max_arrivals, arrival_width(self.tstride), dtype=torch.int32, device=self.device)
        self._keys = fsrtp_def.ForwardKeys(self.batch)
        self._up_dev, self._down_dev = self._slot_state(srtp_def.KEY_WORDS), self._slot_state(srtp_def.KEY_WORDS)
        self._rxs = self._slot_state(srtp_def.RX_WORDS)
        self._rt = self._slot_state(F, fsrtp_def.RT_WORDS)
        self._sout = [self._slot_state(F, P, self.wstride, dtype=torch.uint8) for _ in (0, 1)]
        self._sout_nbytes = [self._slot_state(F, P) for _ in (0, 1)]

    def _init_downlink(self, dl: downlink_def.DownlinkConfig) -> None:
        """the state of the two downlink launches: the listener rows (as after a reset), the routes' memory, the senders' histories,
        and per parity the rows that `forward` returns instead of the route launch's, the layers they were cut to and the
        retransmissions"""
        F, P, R, Q = self.cfg.fanout, self.cfg.burst, dl.history, dl.per_hop
        bits = downlink_def.bucket(dl, self.frames, self.fec_stages, F, self.cfg.keep_fec)      # ValueError: the rates do not fit
        burst_hops = 0 if dl.rate is None else dl.rate.burst_hops
        self._dl = self._slot_state(downlink_def.DL_WORDS, cleared={downlink_def.DL_RATE_Q8: 256 * bits.start_bits,
                                                                    downlink_def.DL_CREDIT: burst_hops * bits.start_bits})
        self._dl_mem = self._slot_state(F)
        self._dl_out = [self._slot_state(F, P, self.tstride, dtype=torch.uint8) for _ in (0, 1)]
        self._dl_nbytes = [self._slot_state(F, P) for _ in (0, 1)]
        self._eff = [self._slot_state(cleared=self.n) for _ in (0, 1)]
        self._hist = None
        if R > 0:
            self._hist = (self._slot_state(R), self._slot_state(R, arrival_width(self.tstride)), self._slot_state(downlink_def.DS_WORDS))
            self._rtx = [(self._slot_state(Q, self.tstride, dtype=torch.uint8), self._slot_state(Q), self._slot_state(Q, cleared=-1))
                         for _ in (0, 1)]

    def _hop(self, p: int) -> Tuple[Tensor, Tensor]:
        if self.srtp is None:
            return self._plain_hop(p)
        st = self.stage
        # the clear row of the ingress is rekey_up: an RX row lives as long as its key, a join under the same key keeps its window
        ops.srtp_unprotect(self._wire_arrivals, self.offsets, self._up_dev, self._rxs, self.tstride, plain=self.arrivals,
                           action=st.row["rekey_up"])
        rows, nbytes = self._plain_hop(p)
        return ops.srtp_protect_routes(rows, nbytes, self._routes, self._new_routes, self._down_dev, self._rt, out=self._sout[p],
                                       out_nbytes=self._sout_nbytes[p], action=st.row["action"], rekey_up=st.row["rekey_up"],
                                       rekey_down=st.row["rekey_down"])

    def _plain_hop(self, p: int) -> Tuple[Tensor, Tensor]:
        """the launches on plain records: classify, (rank,) route, (store, downlink step)"""
        st, args = self.stage, (self.cfg, self.n, self.frames, self.fec_stages, self.cng_order)
        ops.forward_classify(self.arrivals, self.offsets, self._sd, self._pick, self._pick_count, *args, action=st.row["action"])
        ranked = self._sd
        if self.speakers is not None:
            # between the two: the route launch sorts by the shadow rows' (SD_HANG, SD_SINCE), which is the loudness key's order
            ranked = self._shadow[p ^ 1]
            ops.forward_rank(self._sd, st.row["loud"], st.row["room"], self._shadow[p], ranked, self._sp, self.cfg, self.speakers,
                             action=st.row["action"])
        ops.forward_route(self.arrivals, st.row["room"], st.row["layers"], ranked, self._pick, self._pick_count, self._routes,
                          self._new_routes, self._lr, self._out[p], self._out_nbytes[p], *args, action=st.row["action"])
        if self.downlink is None:
            return self._out[p], self._out_nbytes[p]
        history = {}
        if self._hist is not None:
            tags, ring, rows = self._hist
            ops.downlink_store(self.arrivals, self._pick, self._pick_count, tags, ring, rows, self.n, self.frames, self.fec_stages,
                               action=st.row["action"])
            history = dict(zip(("rtx_out", "rtx_nbytes", "rtx_routes"), self._rtx[p]), tags=tags, ring=ring)
        ops.downlink_step(self._routes, self._new_routes, self._out[p], self._out_nbytes[p], st.row["layers"], self._dl, self._dl_mem,
                          self._eff[p], self._dl_out[p], self._dl_nbytes[p], self.downlink, self.cfg, self.n, self.frames,
                          self.fec_stages, action=st.row["action"], **self._fb, **history)
        return self._dl_out[p], self._dl_nbytes[p]

    def _zero(self) -> None:
        """every slot as constructed: in no room, n layers, no route, every row and output zero"""
        st = self.stage
        st.wait()
        st.host.zero_()
        st.h_row["room"].fill_(-1)
        st.h_row["layers"].fill_(self.n)
        st.dev.copy_(st.host)
        super()._zero()
        if self.srtp is not None:
            self.arrivals.zero_()
            self._keys.up.dirty = self._keys.down.dirty = True       # the device key rows are zero again

    def reset(self) -> None:
        """every slot as constructed (in no room, n layers, no route, every row and counter zero) and the first graph next; with
        `srtp`: both key tables empty and every route row zero, its epoch included"""
        self._joined = set()
        self._fb_live = False
        if self.srtp is not None:
            self._keys.reset()
        self._zero()
        self.parity = 0

    # ---------------------------------------------------------------- SRTP (srtp=SrtpConfig())
    def set_uplink_key(self, slot: int, master_key, master_salt, ssrc: Optional[int] = None, roc: int = 0) -> None:
        """from the next hop on, slot `slot`'s arrivals are unprotected under the session keys derived from `master_key` (16 bytes)
        and `master_salt` (14 bytes) with `ssrc` (default: the slot): what its GraphedEncodeHop(srtp=) was given with set_key.  Its
        ingress row is cleared on that hop and begins at rollover counter `roc`, and every route it owns restarts (its SEQ restarts
        with its key).  ValueError: wrong lengths, ssrc or roc out of range, or a key the slot had before; never the key itself."""
        self._need(self.srtp is not None, "set_uplink_key", "srtp=SrtpConfig()")
        self._keys.set_uplink_key(self._slot(slot), master_key, master_salt, ssrc, roc)

    def set_downlink_key(self, slot: int, master_key, master_salt, ssrc: Optional[int] = None) -> None:
        """from the next hop on, the rows sent to listener `slot` are protected under the session keys derived from `master_key` and
        `master_salt`; `ssrc` (default: the slot) is the base of its routes' SSRCs (forward_srtp.route_ssrc).  Every route of the
        listener restarts on that hop.  ValueError as set_uplink_key."""
        self._need(self.srtp is not None, "set_downlink_key", "srtp=SrtpConfig()")
        self._keys.set_downlink_key(self._slot(slot), master_key, master_salt, ssrc)

    def clear_keys(self, slot: int) -> None:
        """from the next hop on, slot `slot` has neither key: its arrivals are rejected and it is sent nothing"""
        self._need(self.srtp is not None, "clear_keys", "srtp=SrtpConfig()")
        self._keys.clear_keys(self._slot(slot))

    def _send_keys(self) -> None:
        """before a replay, on its stream: each key table that has changed since the last hop"""
        for table, dev in ((self._keys.up, self._up_dev), (self._keys.down, self._down_dev)):
            if table.dirty:
                dev.copy_(torch.from_numpy(table.rows))
                table.dirty = False

    @property
    def route_epoch(self) -> Tensor:
        """int32 `[B, fanout]` device view, the RT_EPOCH column of `egress_state`: the epoch of each listener's routes after the last
        hop; a client re-keys route j to forward_srtp.route_ssrc(base, j, epoch) and restarts it when its epoch changed (srtp only)"""
        self._need(self.srtp is not None, "route_epoch", "srtp=SrtpConfig()")
        return self._rt[:, :, fsrtp_def.RT_EPOCH]

    @property
    def egress_state(self) -> Tensor:
        """int32 `[B, fanout, forward_srtp.RT_WORDS]` device view: each route's row after the last hop (forward_srtp.RT_*; srtp only).
        Read-only: written by the graph."""
        self._need(self.srtp is not None, "egress_state", "srtp=SrtpConfig()")
        return self._rt

    @property
    def ingress_state(self) -> Tensor:
        """int32 `[B, srtp.RX_WORDS]` device view: each sender slot's RX row after the last hop (srtp.RX_*; srtp only).  Read-only:
        written by the graph."""
        self._need(self.srtp is not None, "ingress_state", "srtp=SrtpConfig()")
        return self._rxs

    def _slot(self, slot) -> int:
        s = int(slot)
        if not 0 <= s < self.batch:
            raise IndexError(f"slot {slot} outside [0, {self.batch})")
        return s

    def join(self, slot: int, room: int) -> None:
        """from the next hop on, slot `slot` is a new participant of room `room` (an int in [0, B): ValueError), and of no other: its
        sender and listener rows are cleared on that hop, and every route it owned is freed"""
        s, r = self._slot(slot), _int_arg("room", room, 0, self.batch - 1)
        self.stage.wait()                     # the previous upload's copy has left the pinned rows
        self.stage.h_row["room"][s] = r
        self._joined.add(s)

    def leave(self, slot: int) -> None:
        """from the next hop on, slot `slot` is in no room: it is sent nothing and nobody is sent its packets"""
        s = self._slot(slot)
        self.stage.wait()
        self.stage.h_row["room"][s] = -1

    def set_layers(self, slot: int, L: int) -> None:
        """from the next hop on, the packets sent to slot `slot` have at most `L` stages (an int in [1, n]: ValueError; as constructed: n)"""
        s, v = self._slot(slot), _int_arg("L", L, 1, self.n)
        self.stage.wait()
        self.stage.h_row["layers"][s] = v

    @property
    def rooms(self) -> Tuple[int, ...]:
        """each slot's room as the host has it (-1: none)"""
        return tuple(self.stage.h_row["room"].tolist())

    @property
    def layers(self) -> Tuple[int, ...]:
        """each slot's layer count as the host has it"""
        return tuple(self.stage.h_row["layers"].tolist())

    @property
    def routes(self) -> Tensor:
        """int32 `[B, fanout]` device view: the owner of each listener's routes after the last hop (-1: free).  Read-only: written by
        the graph."""
        return self._routes

    @property
    def new_routes(self) -> Tensor:
        """int32 `[B, fanout]` device view: 1 where a route's owner on the last hop is another than before it (the listener restarts
        that route's decoder slot).  Read-only: written by the graph, overwritten by the next call."""
        return self._new_routes

    @property
    def sender_state(self) -> Tensor:
        """int32 `[B, forward.SD_WORDS]` device view: each slot's sender row after the last hop (forward.SD_*).  Read-only: written by
        the graph."""
        return self._sd

    @property
    def listener_state(self) -> Tensor:
        """int32 `[B, forward.LR_WORDS]` device view: each slot's listener row after the last hop (forward.LR_*).  Read-only: written by
        the graph."""
        return self._lr

    @property
    def speaker_state(self) -> Tensor:
        """int32 `[B, audio_level.SP_WORDS]` device view: each slot's speaker row after the last hop (audio_level.SP_*; speakers only).
        Read-only: written by the graph."""
        self._need(self._sp is not None, "speaker_state", "speakers=SpeakerConfig(...)")
        return self._sp

    @property
    def speaker_rank(self) -> Tensor:
        """int32 `[B]` device view, the SP_RANK column of `speaker_state`: each slot's place among its room's speakers, one hop behind
        (0: the room's dominant speaker, -1: no candidate; speakers only).  Read-only: written by the graph."""
        return self.speaker_state[:, level_def.SP_RANK]

    def _last(self, what: str, need_history: bool = False):
        """a downlink view (RuntimeError without the option it belongs to); ping-pong rows: those of the graph that ran last"""
        self._need(self.downlink is not None, what, "downlink=DownlinkConfig(...)")
        self._need(not need_history or self.downlink.history > 0, what, "downlink=DownlinkConfig(history=...)")
        return self.parity ^ 1

    @property
    def eff_layers(self) -> Tensor:
        """int32 `[B]` device view: the layers each listener's rows of the last hop were cut to (downlink only; at most its `layers`).
        Read-only: written by the graph, overwritten by the next-but-one call."""
        p = self._last("eff_layers")
        return self._eff[p]

    @property
    def downlink_state(self) -> Tensor:
        """int32 `[B, downlink.DL_WORDS]` device view: each listener's downlink row after the last hop (downlink.DL_*; downlink only;
        downlink.kbps gives its rate in kbps).  Read-only: written by the graph."""
        self._last("downlink_state")
        return self._dl

    @property
    def history_state(self) -> Tensor:
        """int32 `[B, downlink.DS_WORDS]` device view: the counter row of each sender slot's history after the last hop
        (downlink.DS_*; downlink with history only).  Read-only: written by the graph."""
        self._last("history_state", True)
        return self._hist[2]

    @property
    def rtx_packets(self) -> Tensor:
        """uint8 `[B, per_hop, tb]` device view: the retransmissions of the last hop, zero rows where there is none (downlink with
        history only).  Read-only: written by the graph, overwritten by the next-but-one call."""
        p = self._last("rtx_packets", True)
        return self._rtx[p][0]

    @property
    def rtx_nbytes(self) -> Tensor:
        """int32 `[B, per_hop]` device view: the byte counts of `rtx_packets`, 0 for no retransmission (downlink with history only)"""
        p = self._last("rtx_nbytes", True)
        return self._rtx[p][1]

    @property
    def rtx_routes(self) -> Tensor:
        """int32 `[B, per_hop]` device view: the route each row of `rtx_packets` belongs to, -1 for no retransmission (downlink with
        history only)"""
        p = self._last("rtx_routes", True)
        return self._rtx[p][2]

    def _feedback(self, reports, nacks) -> Optional[dict]:
        """forward's `reports` / `nacks` checked before anything is uploaded -> the feedback rows (downlink.feedback_rows), None for
        none"""
        dl = self.downlink
        if reports is not None:
            self._need(dl is not None and dl.rate is not None, "forward(reports=...)", "downlink=DownlinkConfig(rate=...)")
        if nacks is not None:
            self._need(dl is not None and dl.history > 0, "forward(nacks=...)", "downlink=DownlinkConfig(history=...)")
        if reports is None and nacks is None:
            return None
        return downlink_def.feedback_rows(self.batch, self.cfg.fanout, reports, nacks)

    def forward(self, slots, packets: Tensor, nbytes, levels=None, reports=None, nacks=None) -> Tuple[Tensor, Tensor]:
        """one hop: this hop's arrivals, in push order — `slots` and `nbytes` (A host ints), `packets` uint8 `[A,
        wire.transport_bytes(n, m, frames)]` (host or device), 0 <= A <= max_arrivals.  Returns (out uint8 `[B, fanout, burst, tb]`,
        out_nbytes int32 `[B, fanout, burst]`): row (b, j, k) is the k-th packet of this hop for listener b's route j, cut to its layers
        (0 bytes: none); static views that the next-but-one call overwrites.  With `srtp` the arrivals and the rows returned are
        protected packets, both `wire.srtp_bytes(n, m, frames)` wide.
        `reports` (downlink with rate only) / `nacks` (downlink with history only): (listeners, routes, blobs), this hop's feedback — A
        host ints twice, and a uint8 `[A, 3]` / `[A, 4]` host tensor or a sequence of `bytes` (wire.pack_report / wire.pack_nack); a
        (listener, route) pair named twice keeps its last blob.  With `downlink` the rows returned are cut to `eff_layers`.
        `levels` (speakers only: ValueError without): A host ints, each arrival's audio level as its sender measured it — 0..127, or -1
        for unknown, which counts as the floor level (anything else: ValueError); None: every arrival is unknown."""
        if levels is not None and self.speakers is None:
            raise ValueError("GraphedForwardHop.forward(levels=...): construct with speakers=SpeakerConfig(...)")
        if isinstance(levels, Tensor) and levels.is_cuda:
            raise ValueError("forward: levels must be host ints, not a device tensor")
        fb = self._feedback(reports, nacks)
        arr = check_arrivals("forward", slots, packets, nbytes, self.batch, self.max_arrivals, self.wstride)
        loud = None if self.speakers is None else level_def.loud_row(self.batch, arr.slots, levels, self.speakers)
        st = self.stage
        st.wait()
        if st.one_hop_live or self._joined:   # the join row: 1 for the slots joined since the last hop
            st.put_one_hop("action", sorted(self._joined), 1)
            self._joined = set()
        if fb is not None or self._fb_live:   # the feedback rows, likewise: this hop's feedback, 0 elsewhere
            for name in self._fb_names:
                self._h_fb[name].zero_() if fb is None else self._h_fb[name].copy_(torch.from_numpy(fb[name]))
            self._fb_live = fb is not None
        if loud is not None:                  # the loudness row, likewise: the slots with an arrival on this hop, 0 elsewhere
            heard = np.flatnonzero(loud)
            st.put_one_hop("loud", heard, loud[heard])
        if self.srtp is not None and (st.one_hop_live or self._keys.pending):
            up, down = self._keys.take()                  # the key rows, likewise: the slots given a key since the last hop
            st.put_one_hop("rekey_up", up, 1)
            st.put_one_hop("rekey_down", down, 1)
        st.send_arrivals(arr, packets)
        st.finish()
        if self.srtp is not None:
            self._send_keys()
        return self._replay()
