"""Host side of the graphed hops' per-stream sessions (graph_step.py): the queue of what the next hop does to which slot, and
the layout and filling of the control stage that carries it to the device.  No device is needed here, and nothing in this
module calls into CUDA: the tensors it writes are the stage's host mirror (or plain CPU tensors in the tests)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

# action row of a hop: ACTION_KEEP, ACTION_ZERO (a fresh start), r >= ACTION_LOAD (load record r - ACTION_LOAD)
ACTION_KEEP, ACTION_ZERO, ACTION_LOAD = 0, -1, 1
# hold row of a hop: the slot advances, is held, or (receiver) makes comfort noise from the SID that arrived / while its stream is in DTX
HOLD_ADVANCE, HOLD_HELD, HOLD_SID, HOLD_SILENT = 0, 1, 2, 3
# the rows of a control stage whose entries apply to exactly one hop: the upload after a hop that wrote one must clear it on the device
ONE_HOP_ROWS = ("action", "report", "nack_base", "nack_bitmap", "loud", "cap", "rekey_up", "rekey_down")


def stage_layout(batch: int, rows: Sequence[str], payload_words: int = 0, loads: int = 0, record_len: int = 0):
    """Word offsets of a control stage, "int32 rows per slot | payload | staged records" in one buffer of 4-byte words:
    ({row name: offset}, payload offset, record offset, total words).  Row i of `rows` is `batch` words at i * batch; the payload
    (`payload_words` words: the receiver's packet matrix, or the jitter receiver's CSR offsets and arrival records) follows the
    rows; `loads` records of `record_len` words follow the payload."""
    row_off: Dict[str, int] = {name: i * int(batch) for i, name in enumerate(rows)}
    payload_off = len(rows) * int(batch)
    rec_off = payload_off + int(payload_words)
    return row_off, payload_off, rec_off, rec_off + int(loads) * int(record_len)


def stage_starts(starts: Dict[int, object], action: Tensor, host_records: Tensor) -> Tuple[int, List[Tensor]]:
    """A hop's queued starts (SessionQueue.starts) -> the action row (which the caller has zeroed: ACTION_KEEP) and the record
    region: a fresh start writes ACTION_ZERO; the record at index r writes r + ACTION_LOAD, the records that live on the host first —
    they are copied into rows [0, n_host) of `host_records`, so that they travel with the stage's pinned copy — then those on the
    device, which the caller copies into rows n_host, n_host + 1, ... of the device region.  Returns (n_host, the device records in
    order)."""
    host = [(s, r) for s, r in starts.items() if r is not None and not r.is_cuda]
    dev = [(s, r) for s, r in starts.items() if r is not None and r.is_cuda]
    for slot, rec in starts.items():
        if rec is None:
            action[slot] = ACTION_ZERO
    for r, (slot, rec) in enumerate(host + dev):
        action[slot] = r + ACTION_LOAD
        if r < len(host):
            host_records[r].copy_(rec)
    return len(host), [rec for _slot, rec in dev]


# ---------------------------------------------------------------- one hop's arrivals (GraphedDecodeHop.play, GraphedForwardHop.forward)
def arrival_width(row_bytes: int) -> int:
    """the words of an arrival record: the byte count, then the headed packet of at most `row_bytes` bytes"""
    return 1 + (int(row_bytes) + 3) // 4


def arrival_region_words(batch: int, max_arrivals: int, row_bytes: int) -> int:
    """the payload words of an arrival region: the CSR offsets of the arrivals [batch + 1], then `max_arrivals` records"""
    return int(batch) + 1 + int(max_arrivals) * arrival_width(row_bytes)


def arrival_bytes(records: Tensor, row_bytes: int) -> Tensor:
    """the packet bytes uint8 [A, row_bytes] of arrival records int32 [A, arrival_width(row_bytes)], as a view"""
    return records.view(torch.uint8)[:, 4:4 + int(row_bytes)]


class Arrivals(NamedTuple):
    """one hop's arrivals, checked: their number A, the slots in push order, the stable order that groups them by slot, and the byte
    counts in that order, clipped to [-1, 2^20] (a kernel needs no more to see a bad count)"""
    count: int
    slots: np.ndarray
    order: np.ndarray
    nbytes: np.ndarray


def check_arrivals(who: str, slots, packets, nbytes, batch: int, max_arrivals: int, row_bytes: int) -> Arrivals:
    """One hop's arrivals in push order — `slots` and `nbytes` A host ints (lists, arrays or host tensors), `packets` uint8 [A,
    row_bytes] on the host or the device — checked for the caller `who` ("play" / "forward": the messages' prefix) before anything is
    written: ValueError for a device tensor of ints, more than `max_arrivals`, a length mismatch or another packet shape or dtype,
    IndexError for a slot outside [0, batch)."""
    for name, v in (("slots", slots), ("nbytes", nbytes)):
        if isinstance(v, Tensor) and v.is_cuda:
            raise ValueError(f"{who}: {name} must be host ints, not a device tensor")
    sl = np.asarray(slots.tolist() if isinstance(slots, Tensor) else slots, dtype=np.int64).reshape(-1)
    nb = np.asarray(nbytes.tolist() if isinstance(nbytes, Tensor) else nbytes, dtype=np.int64).reshape(-1)
    A = len(sl)
    if A > max_arrivals:
        raise ValueError(f"{who}: {A} arrivals, at most max_arrivals = {max_arrivals}")
    if len(nb) != A:
        raise ValueError(f"{who}: {A} slots but {len(nb)} byte counts")
    if not isinstance(packets, Tensor) or packets.dtype != torch.uint8 or tuple(packets.shape) != (A, row_bytes):
        raise ValueError(f"{who}: packets must be uint8 [{A}, {row_bytes}]")
    if A and (sl.min() < 0 or sl.max() >= batch):
        raise IndexError(f"{who}: a slot outside [0, {batch})")
    order = np.argsort(sl, kind="stable")
    return Arrivals(A, sl, order, np.clip(nb[order], -1, 1 << 20).astype(np.int32))


def put_arrivals(arr: Arrivals, packets: Tensor, offsets: Tensor, records: Tensor, row_bytes: int) -> None:
    """checked arrivals -> the mirror's views: the CSR `offsets` int32 [batch + 1], the byte counts of `records` int32 [max_arrivals,
    arrival_width(row_bytes)] grouped by slot and, where `packets` are on the host, their bytes (packets on the device are copied on
    the device: ControlStage.send_arrivals).  Records from A on are left as they are: the offsets end at A"""
    offs = offsets.numpy()
    offs[0] = 0
    offs[1:] = np.cumsum(np.bincount(arr.slots, minlength=len(offs) - 1))
    if arr.count:
        records[:arr.count, 0].copy_(torch.from_numpy(arr.nbytes))
        if not packets.is_cuda:
            arrival_bytes(records[:arr.count], row_bytes).copy_(packets[torch.from_numpy(arr.order)])


class SessionQueue:
    """Host side of GraphedHop's per-stream sessions: what the next hop does to which slot, checked here before anything is
    launched (no device).  `starts[slot]` = None (fresh zeros) or the slot's record; `n[slot]` = its new number of quantiser
    stages.  A later call for the same slot replaces an earlier one of the same hop; `start` without `n` resets the slot to
    `n_max`, the graph's default.  `holds` = the slots held on the next hop only, `stops` = the slots held on every hop until
    their next `start`; `held` = both (a held slot does not advance: GraphedHop.step(hold=...))."""

    def __init__(self, batch: int, n_max: int, max_loads: int, layout, one_sided: bool = False):
        """`layout`: the ops.StateLayout of a state block.  `one_sided`: it holds one side's caches (state_layout(side="enc" /
        "dec")) and a record is that side's list alone; otherwise both lists or neither"""
        self.batch, self.n_max, self.max_loads, self.layout = int(batch), int(n_max), int(max_loads), layout
        self.one_sided = bool(one_sided)
        self.n_min = 1                        # the least n a start or a bitrate may ask for (GraphedEncodeHop(fec_stages=m): m)
        self.starts = {}
        self.n = {}
        self.holds = set()
        self.stops = set()

    def slot(self, slot) -> int:
        s = int(slot)
        if not 0 <= s < self.batch:
            raise IndexError(f"slot {slot} outside [0, {self.batch})")
        return s

    def check_n(self, n) -> int:
        v = int(n)
        if not self.n_min <= v <= self.n_max:
            raise ValueError(f"n = {n} outside [{self.n_min}, {self.n_max}] (the graph's n is the maximum)")
        return v

    @property
    def loads(self) -> int:
        return sum(r is not None for r in self.starts.values())

    @property
    def pending(self) -> bool:
        return bool(self.starts or self.n)

    @property
    def held(self) -> frozenset:
        return frozenset(self.holds | self.stops)

    @property
    def stopped(self) -> Tuple[int, ...]:
        return tuple(sorted(self.stops))

    @staticmethod
    def host_slots(hold) -> List[int]:
        """`hold` (None or an iterable of host ints) -> a list; ValueError for a device tensor (no hidden device sync)"""
        if hold is None:
            return []
        if isinstance(hold, Tensor):
            if hold.device.type != "cpu":
                raise ValueError("hold: host ints, not a device tensor")
            hold = hold.reshape(-1).tolist()
        return [int(s) for s in hold]

    def hold(self, slots) -> None:
        """the slots `slots` (host ints) do not advance on the next hop; every slot is checked before any is taken"""
        held = [self.slot(s) for s in self.host_slots(slots)]
        self.holds.update(held)

    def stop(self, slot) -> None:
        self.stops.add(self.slot(slot))

    def _checked(self, name: str, slots, *excluded) -> List[int]:
        """the slot list `name` of a receiver hop, sorted and without repeats: every slot in range (IndexError), none also in one of
        `excluded` — (what the message calls it, that list as checked) pairs, in the order they are reported — and none stopped
        (ValueError)"""
        slots = sorted({self.slot(s) for s in self.host_slots(slots)})
        for what, other in excluded:
            both = set(slots) & {int(s) for s in other}
            if both:
                raise ValueError(f"{name}: slots {sorted(both)} are also {what} on this hop")
        stopped = set(slots) & self.stops
        if stopped:
            raise ValueError(f"{name}: slots {sorted(stopped)} are stopped (start them first)")
        return slots

    def lost_slots(self, lost, hold=()) -> List[int]:
        """the receiver's `lost` (host ints) checked before anything is launched: every slot in range (IndexError), none also in
        `hold` (this hop's checked holds) and none stopped (ValueError: a held slot's packet is not read at all, a stopped slot has
        no stream to conceal)"""
        return self._checked("lost", lost, ("held", hold))

    def fec_slots(self, fec, hold=(), lost=()) -> List[int]:
        """the receiver's `fec` (host ints) checked before anything is launched: every slot in range (IndexError), none also in
        `hold` or `lost` (this hop's checked holds and losses) and none stopped (ValueError: a FEC slot is decoded from the next
        packet's redundant section, so it is neither held nor concealed, and a stopped slot has no stream)"""
        return self._checked("fec", fec, ("held", hold), ("lost", lost))

    def cn_slots(self, sid, silent, hold=(), lost=(), fec=()) -> Tuple[List[int], List[int]]:
        """the receiver's `sid` and `silent` (host ints) checked before anything is launched: every slot in range (IndexError), the two
        disjoint, neither also in `hold`, `lost` or `fec` (this hop's checked holds, losses and FEC slots) and none stopped (ValueError: a
        comfort-noise slot is neither decoded nor held by the caller, and a stopped slot has no stream)"""
        a = sorted({self.slot(s) for s in self.host_slots(sid)})
        b = sorted({self.slot(s) for s in self.host_slots(silent)})
        both = set(a) & set(b)
        if both:
            raise ValueError(f"sid / silent: slots {sorted(both)} are in both")
        others = (("held", hold), ("lost", lost), ("decoded by FEC", fec))
        return self._checked("sid", a, *others), self._checked("silent", b, *others)

    def start(self, slot, cache_enc=None, cache_dec=None, n=None) -> None:
        s = self.slot(slot)
        v = self.n_max if n is None else self.check_n(n)
        rec = None
        if cache_enc is not None or cache_dec is not None:
            if not self.one_sided and (cache_enc is None or cache_dec is None):
                raise ValueError("start: give both cache lists (encoder and decoder) or neither")
            rec = self.layout.record([] if cache_enc is None else cache_enc, [] if cache_dec is None else cache_dec)
            if self.starts.get(s) is None and self.loads >= self.max_loads:
                raise RuntimeError(f"start: more than {self.max_loads} loads queued for one hop (max_loads_per_hop)")
        self.starts[s] = rec
        self.n[s] = v
        self.stops.discard(s)

    def set_bitrate(self, slot, n) -> None:
        s = self.slot(slot)
        self.n[s] = self.check_n(n)

    def clear(self) -> None:
        """after a hop's upload: drops that hop's starts, bitrates and holds (stops stay)"""
        self.starts.clear()
        self.n.clear()
        self.holds.clear()

    def reset(self) -> None:
        self.clear()
        self.stops.clear()
