"""CPU: the per-stream session layer of the graphed hop — ABI 16 entry points, their argument checks, the state-block layout
the kernels address, the fake kernels of the two new ops, and the host-side session checks.  (No kernel is launched here.)"""
import ctypes

import pytest
import torch

from tests.hops import assert_entry_points, bare_model

NEW = ("hilc_state_slots_apply", "hilc_state_slots_gather")


def test_abi16_symbols_exported_and_declared():
    assert_entry_points(NEW)


def test_state_slots_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    # apply(block, slice_off, slice_len, nslices, streams, action, records, nrecords, stream)
    assert lib.hilc_state_slots_apply(None, p, p, 52, 4, p, p, 1, None) == -2
    assert lib.hilc_state_slots_apply(p, None, p, 52, 4, p, p, 1, None) == -2
    assert lib.hilc_state_slots_apply(p, p, None, 52, 4, p, p, 1, None) == -2
    assert lib.hilc_state_slots_apply(p, p, p, 52, 4, None, p, 1, None) == -2
    assert lib.hilc_state_slots_apply(p, p, p, 52, 4, p, None, 1, None) == -2      # records promised, none given
    assert lib.hilc_state_slots_apply(p, p, p, 0, 4, p, p, 1, None) == -1
    assert lib.hilc_state_slots_apply(p, p, p, 52, 0, p, p, 1, None) == -1
    assert lib.hilc_state_slots_apply(p, p, p, 52, 4, p, p, -1, None) == -1
    assert lib.hilc_state_slots_apply(p, p, p, 129, 4, p, p, 1, None) == -4      # the slice table is staged in LDS
    assert lib.hilc_state_slots_gather(p, p, p, 129, 4, p, 1, p, None) == -4
    # gather(block, slice_off, slice_len, nslices, streams, slots, nslots, records, stream)
    assert lib.hilc_state_slots_gather(None, p, p, 52, 4, p, 1, p, None) == -2
    assert lib.hilc_state_slots_gather(p, p, p, 52, 4, None, 1, p, None) == -2
    assert lib.hilc_state_slots_gather(p, p, p, 52, 4, p, 1, None, None) == -2
    assert lib.hilc_state_slots_gather(p, p, p, 0, 4, p, 1, p, None) == -1
    assert lib.hilc_state_slots_gather(p, p, p, 52, -3, p, 1, p, None) == -1
    assert lib.hilc_state_slots_gather(p, p, p, 52, 4, p, 0, p, None) == -1


@pytest.mark.parametrize("name", ["hil_speech", "hil_music"])
def test_layout_matches_state_block_views(name):
    """the table the kernels address (graph_step.state_layout, host-only) is the StateBlock's views: slice k of stream b at
    buffer + off[k] + b * lens[k], 16-B aligned slice bases, one record = 76 479 floats"""
    from hilcodec_amd import graph_step as G
    model = bare_model(name)
    B = 3
    layout = G.state_layout(model, B)
    assert layout.record_len == 76479 and len(layout.shapes) == 52 and layout.n_enc == 22 and layout.streams == B
    blk = G.StateBlock(model, B, torch.device("cpu"))
    assert blk.layout.off == layout.off and blk.layout.lens == layout.lens and blk.buffer.numel() == layout.total
    base = blk.buffer.data_ptr()
    ce, cd = model.initialize_cache(torch.zeros(B, 1, 1))
    for v, ref, o, n in zip(blk.enc + blk.dec, ce + cd, layout.off, layout.lens):
        assert v.shape == ref.shape and n == ref.shape[1] * ref.shape[2] and o % 4 == 0
        for b in range(B):
            assert v[b].data_ptr() == base + 4 * (o + b * n)
    assert layout.lens[0] == 1023                          # the waveform history: stream slices after the first misaligned
    # record <-> caches: concatenation in slice order, split back into B = 1 views
    blk.buffer.copy_(torch.arange(blk.buffer.numel(), dtype=torch.float32))
    enc, dec = [c[1:2] for c in blk.enc], [c[1:2] for c in blk.dec]
    rec = layout.record(enc, dec)
    assert rec.shape == (76479,)
    e2, d2 = layout.split(rec)
    assert len(e2) == 22 and len(d2) == 30
    assert all(torch.equal(a, b) for a, b in zip(e2 + d2, enc + dec))
    assert layout.tables(torch.device("cpu"))[0].dtype == torch.int64


def test_session_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hilcodec_amd import graph_step as G, ops
    layout = G.state_layout(bare_model(), 5)
    for name in ("state_slots_apply", "state_slots_gather"):
        assert hasattr(torch.ops.hilcodec, name)
    schema = str(torch.ops.hilcodec.state_slots_apply.default._schema)
    assert "Tensor(a!) block" in schema
    with FakeTensorMode():
        block = torch.empty(layout.total)
        off = torch.empty(52, dtype=torch.int64)
        lens = torch.empty(52, dtype=torch.int32)
        out = torch.ops.hilcodec.state_slots_gather(block, off, lens, torch.empty(3, dtype=torch.int32), 5, layout.record_len)
        assert out.shape == (3, 76479) and out.dtype == torch.float32
        assert torch.ops.hilcodec.state_slots_apply(block, off, lens, torch.empty(5, dtype=torch.int32),
                                                    torch.empty(4, 76479)) is None
        # the device-resident per-clip n of the quantiser ops: indices keep `n` rows
        z = torch.empty(5, 1, 128)
        cb = torch.empty(8, 1024, 128)
        idx, _, _ = ops.rvq_encode(z, cb, cb.transpose(1, 2).contiguous(), torch.empty(8, 1024), 8, channel_last=True,
                                   stage_major=True, want_q=False, n_clip=torch.empty(5, dtype=torch.int32))
        assert idx.shape == (8, 5, 1) and idx.dtype == torch.int64
        q = ops.rvq_decode(idx, cb, 8, n_clip=torch.empty(5, dtype=torch.int32))
        assert q.shape == (5, 1, 128)
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.state_slots_gather(torch.zeros(layout.total), torch.zeros(52, dtype=torch.int64),
                                              torch.zeros(52, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 5, 76479)


def test_session_queue_checks():
    """everything a GraphedHop(sessions=True) refuses is refused by the host-side queue before any launch"""
    from hilcodec_amd import graph_step as G
    model = bare_model()
    layout = G.state_layout(model, 6)
    q = G.SessionQueue(6, 8, 2, layout)
    for bad in (-1, 6, 100):
        with pytest.raises(IndexError):
            q.start(bad)
        with pytest.raises(IndexError):
            q.set_bitrate(bad, 4)
    for bad in (0, 9, -2):
        with pytest.raises(ValueError):
            q.set_bitrate(1, bad)
        with pytest.raises(ValueError):
            q.start(1, n=bad)
    assert not q.pending
    ce, cd = model.initialize_cache(torch.zeros(1, 1, 1))
    q.start(0, ce, cd, n=4)
    q.start(0, ce, cd)                                    # the same slot again: replaces, not a second load
    q.start(1, ce, cd)
    assert q.loads == 2 and q.n == {0: 8, 1: 8}
    with pytest.raises(RuntimeError):
        q.start(2, ce, cd)                                # a third load in one hop
    q.start(2)                                            # fresh starts are not loads
    q.set_bitrate(2, 1)
    assert q.starts[2] is None and q.n[2] == 1 and q.loads == 2
    with pytest.raises(ValueError):
        q.start(3, ce, None)                              # one list without the other
    with pytest.raises(ValueError):
        q.start(3, ce[:-1], cd)                           # a cache missing
    bad = list(cd)
    bad[4] = torch.zeros(1, bad[4].shape[1], bad[4].shape[2] + 1)
    with pytest.raises(ValueError):
        q.start(3, ce, bad)                               # a shape that does not match
    with pytest.raises(ValueError):
        q.start(3, [c.expand(2, -1, -1) for c in ce], cd)  # B = 2 caches: one stream only
    q.clear()
    assert not q.pending and q.loads == 0


def test_pipelined_hop_refuses_sessions():
    from hilcodec_amd.graph_step import PipelinedHop
    with pytest.raises(NotImplementedError):
        PipelinedHop(None, 4, 320, 8, torch.device("cpu"), sessions=True)


@pytest.mark.parametrize("B", [1, 5, 1024])
def test_stage_layout_matches_the_three_layouts(B):
    """sessions.stage_layout gives the word offsets the three hops used to compute by hand (written out here as literals)"""
    from hilcodec_amd.sessions import arrival_region_words, stage_layout
    for loads, L in ((0, 37), (3, 37)):
        # GraphedHop / GraphedEncodeHop: action, n, hold, then the records
        rows, pay, rec, total = stage_layout(B, ("action", "n_slot", "hold"), 0, loads, L)
        assert rows == {"action": 0, "n_slot": B, "hold": 2 * B}
        assert pay == rec == 3 * B and total == 3 * B + loads * L
        # GraphedDecodeHop.step: (3 + conceal + (m > 0)) rows, the packet matrix rounded up to words, the records
        for conceal in (False, True):
            for m in (0, 2):
                for stride in (1, 7, 10, 13, 255):
                    names = ["action", "n_slot", "hold"] + ["lost"] * conceal + ["fec"] * (m > 0)
                    rows, pay, rec, total = stage_layout(B, names, (B * stride + 3) // 4, loads, L)
                    n_ctl = (3 + conceal + (m > 0)) * B
                    assert (rows["action"], rows["n_slot"], rows["hold"]) == (0, B, 2 * B)
                    assert rows.get("lost") == (3 * B if conceal else None)
                    assert rows.get("fec") == (n_ctl - B if m else None)          # the last row
                    assert pay == n_ctl and rec == n_ctl + (B * stride + 3) // 4 and total == rec + loads * L
        # GraphedDecodeHop.play: action, hold, the CSR offsets [B + 1], max_arrivals records of 1 + ceil(tstride / 4) words
        for max_arrivals in (1, 2 * B, 2 * B + 1):
            for tstride in (3, 13, 16, 257):
                aw = 1 + (tstride + 3) // 4
                assert arrival_region_words(B, max_arrivals, tstride) == B + 1 + max_arrivals * aw
                rows, pay, rec, total = stage_layout(B, ("action", "hold"), arrival_region_words(B, max_arrivals, tstride), loads, L)
                assert rows == {"action": 0, "hold": B} and pay == 2 * B
                assert pay + B + 1 == 3 * B + 1                                    # where the arrival records begin
                assert rec == 3 * B + 1 + max_arrivals * aw and total == rec + loads * L


def test_stage_starts_rule():
    """queued starts -> action row and records: a fresh start writes -1, host records come first, the record at index r writes
    r + 1, a later start for the same slot replaces the earlier one"""
    from types import SimpleNamespace
    from hilcodec_amd import ops
    from hilcodec_amd.sessions import SessionQueue, stage_starts
    B = 6
    layout = ops.StateLayout([(B, 1, 2), (B, 1, 3)], 1)
    q = SessionQueue(B, 8, 4, layout)
    rec = lambda v: ([torch.full((1, 1, 2), float(v))], [torch.full((1, 1, 3), float(v))])
    q.start(4)
    q.start(1, *rec(1.0))
    q.start(5, *rec(5.0))
    q.start(1)                                            # replaces the resume of slot 1 by a fresh start
    q.start(4, *rec(4.0))                                 # replaces the fresh start of slot 4 by a resume
    q.start(0, *rec(7.0))
    on_device = SimpleNamespace(is_cuda=True)             # stands for a record that lives on the device: handed back, not copied
    q.starts[2] = on_device
    q.starts[3] = None
    action = torch.zeros(B, dtype=torch.int32)
    h_records = torch.zeros(4, layout.record_len)
    n_host, dev = stage_starts(q.starts, action, h_records)
    assert n_host == 3 and dev == [on_device]
    # host records in queue order: slot 4, slot 5, slot 0; then the device record of slot 2
    assert action.tolist() == [3, -1, 4, -1, 1, 2]
    assert h_records[:, 0].tolist() == [4.0, 5.0, 7.0, 0.0] and bool((h_records[:3] == h_records[:3, :1]).all())
    assert stage_starts({}, action.zero_(), h_records) == (0, []) and not action.any()


# ---------------------------------------------------------------- one hop's arrivals (sessions.check_arrivals / put_arrivals)
class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: what the refusals look at, without a device"""
    is_cuda = True


def _stage_arrivals(who, slots, packets, nbytes, B, max_a, tb, offsets, records):
    """what GraphedDecodeHop.play and GraphedForwardHop.forward do with a hop's arrivals, on plain host tensors"""
    from hilcodec_amd.sessions import check_arrivals, put_arrivals
    arr = check_arrivals(who, slots, packets, nbytes, B, max_a, tb)
    put_arrivals(arr, packets, offsets, records, tb)
    return arr


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("tb", [13, 16])
def test_arrival_staging_matches_the_numpy_statement(B, tb):
    """seeded arrivals — unsorted slots with repeats, byte counts inside and outside [-1, 2^20], slots and counts as lists, arrays
    and host tensors — staged by sessions.check_arrivals / put_arrivals equal forward.arrival_records bit for bit, offsets and
    records, for A in {0, 1, max_arrivals}"""
    import numpy as np
    from hilcodec_amd import forward
    from hilcodec_amd.sessions import arrival_region_words, arrival_width
    max_a = 2 * B + 1
    aw = arrival_width(tb)
    assert aw == 1 + (tb + 3) // 4 and arrival_region_words(B, max_a, tb) == B + 1 + max_a * aw
    rng = np.random.default_rng(100 * B + tb)
    wild = np.array([-7, -2, -1, 0, 1 << 20, (1 << 20) + 1, 1 << 31, -(1 << 40)], dtype=np.int64)
    for A in (0, 1, max_a):
        slots = rng.integers(0, B, A)
        if A == max_a and B > 1:
            assert len(set(slots.tolist())) < A and list(slots) != sorted(slots)       # repeats, and not already grouped
        nbytes = np.where(rng.random(A) < 0.5, rng.integers(0, tb + 1, A), rng.choice(wild, A))
        if A == max_a:
            nbytes[:len(wild)] = wild[:A]
        packets = rng.integers(0, 256, (A, tb), dtype=np.uint8)
        packets[:, 0] = np.arange(A) & 0xFF                                            # the push order, readable in the records
        rec, offs = forward.arrival_records(slots, packets, nbytes, tb, B, max_a)
        forms = {"list": list, "array": np.asarray, "tensor": lambda v: torch.from_numpy(np.asarray(v))}
        for name, form in forms.items():
            offsets, records = torch.zeros(B + 1, dtype=torch.int32), torch.zeros(max_a, aw, dtype=torch.int32)
            arr = _stage_arrivals("play", form(slots.tolist()), torch.from_numpy(packets), form(nbytes.tolist()), B, max_a, tb,
                                  offsets, records)
            assert arr.count == A and arr.order.tolist() == sorted(range(A), key=lambda a: slots[a]), name
            assert np.array_equal(offsets.numpy(), offs) and offsets.numpy().dtype == offs.dtype, name
            assert np.array_equal(records.numpy(), rec) and records.numpy().dtype == rec.dtype, name
        # grouped by slot, and within a slot in push order; the counts clipped
        got = records.numpy()
        for b in range(B):
            pushed = [a for a in range(A) if slots[a] == b]
            lo, hi = int(offsets[b]), int(offsets[b + 1])
            assert got.view(np.uint8)[lo:hi, 4].tolist() == [a & 0xFF for a in pushed]
            assert got[lo:hi, 0].tolist() == [int(min(max(nbytes[a], -1), 1 << 20)) for a in pushed]


@pytest.mark.parametrize("who", ["play", "forward"])
def test_arrival_staging_refusals(who):
    """every refusal of play / forward comes from the one function, with the caller's name in front, before anything is written"""
    B, max_a, tb = 4, 6, 13
    packets = torch.zeros(3, tb, dtype=torch.uint8)
    device_ints = torch.Tensor._make_subclass(_OnDevice, torch.zeros(3))
    assert isinstance(device_ints, torch.Tensor) and device_ints.is_cuda
    cases = [
        (ValueError, f"{who}: slots must be host ints, not a device tensor", (device_ints, packets, [1, 2, 3])),
        (ValueError, f"{who}: nbytes must be host ints, not a device tensor", ([0, 1, 2], packets, device_ints)),
        (ValueError, f"{who}: 7 arrivals, at most max_arrivals = 6", ([0] * 7, torch.zeros(7, tb, dtype=torch.uint8), [1] * 7)),
        (ValueError, f"{who}: 3 slots but 2 byte counts", ([0, 1, 2], packets, [1, 2])),
        (ValueError, f"{who}: packets must be uint8 [3, 13]", ([0, 1, 2], torch.zeros(3, tb + 1, dtype=torch.uint8), [1, 2, 3])),
        (ValueError, f"{who}: packets must be uint8 [3, 13]", ([0, 1, 2], torch.zeros(2, tb, dtype=torch.uint8), [1, 2, 3])),
        (ValueError, f"{who}: packets must be uint8 [3, 13]", ([0, 1, 2], torch.zeros(3, tb, dtype=torch.int32), [1, 2, 3])),
        (ValueError, f"{who}: packets must be uint8 [3, 13]", ([0, 1, 2], packets.numpy(), [1, 2, 3])),
        (IndexError, f"{who}: a slot outside [0, 4)", ([0, 4, 2], packets, [1, 2, 3])),
        (IndexError, f"{who}: a slot outside [0, 4)", ([0, -1, 2], packets, [1, 2, 3])),
    ]
    offsets = torch.full((B + 1,), 77, dtype=torch.int32)
    records = torch.full((max_a, 1 + (tb + 3) // 4), 77, dtype=torch.int32)
    for kind, message, (slots, pk, nbytes) in cases:
        with pytest.raises(kind) as e:
            _stage_arrivals(who, slots, pk, nbytes, B, max_a, tb, offsets, records)
        assert str(e.value) == message and type(e.value) is kind
        assert bool((offsets == 77).all()) and bool((records == 77).all())
    _stage_arrivals(who, [3, 0, 3], packets, [5, 6, 7], B, max_a, tb, offsets, records)       # and an accepted hop does write
    assert offsets.tolist() == [0, 1, 1, 1, 3] and records[:3, 0].tolist() == [6, 5, 7] and bool((records[3:] == 77).all())


def test_control_stage_refuses_a_payload_beside_arrivals():
    """the arrival region is the stage's whole payload: a payload size of the caller's own beside it is refused, before anything
    is allocated"""
    from hilcodec_amd.graph_step import ControlStage
    with pytest.raises(ValueError, match="payload_words must be 0 with arrivals"):
        ControlStage(4, ("action", "hold"), 5, 0, 0, torch.device("cpu"), arrivals=(2, 13))
