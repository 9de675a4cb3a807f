"""The red-zone harness itself (tests/redzone.py) on CPU tensors, and the ledger of what tests/test_gpu_redzone.py covers.

`guarded` must return what it claims, `check` must see one changed byte at either end of either zone and nothing inside the
operand, and a leak must show: a read one element past the view (the float fill turns a sum into NaN, the two integer fills give two
different sums) and a store one element past it (`check` names offset 0 behind the operand).  The leaky operations are plain torch
on the parent buffer — no kernel is broken to prove that the GPU tests can fail."""
import re

import pytest
import torch

from tests import redzone as R
from tests.alignment import skew_bytes
from tests.entry_rows import ALL_ROWS, entry_of
from tests.hops import parse_header
from tests.slot_cases import MISC

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)
SIZES = (1, 17, 1100)                    # one element, a ragged few, more than 4096 bytes in every type but uint8 ...
BIG_U8 = 4101                            # ... whose own "larger than a zone's minimum" size this is


def operand(dtype, n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    if dtype.is_floating_point:
        return torch.randn(n, generator=g, dtype=dtype)
    return torch.randint(2, 200, (n,), generator=g).to(dtype)          # no 0 and no 1: the operand never looks like a zone


def fills(dtype):
    return (0,) if dtype.is_floating_point else R.INT_FILLS


def sizes(dtype):
    return SIZES + ((BIG_U8,) if dtype == torch.uint8 else ())


def expected_zone(dtype, fill, nbytes):
    return torch.tensor(list(R.pattern(dtype, fill)), dtype=torch.uint8).repeat(nbytes // len(R.pattern(dtype, fill)))


def test_patterns_are_what_the_contract_names():
    assert R.pattern(torch.float32) == bytes([0xA5, 0xA5, 0xC5, 0x7F]) and R.pattern(torch.float64) == bytes([0xA5] * 6 + [0xF8, 0x7F])
    assert torch.frombuffer(bytearray(R.pattern(torch.float32)), dtype=torch.float32).isnan().all()
    assert torch.frombuffer(bytearray(R.pattern(torch.float64)), dtype=torch.float64).isnan().all()
    for dtype in (torch.int32, torch.int64, torch.uint8):
        for fill in R.INT_FILLS:
            assert int(torch.frombuffer(bytearray(R.pattern(dtype, fill)), dtype=dtype)[0]) == fill
        with pytest.raises(AssertionError):
            R.pattern(dtype, 0x7FFFFFFF)                      # nothing a kernel could turn into a wild address
    assert [R.zone_bytes(n) for n in (0, 4, 4096, 4097, 5000, 1 << 20, (1 << 20) + 1, 1 << 24)] == [4096, 4096, 4096, 4112, 5008, 1 << 20,
                                                                                                   1 << 20, 1 << 20]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_guarded_returns_what_it_claims(dtype, k):
    for n in sizes(dtype):
        t = operand(dtype, n).view(1, n) if n > 1 else operand(dtype, n)
        for fill in fills(dtype):
            view, zone = R.guarded(t, k, fill)
            assert view.shape == t.shape and view.dtype == t.dtype and view.device == t.device and view.is_contiguous()
            assert torch.equal(view, t) and view.data_ptr() != t.data_ptr()
            assert view.data_ptr() % 16 == (skew_bytes(dtype, k) if k else 0)
            nbytes = t.numel() * t.element_size()
            z = R.zone_bytes(nbytes)
            assert z % 16 == 0 and z >= max(4096, min(nbytes, 1 << 20))
            # one allocation: zone, operand, zone
            assert zone.buf.data_ptr() + zone.start == view.data_ptr() and zone.end - zone.start == nbytes
            assert zone.start == z + (skew_bytes(dtype, k) if k else 0) and zone.buf.numel() - zone.end == z
            assert torch.equal(zone.buf[:zone.start], expected_zone(dtype, fill, zone.start))
            assert torch.equal(zone.buf[zone.end:], expected_zone(dtype, fill, z))
            assert torch.equal(zone.buf[zone.start:zone.end].view(dtype).view(t.shape), t)
            R.check(zone)
            view.fill_(3)                                     # the operand itself may be overwritten
            R.check(zone)
            assert R.damage(zone) == []


def test_null_stays_null():
    assert R.guarded(None) == (None, None) and R.guarded(None, 1, 1) == (None, None)
    R.check(None)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_check_sees_one_byte_at_every_end(dtype):
    for fill in fills(dtype):
        _, zone = R.guarded(operand(dtype, 17), 1, fill)
        total, nbytes = zone.buf.numel(), zone.end - zone.start
        for at, side, offset in ((0, "in front of", -zone.start), (zone.start - 1, "in front of", -1), (zone.end, "behind", 0),
                                 (total - 1, "behind", total - 1 - zone.end)):
            keep = int(zone.buf[at])
            zone.buf[at] = keep ^ 0x10
            with pytest.raises(AssertionError, match=rf"cache: 1 byte\(s\) changed {side} the operand, byte offsets {offset} \.\. {offset}$"):
                R.check(zone, "cache")
            zone.buf[at] = keep
            R.check(zone)
        zone.buf[zone.start:zone.end] = 0x5A                   # every byte of the operand: silent
        R.check(zone)
        zone.buf[zone.start - 2], zone.buf[zone.end + 5], zone.buf[zone.end + 8] = 0xEE, 0xEE, 0xEE
        assert R.damage(zone) == ["1 byte(s) changed in front of the operand, byte offsets -2 .. -2",
                                  "2 byte(s) changed behind the operand, byte offsets 5 .. 8"]
        assert nbytes == 17 * torch.empty((), dtype=dtype).element_size()


def _sum_one_past(view, zone):
    """a leaky reduction: numel + 1 elements of the parent buffer, from the view's first"""
    size = view.element_size()
    flat = zone.buf[zone.start:zone.end + size].view(view.dtype)
    return flat.double().sum() if view.dtype.is_floating_point else flat.long().sum()


def _store_one_past(view, zone):
    """a leaky copy: writes numel + 1 elements"""
    size = view.element_size()
    zone.buf[zone.start:zone.end + size].view(view.dtype).fill_(7)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("k", [0, 1])
def test_a_leak_is_detected(dtype, k):
    t = operand(dtype, 17, seed=5)
    honest = t.double().sum() if dtype.is_floating_point else t.long().sum()
    got = []
    for fill in fills(dtype):
        view, zone = R.guarded(t, k, fill)
        got.append(_sum_one_past(view, zone))
        R.check(zone)                                          # a read leaves no trace in the zones: only the result shows it
    if dtype.is_floating_point:
        assert torch.isnan(got[0]) and not torch.isnan(honest)
    else:
        assert got[0] != got[1] and [int(g) for g in got] == [int(honest), int(honest) + 1]       # at most one run can equal the baseline
    for fill in fills(dtype):
        view, zone = R.guarded(t, k, fill)
        _store_one_past(view, zone)
        size = t.element_size()
        changed = sum(1 for i, p in enumerate(R.pattern(dtype, fill)) if p != (7).to_bytes(size, "little")[i]) if not dtype.is_floating_point else None
        with pytest.raises(AssertionError, match=r"behind the operand, byte offsets 0 \.\. ") as err:
            R.check(zone, "out")
        assert "in front of" not in str(err.value)
        if changed is not None:
            assert f"{changed} byte(s) changed behind" in str(err.value)


# ======================================================================================================================
# the ledger: every entry point of include/hilcodec_amd.h is in exactly one class
# ======================================================================================================================
# The only names that may ever stand in LATER (the list the project agreed on when these tests were written): a name may leave, none may join.
LATER_ALLOWED = frozenset("""dws_conv_wave_row up_conv_expand_taps resblock_pack_weights resblock_pack_weights_rc resblock_balanced spec_block_pack
rvq_encode_mixed rvq_decode_mixed mse_finalize rvq_ema_stats rvq_ema_update conceal_prepare fec_select dtx_encode jitter_adapt_step mix_gains
mix_rooms_dyn rx_report fec_adapt nack_build rtx_step rate_ceiling rate_charge forward_classify forward_route forward_rank downlink_store
downlink_step rx_bwe rate_cap""".split())

# entry points whose operands are not yet run inside red zones, each with what its case needs
LATER = {
    "up_conv_expand_taps": "a one-off table builder; its output is an input of the up_conv_expanded row, its own call is not guarded yet",
    "resblock_pack_weights": "a one-off re-layout at model load; needs a row whose reference is the packed layout",
    "resblock_pack_weights_rc": "as resblock_pack_weights, per row class",
    "spec_block_pack": "a one-off re-layout at model load",
    "mse_finalize": "training side: a reduction of frame_err to one float",
    "rvq_ema_stats": "training side: cluster statistics",
    "rvq_ema_update": "training side: in place on three tables",
    "dtx_encode": "byte rows and control rows of the DTX sender; case to be modelled on tests/test_gpu_dtx.py",
    "jitter_adapt_step": "jitter_step plus the adapt rows; case to be modelled on tests/test_gpu_jitter_adapt.py",
    "mix_gains": "float64 rows of the levelling mixer; case to be modelled on tests/test_gpu_mix_dyn.py",
    "mix_rooms_dyn": "as mix_gains",
    "rx_report": "int32 rows of the reporting receiver; case to be modelled on tests/test_gpu_report.py",
    "fec_adapt": "as rx_report",
    "nack_build": "int32 and byte rows of the NACK receiver; case to be modelled on tests/test_gpu_rtx.py",
    "rtx_step": "as nack_build, with the sender's history ring",
    "rate_ceiling": "int32 rows of the rate controller; case to be modelled on tests/test_gpu_rate.py",
    "rate_charge": "as rate_ceiling",
    "forward_classify": "arrival records of the forwarder; case to be modelled on tests/test_gpu_forward.py",
    "forward_route": "as forward_classify, with the fan-out rows",
    "forward_rank": "as forward_classify, with the level rows",
    "downlink_store": "the forwarder's per-listener history; case to be modelled on tests/test_gpu_downlink.py",
    "downlink_step": "as downlink_store",
    "rx_bwe": "int32 rows of the bandwidth estimator; case to be modelled on tests/test_gpu_bwe.py",
    "rate_cap": "as rx_bwe",
}


# entry points outside the name patterns below that launch nothing on a caller's operand, each with the reason (read in csrc/): a new
# `hilc_*` function of a similar name is NOT admitted by analogy, it has to be added here with its own
NO_KERNEL = {
    "abi_version": "returns HILC_ABI_VERSION",
    "error_string": "maps a return code to a constant string (rvq.hip): no pointer argument",
    "last_hip_error": "returns the host-side record of the last HIP error (rvq.hip): no pointer argument",
    "dws_conv_wave_row": "the launch heuristic of hilc_dws_conv as a query: a pure function of four ints and the CU count (gemm.hip)",
}


def launches_no_kernel(name):
    """queries that answer from their arguments (and the device's CU count) alone: nothing is launched on a caller's operand"""
    return name in NO_KERNEL or re.search(r"(_supported|_row_classes(_offline)?|_packed_floats)$", name) is not None


def test_ledger():
    protos, _ = parse_header()
    declared = {n[len("hilc_"):] for n in protos}
    assert len(declared) >= 80
    classes = {"row": {entry_of(n) for n in ALL_ROWS}, "misc": set(MISC), "bytes": set(R.BYTE_ENTRY_POINTS) | set(R.MORE_ENTRY_POINTS),
               "no kernel": {n for n in declared if launches_no_kernel(n)}, "later": set(LATER)}
    for cls, names in classes.items():
        assert names <= declared, f"class `{cls}` names what the header does not declare: {sorted(names - declared)}"
    where = {n: [c for c, names in classes.items() if n in names] for n in declared}
    assert not [n for n, c in where.items() if not c], f"entry points in no class (guard them or say why not): {sorted(n for n, c in where.items() if not c)}"
    assert not [n for n, c in where.items() if len(c) > 1], {n: c for n, c in where.items() if len(c) > 1}
    assert set(LATER) <= LATER_ALLOWED and all(reason and "\n" not in reason for reason in LATER.values())
    assert set(MISC) == {"resample_poly", "mix_levels", "mix_rooms", "conceal_gain", "cng_synth", "audio_level", "vbr_select",
                                 "state_slots_apply", "state_slots_gather", "state_slots_hold"}
    assert set(R.BYTE_ENTRY_POINTS) == {"pack_codes_10bit", "pack_codes_10bit_fec", "rvq_decode_packed", "packet_header", "jitter_step",
                                        "srtp_protect", "srtp_unprotect", "srtp_protect_routes"}
