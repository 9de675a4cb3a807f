"""Red zones around operands (tests/test_redzone_cpu.py, tests/test_gpu_redzone.py; DESIGN.md, "Operand bounds").

`guarded(t, k, fill)` puts a copy of `t` between two red zones in ONE allocation, as a cache sits between its neighbours in a
`StateBlock`: [front zone | operand | back zone].  The zones hold a pattern that shows when it is read — a quiet NaN for the float
types, 0 or 1 for the integer types (two runs: a stray integer read can equal the baseline in at most one of them, and neither
value can send a kernel that took it for an index to a wild address) — and `check(zone)` shows when one was written.  No GPU code
of its own: torch fills, views and compares, on whatever device `t` is on.  The rows that run inside the zones are `ALL_ROWS` of
tests/entry_rows.py and `MISC` of tests/slot_cases.py; the byte-row entry points are named below."""
import types

import torch

from tests.alignment import skew_bytes

NAN32 = 0x7FC5A5A5                      # quiet NaNs with a payload no kernel produces
NAN64 = 0x7FF8A5A5A5A5A5A5
INT_FILLS = (0, 1)

# what tests/test_gpu_redzone.py runs besides the C-ABI rows (tests/entry_rows.py) and the per-slot float cases (tests/slot_cases.py),
# named here for the ledger of tests/test_redzone_cpu.py: the kernels that move variable-length byte rows, one case each ...
BYTE_ENTRY_POINTS = ("pack_codes_10bit", "pack_codes_10bit_fec", "rvq_decode_packed", "packet_header", "jitter_step", "srtp_protect",
                     "srtp_unprotect", "srtp_protect_routes")
# ... and the same kind of case for entry points that were on the ledger's LATER list
MORE_ENTRY_POINTS = ("fec_select", "conceal_prepare")


def zone_bytes(nbytes: int) -> int:
    """one red zone: as large as the operand (a stray whole row, channel or stream still lands inside), at least 4 KiB, at most
    1 MiB, a multiple of 16"""
    return (min(max(4096, nbytes), 1 << 20) + 15) // 16 * 16


def pattern(dtype: torch.dtype, fill: int = 0) -> bytes:
    """the bytes of one element of the pattern, in memory order (little endian)"""
    size = torch.empty((), dtype=dtype).element_size()
    if dtype == torch.float32:
        return NAN32.to_bytes(4, "little")
    if dtype == torch.float64:
        return NAN64.to_bytes(8, "little")
    assert dtype in (torch.int32, torch.int64, torch.uint8), dtype
    assert fill in INT_FILLS, "integer red zones hold 0 or 1: anything a kernel might take for an index stays in range"
    return int(fill).to_bytes(size, "little")


def _expected(zone, n):
    """n bytes of the pattern in phase with the operand's elements (both zones start a whole number of elements from it)"""
    pat = torch.tensor(list(zone.pattern), dtype=torch.uint8, device=zone.buf.device)
    return pat.repeat(n // len(zone.pattern))


def guarded(t, k: int = 0, fill: int = 0):
    """-> (view, zone): `view` equals `t` (shape, dtype, device, contiguous) and starts on a 16-byte boundary (k = 0) or
    `skew_bytes(dtype, k)` behind one (k = 1..3); `zone` is what `check` takes.  None (a NULL operand) -> (None, None)."""
    if t is None:
        return None, None
    assert k in (0, 1, 2, 3)
    size, nbytes = t.element_size(), t.numel() * t.element_size()
    pat = pattern(t.dtype, fill)
    off = skew_bytes(t.dtype, k) if k else 0
    front = zone_bytes(nbytes) + off                 # the skew belongs to the front zone: every byte of it holds the pattern
    back = zone_bytes(nbytes)
    buf = torch.empty(front + nbytes + back, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 16 == 0 and front % size == 0 and back % size == 0
    zone = types.SimpleNamespace(buf=buf, start=front, end=front + nbytes, pattern=pat, dtype=t.dtype)
    buf[:front] = _expected(zone, front)
    buf[zone.end:] = _expected(zone, back)
    view = buf[front:zone.end].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.shape == t.shape and view.dtype == t.dtype and view.device == t.device
    assert view.data_ptr() == buf.data_ptr() + front and view.data_ptr() % 16 == off
    return view, zone


def damage(zone):
    """[] if both zones still hold the pattern, else one line per damaged side: the side, the byte offsets of the first and the last
    changed byte (in front: relative to the operand's first byte, negative; behind: relative to the first byte past its end, from
    0) and how many bytes changed"""
    if zone is None:
        return []
    found = []
    for side, lo, hi, origin in (("in front of", 0, zone.start, zone.start), ("behind", zone.end, zone.buf.numel(), zone.end)):
        bad = (zone.buf[lo:hi] != _expected(zone, hi - lo)).nonzero().flatten()
        if bad.numel():
            first, last = int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin
            found.append(f"{bad.numel()} byte(s) changed {side} the operand, byte offsets {first} .. {last}")
    return found


def check(zone, what: str = "operand"):
    """both red zones still hold the pattern, bytewise; the operand itself may hold anything"""
    found = damage(zone)
    assert not found, f"{what}: " + "; ".join(found)
