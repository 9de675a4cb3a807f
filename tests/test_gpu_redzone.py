"""No entry point reads or writes outside its operands ("Operand bounds").

Every other GPU test hands the library fresh allocations: a load a few words before or after one lands in allocator slack — finite,
usually zero — and a store past the end goes where nobody looks.  In a `graph_step.StateBlock` the neighbour is another layer's cache.
Here every operand lies between two red zones of one allocation (tests/redzone.py): quiet NaNs around float operands, 0 or 1 around
integer ones (two runs).  A call must return what the same call returns on plain allocations, bit for bit — a stray value that
reaches an output shows as a NaN or as a difference between the two integer runs, even where it is multiplied by zero — and every
zone must still hold its pattern afterwards.

The C-ABI rows are `ALL_ROWS` of tests/entry_rows.py: the base rows of the alignment sweep (raw pointers, small ragged shapes, a
float64 reference, a checked aligned baseline) plus its `EDGE` rows, which cross the tile edges the base rows lack; the per-slot
float kernels are the `MISC` cases of tests/slot_cases.py plus the layouts below; the kernels that move variable-length byte rows
(`BYTE_ENTRY_POINTS` and `MORE_ENTRY_POINTS` of tests/redzone.py) get one case each against their host models."""
import numpy as np
import pytest
import torch

from tests import alignment as A
from tests import slot_cases
from tests.entry_rows import ALL_ROWS, EDGE, EDGE_FLOORS, FLOORS, ROWS, SENT, aligned, built, check_ok, env, rnd, sentinel  # noqa: F401  (env: the fixture)
from tests.hops import CONCEAL_FADE as F
from tests.hops import pack_model, prepare_model, select_model
from tests.redzone import INT_FILLS, check, damage, guarded

pytestmark = pytest.mark.gpu

# what the fused rows must be: the shapes the library takes in one launch (else the row would test a fall-back)
FUSED = {"resblock-64x132x2": ("hilc_resblock_supported", (64, 132)), "resblock_stream-64x160x5": ("hilc_resblock_stream_supported", (64, 160)),
         "resblock_chain-64x132x2-offline": ("hilc_resblock_chain_supported", (64, 132, 2, 0)),
         "resblock_chain-64x160x5-stream": ("hilc_resblock_chain_supported", (64, 160, 2, 1)),
         "encoder_stage-128x132-r4-offline": ("hilc_encoder_stage_supported", (128, 132, 2, 4, 0)),
         "encoder_stage-128x160-r4-stream": ("hilc_encoder_stage_supported", (128, 160, 2, 4, 1)),
         "decoder_stage-96-r2-Tin66-offline": ("hilc_decoder_stage_supported", (96, 132, 3, 2, 0)),
         "decoder_stage-96-r2-Tin80-stream": ("hilc_decoder_stage_supported", (96, 160, 3, 2, 1)),
         "encoder_stage0-T132-offline": ("hilc_encoder_stage0_supported", (132, 2, 2, 64, 1, 5, 0)),
         "encoder_stage0-T160-stream": ("hilc_encoder_stage0_supported", (160, 2, 2, 64, 1, 5, 1)),
         "decoder_stage_post-96-r2-Tin66-offline": ("hilc_decoder_stage_post_supported", (96, 132, 3, 2, 5)),
         "decoder_stage_post-96-r2-Tin80-stream": ("hilc_decoder_stage_post_supported", (96, 160, 3, 2, 5)),
         "spec_block-n64-T132": ("hilc_spec_block_supported", (64, 1, 64, 132)), "spec_block-n64-T516": ("hilc_spec_block_supported", (64, 1, 64, 516))}


def test_edge_rows(env):
    assert set(ROWS) == set(FLOORS) and set(EDGE) <= set(ROWS) and set(FUSED) <= set(EDGE)          # every row has its floor
    for name, (query, args) in FUSED.items():
        assert getattr(env.lib, query)(*args) == 1, f"{name}: {query}{args} != 1"
    for name in EDGE:
        r = ROWS[name]
        assert r.tol >= 4 * EDGE_FLOORS[name], name
        b = built(env, name)
        assert set(r.cls) == {o for o, t in b.ins.items() if t is not None} | set(b.outs), name


# ======================================================================================================================
# the rows inside red zones
# ======================================================================================================================
def _out_spec(shape):
    return shape if isinstance(shape[0], tuple) else (shape, torch.float32)


def _has_int(b):
    return any(t is not None and not t.is_floating_point() for t in b.ins.values()) or \
        any(not _out_spec(s)[1].is_floating_point for s in b.outs.values())


def fills_of(b):
    return INT_FILLS if _has_int(b) else (0,)


def run_guarded(e, name, guard=None, k=0, fill=0):
    """one call of the row with the operands `guard` (None: every one, inputs and outputs) inside red zones, `k` * 4 bytes off a
    16-byte boundary; the others are plain allocations.  -> (return code, {output: CPU tensor}, {operand: zone}, [inputs the call
    changed])"""
    b = built(e, name)
    ins, outs, zones = {}, {}, {}
    for o, t in b.ins.items():
        if t is not None and (guard is None or o in guard):
            ins[o], zones[o] = guarded(t, k, fill)
        else:
            ins[o] = None if t is None else t.clone()
    for o, shape in b.outs.items():
        shape, dtype = _out_spec(shape)
        t = torch.full(shape, SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device=e.dev)
        if guard is None or o in guard:
            outs[o], zones[o] = guarded(t, k, fill)
        else:
            outs[o] = t
    p = {}
    for o, t in list(ins.items()) + list(outs.items()):
        p[o] = None if t is None else t.data_ptr()
        assert t is None or p[o] % 16 == (A.skew_bytes(t.dtype, k) if k and o in zones else 0), (name, o)
    rc = b.call(p)
    torch.cuda.synchronize()
    changed = [o for o, t in ins.items() if t is not None and not torch.equal(t, b.ins[o])]
    return rc, {o: t.cpu() for o, t in outs.items()}, zones, changed


def _differs(t, want):
    if torch.equal(t, want):
        return None
    bad = t != want
    nan = int(torch.isnan(t).sum()) if t.is_floating_point() else 0
    first = int(bad.flatten().nonzero()[0])
    return f"{int(bad.sum())} of {t.numel()} elements differ from the call on plain allocations ({nan} NaN), the first at flat index {first}"


def verdict(name, base, rc, outs, zones, changed, exact=True):
    """what is wrong with one guarded call, as a list of lines (empty: nothing)"""
    if rc != 0:
        return [f"the call returned {rc}"]
    lines = [f"input `{o}` was changed" for o in changed]
    for o, t in outs.items():
        if sentinel(t):
            lines.append(f"output `{o}` was not written")
        elif exact is True or o in exact:
            d = _differs(t, base[o])
            if d:
                lines.append(f"output `{o}`: {d}")
    for o, z in zones.items():
        lines += [f"red zone of `{o}`: {d}" for d in damage(z)]
    return lines


def diagnose(e, name, base, fill):
    """after a failed all-guarded call (which returned normally): the same call with ONE input inside red zones at a time — the inputs
    whose surroundings alone reach an output"""
    b = built(e, name)
    lines = []
    for o, t in b.ins.items():
        if t is None:
            continue
        rc, outs, _, _ = run_guarded(e, name, {o}, 0, fill)
        hit = [u for u, v in outs.items() if rc == 0 and not torch.equal(v, base[u])]
        if hit:
            lines.append(f"with only `{o}` guarded: {', '.join('`' + u + '`' for u in hit)} change{'s' if len(hit) == 1 else ''}")
    return lines or ["no single guarded input changes an output on its own"]


@pytest.mark.parametrize("name", ALL_ROWS)
def test_all_operands_guarded(env, name):
    """every input and every caller-owned output in red zones of its own, outputs pre-filled with the sentinel, once per integer fill:
    return code 0, every output equal to the aligned call on plain allocations and written, every zone intact, inputs unchanged"""
    base = aligned(env, name)
    for fill in fills_of(built(env, name)):
        rc, outs, zones, changed = run_guarded(env, name, None, 0, fill)
        assert set(zones) == set(ROWS[name].cls)
        lines = verdict(name, base, rc, outs, zones, changed)
        if lines:
            if rc == 0:
                written = [o for o, z in zones.items() if damage(z)]
                lines.append("zones written: " + (", ".join(written) or "none"))
                lines += diagnose(env, name, base, fill)
            raise AssertionError(f"{name} [all operands guarded, integer fill {fill}]:\n  " + "\n  ".join(lines))


@pytest.mark.parametrize("name", ALL_ROWS)
def test_one_operand_guarded_and_skewed(env, name):
    """every operand of class S or F in turn inside red zones AND 4 bytes off a 16-byte boundary, the others plain: the assertions of
    test_one_operand_skewed (within the row's tolerance of the float64 reference; equal to the aligned call wherever the row says so)
    and intact zones — the scalar fall-back kernels have tile edges of their own"""
    e, r = env, ROWS[name]
    base = aligned(e, name)
    b = built(e, name)
    failed = []
    for operand, cls in r.cls.items():
        if cls not in ("S", "F"):
            continue
        for fill in fills_of(b):
            what = f"{operand} guarded + 4 B, integer fill {fill}"
            rc, outs, zones, changed = run_guarded(e, name, {operand}, 1, fill)
            assert list(zones) == [operand]
            lines = verdict(name, base, rc, outs, zones, changed, r.exact)
            if not lines:
                check_ok(e, name, outs, what)
                check(zones[operand], f"{name} [{what}] `{operand}`")
            failed += [f"[{what}] {line}" for line in lines]
    assert not failed, f"{name}:\n  " + "\n  ".join(failed)


# ======================================================================================================================
# cases through hilcodec_amd.ops: (operands {name: CPU tensor}, written operand names, fn(ops, t) -> {returned: tensor}, expected)
# — the form of the alignment sweep's `_misc_cases`.  None of these wrappers copies an aligned contiguous operand (ops.py: each hands
# `_ptr(t)` to the C ABI), so the guarded views are what the kernels get.
# ======================================================================================================================
def run_case(e, case, guard=(), fill=0):
    """`guard`: None = every operand of the case's dict (written ones included), else the names to guard.
    -> ({returned or written: CPU tensor}, {operand: zone})"""
    t0, writes, fn, _ = case
    t, zones = {}, {}
    for o, v in t0.items():
        d = v.clone().to(e.dev)
        if guard is None or o in guard:
            t[o], zones[o] = guarded(d, 0, fill)
            assert t[o].data_ptr() % 16 == 0
        else:
            t[o] = d
    got = dict(fn(e.ops, t))
    torch.cuda.synchronize()
    for o, v in t0.items():
        if o not in writes:
            assert torch.equal(t[o].cpu(), v), f"the call changed its input `{o}`"
    got.update({o: t[o] for o in writes})
    return {o: v.cpu() for o, v in got.items()}, zones


def _same(got, want):
    return got.dtype == want.dtype and torch.equal(got, want)


def case_fills(case):
    return INT_FILLS if any(not v.is_floating_point() for v in case[0].values()) else (0,)


def check_case(e, label, case, base=None):
    """the unguarded call equals the host model; the all-guarded call equals the unguarded one, zones intact.  On a failure the call is
    repeated with one operand guarded at a time to name the operands whose surroundings reach an output."""
    expected = case[3]
    if base is None:
        base, _ = run_case(e, case)
    assert set(base) == set(expected), (label, sorted(base), sorted(expected))
    for o, want in expected.items():
        assert base[o].dtype == want.dtype and base[o].shape == want.shape and torch.equal(base[o], want), f"{label}: `{o}` differs from the host model"
    for fill in case_fills(case):
        got, zones = run_case(e, case, None, fill)
        lines = [f"`{o}`: {d}" for o, d in ((o, _differs(got[o], base[o])) for o in base) if d]
        for o, z in zones.items():
            lines += [f"red zone of `{o}`: {d}" for d in damage(z)]
        if lines:
            for o in case[0]:
                one, _ = run_case(e, case, {o}, fill)
                hit = [u for u in base if not torch.equal(one[u], base[u])]
                if hit:
                    lines.append(f"with only `{o}` guarded: {', '.join('`' + u + '`' for u in hit)} differ")
            raise AssertionError(f"{label} [all operands guarded, integer fill {fill}]:\n  " + "\n  ".join(lines))


# ---- the per-slot float kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(slot_cases.MISC))
def test_per_slot_float_kernels(env, name):
    base, _ = slot_cases.misc_run(env, name)                      # the unguarded baseline the alignment sweep pins to the host model
    case = slot_cases.CASES[name]
    assert set(case[0]) == set(slot_cases.MISC[name])
    check_case(env, name, case, base)


def _slots_cases():
    """the state-slot copies through `hilcodec_amd.ops` on a layout in which no length is a multiple of 4: slices of 1, 3 and 5 floats
    per stream, the last slot loaded from the last record.  `StateLayout` starts every slice on a 16-byte boundary (offsets 0, 8, 24),
    so through `ops` the first stream's piece of each slice is aligned and only the others are not; the layout in which EVERY piece is
    off a boundary needs offset tables made by hand: `_raw_slots_cases`"""
    from hilcodec_amd.ops import StateLayout
    g = torch.Generator().manual_seed(5)
    B = 5
    layout = StateLayout([(B, 1, 1), (B, 1, 3), (B, 5, 1)], 1)
    assert layout.lens == [1, 3, 5] and layout.off == [0, 8, 24] and layout.total == 52 and layout.record_len == 9
    block = torch.randn(layout.total, generator=g)
    records = torch.randn(3, layout.record_len, generator=g)
    action = torch.tensor([2, -1, 0, 1, 3], dtype=torch.int32)

    def part(k, b):
        return slice(layout.off[k] + b * layout.lens[k], layout.off[k] + (b + 1) * layout.lens[k])
    rec_off = [sum(layout.lens[:k]) for k in range(len(layout.lens))]
    want = block.clone()
    for k in range(len(layout.lens)):
        for b, a in enumerate(action.tolist()):
            if a == -1:
                want[part(k, b)] = 0
            elif a >= 1:
                want[part(k, b)] = records[a - 1, rec_off[k]: rec_off[k] + layout.lens[k]]
    cases = {"state_slots_apply": ({"block": block, "action": action, "records": records}, ("block",),
                                   lambda ops, t: ops.state_slots_apply(t["block"], layout, t["action"], t["records"]) or {}, {"block": want})}
    slots = torch.tensor([4, 0, 2, 4], dtype=torch.int32)
    rec = torch.stack([torch.cat([block[part(k, b)] for k in range(len(layout.lens))]) for b in slots.tolist()])
    cases["state_slots_gather"] = ({"block": block, "slots": slots}, (), lambda ops, t: {"records": ops.state_slots_gather(t["block"], layout, t["slots"])},
                                   {"records": rec})
    dst = torch.randn(layout.total, generator=g)
    hold = torch.tensor([1, 0, 0, 2, 1], dtype=torch.int32)
    want = dst.clone()
    for k in range(len(layout.lens)):
        for b, h in enumerate(hold.tolist()):
            if h:
                want[part(k, b)] = block[part(k, b)]
    wav = torch.randn(B, 1, 37, generator=g)
    want_wav = wav.clone()
    want_wav[hold != 0] = 0
    cases["state_slots_hold"] = ({"src": block, "dst": dst, "hold": hold, "wav": wav}, ("dst", "wav"),
                                 lambda ops, t: ops.state_slots_hold(t["src"], t["dst"], layout, t["hold"], wav=t["wav"]) or {},
                                 {"dst": want, "wav": want_wav})
    return cases


def _raw_slots_cases():
    """slices of 1, 3 and 5 floats at hand-made offsets 1, 7 and 17 for 3 streams: the pieces start at floats 1, 2, 3 / 7, 10, 13 / 17,
    22, 27 — none on a 16-byte boundary (with four streams or more an odd length always puts one piece on one, so 3 it is).  The
    registered ops take the offset and length tables as tensors (what `StateLayout.tables` hands them), so the tables are operands of
    the case and guarded too; the last slot is loaded from the last record"""
    H = torch.ops.hilcodec
    g = torch.Generator().manual_seed(6)
    B, off, lens, total, rlen = 3, [1, 7, 17], [1, 3, 5], 32, 9
    assert all((o + b * n) % 4 for o, n in zip(off, lens) for b in range(B)) and off[2] + B * lens[2] == total
    tables = {"slice_off": torch.tensor(off, dtype=torch.int64), "slice_len": torch.tensor(lens, dtype=torch.int32)}
    block = torch.randn(total, generator=g)
    records = torch.randn(2, rlen, generator=g)
    action = torch.tensor([1, -1, 2], dtype=torch.int32)

    def part(k, b):
        return slice(off[k] + b * lens[k], off[k] + (b + 1) * lens[k])
    rec_off = [0, 1, 4]
    want = block.clone()
    for k in range(3):
        for b, a in enumerate(action.tolist()):
            want[part(k, b)] = 0 if a == -1 else records[a - 1, rec_off[k]: rec_off[k] + lens[k]]
    cases = {"state_slots_apply": (dict(tables, block=block, action=action, records=records), ("block",),
                                   lambda ops, t: H.state_slots_apply(t["block"], t["slice_off"], t["slice_len"], t["action"], t["records"]) or {},
                                   {"block": want})}
    slots = torch.tensor([2, 0, 2], dtype=torch.int32)
    rec = torch.stack([torch.cat([block[part(k, b)] for k in range(3)]) for b in slots.tolist()])
    cases["state_slots_gather"] = (dict(tables, block=block, slots=slots), (),
                                   lambda ops, t: {"records": H.state_slots_gather(t["block"], t["slice_off"], t["slice_len"], t["slots"], B, rlen)},
                                   {"records": rec})
    dst = torch.randn(total, generator=g)
    hold = torch.tensor([1, 0, 2], dtype=torch.int32)
    want = dst.clone()
    for k in range(3):
        for b, h in enumerate(hold.tolist()):
            if h:
                want[part(k, b)] = block[part(k, b)]
    wav = torch.randn(B, 1, 37, generator=g)
    want_wav = wav.clone()
    want_wav[hold != 0] = 0
    cases["state_slots_hold"] = (dict(tables, src=block, dst=dst, hold=hold, wav=wav), ("dst", "wav"),
                                 lambda ops, t: H.state_slots_hold(t["src"], t["dst"], t["slice_off"], t["slice_len"], t["hold"], t["wav"], None, None,
                                                                   None) or {},
                                 {"dst": want, "wav": want_wav})
    return cases


@pytest.mark.parametrize("name", ["state_slots_apply", "state_slots_gather", "state_slots_hold"])
def test_state_slots_on_an_odd_layout(env, name):
    check_case(env, f"{name} [slices of 1, 3, 5 floats]", _slots_cases()[name])


@pytest.mark.parametrize("name", ["state_slots_apply", "state_slots_gather", "state_slots_hold"])
def test_state_slots_with_every_piece_off_a_boundary(env, name):
    check_case(env, f"{name} [slices of 1, 3, 5 floats at offsets 1, 7, 17]", _raw_slots_cases()[name])


@pytest.mark.parametrize("B,T", [(2, 43), (17, 5)], ids=["Tout-65", "B-17"])
def test_resample_poly_edges(env, B, T):
    """16 -> 24 kHz (L = 3, M = 2).  T = 43: 65 outputs per stream, one more than a round of 64; B = 17: one stream more than the 16 of a
    workgroup"""
    from hilcodec_amd.resample import design, device_taps, reference
    sp = design(16000, 24000)
    g = torch.Generator().manual_seed(B * 100 + T)
    t = {"x": torch.rand(B, 1, T, generator=g) * 2 - 1, "hist": torch.randn(B, 1, sp.Q - 1, generator=g) * 0.5,
         "hist_out": torch.full((B, 1, sp.Q - 1), SENT), "taps": device_taps(sp, env.dev).cpu()}
    y, h = reference(t["x"], sp, t["hist"])
    assert y.shape[2] == (T * sp.L + sp.M - 1) // sp.M and (T != 43 or y.shape[2] == 65)
    case = (t, ("hist_out",), lambda ops, t: {"y": ops.resample_poly(t["x"], t["taps"], sp.L, sp.M, hist=t["hist"], hist_out=t["hist_out"])},
            {"y": y, "hist_out": h})
    check_case(env, f"resample_poly [B = {B}, T = {T}]", case)


# ---- the kernels that move variable-length byte rows: B = 65 (one slot more than a workgroup of 64), the last slot carries the
# longest row; caller-owned outputs wherever the wrapper takes them (what a wrapper allocates itself cannot be guarded) --------------------
# (tests/redzone.py names them for the ledger: `BYTE_ENTRY_POINTS`, `MORE_ENTRY_POINTS`)
NB = 65
# byte counts of the SRTP rows (tests/hops.py, `SRTP_LENGTHS`): nothing, no header, a bare header, one below / at / above the AES
# block edges (payloads of 16, 32, 48 bytes: 19, 35, 51) and the SHA-1 padding edges (51, 52, 59, 60), the whole row
SRTP_LENGTHS = (0, 2, 3, 13, 18, 19, 20, 34, 35, 36, 50, 51, 52, 53, 58, 59, 60, 61, 80)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8)))


def _ragged_codes(n, T, seed):
    """stage-major codes [n, NB, T] with per-stream stage counts spanning 1..n, the last slot all n; rows past a stream's own are -1"""
    g = torch.Generator().manual_seed(seed)
    n_list = [1 + (b % n) for b in range(NB - 1)] + [n]
    idx = torch.randint(0, 1024, (n, NB, T), generator=g)
    for b, nb in enumerate(n_list):
        idx[nb:, b] = -1
    return idx, n_list


def _host_packets(idx, n_list):
    from hilcodec_amd import wire
    n, B, T = idx.shape
    out = torch.zeros(B, wire.packet_bytes(n, T), dtype=torch.uint8)
    for b in range(B):
        blob = wire.pack_stream_packet(idx[:n_list[b], b])
        out[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    return out, torch.tensor([wire.packet_bytes(nb, T) for nb in n_list], dtype=torch.int32)


# rows of 20 bytes (whole words) and of 27 (not)
@pytest.mark.parametrize("n,T", [(8, 2), (7, 3)], ids=["20-bytes", "27-bytes"])
def test_pack_codes_10bit(env, n, T):
    idx, n_list = _ragged_codes(n, T, 3)
    packets, nbytes = _host_packets(idx, n_list)
    assert packets.shape[1] == {2: 20, 3: 27}[T] and int(nbytes[-1]) == packets.shape[1] and int(nbytes.min()) == (10 * T + 7) // 8

    def fn(ops, t):
        p, nb = ops.pack_codes_10bit(t["indices"], t["n_clip"])
        return {"packets": p, "nbytes": nb}
    check_case(env, f"pack_codes_10bit [n = {n}, T = {T}]", ({"indices": idx, "n_clip": _i32(n_list)}, (), fn, {"packets": packets, "nbytes": nbytes}))


@pytest.mark.parametrize("n,m,T", [(6, 2, 2), (8, 3, 1)], ids=["20-bytes", "14-bytes"])
def test_pack_codes_10bit_fec(env, n, m, T):
    g = torch.Generator().manual_seed(n + m)
    W = 1 + m * T
    idx = torch.randint(-2, 1100, (n, NB, T), generator=g)
    n_slot = torch.tensor([b % (n + 2) for b in range(NB - 1)] + [n], dtype=torch.int32)
    prev_in = torch.randint(0, 2048, (NB, W), generator=g, dtype=torch.int32)
    prev_in[:, 0] = torch.randint(0, 3, (NB,), generator=g)
    action = torch.randint(-1, 3, (NB,), generator=g, dtype=torch.int32) * (torch.randint(0, 4, (NB,), generator=g) == 0)
    hold = (torch.randint(0, 5, (NB,), generator=g) == 0).to(torch.int32)
    prev_in[-1, 0], action[-1], hold[-1] = 1, 0, 0                             # the last slot: all n stages and the redundant section
    packets, nbytes, prev_out = pack_model(idx, n_slot, prev_in, action, hold, m)
    assert int(nbytes[-1]) == packets.shape[1] and int(nbytes.min()) == 0
    t = {"indices": idx, "n_clip": n_slot, "prev_in": prev_in, "prev_out": torch.full((NB, W), 77, dtype=torch.int32), "action": action, "hold": hold}

    def fn(ops, t):
        p, nb = ops.pack_codes_10bit_fec(t["indices"], t["prev_in"], t["prev_out"], m, t["n_clip"], t["action"], t["hold"])
        return {"packets": p, "nbytes": nb}
    check_case(env, f"pack_codes_10bit_fec [n = {n}, m = {m}, T = {T}]", (t, ("prev_out",), fn, {"packets": packets, "nbytes": nbytes, "prev_out": prev_out}))


@pytest.mark.parametrize("n,m,T", [(6, 2, 2), (8, 3, 1)], ids=["20-to-15-bytes", "14-to-10-bytes"])
def test_fec_select(env, n, m, T):
    """the FEC receiver's compaction against the host model of tests/hops.py: wide rows with every bit set at random, the redundant
    section taken in a third of the slots and in the last one"""
    from hilcodec_amd import wire
    g = torch.Generator().manual_seed(10 * n + m)
    wide = torch.randint(0, 256, (NB, wire.fec_packet_bytes(n, m, T)), generator=g, dtype=torch.uint8)
    fec = torch.tensor([int(b % 3 == 0) * (1 + b % 2) for b in range(NB - 1)] + [1], dtype=torch.int32)
    n_slot = torch.tensor([b % (n + 4) - 1 for b in range(NB - 1)] + [n], dtype=torch.int32)          # garbage at both ends: clamped
    out, n_out = select_model(wide, fec, n_slot, n, m, T)
    case = ({"packets": wide, "fec": fec, "n_slot": n_slot}, ("n_slot",),
            lambda ops, t: {"rows": ops.fec_select(t["packets"], t["fec"], t["n_slot"], n, m, T)}, {"rows": out, "n_slot": n_out})
    check_case(env, f"fec_select [n = {n}, m = {m}, T = {T}]", case)


@pytest.mark.parametrize("n,T", [(8, 2), (7, 3)], ids=["20-bytes", "27-bytes"])
def test_conceal_prepare(env, n, T):
    """the receiver's concealment step against the host model of its table in tests/hops.py: received, lost (with and without
    something to repeat, at every run length) and held slots, starts; the last slot is lost and gets the longest substitute packet"""
    g = torch.Generator().manual_seed(n + T)
    idx, n_list = _ragged_codes(n, T, 21)
    packets, _ = _host_packets(idx, n_list)
    state = torch.zeros(NB, n + 3, dtype=torch.int32)
    state[:, 0] = torch.randint(0, F + 2, (NB,), generator=g)
    state[:, 1] = torch.randint(0, 2, (NB,), generator=g)
    state[:, 2] = torch.randint(0, n + 1, (NB,), generator=g)
    state[:, 3:] = torch.randint(0, 2048, (NB, n), generator=g)
    kind = torch.tensor([b % 8 for b in range(NB)])
    hold, lost = (kind == 0).to(torch.int32), ((kind >= 1) & (kind <= 4)).to(torch.int32)
    action = torch.tensor([(-1, 1)[b % 2] * int(b % 6 == 5) for b in range(NB)], dtype=torch.int32)
    state[-1, :3] = torch.tensor([1, 1, n], dtype=torch.int32)
    hold[-1], lost[-1], action[-1] = 0, 1, 0
    n_slot = torch.tensor(n_list, dtype=torch.int32)
    n_slot[lost.bool() | hold.bool()] = n
    e_state, e_hold, e_n, e_packets, e_ramp = prepare_model(state, action, hold, lost, n_slot, packets, T, F)
    assert int(e_ramp[-1]) == 2 and int(e_n[-1]) == n and (e_hold != hold).any()
    t = {"state": state, "action": action, "hold": hold, "lost": lost, "n_slot": n_slot, "packets": packets}
    case = (t, ("state", "hold", "n_slot", "packets"),
            lambda ops, t: {"ramp": ops.conceal_prepare(t["state"], t["action"], t["hold"], t["lost"], t["n_slot"], t["packets"], T, F)},
            {"state": e_state, "hold": e_hold, "n_slot": e_n, "packets": e_packets, "ramp": e_ramp})
    check_case(env, f"conceal_prepare [n = {n}, T = {T}]", case)


@pytest.mark.parametrize("n,T,C", [(8, 2, 128), (7, 3, 32)], ids=["20-bytes", "27-bytes"])
def test_rvq_decode_packed(env, n, T, C):
    """the packed dequantiser: the float32 sum of the code vectors in stage order, one rounding per addition (csrc/packets.hip) — the
    same chain in torch on the CPU, so the comparison is exact.  130 / 195 frames: a ragged last workgroup of 2 / 8 frames"""
    idx, n_list = _ragged_codes(n, T, 9)
    packets, _ = _host_packets(idx, n_list)
    cb = rnd(5, n, 1024, C) * 0.3
    q = torch.zeros(NB, T, C)
    for b, nb in enumerate(n_list):
        for s in range(nb):
            q[b] = q[b] + cb[s][idx[s, b]]
    case = ({"packets": packets, "n_clip": _i32(n_list), "codebooks": cb}, (),
            lambda ops, t: {"q": ops.rvq_decode_packed(t["packets"], t["codebooks"], n, T, n_clip=t["n_clip"])}, {"q": q})
    check_case(env, f"rvq_decode_packed [n = {n}, T = {T}, C = {C}]", case)


@pytest.mark.parametrize("T,m,dtx_on", [(2, 2, False), (1, 2, True)], ids=["25-to-28-bytes", "13-to-16-bytes-dtx"])
def test_packet_header(env, T, m, dtx_on):
    from hilcodec_amd import dtx, wire
    B, n = NB, 8
    rng = np.random.default_rng(10 * T + m)
    stride = wire.packet_bytes(n + m, T)
    n_b = np.array([max(m, 1) + b % (n + 1 - max(m, 1)) for b in range(B - 1)] + [n])
    kind = rng.integers(0, 4, B) if dtx_on else np.ones(B, dtype=np.int64)
    hold = (kind == dtx.HELD).astype(np.int32) if dtx_on else (rng.random(B) < 0.1).astype(np.int32)
    action = (rng.random(B) < 0.15).astype(np.int32)
    kind[-1], hold[-1] = dtx.SPEECH, 0
    ctr = rng.integers(0, 65536, B).astype(np.int32)
    ctr[:4] = [65535, 0, 65534, 1]
    packets = np.zeros((B, stride), dtype=np.uint8)
    nbytes = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if hold[b] or kind[b] == dtx.SILENT:
            continue
        if kind[b] == dtx.SID:
            L = dtx.sid_bytes(8)
        else:
            L = wire.fec_packet_bytes(n_b[b], m, T) if b == B - 1 or b % 3 else wire.packet_bytes(n_b[b], T)
        packets[b, :L] = rng.integers(0, 256, L)
        nbytes[b] = L
    assert nbytes[-1] == stride and (nbytes == 0).any()
    want = np.zeros((B, wire.transport_bytes(n, m, T)), dtype=np.uint8)
    want_cnt, want_ctr = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        c = 0 if action[b] else int(ctr[b])
        want_ctr[b] = c if hold[b] else (c + 1) & 0xFFFF
        if hold[b] or nbytes[b] == 0:
            continue
        if kind[b] == dtx.SID:
            pkt = wire.pack_transport(c, packets[b, :nbytes[b]].tobytes(), 0, sid=True)
        else:
            pkt = wire.pack_transport(c, packets[b, :nbytes[b]].tobytes(), int(n_b[b]), fec=wire.fec_present(int(nbytes[b]), int(n_b[b]), m, T))
        want[b, :len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
        want_cnt[b] = len(pkt)
    assert want_cnt[-1] == want.shape[1]
    t = {"packets": _u8(packets), "nbytes": _i32(nbytes), "n_clip": _i32(n_b), "action": _i32(action), "hold": _i32(hold), "ctr_in": _i32(ctr),
         "ctr_out": torch.full((B,), -7, dtype=torch.int32)}
    if dtx_on:
        t["kind"] = _i32(kind)

    def fn(ops, t):
        out, cnt = ops.packet_header(t["packets"], t["nbytes"], t["ctr_in"], t["ctr_out"], n, m, T, n_clip=t["n_clip"], kind=t.get("kind"),
                                     action=t["action"], hold=t["hold"])
        return {"rows": out, "counts": cnt}
    check_case(env, f"packet_header [T = {T}, m = {m}]", (t, ("ctr_out",), fn, {"rows": _u8(want), "counts": _i32(want_cnt), "ctr_out": _i32(want_ctr)}))


@pytest.mark.parametrize("n,m,K,T,conceal,D,C", [(8, 2, 8, 2, True, 1, 4), (8, 3, 4, 1, False, 0, 2)], ids=["25-byte-rows", "14-byte-rows"])
def test_jitter_step(env, n, m, K, T, conceal, D, C):
    """three hops against jitter.JitterModel on plain tensors, then the fourth from the same state inside red zones.  Every hop each slot
    gets its sender's packet (stage counts spanning m..n, with and without the redundant section, SIDs), some a truncated or an empty
    record besides; the last slot's packet fills the whole row and its record is the last one"""
    from hilcodec_amd import dtx, forward, jitter, wire
    from hilcodec_amd.jitter import JitterConfig, JitterModel
    B = NB
    model = JitterModel(B, JitterConfig(depth=D, capacity=C), n, m, T, K, conceal)
    rng = np.random.default_rng(n + m + T)
    stride, tbytes = wire.packet_bytes(n + m, T), wire.transport_bytes(n, m, T)
    dev = env.dev
    state = torch.zeros(B, jitter.ST_WORDS, dtype=torch.int32, device=dev)
    meta = torch.zeros(B, C, dtype=torch.int32, device=dev)
    ring = torch.zeros(B, C, (stride + 3) // 4, dtype=torch.int32, device=dev)

    def hop(h):
        arrived = []
        for b in range(B):
            if b % 11 == 3 and h != 1:
                continue                                                      # lost
            if b % 7 == 5:
                body, nb, sid, fec = rng.integers(0, 256, dtx.sid_bytes(K)).astype(np.uint8).tobytes(), 0, True, False
            else:
                nb = n if b == B - 1 else max(m, 1) + (b + h) % (n + 1 - max(m, 1))
                fec = b == B - 1 or b % 2 == 0
                codes = torch.from_numpy(rng.integers(0, 1024, (nb + (m if fec else 0), T)))
                body, sid = wire.pack_stream_packet(codes), False
            p = wire.pack_transport((65534 + h) & 0xFFFF if b < 8 else h, body, nb, sid=sid, fec=fec)
            if b % 13 == 1:
                arrived.append((b, p, 0))                                     # an empty record
            if b % 13 == 2:
                arrived.append((b, p, 3))                                     # a bare header
            if b % 13 == 4:
                arrived.append((b, p, len(p) - 1))                            # one byte short
            arrived.append((b, p, len(p)))
        assert arrived[-1][0] == B - 1 and arrived[-1][2] == tbytes
        packets = np.zeros((len(arrived), tbytes), dtype=np.uint8)
        for a, (_, p, _) in enumerate(arrived):
            packets[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        slots, counts = [s for s, _, _ in arrived], [c for _, _, c in arrived]
        action = (np.arange(B) % 17 == 6).astype(np.int32) * (h == 2)
        hold = (np.arange(B) % 19 == 7).astype(np.int32)
        rec, offs = forward.arrival_records(slots, packets, counts, tbytes, B, len(arrived))
        return action, hold, slots, packets, counts, rec, offs

    def fn(ops, t):
        ops.jitter_step(t["arrivals"], t["offsets"], t["hold"], t["n_slot"], t["packets"], t["state"], t["meta"], t["ring"], n, m, T, K, D,
                        action=t["action"], lost=t.get("lost"), fec=t["fec"])
        return {}
    writes = ("hold", "n_slot", "packets", "state", "meta", "ring", "fec") + (("lost",) if conceal else ())
    for h in range(4):
        action, hold, slots, packets, counts, rec, offs = hop(h)
        t = {"arrivals": torch.from_numpy(rec), "offsets": torch.from_numpy(offs), "action": _i32(action), "hold": _i32(hold),
             "n_slot": torch.full((B,), -9, dtype=torch.int32), "fec": torch.full((B,), -9, dtype=torch.int32),
             "packets": torch.full((B, stride), 0xEE, dtype=torch.uint8), "state": state.cpu(), "meta": meta.cpu(), "ring": ring.cpu()}
        if conceal:
            t["lost"] = torch.full((B,), -9, dtype=torch.int32)
        want = model.step(action, hold, slots, packets, counts)
        case = (t, writes, fn, None)
        got, _ = run_case(env, case)
        expected = {"hold": _i32(want["hold"]), "n_slot": _i32(want["n"]), "fec": _i32(want["fec"]), "packets": _u8(want["packets"]),
                    "state": _i32(model.state), "meta": _i32(model.meta), "ring": got["ring"]}           # the model keeps no ring: the plain call's
        if conceal:
            expected["lost"] = _i32(want["lost"])
        if h == 3:
            check_case(env, f"jitter_step [stride {stride}]", (t, writes, fn, expected), got)
        for o, w in expected.items():
            assert _same(got[o], w), (h, o)
        state, meta, ring = got["state"].to(dev), got["meta"].to(dev), got["ring"].to(dev)
    st = model.state
    assert st[:, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index("decoded")].sum() > 0
    assert st[:, jitter.STAT_ACCEPTED + jitter.STAT_NAMES.index("malformed")].sum() > 0


def _keyed(model, rng, unkeyed):
    for b in range(model.B):
        if b not in unkeyed:
            model.keys.set_key(b, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes(),
                               ssrc=int(rng.integers(0, 1 << 32)), roc=int(b % 3 == 0) * 0x01020304)


def _srtp_rows(rng, B, tb, seq):
    """headed rows of every length of SRTP_LENGTHS in turn (cut to the row), the last slot the whole row; garbage past the byte count"""
    packets = rng.integers(0, 256, (B, tb), dtype=np.uint8)
    nbytes = np.array([min(SRTP_LENGTHS[b % len(SRTP_LENGTHS)], tb) for b in range(B - 1)] + [tb], dtype=np.int32)
    packets[:, 0], packets[:, 1] = seq >> 8, seq & 255
    return packets, nbytes


# 80: rows and protected rows (90 bytes) ... word path in, byte path out; 78: byte path in, word path out (88); 41: bytes both ways
@pytest.mark.parametrize("tb", [80, 41, 78])
def test_srtp_protect(env, tb):
    from hilcodec_amd import srtp
    B = NB
    model = srtp.SenderModel(B, tb)
    rng = np.random.default_rng(11 + tb)
    _keyed(model, rng, (5, 33))
    model.protect(np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32))     # the keys' ROCs
    model.state[:, srtp.TX_LAST], model.state[:, srtp.TX_SENT] = 0xFFFE, 1
    packets, nbytes = _srtp_rows(rng, B, tb, np.full(B, 0xFFFF, dtype=np.int64))
    action = (np.arange(B) % 9 == 4).astype(np.int32)
    t = {"packets": _u8(packets), "nbytes": _i32(nbytes), "keys": _i32(model.keys.rows), "rows": _i32(model.state.copy()),
         "out": torch.full((B, tb + 10), 0xAB, dtype=torch.uint8), "out_nbytes": torch.full((B,), -9, dtype=torch.int32), "action": _i32(action)}
    want = model.protect(packets, nbytes, action)
    assert want["nbytes"][-1] == tb + 10 and set(nbytes.tolist()) >= set(min(v, tb) for v in SRTP_LENGTHS)

    def fn(ops, t):
        ops.srtp_protect(t["packets"], t["nbytes"], t["keys"], t["rows"], out=t["out"], out_nbytes=t["out_nbytes"], action=t["action"])
        return {}
    case = (t, ("rows", "out", "out_nbytes"), fn,
            {"rows": _i32(model.state), "out": _u8(want["packets"]), "out_nbytes": _i32(want["nbytes"])})
    check_case(env, f"srtp_protect [row_bytes = {tb}]", case)


@pytest.mark.parametrize("tb", [80, 41, 78])
def test_srtp_unprotect(env, tb):
    """one hop of arrivals against srtp.ReceiverModel: per slot the genuine packet of its length, for some a forgery (a flipped bit), a
    truncation or a duplicate in front of it; `plain` has exactly one record per arrival, so the last slot's — the whole row — is the
    last record of both buffers"""
    from hilcodec_amd import forward, srtp
    B = NB
    tx, model = srtp.SenderModel(B, tb), srtp.ReceiverModel(B, tb)
    _keyed(tx, np.random.default_rng(3), (5, 33))
    _keyed(model, np.random.default_rng(3), (5, 33))
    rng = np.random.default_rng(100 + tb)
    start = np.ones(B, dtype=np.int32)
    tx.protect(np.zeros((B, tb), dtype=np.uint8), np.zeros(B, dtype=np.int32), start)
    tx.state[:, srtp.TX_LAST], tx.state[:, srtp.TX_SENT] = 0xFFFE, 1
    model.start(start)
    model.state[::2, srtp.RX_SL], model.state[::2, srtp.RX_SEEN] = 0xFFFE, 1
    packets, nbytes = _srtp_rows(rng, B, tb, np.full(B, 0xFFFF, dtype=np.int64))
    out = tx.protect(packets, nbytes)
    arrived = []
    for b in range(B):
        L = int(out["nbytes"][b])
        p = out["packets"][b, :L].tobytes() if L else bytes(out["packets"][b, :int(nbytes[b])])
        if L and b % 5 == 1:
            bit = int(rng.integers(0, 8 * L))
            arrived.append((b, p[:bit >> 3] + bytes([p[bit >> 3] ^ (1 << (bit & 7))]) + p[(bit >> 3) + 1:]))
        if L and b % 5 == 2:
            arrived.append((b, p[:int(rng.integers(0, L))]))
        if L and b % 5 == 3:
            arrived.append((b, p))
        arrived.append((b, p))
    assert arrived[-1][0] == B - 1 and len(arrived[-1][1]) == tb + 10
    data = np.zeros((len(arrived), tb + 10), dtype=np.uint8)
    for a, (_, p) in enumerate(arrived):
        data[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    rec, offs = forward.arrival_records([s for s, _ in arrived], data, [len(p) for _, p in arrived], tb + 10, B, len(arrived))
    action = (np.arange(B) % 9 == 4).astype(np.int32)
    t = {"arrivals": torch.from_numpy(rec), "offsets": torch.from_numpy(offs), "keys": _i32(model.keys.rows), "rows": _i32(model.state.copy()),
         "plain": torch.full((len(arrived), 1 + (tb + 3) // 4), -7, dtype=torch.int32), "action": _i32(action)}
    want = model.unprotect(rec, offs, action)
    assert want.shape == t["plain"].shape and want[-1, 0] == tb and model.state[:, srtp.RX_OK].sum() > B // 2

    def fn(ops, t):
        ops.srtp_unprotect(t["arrivals"], t["offsets"], t["keys"], t["rows"], tb, plain=t["plain"], action=t["action"])
        return {}
    case = (t, ("rows", "plain"), fn,
            {"rows": _i32(model.state), "plain": torch.from_numpy(np.ascontiguousarray(want))})
    check_case(env, f"srtp_unprotect [row_bytes = {tb}]", case)


@pytest.mark.parametrize("tb", [80, 41, 78])
def test_srtp_protect_routes(env, tb):
    """one hop of 65 listeners x 2 routes x 2 rows against forward_srtp.RouteModel (260 rows: the last workgroup is partial); the last
    row of the last route of the last listener is the whole row"""
    from hilcodec_amd import forward_srtp
    from hilcodec_amd.forward_srtp import RT_SEEN, RT_SL
    B, F, P = NB, 2, 2
    rng = np.random.default_rng(1000 + tb)
    model = forward_srtp.RouteModel(B, F, P, tb)
    for b in range(B):
        if b not in (1, 33):
            model.keys.set_key(b, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes(),
                               ssrc=int(rng.integers(0, 1 << 32)))
    model.state[:, :, RT_SL], model.state[:, :, RT_SEEN] = 0xFFFE, 1
    rows = rng.integers(0, 256, (B, F, P, tb), dtype=np.uint8)
    lengths = [min(v, tb) for v in SRTP_LENGTHS]
    nbytes = np.array([lengths[i % len(lengths)] for i in range(B * F * P)], dtype=np.int32).reshape(B, F, P)
    nbytes[-1, -1, -1] = tb
    seq = 0xFFFF + np.arange(P)[None, None, :] + np.zeros((B, F, 1), dtype=np.int64)
    rows[..., 0], rows[..., 1] = (seq >> 8) & 255, seq & 255
    routes = rng.integers(-1, B, (B, F)).astype(np.int32)
    routes[-1, -1] = 7
    new_routes = (rng.random((B, F)) < 0.08).astype(np.int32)
    flags = [(np.arange(B) % m == 2).astype(np.int32) for m in (9, 13, 17)]
    t = {"rows": _u8(rows), "nbytes": _i32(nbytes), "routes": _i32(routes), "new_routes": _i32(new_routes), "keys": _i32(model.keys.rows),
         "route_rows": _i32(model.state.copy()), "out": torch.full((B, F, P, tb + 10), 0xAB, dtype=torch.uint8),
         "out_nbytes": torch.full((B, F, P), -9, dtype=torch.int32), "action": _i32(flags[0]), "rekey_up": _i32(flags[1]), "rekey_down": _i32(flags[2])}
    want = model.protect(rows, nbytes, routes, new_routes, *flags)
    assert want["out_nbytes"][-1, -1, -1] == tb + 10

    def fn(ops, t):
        ops.srtp_protect_routes(t["rows"], t["nbytes"], t["routes"], t["new_routes"], t["keys"], t["route_rows"], out=t["out"],
                                out_nbytes=t["out_nbytes"], action=t["action"], rekey_up=t["rekey_up"], rekey_down=t["rekey_down"])
        return {}
    check_case(env, f"srtp_protect_routes [row_bytes = {tb}]",
               (t, ("route_rows", "out", "out_nbytes"), fn,
                {"route_rows": _i32(model.state), "out": _u8(want["out"]), "out_nbytes": _i32(want["out_nbytes"])}))
