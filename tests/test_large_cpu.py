"""The large-tensor tests' own machinery, on the CPU (tests/large.py, tests/large_families.py; the GPU side is tests/test_gpu_large.py).

  * every row's builder at a small size with its float32 reference as the "kernel": the whole-tensor compare passes, and fails for
    each of three injected faults — an offset that wraps modulo 2^k elements, a clip base taken from another clip, a row read from
    its neighbour; the (P, k) pairs of the GPU rows are listed and their visibility asserted;
  * the boundary arithmetic of every row: "below" < 2^32 <= "at", both legal, one legal step apart, the memory estimate under its cap;
  * the guards at one below, at and one above 2^32: the `hilcodec_amd.ops` mirrors against the C entry points;
  * the model's receptive field on a four-period clip through the oracle."""
import ctypes
import types

import pytest
import torch

from hilcodec_amd import synth
from tests import large as L
from tests import large_families as G
from tests.entry_rows import ROWS, cast


class _Lib:
    """queries answer from the real library (no launch); an entry point is never called here"""

    def __getattr__(self, name):
        from hilcodec_amd._lib import lib
        assert name.endswith("_supported") or name == "hilc_dws_conv_wave_row", f"{name}: only shape queries run without a GPU"
        return getattr(lib, name)


class _Ops:
    """`hilcodec_amd.ops` with the layout-only device functions replaced by stand-ins: the reference never reads a packed table"""

    def __getattr__(self, name):
        from hilcodec_amd import ops
        return getattr(ops, name)

    resblock_pack = staticmethod(lambda w: w)
    resblock_chain_pack = staticmethod(lambda w, streaming=True: w)
    spec_block_tables = staticmethod(lambda bt, wt, n: (bt, bt[:, 0].contiguous(), wt))


@pytest.fixture(scope="module")
def cpu_env():
    from hilcodec_amd import fold
    return types.SimpleNamespace(ops=_Ops(), fold=fold, lib=_Lib(), L=None, dev=torch.device("cpu"), stream=lambda: None)


def small(c):
    """the row at a size the CPU takes: five clips (two patterns twice), five periods and a ragged rest — one hop for a streaming form"""
    d = dict(c.sizes["below"], B=5)
    if c.stream_guard is None:
        d["T"] = 5 * c.P + 12 * (d.get("r", 1) if c.family in ("enc", "dec", "dws") else 1) + (3 if L.step(c) == 1 else 0)
    assert L.legal(c, d), (c.name, d)
    return d


_SIM = {}


def simulated(e, name):
    """the row's operands at the small size, its float64 three-period reference, and the float32 reference of the FULL clips as the kernel"""
    if name not in _SIM:
        c = L.CASES[name]
        f = G.FAMILIES[c.family](e, c, small(c))
        ref, floor = G.references(f)
        with torch.no_grad():
            y = f.ref(cast(f.o.full_aux(), torch.float32))
        _SIM[name] = (c, f, ref, floor, {k: (v.to(torch.int64) if f.o.outs[k][1] == torch.int64 else v.float()) for k, v in y.items()})
    return _SIM[name]


def compare(f, name, y, want):
    if name in f.o.rates:
        return L.compare_periodic(y, want, f.o._n(f.o.P, f.o.rates[name]), chunk_bytes=1 << 16)
    return L.compare_periodic(y, want, want.shape[2], chunk_bytes=1 << 16)


@pytest.mark.parametrize("name", list(L.CASES))
def test_reference_as_kernel_passes_the_whole_tensor_compare(cpu_env, name):
    c, f, ref, floor, y = simulated(cpu_env, name)
    tol = ROWS[c.tolrow].tol
    assert set(y) == set(f.o.outs) == set(ref), (set(y), set(f.o.outs))
    assert tol >= 4 * floor, f"{name}: tolerance {tol:.1e} is below 4 x the reference's own rounding {floor:.2e}"
    for k, want in ref.items():
        assert tuple(y[k].shape) == f.o.outs[k][0], (name, k, y[k].shape, f.o.outs[k][0])
        got = compare(f, k, y[k], want)
        assert got.finite and got.err <= tol, f"{name} `{k}`: {got.err:.3e} at clip {got.clip} row {got.row} t {got.t}"
    # (clips with the same pattern are bit-identical on the device — the kernels' promise; the CPU's float32 convs make none)
    x = next(t for t in f.o.full.values() if torch.is_tensor(t) and t.dim() == 3 and t.shape[0] == 5)
    assert L.identical_clips_equal(x, chunk_bytes=1 << 16) and not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])


def main_output(c, f, y):
    k = next(o for o in L.OUTPUTS[c.family] if o in y and y[o].dtype != torch.int64)
    return k, y[k]


@pytest.mark.parametrize("name", list(L.CASES))
def test_injected_faults_are_detected(cpu_env, name):
    """on the row's main output: (1) every element from 2^k on reads the element 2^k in front of it — what an offset that loses bit k
    does —, (2) one clip takes another clip's base, (3) one row is its neighbour.  Each must show as an error far above the tolerance."""
    c, f, ref, floor, ys = simulated(cpu_env, name)
    k, y = main_output(c, f, ys)
    tol, want = ROWS[c.tolrow].tol, ref[k]
    B, R, T = y.shape
    P = f.o._n(f.o.P, f.o.rates[k])
    kk = max(j for j in range(4, 31) if (1 << j) < y[0].numel() // 2)            # the wrap of this small tensor
    assert L.wraps_visible(P, (kk,)) or T <= P, (name, P, kk)
    wrapped = y.clone().reshape(-1)
    wrapped[1 << kk:] = y.reshape(-1)[:wrapped.numel() - (1 << kk)]
    assert compare(f, k, wrapped.view(B, R, T), want).err > 100 * tol, f"{name}: a wrap modulo 2^{kk} elements goes unseen"
    clip = y.clone()
    clip[4] = y[3]
    bad = compare(f, k, clip, want)
    assert bad.err > 100 * tol and bad.clip == 4, f"{name}: a clip base taken from the wrong clip goes unseen"
    assert not L.identical_clips_equal(clip)
    if R > 1:
        row = y.clone()
        row[:, R // 2] = y[:, R // 2 - 1]
        bad = compare(f, k, row, want)
        assert bad.err > 100 * tol and bad.row == R // 2, f"{name}: a row read from its neighbour goes unseen"
    nan = y.clone()
    nan[B - 1, R - 1, T - 1] = float("nan")
    got = compare(f, k, nan, want)
    assert not got.finite and (got.clip, got.row, got.t) == (B - 1, R - 1, T - 1)
    assert got.byte_offset == (y.numel() - 1) * 4


def test_period_conditions_of_every_row():
    """the (P, k) pairs of the GPU rows: a wrap of 2^29, 2^30 or 2^31 elements lands on another phase, P is at least twice the receptive
    field, and for a streaming form (one hop per clip: P = T) on another row or clip of the three-pattern cycle"""
    pairs = sorted({(c.P, k) for c in L.CASES.values() for k in L.WRAPS} | {(L.MODEL_P, k) for k in L.WRAPS})
    assert pairs == [(P, k) for P in (60, 160, 300, 320, 1500, 12800) for k in L.WRAPS]
    for P, k in pairs:
        assert (1 << k) % P != 0, (P, k)
    for c in L.CASES.values():
        rf = L.receptive_field(c.layers)
        if c.stream_guard is None:
            L.check_period(c.P, rf)
            for d in c.sizes.values():
                assert d["T"] > 3 * c.P and all(c.P % s == 0 for s in (d.get("r", 1), d.get("s", 1)))
        else:
            assert c.P == c.sizes["at"]["T"] in (160, 320) and L.wraps_visible(c.P)
            cyc = L.NPAT * max(L.bytes_of(s, 1) // s[0] for s in L.tensors(c, c.sizes["at"]).values())
            assert all((1 << k) % cyc != 0 for k in L.WRAPS), c.name
    assert L.receptive_field([("conv", 5, 1)]) == 5 and L.receptive_field([("conv", 8, 4), ("conv", 5, 1)]) == 24
    assert L.receptive_field([("convtr", 2), ("conv", 5, 1)]) == 4          # two input frames, then four half-frame taps more
    assert L.receptive_field(L.RESBLOCK) == 9


def test_boundary_arithmetic_of_every_row():
    for c in L.CASES.values():
        below, at = c.sizes["below"], c.sizes["at"]
        gb, ga = L.governing_bytes(c, below), L.governing_bytes(c, at)
        assert gb < L.LIMIT <= ga, (c.name, gb, ga)
        assert L.legal(c, below) and L.legal(c, at), c.name
        key = "B" if c.stream_guard is not None else "T"
        assert at[key] - below[key] == L.step(c) and {k: v for k, v in at.items() if k != key} == {k: v for k, v in below.items() if k != key}, c.name
        if "b3" in c.sizes:          # three clips, each a little over 2 GiB: the bases of clips 1 and 2 lie beyond 2^31 and 2^32 bytes
            d = c.sizes["b3"]
            per_clip = L.governing_bytes(c, d) // 3
            assert d["B"] == 3 and L.legal(c, d) and (1 << 31) <= per_clip < (1 << 31) + (1 << 16), (c.name, per_clip)
        for size in c.sizes:
            assert L.need_bytes(c, size) < L.MEMORY_CAP, (c.name, size, L.need_bytes(c, size))
            assert L.need_bytes(c, size) <= 6 * L.governing_bytes(c, c.sizes[size]) + (4 << 30), (c.name, size)
    # the long clip: 34 956 frames is the first whole number of 4-frame groups whose [1, 96, T] decoder activation reaches 4 GiB
    from hilcodec_amd import engine
    mk = synth.model_kwargs("hil_speech")
    width = [mk["channels_dec"] * 2 ** (len(mk["strides"]) - 1 - i) for i in range(len(mk["strides"]))]
    ds = types.SimpleNamespace(pre_dw_w=torch.empty(2 * width[0], 5),
                               stages=[types.SimpleNamespace(tr_w=torch.empty(2 * w, 2 * r), pw_wt=torch.empty(2 * w, w), ratio=r)
                                       for w, r in zip(width, mk["strides"])])
    assert L.MODEL_T_AT % 320 == 0 and engine._decoder_clip_elems(ds, L.MODEL_T_AT // 320) * 4 >= L.LIMIT
    assert engine._decoder_clip_elems(ds, L.MODEL_T_BELOW // 320) * 4 < L.LIMIT and L.MODEL_T_BELOW == L.MODEL_T_AT - 4 * 320
    assert (L.MODEL_T_AT // 320) % 4 == 0 and engine._decoder_clip_elems(ds, L.MODEL_T_AT // 320) == 96 * L.MODEL_T_AT
    assert engine._clip_chunks(1, engine._decoder_clip_elems(ds, L.MODEL_T_AT // 320)) == [(0, 1)]          # one clip cannot be chunked


def _ptr(n=1):
    """16-byte aligned non-NULL stand-ins for device pointers: every call below is refused in front of its first launch"""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def test_guards_at_the_boundary_agree_with_the_library():
    """For each guarded product one below, at and one above 2^32 bytes (B - 1, B, B + 1 streams of one hop): the `ops` mirror declines
    exactly from 2^32 on, and where it declines the C entry point refuses too (HILC_ERR_UNSUPPORTED, returned in front of the launch, so
    the call is safe without a device).  Where the mirror ACCEPTS, the library's answer is a launch: that half of the agreement is the
    "below" case of each streaming row of tests/test_gpu_large.py, which asserts the mirror and runs the entry.  hilc_dws_conv_stream's
    long-hop guard is `lin_ok` on the bytes of x `[B,K,T]`: `ops.dws_conv_stream_supported(..., B, M, K)` carries the same bound."""
    from hilcodec_amd import _lib, ops
    lib = _lib.lib
    blk = (_lib.ResblockParams * 3)()
    for i in range(3):
        blk[i] = _lib.ResblockParams(*[4096 + 256 * j for j in range(10)], 1.0, 1.0)
    void = lambda obj: ctypes.cast(ctypes.pointer(obj), ctypes.c_void_p)          # noqa: E731
    p = _ptr(16)
    seen = 0
    for c in L.CASES.values():
        if c.stream_guard is None:
            continue
        at = c.sizes["at"]
        C, r, n, T = at.get("C", 0), at.get("r", 0), at.get("n", 1), at["T"]
        for B in (at["B"] - 1, at["B"], at["B"] + 1):
            d = dict(at, B=B)
            declines = c.stream_guard(d) >= L.LIMIT
            assert declines == (B >= at["B"])
            if c.family == "dwss":
                K, M = at["K"], at["M"]
                mirror = ops.dws_conv_stream_supported(T, 2 * r, r, True, B, M, K) and ops.dws_conv_stream_profitable(T, 2 * r, r, False, B, M, K)
                assert mirror == ops.dws_conv_stream_supported(T, 2 * r, r, False, B, M, K)          # with or without a shortcut
                call = lambda: lib.hilc_dws_conv_stream(*p[:8], B, K, M, T, 2 * r, r, 1.0, 1, 1.0, 0, None)          # noqa: E731
                query = 1          # (no shape query: the mirror is the only host-side predicate)
            elif c.family == "res":
                mirror = ops.resblock_supported(C, T, B, True)
                call = lambda: lib.hilc_resblock_stream(*p[:12], B, C, T, 1.0, 1.0, None)          # noqa: E731
                query = lib.hilc_resblock_stream_supported(C, T)
            elif c.family == "chain":
                mirror = ops.resblock_chain_supported(C, T, n, B, True)
                call = lambda: lib.hilc_resblock_chain(p[0], p[1], void(blk), n, 1, B, C, T, None)          # noqa: E731
                query = lib.hilc_resblock_chain_supported(C, T, n, 1)
            elif c.family == "enc":
                down = _lib.DownParams(*[4096 + 256 * j for j in range(20, 28)], 1.0, r)
                if c.kw.get("stage0"):
                    spec = _lib.Spec0Params(*[4096 + 256 * j for j in range(30, 38)], 63, 1.0, 0.0, 1.0, 1.0, 1, 64, 1, 5)
                    mirror = ops.encoder_stage0_supported(T, n, r, 64, 1, 5, B, True)
                    call = lambda: lib.hilc_encoder_stage0(void(spec), void(blk), n, void(down), 1, B, T, None)          # noqa: E731
                    query = lib.hilc_encoder_stage0_supported(T, n, r, 64, 1, 5, 1)
                else:
                    mirror = ops.encoder_stage_supported(C, T, n, r, B, True)
                    call = lambda: lib.hilc_encoder_stage(p[0], void(blk), n, void(down), 1, B, C, T, None)          # noqa: E731
                    query = lib.hilc_encoder_stage_supported(C, T, n, r, 1)
            else:
                assert c.family == "dec"
                up = _lib.UpParams(*[4096 + 256 * j for j in range(40, 47)], 1.0, r)
                if c.kw.get("post"):
                    post = _lib.PostParams(*[4096 + 256 * j for j in range(50, 55)], 1.0, 1.0, 1, 5)
                    mirror = ops.decoder_stage_supported(C, T, n, r, B, True) and ops.decoder_stage_post_supported(C, T, n, r, 5)
                    call = lambda: lib.hilc_decoder_stage_post(void(up), void(blk), n, void(post), 1, B, C, T, None)          # noqa: E731
                    query = lib.hilc_decoder_stage_supported(C, T, n, r, 1) and lib.hilc_decoder_stage_post_supported(C, T, n, r, 5)
                else:
                    mirror = ops.decoder_stage_supported(C, T, n, r, B, True)
                    call = lambda: lib.hilc_decoder_stage(void(up), void(blk), n, p[1], 1, B, C, T, None)          # noqa: E731
                    query = lib.hilc_decoder_stage_supported(C, T, n, r, 1)
            assert query, f"{c.name}: the shape query (which knows no batch size) must accept C = {C}, T = {T}"
            assert mirror == (not declines), (c.name, B, mirror)
            if declines and not torch.cuda.is_available():          # (with a device the GPU file's refusal cases make this call, on real buffers)
                # the pointers are invented: this is safe only because every guard returns in front of its launch.  A guard that stopped
                # refusing would reach the launch path here — with no device that is a HIP launch error (-3), not a clean -4
                assert call() == -4, f"{c.name}: B = {B} passes the launch path's guard"
                seen += 1
    assert seen == (0 if torch.cuda.is_available() else 14)
    # the offline forms take any size: their mirrors know no limit
    big = 1 << 20
    assert ops.resblock_supported(64, 1 << 24, big) and ops.resblock_chain_supported(96, 11184812, 3, big, streaming=False)
    assert ops.encoder_stage_supported(64, 1 << 24, 2, 2, big, streaming=False) and ops.encoder_stage0_supported(1 << 24, 2, 2, 64, 1, 5, big, False)
    assert ops.decoder_stage_supported(96, 11184812, 3, 2, big, streaming=False) and ops.decoder_stage_post_supported(96, 11184812, 3, 2, 5)
    assert L.lin_ok(1, 16, (1 << 26) - 4) and not L.lin_ok(1, 16, 1 << 26) and L.lin_ok(1, 16, 1 << 24)


def test_model_receptive_field_on_four_periods():
    """the long clip's period: the receptive field derived from the model's kernel sizes and strides is below P / 2, and through the
    oracle periods 2 and 3 of a four-period clip agree within a quarter of the bars the GPU test uses (a bar is at least 4 x its
    reference's own noise) — so the oracle's third period stands for every later one"""
    from oracle import hilcodec_oracle as O
    mk = synth.model_kwargs("hil_speech")
    rf = L.model_receptive_field(mk)
    assert 5000 < rf < L.MODEL_P // 2 and L.MODEL_P % 320 == 0 and L.wraps_visible(L.MODEL_P)
    sd = synth.synth_state_dict("hil_speech", seed=7)
    P, Fp = L.MODEL_P, L.MODEL_P // 320
    x = L.periodic(L.model_pattern(), 4 * P)
    assert torch.equal(x[:, :, :P], x[:, :, 3 * P:])
    with torch.no_grad():
        wav, _, _, aux = O.codec_forward(sd, x, mk)
    z, idx = aux["z"], aux["indices"]
    dz = float((z[:, :, 2 * Fp:3 * Fp] - z[:, :, 3 * Fp:]).abs().max())
    dw = float((wav[:, :, 2 * P:3 * P] - wav[:, :, 3 * P:]).abs().max())
    assert dz <= 1e-5 / 4 and dw <= 1e-4 / 4, (dz, dw)
    assert torch.equal(idx[:, :, 2 * Fp:3 * Fp], idx[:, :, 3 * Fp:])
    # the history reaches into period 0 only: period 1 already equals period 2, and period 0 does not
    assert float((z[:, :, Fp:2 * Fp] - z[:, :, 2 * Fp:3 * Fp]).abs().max()) <= 1e-5 / 4
    assert float((wav[:, :, :P] - wav[:, :, 2 * P:3 * P]).abs().max()) > 1e-4


def test_specblock_waveform_stays_clear_of_the_log_clamp():
    """tests/large_families.py: SPEC_WAV_SEED.  log(max(|STFT|, 1e-5)) magnifies the rounding of a nearly cancelled bin beyond the rows'
    tolerance; the seed's three patterns keep every magnitude a decade above the clamp (measured 9.8e-5), whatever `synth` becomes."""
    from hilcodec_amd import fold
    from tests import alignment as A
    N, P = 64, 1500
    bt = fold.stft_basis_layout(synth.stft_basis(N)).double()
    wav = L.periodic(synth.synth_clips(L.NPAT, P, seed=G.SPEC_WAV_SEED), 4 * P + 500, L.NPAT).double()
    for hist in (None, synth.synth_clips(L.NPAT, N - 1, seed=9).double()):
        mag = A.ref_stft(wav, hist, bt, N, 1, 0.0, 1.0, 2)
        if hist is None:          # (a window that is mostly zero padding is small because the Hann window is, not by cancellation)
            mag = mag[:, :, N - 1:]
        assert float(mag.min()) > 5e-5, float(mag.min())
