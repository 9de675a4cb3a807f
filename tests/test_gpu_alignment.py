"""Every entry point of the hot path on 4-byte-aligned views: fall back or refuse ("Pointer alignment").

One row per entry point and shape.  A row builds its operands on the device, calls the C ABI with raw pointers, and has a plain
float64 reference on the CPU (tests/alignment.py).  The call runs once with every operand 16-byte aligned, then once per operand
and k = 1, 2, 3 with only that operand moved 4 * k bytes off (`skew`).  The row's table gives the audited class of every operand:

  S / F  the call succeeds, is within the op's tolerance of the float64 reference and — caches and every other output included —
         `torch.equal` to the aligned call (the fall-backs promise the same fmaf chains);
  R      the call is refused (RuntimeError out of `check`), every caller-owned output still holds its sentinel, and the device
         is healthy afterwards.

The tolerance of a row is the one the op's own test in tests/test_gpu_ops.py uses; it may not be below 4 x the rounding of the
reference itself (float32 against float64 on the CPU, the `FLOORS` table as measured, asserted again at run time).
Copyable R operands are tested a second time through `hilcodec_amd.ops`, where the wrapper copies them: equal to the aligned call."""
import ctypes
import types

import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from tests import alignment as A
from tests.alignment import skew

pytestmark = pytest.mark.gpu

SENT = -12345.5          # what every caller-owned output holds before a call (no kernel here produces it)
RS = 0.5773502691896258
KS = (1, 2, 3)


def rnd(seed, *shape):
    return torch.from_numpy(synth.normalish(seed, int(np.prod(shape)))).view(*shape)


@pytest.fixture(scope="module")
def env():
    from hilcodec_amd import _lib, fold, ops
    return types.SimpleNamespace(ops=ops, fold=fold, lib=_lib.lib, L=_lib, dev=torch.device("cuda:0"),
                                 stream=lambda: torch.cuda.current_stream().cuda_stream)


def void(obj):
    return ctypes.cast(ctypes.pointer(obj), ctypes.c_void_p)


class Built:
    """ins: operand -> aligned device tensor (None = NULL); outs: operand -> shape of a caller-owned output; aux: what `ref` needs
    (CPU float32 tensors and scalars); call(p) -> return code, p = operand -> pointer."""

    def __init__(self, ins, outs, aux, call):
        self.ins, self.outs, self.aux, self.call = ins, outs, aux, call


def cast(aux, dtype):
    def one(v):
        if torch.is_tensor(v):
            return v.to(dtype) if v.is_floating_point() else v
        if isinstance(v, (list, tuple)):
            return type(v)(one(u) for u in v)
        return v
    return {k: one(v) for k, v in aux.items()}


# ======================================================================================================================
# rows: name -> (tolerance, bit-identical to the aligned call, {operand: class}, build(env) -> Built, ref(aux) -> {output: tensor})
# ======================================================================================================================
ROWS = {}


def row(name, tol, cls, exact=True):
    def deco(fn):
        build, ref = fn()
        ROWS[name] = types.SimpleNamespace(name=name, tol=tol, cls=cls, exact=exact, build=build, ref=ref)
        return fn
    return deco


def _pw(name, B, K, M, T, tol=1e-5):
    t1 = T == 1
    cls = {"x": "S" if t1 else "F", "wt": "R", "bias": "S", "res": "S" if t1 else "F", "y": "S" if t1 else "F"}

    @row(name, tol, cls)
    def _():
        def build(e):
            x, w, b, r = rnd(B * 7 + K, B, K, T), rnd(K + M, K, M) / K ** 0.5, rnd(M, M) * 0.1, rnd(3, B, M, T)
            ins = {"x": x, "wt": w, "bias": b, "res": r}

            def call(p):
                return e.lib.hilc_pw_conv(p["x"], p["wt"], p["bias"], p["res"], p["y"], B, K, M, T, 0.77, 1, 0.61, e.stream())
            return Built(ins, {"y": (B, M, T)}, dict(ins), call)

        def ref(a):
            return {"y": A.ref_pw_conv(a["x"], a["wt"], a["bias"], a["res"], 0.77, True, 0.61)}
        return build, ref


_pw("pw_conv-3x33x96x8", 3, 33, 96, 8)      # one ragged tile
_pw("pw_conv-2x17x64x132", 2, 17, 64, 132)      # T > BN = 128, ragged last tile
_pw("pw_conv-frame1-5x33x96x1", 5, 33, 96, 1)      # the single-frame kernel


def _dwc(name, B, C, T, k, s, hist, res):
    cls = {"x": "F", "hist": "S", "w": "S", "bias": "S", "res": "S", "y": "F", "hist_out": "S"}
    cls = {o: c for o, c in cls.items() if (hist or o not in ("hist", "hist_out")) and (res or o != "res")}

    @row(name, 5e-6, cls)
    def _():
        pad = k - s
        To = (T + s - 1) // s

        def build(e):
            ins = {"x": rnd(C + T, B, C, T), "w": rnd(C + k, C, k), "bias": rnd(C, C) * 0.1}
            if hist:
                ins["hist"] = rnd(5, B, C, pad) * 0.7
            if res:
                ins["res"] = rnd(6, B, C, To)
            outs = {"y": (B, C, To)}
            if hist:
                outs["hist_out"] = (B, C, pad)

            def call(p):
                return e.lib.hilc_dw_conv(p["x"], p.get("hist"), p["w"], p["bias"], p.get("res"), p["y"], p.get("hist_out"), B, C, T, k, s,
                                          0.9, 1, 0.4, 1, e.stream())
            return Built(ins, outs, dict(ins), call)

        def ref(a):
            y, h = A.ref_dw_conv(a["x"], a.get("hist"), a["w"], a["bias"], a.get("res"), s, 0.9, True, 0.4, True)
            return {"y": y, "hist_out": h} if hist else {"y": y}
        return build, ref


_dwc("dw_conv-24x36-k5", 2, 24, 36, 5, 1, False, False)
_dwc("dw_conv-24x36-k5-hist-res", 2, 24, 36, 5, 1, True, True)
_dwc("dw_conv-16x40-k8s4-hist", 2, 16, 40, 8, 4, True, False)


@row("dw_convtr-16x12-r4", 5e-6, {"x": "S", "hist": "S", "w": "S", "y": "S", "hist_out": "S"})
def _():
    B, C, T, r = 2, 16, 12, 4

    def build(e):
        ins = {"x": rnd(1, B, C, T), "hist": rnd(2, B, C, 1) * 0.5, "w": rnd(3, C, 2 * r)}

        def call(p):
            return e.lib.hilc_dw_convtr(p["x"], p["hist"], p["w"], p["y"], p["hist_out"], B, C, T, r, 0.7, 1, e.stream())
        return Built(ins, {"y": (B, C, T * r), "hist_out": (B, C, 1)}, dict(ins), call)

    def ref(a):
        y, h = A.ref_dw_convtr(a["x"], a["hist"], a["w"], r, 0.7, True)
        return {"y": y, "hist_out": h}
    return build, ref


@row("conv_pre-24x36-k5", 2e-5, {"wav": "F", "hist": "S", "w": "S", "bias": "S", "y": "F"})
def _():
    B, C, T, k, HL = 2, 24, 36, 5, 6

    def build(e):
        ins = {"wav": synth.synth_clips(B, T, seed=5), "hist": synth.synth_clips(B, HL, seed=6), "w": rnd(1, C, k), "bias": rnd(2, C) * 0.1}

        def call(p):
            return e.lib.hilc_conv_pre(p["wav"], p["hist"], HL, p["w"], p["bias"], p["y"], B, C, T, k, 1 / 0.1122080159, e.stream())
        return Built(ins, {"y": (B, C, T)}, dict(ins), call)

    def ref(a):
        return {"y": A.ref_conv_pre(a["wav"], a["hist"], a["w"], a["bias"], 1 / 0.1122080159)}
    return build, ref


# The one row that is NOT bit-identical to its aligned call, as include/hilcodec_amd.h documents for hilc_conv_post: with ksize 5,
# T % 4 == 0 and 16-byte aligned x / hist the channels are summed in eight classes c mod 8 (csrc/dwconv.hip, conv_post_k5_kernel:
# `for (c = wave; c < C; c += NCLS)`, then `part[0] + part[1] + ...`), the generic kernel sums them in sequence (conv_post_kernel:
# `for (c = 0; c < C; ++c)`).  The caches are copies and stay bit-identical.
@row("conv_post-24x36-k5-hist", 2e-6, {"x": "F", "hist": "F", "w": "S", "bias": "S", "y": "S", "hist_out": "S"}, exact=("hist_out",))
def _():
    B, C, T, k = 2, 24, 36, 5

    def build(e):
        ins = {"x": rnd(9, B, C, T), "hist": rnd(8, B, C, 4) * 0.6, "w": rnd(3, C, k) / 20, "bias": rnd(4, 1) * 0.1}

        def call(p):
            return e.lib.hilc_conv_post(p["x"], p["hist"], p["w"], p["bias"], p["y"], p["hist_out"], B, C, T, k, 0.707, 1, 0.1122080159, 1,
                                        e.stream())
        return Built(ins, {"y": (B, 1, T), "hist_out": (B, C, 4)}, dict(ins), call)

    def ref(a):
        y, h = A.ref_conv_post(a["x"], a["hist"], a["w"], a["bias"], 0.707, True, 0.1122080159, True)
        return {"y": y, "hist_out": h}
    return build, ref


def _dws(name, B, K, M, T, r, res):
    k5 = r == 1
    cls = {"x": "F", "wt": "R", "dw_w": "S", "dw_b": "S", "y": "F" if k5 else "S"}
    if res:
        cls["res"] = "F"

    @row(name, 2e-5, cls)
    def _():
        k = 5 if k5 else 2 * r
        To = (T + r - 1) // r

        def build(e):
            ins = {"x": rnd(B * 3 + K + T, B, K, T), "wt": rnd(K + M, K, M) / K ** 0.5, "dw_w": rnd(M + k, M, k) * 0.5, "dw_b": rnd(M, M) * 0.1}
            if res:
                ins["res"] = rnd(11, B, M, To)

            def call(p):
                return e.lib.hilc_dws_conv(p["x"], p["wt"], p["dw_w"], p["dw_b"], p.get("res"), p["y"], B, K, M, T, k, r, 0.86, 1,
                                           0.37 if k5 else 1.0, 0, e.stream())
            return Built(ins, {"y": (B, M, To)}, dict(ins), call)

        def ref(a):
            return {"y": A.ref_dws(a["x"], a["wt"], a["dw_w"], a["dw_b"], None, a.get("res"), r, 0.86, True, 0.37 if k5 else 1.0, False)[0]}
        return build, ref


_dws("dws_conv-k5-2x33x96x36", 2, 33, 96, 36, 1, False)
_dws("dws_conv-k5-2x33x96x36-res", 2, 33, 96, 36, 1, True)
_dws("dws_conv-k5-1x16x128x260", 1, 16, 128, 260, 1, False)
_dws("dws_conv-k5-1x16x128x260-res", 1, 16, 128, 260, 1, True)
_dws("dws_conv-r2-2x16x32x64", 2, 16, 32, 64, 2, False)
_dws("dws_conv-r4-2x16x32x64", 2, 16, 32, 64, 4, False)


def _dwss(name, B, K, M, T, k, r, cls, res=True):
    @row(name, 2e-5, cls)
    def _():
        pad = k - r
        k5 = r == 1

        def build(e):
            ins = {"x": rnd(B + K + T, B, K, T), "wt": rnd(K + M, K, M) / K ** 0.5, "dw_w": rnd(M + k, M, k) * 0.5, "dw_b": rnd(M, M) * 0.1,
                   "hist": rnd(12, B, M, pad) * 0.7}
            if res:
                ins["res"] = rnd(11, B, M, T // r)

            def call(p):
                return e.lib.hilc_dws_conv_stream(p["x"], p["wt"], p["dw_w"], p["dw_b"], p["hist"], p["hist_out"], p.get("res"), p["y"], B, K, M, T,
                                                  k, r, 0.86, 1, 0.37 if k5 else 1.0, 1 if k5 else 0, e.stream())
            return Built(ins, {"y": (B, M, T // r), "hist_out": (B, M, pad)}, dict(ins), call)

        def ref(a):
            y, h = A.ref_dws(a["x"], a["wt"], a["dw_w"], a["dw_b"], a["hist"], a.get("res"), r, 0.86, True, 0.37 if k5 else 1.0, k5)
            return {"y": y, "hist_out": h}
        return build, ref


# T <= 128: whole clips per tile.  k5: the `al` switch between Dw5SegEpilogue and DwSegEpilogue; k = 2r with r = 5 / 8: DwSegEpilogue
# reads a row's taps as f32x2 / f32x4 words (gemm_epilogues.h, `body<MB, KS>`), so dw_w is refused there
_dwss("dws_conv_stream-k5-5x32x32x8", 5, 32, 32, 8, 5, 1,
      {"x": "F", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "F", "hist_out": "F", "res": "F", "y": "F"})
_dwss("dws_conv_stream-r5-5x16x32x40", 5, 16, 32, 40, 10, 5,
      {"x": "F", "wt": "R", "dw_w": "R", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})
_dwss("dws_conv_stream-frame1-5x32x32x1", 5, 32, 32, 1, 5, 1,
      {"x": "S", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})
# T > 128: no scalar loader (x refused); DwStrideFlatEpilogue reads hist and res and writes y and hist_out word by word
# (gemm_epilogues.h: `hist[(bq * M + m) * r + j]`, `y[yo] = ... res[yo]`, `hist_out[...] = smem[...]`; its f32x4 reads are LDS)
_dwss("dws_conv_stream-r4-3x16x32x160", 3, 16, 32, 160, 8, 4,
      {"x": "R", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})


def _up(name, entry, B, K, M, Tin, r):
    stream = entry != "hilc_up_conv"
    cls = {"x": "S", "tr_w": "F", "wt": "R", "bias": "S", "y": "F"}
    if stream:
        cls.update({"hist": "S", "hist_out": "S"})
    if entry == "hilc_up_conv_expanded":
        cls["expanded"] = "F"

    @row(name, 3e-5, cls)
    def _():
        def build(e):
            ins = {"x": rnd(100 + K, B, K, Tin), "tr_w": rnd(80, K, 2 * r) * 0.3, "wt": rnd(81, K, M) / K ** 0.5, "bias": rnd(82, M) * 0.1}
            aux = dict(ins)
            outs = {"y": (B, M, Tin * r)}
            if stream:
                aux["hist"] = ins["hist"] = rnd(30, B, K, 1) * 0.6
                outs["hist_out"] = (B, K, 1)
            if "expanded" in cls:
                ins["expanded"] = e.ops.up_conv_taps(ins["tr_w"].to(e.dev), r)        # a layout table: no arithmetic

            def call(p):
                if entry == "hilc_up_conv":
                    return e.lib.hilc_up_conv(p["x"], p["tr_w"], p["wt"], p["bias"], p["y"], B, K, M, Tin, r, 0.7071, 1, e.stream())
                if entry == "hilc_up_conv_stream":
                    return e.lib.hilc_up_conv_stream(p["x"], p["hist"], p["hist_out"], p["tr_w"], p["wt"], p["bias"], p["y"], B, K, M, Tin, r,
                                                     0.7071, 1, e.stream())
                return e.lib.hilc_up_conv_expanded(p["x"], p["hist"], p["hist_out"], p["tr_w"], p["expanded"], p["wt"], p["bias"], p["y"], B, K, M,
                                                   Tin, r, 0.7071, 1, e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            y, h = A.ref_up_conv(a["x"], a.get("hist"), a["tr_w"], a["wt"], a["bias"], r, 0.7071, True)
            return {"y": y, "hist_out": h} if stream else {"y": y}
        return build, ref


# tolerance: tests/test_gpu_ops.py uses 3e-5 for up_conv
_up("up_conv-2x32x16x6-r2", "hilc_up_conv", 2, 32, 16, 6, 2)
_up("up_conv_stream-2x32x16x4-r4", "hilc_up_conv_stream", 2, 32, 16, 4, 4)
_up("up_conv_expanded-2x48x24x4-r5", "hilc_up_conv_expanded", 2, 48, 24, 4, 5)


def _stft(name, B, T, n_fft, hop, hist):
    cls = {"wav": "S", "basis_t": "R", "spec": "S"}
    if hist:
        cls["hist"] = "S"

    @row(name, 2e-5, cls)
    def _():
        HL = n_fft - 1 + 5

        def build(e):
            ins = {"wav": synth.synth_clips(B, T, seed=n_fft), "basis_t": e.fold.stft_basis_layout(synth.stft_basis(n_fft))}
            if hist:
                ins["hist"] = synth.synth_clips(B, HL, seed=77)
            Tf = (T - 1) // hop + 1

            def call(p):
                return e.lib.hilc_stft_logmag(p["wav"], p.get("hist"), HL if hist else 0, p["basis_t"], p["spec"], B, T, n_fft, hop, 0.0, 1.0, 2,
                                              e.stream())
            return Built(ins, {"spec": (B, n_fft // 2 + 1, Tf)}, dict(ins), call)

        def ref(a):
            return {"spec": A.ref_stft(a["wav"], a.get("hist"), a["basis_t"], n_fft, hop, 0.0, 1.0, 2)}
        return build, ref


_stft("stft_logmag-n16-T64-hist", 2, 64, 16, 1, True)      # the generic loader
_stft("stft_logmag-n16-T512-seg", 1, 512, 16, 1, False)      # per-clip LDS segments (Tf >= 512)


def _spec(name, pre):
    cls = {"wav": "S", "hist": "S", "dft_packed": "R", "nyq_sin": "S", "pw_packed": "R", "bias": "S", "y": "R"}
    cls.update({"pre_w": "S", "pre_b": "S"} if pre else {"x": "R"})

    @row(name, 2e-4, cls)
    def _():
        B, T, N = 2, 128, 64

        def build(e):
            bt = e.fold.stft_basis_layout(synth.stft_basis(N))
            wt = rnd(N + 1, N // 2 + 1, N) / (N // 2 + 1) ** 0.5
            dft_p, nyq, pw_p = e.ops.spec_block_tables(bt.to(e.dev), wt.to(e.dev), N)          # layout only
            ins = {"wav": synth.synth_clips(B, T, seed=T + B), "hist": synth.synth_clips(B, N - 1, seed=3), "dft_packed": dft_p, "nyq_sin": nyq,
                   "pw_packed": pw_p, "bias": rnd(N + 2, N) * 0.1}
            aux = {"wav": ins["wav"], "hist": ins["hist"], "bias": ins["bias"], "basis_t": bt, "wt": wt}
            if pre:
                aux["pre_w"] = ins["pre_w"] = rnd(71, N, 5) * 0.5
                aux["pre_b"] = ins["pre_b"] = rnd(72, N) * 0.1
            else:
                aux["x"] = ins["x"] = rnd(9, B, N, T)

            def call(p):
                if pre:
                    return e.lib.hilc_spec_block_conv_pre(p["wav"], p["hist"], N - 1, p["dft_packed"], p["nyq_sin"], p["pw_packed"], p["bias"],
                                                          p["pre_w"], p["pre_b"], 1 / 0.1122080159, p["y"], B, T, N, 1, 5, -4.0, 2.8, 1, 0.37,
                                                          e.stream())
                return e.lib.hilc_spec_block(p["wav"], p["hist"], N - 1, p["dft_packed"], p["nyq_sin"], p["pw_packed"], p["bias"], p["x"], p["y"],
                                             B, T, N, 1, -4.0, 2.8, 1, 0.37, e.stream())
            return Built(ins, {"y": (B, N, T)}, aux, call)

        def ref(a):
            x = A.ref_conv_pre(a["wav"], a["hist"], a["pre_w"], a["pre_b"], 1 / 0.1122080159) if pre else a["x"]
            return {"y": A.ref_spec_block(a["wav"], a["hist"], a["basis_t"], a["wt"], a["bias"], x, 64, 1, -4.0, 2.8, 1, 0.37)}
        return build, ref


_spec("spec_block-n64-T128", False)
_spec("spec_block_conv_pre-n64-T128", True)


# ---- the stage kernel's entries ------------------------------------------------------------------------------------------------------
def raw_blocks(C, n):
    return [(rnd(10 * j + 1, C, C) / C ** 0.5, rnd(10 * j + 2, C, 5) * 0.5, rnd(10 * j + 3, C) * 0.2, rnd(10 * j + 4, C, C) / C ** 0.5,
             rnd(10 * j + 5, C, 5) * 0.5, rnd(10 * j + 6, C) * 0.2, (1 + j * RS ** 2) ** -0.5, 0.4 + 0.1 * j) for j in range(n)]


BLK = ("w1t", "dw1_w", "dw1_b", "w2t", "dw2_w", "dw2_b")


def block_cls(n, streaming):
    cls = {}
    for j in range(n):
        cls.update({f"b{j}.w1t": "R", f"b{j}.dw1_w": "S", f"b{j}.dw1_b": "S", f"b{j}.w2t": "R", f"b{j}.dw2_w": "S", f"b{j}.dw2_b": "S"})
        if streaming:
            cls.update({f"b{j}.hist1": "R", f"b{j}.hist2": "R", f"b{j}.hist1_out": "R", f"b{j}.hist2_out": "R"})
    return cls


def block_operands(e, raw, B, C, streaming, pack, ins, outs, aux):
    aux["blocks"] = [tuple(b) for b in raw]
    aux["caches"] = []
    for j, b in enumerate(raw):
        for nm, t in zip(BLK, b[:6]):
            ins[f"b{j}.{nm}"] = pack(t.to(e.dev)) if nm in ("w1t", "w2t") else t
        if streaming:
            h1, h2 = rnd(7 + j, B, C, 4) * 0.7, rnd(8 + j, B, C, 4) * 0.7
            ins[f"b{j}.hist1"], ins[f"b{j}.hist2"] = h1, h2
            outs[f"b{j}.hist1_out"] = outs[f"b{j}.hist2_out"] = (B, C, 4)
            aux["caches"].append((h1, h2))


def block_structs(e, p, raw, streaming):
    n = len(raw)
    arr = (e.L.ResblockParams * n)()
    for j, b in enumerate(raw):
        caches = [p.get(f"b{j}.{nm}") for nm in ("hist1", "hist2", "hist1_out", "hist2_out")] if streaming else [None] * 4
        arr[j] = e.L.ResblockParams(*[p[f"b{j}.{nm}"] for nm in BLK], *caches, float(b[6]), float(b[7]))
    return arr


ref_blocks = A.ref_blocks          # (the compositions live in tests/alignment.py: tests/test_gpu_large.py shares them)


def _resblock(name, B, C, T, streaming):
    cls = {"x": "R", "y": "R"}
    cls.update(block_cls(1, streaming))

    @row(name, 2e-5, cls)
    def _():
        raw = raw_blocks(C, 1)

        def build(e):
            ins, outs, aux = {"x": rnd(C + T, B, C, T)}, {"y": (B, C, T)}, {}
            aux["x"] = ins["x"]
            block_operands(e, raw, B, C, streaming, e.ops.resblock_pack, ins, outs, aux)

            def call(p):
                w = [p[f"b0.{nm}"] for nm in BLK]
                if not streaming:
                    return e.lib.hilc_resblock(p["x"], *w, p["y"], B, C, T, float(raw[0][6]), float(raw[0][7]), e.stream())
                return e.lib.hilc_resblock_stream(p["x"], *w, p["b0.hist1"], p["b0.hist2"], p["b0.hist1_out"], p["b0.hist2_out"], p["y"], B, C, T,
                                                  float(raw[0][6]), float(raw[0][7]), e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            out = {}
            out["y"] = ref_blocks(a, a["x"], streaming, out)
            return out
        return build, ref


_resblock("resblock-64x8x2", 2, 64, 8, False)
_resblock("resblock_stream-64x8x3", 3, 64, 8, True)


def _chain(name, B, C, T, n, streaming):
    cls = {"x": "R", "y": "R"}
    cls.update(block_cls(n, streaming))

    @row(name, 5e-5, cls)
    def _():
        raw = raw_blocks(C, n)

        def build(e):
            ins, outs, aux = {"x": rnd(C + T, B, C, T)}, {"y": (B, C, T)}, {}
            aux["x"] = ins["x"]
            block_operands(e, raw, B, C, streaming, lambda w: e.ops.resblock_chain_pack(w, streaming), ins, outs, aux)

            def call(p):
                return e.lib.hilc_resblock_chain(p["x"], p["y"], void(block_structs(e, p, raw, streaming)), n, int(streaming), B, C, T, e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            out = {}
            out["y"] = ref_blocks(a, a["x"], streaming, out)
            return out
        return build, ref


_chain("resblock_chain-64x8x2-offline", 2, 64, 8, 2, False)
_chain("resblock_chain-64x8x3-stream", 3, 64, 8, 2, True)


def _enc(name, B, C, T, r, n, streaming, stage0=False):
    # down.dw_w: the wide stages (C = 256 / 512, `DWIDE`) read a row's taps as f32x2 / f32x4 words (resblock_kernel.h: `taps_of`), the
    # narrow ones one by one (`a.dn.dw_w[mc * 2 * DR + j]`)
    cls = {"down.w_lo": "R", "down.w_hi": "R", "down.dw_w": "R" if C >= 256 else "S", "down.dw_b": "S", "down.res": "R", "down.y": "R"}
    if stage0:
        cls.update({"spec.wav": "S", "spec.dft_packed": "R", "spec.nyq_sin": "S", "spec.pw_packed": "R", "spec.bias": "S", "spec.pre_w": "S",
                    "spec.pre_b": "S"})
    else:
        cls["x"] = "R"
    if streaming:
        cls.update({"down.hist": "R", "down.hist_out": "R"})
        if stage0:
            cls["spec.hist"] = "S"
    cls.update(block_cls(n, streaming))

    @row(name, 2e-4 if stage0 else 5e-5, cls)
    def _():
        raw = raw_blocks(C, n)
        in_scale = (1 + n * RS ** 2) ** -0.5
        N = 64

        def build(e):
            ins, outs, aux = {}, {"down.y": (B, 2 * C, T // r)}, {}
            pack = lambda w: e.ops.resblock_chain_pack(w, streaming)          # noqa: E731
            if stage0:
                bt = e.fold.stft_basis_layout(synth.stft_basis(N))
                wt = rnd(N + 1, N // 2 + 1, C) / (N // 2 + 1) ** 0.5
                dft_p, nyq, pw_p = e.ops.spec_block_tables(bt.to(e.dev), wt.to(e.dev), N)
                ins.update({"spec.wav": synth.synth_clips(B, T, seed=T + B), "spec.dft_packed": dft_p, "spec.nyq_sin": nyq, "spec.pw_packed": pw_p,
                            "spec.bias": rnd(N + 2, C) * 0.1, "spec.pre_w": rnd(71, C, 5) * 0.5, "spec.pre_b": rnd(72, C) * 0.1})
                if streaming:
                    ins["spec.hist"] = synth.synth_clips(B, N - 1, seed=9)
                aux.update({"wav": ins["spec.wav"], "whist": ins.get("spec.hist"), "sbias": ins["spec.bias"], "pre_w": ins["spec.pre_w"],
                            "pre_b": ins["spec.pre_b"], "basis_t": bt, "swt": wt})
            else:
                aux["x"] = ins["x"] = rnd(C + T + r, B, C, T)
            block_operands(e, raw, B, C, streaming, pack, ins, outs, aux)
            wd = rnd(70, C, 2 * C) / C ** 0.5                               # k-major [C, 2C]
            ins["down.w_lo"], ins["down.w_hi"] = pack(wd[:, :C].contiguous().to(e.dev)), pack(wd[:, C:].contiguous().to(e.dev))
            ins["down.dw_w"], ins["down.dw_b"], ins["down.res"] = rnd(73, 2 * C, 2 * r) * 0.3, rnd(74, 2 * C) * 0.1, rnd(75, B, 2 * C, T // r) * 0.5
            aux.update({"wd": wd, "ddw": ins["down.dw_w"], "ddb": ins["down.dw_b"], "dres": ins["down.res"], "dhist": None})
            if streaming:
                aux["dhist"] = ins["down.hist"] = rnd(30, B, 2 * C, r) * 0.6
                outs["down.hist_out"] = (B, 2 * C, r)

            def call(p):
                down = e.L.DownParams(p["down.w_lo"], p["down.w_hi"], p["down.dw_w"], p["down.dw_b"], p.get("down.hist"), p.get("down.hist_out"),
                                      p["down.res"], p["down.y"], in_scale, r)
                blocks = block_structs(e, p, raw, streaming)
                if stage0:
                    spec = e.L.Spec0Params(p["spec.wav"], p["spec.dft_packed"], p["spec.nyq_sin"], p["spec.pw_packed"], p["spec.bias"], p["spec.pre_w"],
                                           p["spec.pre_b"], p.get("spec.hist"), N - 1 if streaming else 0, 1 / 0.1122080159, -4.0, 2.8, 0.37, 1, N, 1, 5)
                    return e.lib.hilc_encoder_stage0(void(spec), void(blocks), n, void(down), int(streaming), B, T, e.stream())
                return e.lib.hilc_encoder_stage(p["x"], void(blocks), n, void(down), int(streaming), B, C, T, e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            return A.ref_encoder_stage(a, streaming, stage0, r, in_scale, N)
        return build, ref


# tolerances: 5e-5 (test_encoder_stage_offline_vs_oracle_composition), 2e-4 (test_encoder_stage0_vs_oracle_composition)
_enc("encoder_stage-128x8-r4-offline", 2, 128, 8, 4, 2, False)
_enc("encoder_stage-128x8-r4-stream", 3, 128, 8, 4, 2, True)
_enc("encoder_stage-512x8-r8-offline", 2, 512, 8, 8, 2, False)
_enc("encoder_stage-512x8-r8-stream", 3, 512, 8, 8, 2, True)
_enc("encoder_stage0-T8-offline", 2, 64, 8, 2, 2, False, stage0=True)
_enc("encoder_stage0-T128-stream", 3, 64, 128, 2, 2, True, stage0=True)


def _dec(name, B, C, Tin, r, n, streaming, post=False):
    cls = {"up.x": "S", "up.tr_w": "R", "up.w_lo": "R", "up.w_hi": "R", "up.bias": "S"}
    if streaming:
        cls.update({"up.hist": "S", "up.hist_out": "S"})
    if post:
        cls.update({"post.w": "S", "post.bias": "S", "post.wav": "R"})
        if streaming:
            cls.update({"post.hist": "R", "post.hist_out": "R"})
    else:
        cls["y"] = "R"
    cls.update(block_cls(n, streaming))

    @row(name, 2e-5 if post else 5e-5, cls)
    def _():
        raw = raw_blocks(C, n)
        T = Tin * r

        def build(e):
            ins, outs, aux = {"up.x": rnd(100 + C, B, 2 * C, Tin)}, {}, {}
            pack = lambda w: e.ops.resblock_chain_pack(w, streaming)          # noqa: E731
            tw, wu, bu = rnd(80, 2 * C, 2 * r) * 0.3, rnd(81, 2 * C, C) / (2 * C) ** 0.5, rnd(82, C) * 0.1
            taps = e.ops.up_conv_taps(tw.to(e.dev), r)                       # r = 5: the expanded table
            ins.update({"up.tr_w": tw if taps is None else taps, "up.w_lo": pack(wu[:C].contiguous().to(e.dev)),
                        "up.w_hi": pack(wu[C:].contiguous().to(e.dev)), "up.bias": bu})
            aux.update({"xin": ins["up.x"], "tw": tw, "wu": wu, "bu": bu, "uhist": None, "phist": None})
            if streaming:
                aux["uhist"] = ins["up.hist"] = rnd(30, B, 2 * C, 1) * 0.6
                outs["up.hist_out"] = (B, 2 * C, 1)
            block_operands(e, raw, B, C, streaming, pack, ins, outs, aux)
            if post:
                aux["pw"], aux["pb"] = ins["post.w"], ins["post.bias"] = rnd(83, C, 5) * 0.2, rnd(84, 1) * 0.1
                outs["post.wav"] = (B, 1, T)
                if streaming:
                    aux["phist"] = ins["post.hist"] = rnd(31, B, C, 4) * 0.6
                    outs["post.hist_out"] = (B, C, 4)
            else:
                outs["y"] = (B, C, T)

            def call(p):
                up = e.L.UpParams(p["up.x"], p["up.tr_w"], p["up.w_lo"], p["up.w_hi"], p["up.bias"], p.get("up.hist"), p.get("up.hist_out"), 0.7071, r)
                blocks = block_structs(e, p, raw, streaming)
                if post:
                    ps = e.L.PostParams(p["post.w"], p["post.bias"], p["post.wav"], p.get("post.hist"), p.get("post.hist_out"), 0.5, 0.1122, 1, 5)
                    return e.lib.hilc_decoder_stage_post(void(up), void(blocks), n, void(ps), int(streaming), B, C, T, e.stream())
                return e.lib.hilc_decoder_stage(void(up), void(blocks), n, p["y"], int(streaming), B, C, T, e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            return A.ref_decoder_stage(a, streaming, post, r)
        return build, ref


# tolerances: 5e-5 (test_decoder_stage_offline_vs_oracle_composition), 2e-5 (test_decoder_stage_post_equals_stage_then_conv_post_and_oracle)
_dec("decoder_stage-96-r2-Tin2-offline", 2, 96, 2, 2, 3, False)
_dec("decoder_stage-96-r2-Tin2-stream", 3, 96, 2, 2, 3, True)
_dec("decoder_stage-384-r5-Tin4-offline", 2, 384, 4, 5, 3, False)
_dec("decoder_stage-384-r5-Tin4-stream", 3, 384, 4, 5, 3, True)
_dec("decoder_stage_post-96-r2-Tin2-offline", 2, 96, 2, 2, 3, False, post=True)
_dec("decoder_stage_post-96-r2-Tin2-stream", 3, 96, 2, 2, 3, True, post=True)


# ---- the remaining float entry points: every operand is read and written word by word (class S) --------------------------------------
@row("l2norm-3x128x5", 1e-6, {"x": "S", "y": "S"})
def _():
    B, C, T = 3, 128, 5

    def build(e):
        ins = {"x": rnd(1, B, C, T)}
        return Built(ins, {"y": (B, T, C)}, dict(ins), lambda p: e.lib.hilc_l2norm(p["x"], p["y"], B, C, T, 1e-12, 1.0, 1, e.stream()))
    return build, lambda a: {"y": A.ref_l2norm(a["x"], 1e-12, 1.0, True)}


@row("tail-2x3x7-pad9", 0.0, {"x": "S", "hist": "S", "out": "S"})
def _():
    def build(e):
        ins = {"x": rnd(1, 2, 3, 7), "hist": rnd(2, 2, 3, 10)}
        return Built(ins, {"out": (2, 3, 9)}, dict(ins), lambda p: e.lib.hilc_tail(p["x"], p["hist"], p["out"], 6, 7, 9, 10, e.stream()))
    return build, lambda a: {"out": torch.cat([a["hist"], a["x"]], dim=2)[:, :, -9:]}


def _rvq_tables(Nq, K, C):
    cb = rnd(5, Nq, K, C) * 0.3
    return cb, cb.transpose(1, 2).contiguous(), cb.pow(2).sum(-1)


def _rvq_enc(name, B, T):
    # 8 192 frames and more: the matrix-pipe form reads codebooks_t and norms as 16-byte words and falls back to the VALU form (csrc/rvq.hip)
    @row(name, 1e-5, {"z": "S", "codebooks": "S", "codebooks_t": "F", "norms": "F", "indices": "S", "q": "S", "frame_err": "S"})
    def _():
        Nq, K, C, n = 3, 1024, 128, 2

        def build(e):
            cb, cbt, nrm = _rvq_tables(Nq, K, C)
            ins = {"z": rnd(7, B, C, T) * 0.4, "codebooks": cb, "codebooks_t": cbt, "norms": nrm}

            def call(p):
                return e.lib.hilc_rvq_encode(p["z"], p["codebooks"], p["codebooks_t"], p["norms"], p["indices"], p["q"], p["frame_err"], B, C, T, K, Nq,
                                             n, 0, 0, 0, e.stream())
            return Built(ins, {"indices": ((B, n, T), torch.int64), "q": (B, C, T), "frame_err": (B * T,)}, dict(ins), call)

        def ref(a):
            """the quantised sum of the indices the call returned must be what float64 sums; the indices themselves are pinned by
            tests/test_gpu_rvq.py and, here, by equality with the aligned call"""
            return {}
        return build, ref


_rvq_enc("rvq_encode-valu-2x128x9", 2, 9)
_rvq_enc("rvq_encode-mfma-8x128x1024", 8, 1024)


@row("rvq_decode-2x128x9", 1e-6, {"indices": "S", "codebooks": "S", "q": "S"})
def _():
    B, T, Nq, K, C, n = 2, 9, 3, 1024, 128, 3

    def build(e):
        cb = _rvq_tables(Nq, K, C)[0]
        idx = torch.from_numpy(np.random.RandomState(3).randint(0, K, size=(B, n, T))).to(torch.int64)
        ins = {"indices": idx, "codebooks": cb}
        return Built(ins, {"q": (B, C, T)}, dict(ins),
                     lambda p: e.lib.hilc_rvq_decode(p["indices"], p["codebooks"], p["q"], B, C, T, K, Nq, n, 0, 0, e.stream()))

    def ref(a):
        q = sum(a["codebooks"][s][a["indices"][:, s]] for s in range(n))          # [B, T, C]
        return {"q": q.transpose(1, 2)}
    return build, ref


# The floor of every row: the largest difference between its reference evaluated in float32 and in float64 on the CPU, as measured
# (figures of one CPU; the float32 sums depend on the host's BLAS blocking, so the sweep measures the floor again where it runs
# and asserts tolerance >= 4 x that).  The RVQ encode rows
# compare integers and consistency, `tail` copies: no rounding.
FLOORS = {
    "pw_conv-3x33x96x8": 3.68e-07,
    "pw_conv-2x17x64x132": 3.48e-07,
    "pw_conv-frame1-5x33x96x1": 2.42e-07,
    "dw_conv-24x36-k5": 2.28e-07,
    "dw_conv-24x36-k5-hist-res": 2.50e-07,
    "dw_conv-16x40-k8s4-hist": 1.12e-07,
    "dw_convtr-16x12-r4": 2.36e-07,
    "conv_pre-24x36-k5": 9.12e-07,
    "conv_post-24x36-k5-hist": 8.82e-08,
    "dws_conv-k5-2x33x96x36": 2.41e-07,
    "dws_conv-k5-2x33x96x36-res": 2.41e-07,
    "dws_conv-k5-1x16x128x260": 2.98e-07,
    "dws_conv-k5-1x16x128x260-res": 2.87e-07,
    "dws_conv-r2-2x16x32x64": 4.59e-07,
    "dws_conv-r4-2x16x32x64": 4.53e-07,
    "dws_conv_stream-k5-5x32x32x8": 4.83e-07,
    "dws_conv_stream-r5-5x16x32x40": 6.90e-07,
    "dws_conv_stream-frame1-5x32x32x1": 3.10e-07,
    "dws_conv_stream-r4-3x16x32x160": 6.07e-07,
    "up_conv-2x32x16x6-r2": 1.76e-07,
    "up_conv_stream-2x32x16x4-r4": 1.79e-07,
    "up_conv_expanded-2x48x24x4-r5": 2.23e-07,
    "stft_logmag-n16-T64-hist": 1.49e-07,
    "stft_logmag-n16-T512-seg": 1.31e-07,
    "spec_block-n64-T128": 4.66e-07,
    "spec_block_conv_pre-n64-T128": 9.52e-07,
    "resblock-64x8x2": 2.59e-07,
    "resblock_stream-64x8x3": 8.59e-07,
    "resblock_chain-64x8x2-offline": 3.78e-07,
    "resblock_chain-64x8x3-stream": 8.59e-07,
    "encoder_stage-128x8-r4-offline": 6.37e-07,
    "encoder_stage-128x8-r4-stream": 1.11e-06,
    "encoder_stage-512x8-r8-offline": 9.13e-07,
    "encoder_stage-512x8-r8-stream": 1.81e-06,
    "encoder_stage0-T8-offline": 3.69e-07,
    "encoder_stage0-T128-stream": 1.54e-06,
    "decoder_stage-96-r2-Tin2-offline": 3.34e-07,
    "decoder_stage-96-r2-Tin2-stream": 8.02e-07,
    "decoder_stage-384-r5-Tin4-offline": 6.44e-07,
    "decoder_stage-384-r5-Tin4-stream": 1.01e-06,
    "decoder_stage_post-96-r2-Tin2-offline": 2.41e-08,
    "decoder_stage_post-96-r2-Tin2-stream": 8.02e-07,
    "l2norm-3x128x5": 1.78e-08,
    "tail-2x3x7-pad9": 0.00e+00,
    "rvq_encode-valu-2x128x9": 0.00e+00,
    "rvq_encode-mfma-8x128x1024": 0.00e+00,
    "rvq_decode-2x128x9": 1.19e-07,
}

# ======================================================================================================================
# the sweep
# ======================================================================================================================
_BUILT, _ALIGNED, _REF = {}, {}, {}


def built(e, name):
    if name not in _BUILT:
        b = ROWS[name].build(e)
        b.ins = {k: (None if v is None else v.to(e.dev).contiguous()) for k, v in b.ins.items()}
        for t in b.ins.values():
            assert t is None or t.data_ptr() % 16 == 0
        _BUILT[name] = b
    return _BUILT[name]


def reference(e, name):
    """float64 reference of the row and the floor under its tolerance: 4 x the largest difference between the same reference in
    float32 and in float64 — computed once per row"""
    if name not in _REF:
        b = built(e, name)
        r64 = ROWS[name].ref(cast(b.aux, torch.float64))
        r32 = ROWS[name].ref(cast(b.aux, torch.float32))
        floor = max([float((r32[k].double() - r64[k]).abs().max()) for k in r64] + [0.0])
        _REF[name] = (r64, floor)
    return _REF[name]


def run(e, name, operand=None, k=0):
    """one call of the row with `operand` (an input or an output) skewed by k; -> (return code, {output: CPU tensor})"""
    b = built(e, name)
    ins = {o: (skew(t, k) if o == operand else t) for o, t in b.ins.items()}
    outs = {}
    for o, shape in b.outs.items():
        shape, dtype = shape if isinstance(shape[0], tuple) else (shape, torch.float32)
        t = torch.full(shape, SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device=e.dev)
        outs[o] = skew(t, k) if o == operand else t
    p = {o: (None if t is None else t.data_ptr()) for o, t in list(ins.items()) + list(outs.items())}
    if operand is not None:
        assert p[operand] % 16 != 0 and all(v is None or v % 16 == 0 for o, v in p.items() if o != operand)
    before = {o: t.clone() for o, t in ins.items() if t is not None}
    rc = b.call(p)
    torch.cuda.synchronize()
    for o, t in before.items():
        assert torch.equal(ins[o], t), f"{name}: the call changed its input `{o}`"
    return rc, {o: t.cpu() for o, t in outs.items()}


def sentinel(t):
    return bool((t == (SENT if t.is_floating_point() else int(SENT))).all())


def check_ok(e, name, outs, what):
    r = ROWS[name]
    ref, floor = reference(e, name)
    assert r.tol >= 4 * floor or not ref, f"{name}: tolerance {r.tol:.1e} is below 4 x the reference's own rounding {floor:.2e}"
    for o, want in ref.items():
        assert outs[o].shape == want.shape, (name, o, outs[o].shape, want.shape)
        d = float((outs[o].double() - want).abs().max())
        print(f"{name} [{what}] {o}: max |y - ref64| = {d:.3e} (tolerance {r.tol:.1e}, floor {floor:.2e})")
        assert d <= r.tol, f"{name} [{what}] `{o}`: {d:.3e} > {r.tol:.1e}"
    for o, t in outs.items():
        assert not sentinel(t), f"{name} [{what}]: output `{o}` was not written"


def aligned(e, name):
    if name not in _ALIGNED:
        rc, outs = run(e, name)
        assert rc == 0, f"{name}: the aligned call failed with {rc}"
        check_ok(e, name, outs, "aligned")
        _ALIGNED[name] = outs
    return _ALIGNED[name]


def test_every_operand_has_a_class(env):
    assert set(FLOORS) == set(ROWS)
    for name, r in ROWS.items():
        assert r.tol >= 4 * FLOORS[name], name
        b = built(env, name)
        assert set(r.cls) == {o for o, t in b.ins.items() if t is not None} | set(b.outs), name
        assert set(r.cls.values()) <= {"S", "F", "R"}, name


@pytest.mark.parametrize("name", list(ROWS))
def test_aligned_call(env, name):
    aligned(env, name)


@pytest.mark.parametrize("name,operand", [(n, o) for n, r in ROWS.items() for o in r.cls])
def test_one_operand_skewed(env, name, operand):
    e, r = env, ROWS[name]
    base = aligned(e, name)
    for k in KS:
        rc, outs = run(e, name, operand, k)
        what = f"{operand} + {4 * k} B"
        if r.cls[operand] == "R":
            assert rc == -4, f"{name} [{what}]: expected HILC_ERR_UNSUPPORTED, got {rc}"
            with pytest.raises(RuntimeError):
                e.L.check(rc, name)
            for o, t in outs.items():
                assert sentinel(t), f"{name} [{what}]: the refused call wrote `{o}`"
            torch.cuda.synchronize()
            continue
        assert rc == 0, f"{name} [{what}]: class {r.cls[operand]} but the call returned {rc}"
        check_ok(e, name, outs, what)
        for o, t in outs.items():
            if r.exact is True or o in r.exact:
                assert torch.equal(t, base[o]), f"{name} [{what}]: `{o}` differs from the aligned call by {float((t.double() - base[o].double()).abs().max()):.3e}"


def test_rvq_encode_sums_its_own_indices(env):
    """the RVQ rows have no float64 reference of their arg-min (a near-tie may legitimately flip); what they return must be consistent:
    q = the float64 sum of the code vectors of the returned indices, frame_err = |z - q|^2"""
    for name in ("rvq_encode-valu-2x128x9", "rvq_encode-mfma-8x128x1024"):
        outs, a = aligned(env, name), built(env, name).aux
        idx, cb = outs["indices"], a["codebooks"].double()
        assert int(idx.min()) >= 0 and int(idx.max()) < cb.shape[1]
        q = sum(cb[s][idx[:, s]] for s in range(idx.shape[1])).transpose(1, 2)
        assert float((outs["q"].double() - q).abs().max()) <= 1e-6
        err = (a["z"].double() - q).pow(2).sum(1).reshape(-1)
        assert float((outs["frame_err"].double() - err).abs().max()) <= 1e-5 * float(err.max())
        # and the indices are the float64 arg-min wherever float64 sees a clear winner
        res = a["z"].double().transpose(1, 2).reshape(-1, cb.shape[2])
        for s in range(idx.shape[1]):
            d = cb[s].pow(2).sum(-1)[None] - 2 * res @ cb[s].t()
            best2 = d.topk(2, dim=1, largest=False)
            got = idx[:, s].reshape(-1)
            clear = (best2.values[:, 1] - best2.values[:, 0]) > 1e-4
            assert torch.equal(got[clear], best2.indices[:, 0][clear]), (name, s)
            res = res - cb[s][got]


# ======================================================================================================================
# the model layer copies what the library would refuse
# ======================================================================================================================
def _ops_cases(e):
    """(name, fn(t) -> outputs, {operand: aligned tensor}) — `fn` calls hilcodec_amd.ops with the operands of the dict, one case per
    wrapper that copies (`_al16`), streaming and offline; packed tables are held in the dict, so they are what gets skewed"""
    ops, dev = e.ops, e.dev
    cases = []

    def add(name, fn, t):
        cases.append((name, fn, t))

    def D(t):
        return t.to(dev)
    B, K, M, T = 2, 17, 64, 132
    t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "res": D(rnd(3, B, M, T))}
    add("pw_conv", lambda t: (ops.pw_conv(t["x"], t["wt"], None, res=t["res"], in_scale=0.8, in_elu=True),), t)
    B, K, M, T = 2, 33, 96, 36
    t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "dw_w": D(rnd(3, M, 5) * 0.5), "dw_b": D(rnd(4, M) * 0.1), "res": D(rnd(5, B, M, T))}
    add("dws_conv-k5", lambda t: (ops.dws_conv(t["x"], t["wt"], t["dw_w"], t["dw_b"], res=t["res"], in_scale=0.86, in_elu=True, out_scale=0.37),), t)
    t = {"x": D(rnd(1, 2, 16, 64)), "wt": D(rnd(2, 16, 32) / 4), "dw_w": D(rnd(3, 32, 8) * 0.5), "dw_b": D(rnd(4, 32) * 0.1)}
    add("dws_conv-r4", lambda t: (ops.dws_conv(t["x"], t["wt"], t["dw_w"], t["dw_b"], stride=4, in_scale=0.86, in_elu=True),), t)
    for name, (B, K, M, T, k, r) in (("dws_conv_stream-long", (3, 16, 32, 160, 8, 4)), ("dws_conv_stream-r5", (5, 16, 32, 40, 10, 5)),
                                     ("dws_conv_stream-k5", (5, 32, 32, 8, 5, 1))):
        t = {"x": D(rnd(1, B, K, T)), "wt": D(rnd(2, K, M) / K ** 0.5), "dw_w": D(rnd(3, M, k) * 0.5), "dw_b": D(rnd(4, M)), "hist": D(rnd(5, B, M, k - r))}
        add(name, lambda t, r=r: ops.dws_conv_stream(t["x"], t["wt"], t["dw_w"], t["dw_b"], t["hist"], stride=r, in_elu=True), t)
    # the up-sampling stage: offline r = 2, a hop with its cache r = 4, the expanded table r = 5
    for name, (B, K, M, Tin, r, stream) in (("up_conv-r2", (2, 32, 16, 6, 2, False)), ("up_conv-r4-stream", (2, 32, 16, 4, 4, True)),
                                            ("up_conv-r5-expanded-stream", (2, 48, 24, 4, 5, True))):
        t = {"x": D(rnd(100 + K, B, K, Tin)), "tr_w": D(rnd(80, K, 2 * r) * 0.3), "wt": D(rnd(81, K, M) / K ** 0.5), "bias": D(rnd(82, M) * 0.1)}
        if r == 5:
            t["taps"] = ops.up_conv_taps(t["tr_w"], r)
        if stream:
            t["hist"] = D(rnd(30, B, K, 1) * 0.6)
        add(name, lambda t, r=r, stream=stream: tuple(ops.up_conv(t["x"], t["tr_w"], t["wt"], t["bias"], r, in_scale=0.7071, hist=t.get("hist"),
                                                                  want_hist=True, taps=t.get("taps"))) if stream
            else (ops.up_conv(t["x"], t["tr_w"], t["wt"], t["bias"], r, in_scale=0.7071),), t)
    t = {"wav": D(synth.synth_clips(2, 64, seed=1)), "basis_t": D(e.fold.stft_basis_layout(synth.stft_basis(16)))}
    add("stft_logmag", lambda t: (ops.stft_logmag(t["wav"], t["basis_t"], 16, 1, normalize=2),), t)
    # hilc_conv_post's generic kernel sums the channels in another order (the sweep's one exception): ops copies, the bits stay
    t = {"x": D(rnd(9, 2, 24, 36)), "hist": D(rnd(8, 2, 24, 4) * 0.6), "w": D(rnd(3, 24, 5) / 20)}
    add("conv_post", lambda t: ops.conv_post(t["x"], t["w"], None, in_scale=0.707, hist=t["hist"], want_hist=True), t)
    N = 64
    dft_p, nyq, pw_p = ops.spec_block_tables(D(e.fold.stft_basis_layout(synth.stft_basis(N))), D(rnd(N + 1, N // 2 + 1, N) / 6), N)
    sp = {"wav": D(synth.synth_clips(2, 128, seed=2)), "whist": D(synth.synth_clips(2, N - 1, seed=3)), "dft": dft_p, "nyq": nyq, "pw": pw_p,
          "sbias": D(rnd(N + 2, N) * 0.1)}
    t = dict(sp, x=D(rnd(9, 2, N, 128)))
    add("spec_block", lambda t: (ops.spec_block(t["wav"], t["dft"], t["nyq"], t["pw"], t["sbias"], t["x"], N, 1, -4.0, 2.8, True, 0.37, hist=t["whist"]),), t)
    t = dict(sp, pre_w=D(rnd(71, N, 5) * 0.5), pre_b=D(rnd(72, N) * 0.1))
    add("spec_block_conv_pre", lambda t: (ops.spec_block_conv_pre(t["wav"], t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159,
                                                                  N, 1, -4.0, 2.8, True, 0.37, hist=t["whist"]),), t)

    # ---- the fused block, the chain and the stage ops, a hop with every cache and the offline form
    def block_dict(C, n, B, streaming, pack):
        raw = raw_blocks(C, n)
        t = {}
        for j, b in enumerate(raw):
            for nm, w in zip(BLK, b[:6]):
                t[f"b{j}.{nm}"] = pack(D(w)) if nm in ("w1t", "w2t") else D(w)
            if streaming:
                t[f"b{j}.hist1"], t[f"b{j}.hist2"] = D(rnd(7 + j, B, C, 4) * 0.7), D(rnd(8 + j, B, C, 4) * 0.7)
        return raw, t

    def blocks_of(t, raw, streaming):
        n = len(raw)
        return ([tuple(t[f"b{j}.{nm}"] for nm in BLK) + (raw[j][6], raw[j][7]) for j in range(n)],
                [[t[f"b{j}.hist1"], t[f"b{j}.hist2"]] for j in range(n)] if streaming else None)

    def flat(r):
        """(y, [caches], cache, ...) or y -> a flat list of tensors"""
        if torch.is_tensor(r):
            return [r]
        out = []
        for v in r:
            out.extend(flat(v))
        return out
    B = 3
    for streaming in (True, False):
        tag = "stream" if streaming else "offline"
        pack = lambda w, s=streaming: ops.resblock_chain_pack(w, s)          # noqa: E731
        # one block: the packed matrices are operands of the dict
        C, T = 64, 8
        raw, t = block_dict(C, 1, B, streaming, ops.resblock_pack)
        t["x"] = D(rnd(C, B, C, T))
        add(f"resblock-{tag}", lambda t, raw=raw, s=streaming: flat(ops.resblock(t["x"], *[t[f"b0.{nm}"] for nm in BLK], raw[0][6], raw[0][7],
                                                                          hist=[t["b0.hist1"], t["b0.hist2"]] if s else None)), t)
        raw, t = block_dict(C, 2, B, streaming, pack)
        t["x"] = D(rnd(C, B, C, T))
        add(f"resblock_chain-{tag}", lambda t, raw=raw, s=streaming: flat(ops.resblock_chain(t["x"], *blocks_of(t, raw, s))), t)
        # encoder stages: narrow (C = 128, r = 4: the taps are class S) and wide (C = 512, r = 8: class R)
        for C, r in ((128, 4), (512, 8)):
            raw, t = block_dict(C, 2, B, streaming, pack)
            wd = D(rnd(70, C, 2 * C) / C ** 0.5)
            t.update({"x": D(rnd(C + 1, B, C, T)), "w_lo": pack(wd[:, :C].contiguous()), "w_hi": pack(wd[:, C:].contiguous()),
                      "dw_w": D(rnd(73, 2 * C, 2 * r) * 0.3), "dw_b": D(rnd(74, 2 * C) * 0.1), "res": D(rnd(75, B, 2 * C, T // r) * 0.5)})
            if streaming:
                t["dhist"] = D(rnd(30, B, 2 * C, r) * 0.6)

            def enc(t, raw=raw, s=streaming, r=r):
                blocks, hist = blocks_of(t, raw, s)
                return flat(ops.encoder_stage(t["x"], blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, r), hist=hist, down_hist=t.get("dhist"),
                                              res=t["res"]))
            add(f"encoder_stage-{C}-{tag}", enc, t)
        # the encoder's first stage with the first conv and its SpecBlock
        C, T0 = 64, 128 if streaming else 8
        raw, t = block_dict(C, 2, B, streaming, pack)
        wd = D(rnd(70, C, 2 * C) / C ** 0.5)
        t.update({"wav": D(synth.synth_clips(B, T0, seed=T0)), "dft": dft_p, "nyq": nyq, "pw": pw_p, "sbias": sp["sbias"], "pre_w": D(rnd(71, C, 5) * 0.5),
                  "pre_b": D(rnd(72, C) * 0.1), "w_lo": pack(wd[:, :C].contiguous()), "w_hi": pack(wd[:, C:].contiguous()),
                  "dw_w": D(rnd(73, 2 * C, 4) * 0.3), "dw_b": D(rnd(74, 2 * C) * 0.1), "res": D(rnd(75, B, 2 * C, T0 // 2) * 0.5)})
        if streaming:
            t["dhist"], t["whist"] = D(rnd(30, B, 2 * C, 2) * 0.6), D(synth.synth_clips(B, N - 1, seed=9))

        def enc0(t, raw=raw, s=streaming):
            blocks, hist = blocks_of(t, raw, s)
            spec = (t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159, -4.0, 2.8, True, 0.37)
            return flat(ops.encoder_stage0(t["wav"], spec, blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 2), res=t["res"], hist=hist,
                                           down_hist=t.get("dhist"), wav_hist=t.get("whist")))
        add(f"encoder_stage0-{tag}", enc0, t)
        # decoder stages: C = 96 / r = 2 and C = 384 / r = 5 (the expanded tap table), and the last stage with the closing conv
        for C, r, Tin, post in ((96, 2, 2, False), (384, 5, 4, False), (96, 2, 2, True)):
            raw, t = block_dict(C, 3, B, streaming, pack)
            tw, wu = D(rnd(80, 2 * C, 2 * r) * 0.3), D(rnd(81, 2 * C, C) / (2 * C) ** 0.5)
            taps = ops.up_conv_taps(tw, r)
            t.update({"xin": D(rnd(5, B, 2 * C, Tin)), "tr_w": tw if taps is None else taps, "w_lo": pack(wu[:C].contiguous()), "w_hi": pack(wu[C:].contiguous()),
                      "bias": D(rnd(82, C) * 0.1)})
            if streaming:
                t["uhist"] = D(rnd(30, B, 2 * C, 1) * 0.6)
            if post:
                t["post_w"], t["post_b"] = D(rnd(83, C, 5) * 0.2), D(rnd(84, 1) * 0.1)
                if streaming:
                    t["phist"] = D(rnd(31, B, C, 4) * 0.6)

            def dec(t, raw=raw, s=streaming, r=r, post=post):
                blocks, hist = blocks_of(t, raw, s)
                up = (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, r)
                if post:
                    return flat(ops.decoder_stage_post(t["xin"], up, blocks, (t["post_w"], t["post_b"], 0.5, 0.1122, True), hist, t.get("uhist"),
                                                       t.get("phist")))
                return flat(ops.decoder_stage(t["xin"], up, blocks, hist, t.get("uhist")))
            add(f"decoder_stage{'_post' if post else ''}-{C}-{tag}", dec, t)
    return cases


OPS_CASES = ["pw_conv", "dws_conv-k5", "dws_conv-r4", "dws_conv_stream-long", "dws_conv_stream-r5", "dws_conv_stream-k5", "up_conv-r2", "up_conv-r4-stream",
             "up_conv-r5-expanded-stream", "stft_logmag", "conv_post", "spec_block", "spec_block_conv_pre"] + [
    f"{n}-{tag}" for tag in ("stream", "offline") for n in ("resblock", "resblock_chain", "encoder_stage-128", "encoder_stage-512", "encoder_stage0",
                                                            "decoder_stage-96", "decoder_stage-384", "decoder_stage_post-96")]
_OPS_CASES = {}


@pytest.mark.parametrize("name", OPS_CASES)
def test_ops_copy_misaligned_inputs(env, name):
    """Through hilcodec_amd.ops no contiguous input raises: whatever the library would refuse is copied to a fresh allocation first, and the
    result — every cache included — is `torch.equal` to the call on aligned operands.  Every tensor operand of the wrapper is skewed in turn."""
    if not _OPS_CASES:
        _OPS_CASES.update({n: (fn, t) for n, fn, t in _ops_cases(env)})
        assert list(_OPS_CASES) == OPS_CASES
    fn, t = _OPS_CASES[name]
    assert all(v.data_ptr() % 16 == 0 for v in t.values())
    base = [o.clone() for o in fn(t)]
    for operand in t:
        for k in KS:
            got = fn({o: (skew(v, k) if o == operand else v) for o, v in t.items()})
            torch.cuda.synchronize()
            assert len(got) == len(base)
            for i, (a, b) in enumerate(zip(got, base)):
                assert torch.equal(a, b), f"ops.{name}: `{operand}` + {4 * k} B changes output {i} by {float((a - b).abs().max()):.3e}"


OUT_CASES = {"resblock-stream": ("hist_out", r"resblock: `hist2_out`"), "resblock_chain-stream": ("hist_out", r"resblock_chain: `hist_out\[3\]`"),
             "encoder_stage-128-stream": ("down_hist_out", r"encoder_stage: `dhist_out`"), "encoder_stage0-stream": ("down_hist_out", r"encoder_stage0: `dhist_out`"),
             "decoder_stage-96-stream": ("hist_out", r"decoder_stage: `hist_out\[5\]`"),
             "decoder_stage_post-96-stream": ("post_hist_out", r"decoder_stage_post: `post_hist_out`")}


@pytest.mark.parametrize("name", list(OUT_CASES))
def test_ops_name_the_misaligned_output(env, name):
    """A cache the caller owns as an output cannot be copied: a misaligned one that the kernel writes as 16-byte words raises before anything
    is launched, and the message names the wrapper, the operand and the 16-byte rule.  The same call with aligned outputs fills them."""
    ops, dev = env.ops, env.dev
    if not _OPS_CASES:
        _OPS_CASES.update({n: (fn, t) for n, fn, t in _ops_cases(env)})
    _, t = _OPS_CASES[name]
    kind, message = OUT_CASES[name]
    B = 3

    def call(last):
        """the wrapper with caller-owned outputs; `last` = the one named in the message"""
        def fresh(*shape):
            return torch.full(shape, SENT, device=dev)
        n = sum(1 for o in t if o.endswith(".w1t"))
        C = t["b0.dw1_b"].shape[0]
        raw = raw_blocks(C, n)
        blocks = [tuple(t[f"b{j}.{nm}"] for nm in BLK) + (raw[j][6], raw[j][7]) for j in range(n)]
        hist = [[t[f"b{j}.hist1"], t[f"b{j}.hist2"]] for j in range(n)]
        outs = [[fresh(B, C, 4), fresh(B, C, 4)] for _ in range(n)]
        if kind == "hist_out":
            outs[-1][1] = last(B, C, 4)
        owned = [o for pair in outs for o in pair]
        if name.startswith("resblock-"):
            ops.resblock(t["x"], *[t[f"b0.{nm}"] for nm in BLK], raw[0][6], raw[0][7], hist=hist[0], hist_out=outs[0])
        elif name.startswith("resblock_chain"):
            ops.resblock_chain(t["x"], blocks, hist, hist_out=outs)
        elif name.startswith("encoder_stage0"):
            owned.append(last(B, 2 * C, 2))
            spec = (t["dft"], t["nyq"], t["pw"], t["sbias"], t["pre_w"], t["pre_b"], 1 / 0.1122080159, -4.0, 2.8, True, 0.37)
            ops.encoder_stage0(t["wav"], spec, blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 2), res=t["res"], hist=hist, hist_out=outs,
                               down_hist=t["dhist"], down_hist_out=owned[-1], wav_hist=t["whist"])
        elif name.startswith("encoder_stage"):
            owned.append(last(B, 2 * C, 4))
            ops.encoder_stage(t["x"], blocks, (t["w_lo"], t["w_hi"], t["dw_w"], t["dw_b"], 0.77, 4), hist=hist, hist_out=outs, down_hist=t["dhist"],
                              down_hist_out=owned[-1], res=t["res"])
        elif name.startswith("decoder_stage_post"):
            owned.append(last(B, C, 4))
            ops.decoder_stage_post(t["xin"], (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, 2), blocks, (t["post_w"], t["post_b"], 0.5, 0.1122, True),
                                   hist, t["uhist"], t["phist"], hist_out=outs, post_hist_out=owned[-1])
        else:
            ops.decoder_stage(t["xin"], (t["tr_w"], t["w_lo"], t["w_hi"], t["bias"], 0.7071, 2), blocks, hist, t["uhist"], hist_out=outs)
        torch.cuda.synchronize()
        return owned
    for k in KS:
        made = []

        def skewed(*shape):
            made.append(skew(torch.full(shape, SENT, device=dev), k))
            return made[-1]
        with pytest.raises(RuntimeError, match=message + r".*16-byte"):
            call(skewed)
        torch.cuda.synchronize()
        assert len(made) == 1 and sentinel(made[0].cpu())
    owned = call(lambda *shape: torch.full(shape, SENT, device=dev))
    assert all(not sentinel(o.cpu()) for o in owned)


# ======================================================================================================================
# the per-slot float entry points (resampler, mixer, concealment gain, comfort noise, audio level, VBR: every operand class S; the
# state-slot copies: class F, decided in the kernel).
# Each has its definition as a host model in hilcodec_amd/*.py, bit for bit; the aligned call must equal that definition and every
# call with one operand skewed — float32, float64, int32, int64 and uint8 rows alike — must equal the aligned call.
# ======================================================================================================================
def _misc_cases(dev):
    """name -> (operands {name: CPU tensor}, written operand names, fn(ops, t) -> {returned: tensor}, expected {name: CPU tensor})"""
    from hilcodec_amd import audio_level, dtx, mixer, vbr, wire
    from hilcodec_amd.resample import design, device_taps, reference
    cases = {}
    g = torch.Generator().manual_seed(1)
    # polyphase resampler, 16 kHz -> 24 kHz, a ragged hop with a history
    sp = design(16000, 24000)
    t = {"x": torch.rand(2, 1, 37, generator=g) * 2 - 1, "hist": torch.randn(2, 1, sp.Q - 1, generator=g) * 0.5, "hist_out": torch.full((2, 1, sp.Q - 1), SENT),
         "taps": device_taps(sp, dev).cpu()}
    y, h = reference(t["x"], sp, t["hist"])
    cases["resample_poly"] = (t, ("hist_out",), lambda ops, t: {"y": ops.resample_poly(t["x"], t["taps"], sp.L, sp.M, hist=t["hist"], hist_out=t["hist_out"])},
                              {"y": y, "hist_out": h})
    # mixer: levels, then rooms
    B, L = 6, 70
    rng = np.random.default_rng(7)
    wav = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
    prev = rng.random(B) * np.array([1.0, 0.0, 1e4, 1.0, 1.0, 0.5])
    action = np.array([0, 0, 1, 0, 0, 0], dtype=np.int32)
    model = mixer.MixModel(B, mixer.MixConfig(1))
    model.score = torch.from_numpy(prev.copy())
    model.step(wav, [-1] * B, action)
    t = {"wav": torch.from_numpy(wav), "score": torch.from_numpy(prev.copy()), "action": torch.from_numpy(action)}
    cases["mix_levels"] = (t, ("score",), lambda ops, t: ops.mix_levels(t["wav"], t["score"], t["action"]) or {}, {"score": model.score.clone()})
    room = np.array([0, 0, 0, 1, -1, 1])
    score = rng.choice(np.array([0.0, 0.25, 1.0, 4.0]), B)
    speakers = mixer.select(room, score, 3)
    t = {"wav": torch.from_numpy(wav), "room": torch.from_numpy(room.astype(np.int32)), "score": torch.from_numpy(score),
         "mixed": torch.full((B, 1, L), SENT), "speakers": torch.full((B,), -9, dtype=torch.int32)}
    cases["mix_rooms"] = (t, ("mixed", "speakers"), lambda ops, t: ops.mix_rooms(t["wav"], t["room"], t["score"], 3, t["mixed"], t["speakers"]) or {},
                          {"mixed": torch.from_numpy(mixer.mix(wav.reshape(B, L), room, speakers)).view(B, 1, L), "speakers": torch.from_numpy(speakers)})
    # concealment gain: every ramp word of a 4-hop fade, an idle row and one out of range
    F, S = 4, 320
    G, W = wire.conceal_tables(F, S)
    ramp = torch.tensor([0, F + 1] + list(range(-F, 0)) + list(range(1, F + 1)), dtype=torch.int32)
    cw = torch.randn(len(ramp), 1, S, generator=g)
    exp = cw.clone()
    for b, r in enumerate(ramp.tolist()):
        if r != 0 and abs(r) <= F:
            a, c = (r - 1, r) if r > 0 else (-r, 0)
            exp[b] = cw[b] * (G[a] + (G[c] - G[a]) * W)              # fp32, one rounding per operation
    t = {"wav": cw, "ramp": ramp, "gains": G, "weights": W}
    cases["conceal_gain"] = (t, ("wav",), lambda ops, t: ops.conceal_gain(t["wav"], t["ramp"], t["gains"], t["weights"]) or {}, {"wav": exp})
    # comfort noise: a SID in every slot's row, then what dtx.cng_model makes of it
    K, T, B = 10, 1, 5
    stride = max(wire.packet_bytes(8, T), 1 + K)
    packets = torch.randint(0, 256, (B, stride), generator=g, dtype=torch.uint8)
    packets[:, 0] = torch.randint(0, 100, (B,), generator=g, dtype=torch.uint8)
    hold = torch.full((B,), 2, dtype=torch.int32)
    hold[3] = 0
    state = torch.zeros(B, dtx.state_words(K), dtype=torch.int32)
    e_state, e_hold, e_restore, noise = dtx.cng_model(state, packets, hold, None, K, T)
    t = {"packets": packets, "hold": hold, "state": state, "wav": torch.full((B, 1, 320 * T), 7.0), "gains": torch.from_numpy(dtx.gain_table()),
         "restore": torch.full((B,), 5, dtype=torch.int32)}
    cases["cng_synth"] = (t, ("hold", "state", "wav", "restore"),
                          lambda ops, t, K=K: ops.cng_synth(t["packets"], t["hold"], t["state"], t["wav"], t["gains"], K, None, t["restore"]) or {},
                          {"hold": e_hold, "state": e_state, "restore": e_restore,
                           "wav": torch.where(e_restore.bool()[:, None], noise, torch.full((B, 320 * T), 7.0)).view(B, 1, 320 * T)})
    # audio level of a hop
    x = (torch.rand(5, 1, 320, generator=g) * 2 - 1) * torch.tensor([1.0, 0.1, 1e-3, 0.0, 0.5]).view(5, 1, 1)
    t = {"x": x, "thr": torch.from_numpy(dtx.level_table()), "hold": torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32), "level": torch.full((5,), -9, dtype=torch.int32)}
    want = audio_level.hop_level(x.numpy()).copy()
    want[4] = 127
    cases["audio_level"] = (t, ("level",), lambda ops, t: (ops.audio_level(t["x"], t["thr"], t["level"], t["hold"]), {})[1], {"level": torch.from_numpy(want.astype(np.int32))})
    # quality-targeted bitrate: vbr.VbrModel
    B, T, n, C, K = 5, 3, 8, 128, 1024
    cb = torch.randn(n + 1, K, C, generator=g) * 0.05
    cfg = vbr.VbrConfig(0.01, n_min=2)
    z = torch.randn(B, T, C, generator=g)
    idx = torch.randint(0, K, (n, B, T), generator=g)
    n_b = torch.randint(1, n + 1, (B,), generator=g, dtype=torch.int32)
    e_n, e_D, e_idx = vbr.VbrModel(B, cfg, n, T).step(z, idx, cb, n_b, None, None)
    t = {"z": z, "indices": idx.clone(), "codebooks": cb, "n_clip": n_b}

    def vbr_fn(ops, t):
        n_eff, D = ops.vbr_select(t["z"], t["indices"], t["codebooks"], min(n, vbr.floor_stages(cfg, 0)), cfg.rho, *vbr.bucket_bits(cfg, T, 0), t["n_clip"])
        return {"n_eff": n_eff, "distortion": D}
    cases["vbr_select"] = (t, ("indices",), vbr_fn, {"n_eff": e_n, "distortion": e_D, "indices": e_idx})
    # the state-slot entry points: `move` (csrc/state.hip) copies a piece as f32x4 words where both addresses are 16-byte aligned and its length
    # is a multiple of 4, word by word otherwise — decided per piece in the kernel.  Slices of 32, 15 and 16 floats per stream: in an aligned
    # block both forms occur, in a skewed one only the second; the result is a copy either way.
    from hilcodec_amd.ops import StateLayout
    B = 5
    layout = StateLayout([(B, 8, 4), (B, 3, 5), (B, 1, 16)], 1)
    block = torch.randn(layout.total, generator=g)
    records = torch.randn(3, layout.record_len, generator=g)
    action = torch.tensor([0, -1, 2, 1, 3], dtype=torch.int32)

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
    t = {"block": block, "action": action, "records": records}
    cases["state_slots_apply"] = (t, ("block",), lambda ops, t: ops.state_slots_apply(t["block"], layout, t["action"], t["records"]) or {}, {"block": want})
    slots = torch.tensor([4, 0, 2], dtype=torch.int32)
    rec = torch.stack([torch.cat([block[part(k, b)] for k in range(len(layout.lens))]) for b in slots.tolist()])
    cases["state_slots_gather"] = ({"block": block, "slots": slots}, (), lambda ops, t: {"records": ops.state_slots_gather(t["block"], layout, t["slots"])},
                                   {"records": rec})
    dst = torch.randn(layout.total, generator=g)
    hold = torch.tensor([0, 1, 0, 2, 0], dtype=torch.int32)
    want = dst.clone()
    for k in range(len(layout.lens)):
        for b, h in enumerate(hold.tolist()):
            if h:
                want[part(k, b)] = block[part(k, b)]
    wav = torch.randn(B, 1, 37, generator=g)
    want_wav = wav.clone()
    want_wav[hold != 0] = 0
    t = {"src": block, "dst": dst, "hold": hold, "wav": wav}
    cases["state_slots_hold"] = (t, ("dst", "wav"), lambda ops, t: ops.state_slots_hold(t["src"], t["dst"], layout, t["hold"], wav=t["wav"]) or {},
                                 {"dst": want, "wav": want_wav})
    return cases


MISC = {"resample_poly": ("x", "hist", "hist_out", "taps"), "mix_levels": ("wav", "score", "action"),
        "mix_rooms": ("wav", "room", "score", "mixed", "speakers"), "conceal_gain": ("wav", "ramp", "gains", "weights"),
        "cng_synth": ("packets", "hold", "state", "wav", "gains", "restore"), "audio_level": ("x", "thr", "hold", "level"),
        "vbr_select": ("z", "indices", "codebooks", "n_clip"), "state_slots_apply": ("block", "action", "records"),
        "state_slots_gather": ("block", "slots"), "state_slots_hold": ("src", "dst", "hold", "wav")}
_MISC = {}


def _misc_run(e, name, operand=None, k=0):
    if not _MISC:
        _MISC.update(_misc_cases(e.dev))
    t0, writes, fn, expected = _MISC[name]
    assert tuple(t0) == MISC[name]
    t = {o: v.clone().to(e.dev) for o, v in t0.items()}
    if operand is not None:
        t[operand] = skew(t[operand], k)
    got = dict(fn(e.ops, t))
    torch.cuda.synchronize()
    for o, v in t0.items():
        if o not in writes:
            assert torch.equal(t[o].cpu(), v), f"{name}: the call changed its input `{o}`"
    got.update({o: t[o] for o in writes})
    return {o: v.cpu() for o, v in got.items()}, expected


@pytest.mark.parametrize("name,operand", [(n, o) for n, ops_ in MISC.items() for o in (None,) + ops_])
def test_per_slot_entry_points(env, name, operand):
    base, expected = _misc_run(env, name)
    assert set(base) == set(expected)
    for o, want in expected.items():
        assert base[o].dtype == want.dtype and torch.equal(base[o], want), f"{name}: `{o}` differs from the host model"
    if operand is None:
        return
    for k in KS:
        got, _ = _misc_run(env, name, operand, k)
        for o in base:
            assert torch.equal(got[o], base[o]), f"{name} [{operand} + {skew(_MISC[name][0][operand], k).data_ptr() % 16} B]: `{o}` differs from the aligned call"


# ======================================================================================================================
# model level
# ======================================================================================================================
def _set_stage_launches(model, on):
    for half in (model.encoder, model.decoder):
        half.exec_options.stage_launches = on


@pytest.mark.parametrize("stage_launches", [True, False])
def test_offline_model_on_a_trimmed_recording(env, stage_launches):
    """One recording trimmed at the front, `rec[:, :, k:k + 1280]` with B = 1: contiguous, 4 * k bytes off, accepted by the model — indices
    and waveform equal the same call on a copy of the slice."""
    import hilcodec_amd
    m = hilcodec_amd.HILCodec(24000, 1, **synth.model_kwargs("hil_speech")).eval()
    m.load_state_dict(synth.synth_state_dict("hil_speech", seed=7), strict=False)
    for layer in m.quantizer.layers:
        layer.initted = True
    rec = synth.synth_clips(1, 1280 + 8, seed=11).to(env.dev)
    assert rec.data_ptr() % 16 == 0
    _set_stage_launches(m, stage_launches)
    try:
        with torch.no_grad():
            for k in KS:
                x = rec[:, :, k:k + 1280]
                assert x.is_contiguous() and x.data_ptr() % 16 == 4 * k
                outs = []
                for inp in (x.clone(), x):
                    z = m.encoder(inp)
                    q, _, _, idx = m.quantizer(z, None, return_indices=True)
                    outs.append((idx, m.decoder(q)))
                torch.cuda.synchronize()
                assert outs[0][0].shape[2] == 4 and outs[0][1].shape == (1, 1, 1280)
                assert torch.equal(outs[0][0], outs[1][0]), k
                assert torch.equal(outs[0][1], outs[1][1]), (k, float((outs[0][1] - outs[1][1]).abs().max()))
    finally:
        _set_stage_launches(m, True)


@pytest.mark.parametrize("stage_launches", [True, False])
def test_streaming_model_with_every_cache_a_misaligned_view(env, stage_launches):
    """The eager streaming model keeps the caches it is handed as views: B = 3, two hops, every cache tensor replaced by `skew(cache, 1)` —
    indices, waveform and all new caches equal the run on the aligned caches."""
    from tests.hops import build_streaming
    model, mk, sd = build_streaming(seed=11)
    B = 3
    x = synth.synth_clips(B, 640, seed=5).to(env.dev)
    _set_stage_launches(model, stage_launches)
    try:
        def two_hops(prepare):
            ce, cd = model.initialize_cache(x)
            out = []
            with torch.no_grad():
                for h in range(2):
                    ce, cd = [prepare(c) for c in ce], [prepare(c) for c in cd]
                    z, ce = model.encoder(x[:, :, 320 * h: 320 * (h + 1)], *ce)
                    idx = model.quantizer(z, 8)
                    w, cd = model.decoder(model.dequantizer(idx, 8), *cd)
                    out.append((idx, w, list(ce), list(cd)))
            torch.cuda.synchronize()
            return out

        def skewed(c):
            v = skew(c, 1)
            assert v.data_ptr() % 16 == 4
            return v
        base, got = two_hops(lambda c: c), two_hops(skewed)
        for h in range(2):
            assert torch.equal(base[h][0], got[h][0]), h
            assert torch.equal(base[h][1], got[h][1]), (h, float((base[h][1] - got[h][1]).abs().max()))
            for which in (2, 3):
                assert len(base[h][which]) == len(got[h][which])
                for i, (a, b) in enumerate(zip(base[h][which], got[h][which])):
                    assert torch.equal(a, b), (h, which, i)
    finally:
        _set_stage_launches(model, True)
