"""The table of C-ABI entry-point rows and what runs one (no tests here; tests/test_gpu_alignment.py, tests/test_gpu_redzone.py and
tests/test_gpu_large.py run it, tests/test_large_cpu.py and tests/test_redzone_cpu.py read it).

One row per entry point and shape.  A row builds its operands on the device, calls the C ABI with raw pointers, and has a plain
float64 reference on the CPU (tests/alignment.py).  Its table gives the audited class of every operand — S / F: a 4-byte-aligned
view succeeds and equals the aligned call, R: it is refused (tests/test_gpu_alignment.py says what each is held to).

The tolerance of a row is the one the op's own test in tests/test_gpu_ops.py uses; it may not be below 4 x the rounding of the
reference itself (float32 against float64 on the CPU, the `FLOORS` table as measured, asserted again at run time).

`BASE` names the rows of the alignment sweep: small ragged shapes.  The edge rows behind them (`EDGE`, `row.edge`) are the same
builders at shapes that cross each kernel's tile edges; the red-zone tests run `ALL_ROWS`, base then edge.  `built`, `reference`,
`run` and `aligned` cache per row name: a row is built once and its checked aligned baseline runs once, whoever asks first."""
import ctypes
import types

import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from tests import alignment as A
from tests.alignment import skew

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
        ROWS[name] = types.SimpleNamespace(name=name, tol=tol, cls=cls, exact=exact, build=build, ref=ref, edge=False)
        return fn
    return deco


def pw_row(name, B, K, M, T, tol=1e-5):
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


pw_row("pw_conv-3x33x96x8", 3, 33, 96, 8)      # one ragged tile
pw_row("pw_conv-2x17x64x132", 2, 17, 64, 132)      # T > BN = 128, ragged last tile
pw_row("pw_conv-frame1-5x33x96x1", 5, 33, 96, 1)      # the single-frame kernel


def dwc_row(name, B, C, T, k, s, hist, res):
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


dwc_row("dw_conv-24x36-k5", 2, 24, 36, 5, 1, False, False)
dwc_row("dw_conv-24x36-k5-hist-res", 2, 24, 36, 5, 1, True, True)
dwc_row("dw_conv-16x40-k8s4-hist", 2, 16, 40, 8, 4, True, False)


def dw_convtr_row(name, B, C, T, r, seeds):
    @row(name, 5e-6, {"x": "S", "hist": "S", "w": "S", "y": "S", "hist_out": "S"})
    def _():
        def build(e):
            ins = {"x": rnd(seeds[0], B, C, T), "hist": rnd(seeds[1], B, C, 1) * 0.5, "w": rnd(seeds[2], C, 2 * r)}

            def call(p):
                return e.lib.hilc_dw_convtr(p["x"], p["hist"], p["w"], p["y"], p["hist_out"], B, C, T, r, 0.7, 1, e.stream())
            return Built(ins, {"y": (B, C, T * r), "hist_out": (B, C, 1)}, dict(ins), call)

        def ref(a):
            y, h = A.ref_dw_convtr(a["x"], a["hist"], a["w"], r, 0.7, True)
            return {"y": y, "hist_out": h}
        return build, ref


dw_convtr_row("dw_convtr-16x12-r4", 2, 16, 12, 4, (1, 2, 3))


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
def conv_post_row(name, B, C, T, seeds):
    @row(name, 2e-6, {"x": "F", "hist": "F", "w": "S", "bias": "S", "y": "S", "hist_out": "S"}, exact=("hist_out",))
    def _():
        k = 5

        def build(e):
            ins = {"x": rnd(seeds[0], B, C, T), "hist": rnd(seeds[1], B, C, 4) * 0.6, "w": rnd(seeds[2], C, k) / 20, "bias": rnd(seeds[3], 1) * 0.1}

            def call(p):
                return e.lib.hilc_conv_post(p["x"], p["hist"], p["w"], p["bias"], p["y"], p["hist_out"], B, C, T, k, 0.707, 1, 0.1122080159, 1,
                                            e.stream())
            return Built(ins, {"y": (B, 1, T), "hist_out": (B, C, 4)}, dict(ins), call)

        def ref(a):
            y, h = A.ref_conv_post(a["x"], a["hist"], a["w"], a["bias"], 0.707, True, 0.1122080159, True)
            return {"y": y, "hist_out": h}
        return build, ref


conv_post_row("conv_post-24x36-k5-hist", 2, 24, 36, (9, 8, 3, 4))


def dws_row(name, B, K, M, T, r, res):
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


dws_row("dws_conv-k5-2x33x96x36", 2, 33, 96, 36, 1, False)
dws_row("dws_conv-k5-2x33x96x36-res", 2, 33, 96, 36, 1, True)
dws_row("dws_conv-k5-1x16x128x260", 1, 16, 128, 260, 1, False)
dws_row("dws_conv-k5-1x16x128x260-res", 1, 16, 128, 260, 1, True)
dws_row("dws_conv-r2-2x16x32x64", 2, 16, 32, 64, 2, False)
dws_row("dws_conv-r4-2x16x32x64", 2, 16, 32, 64, 4, False)


def dwss_row(name, B, K, M, T, k, r, cls, res=True):
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
dwss_row("dws_conv_stream-k5-5x32x32x8", 5, 32, 32, 8, 5, 1,
      {"x": "F", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "F", "hist_out": "F", "res": "F", "y": "F"})
dwss_row("dws_conv_stream-r5-5x16x32x40", 5, 16, 32, 40, 10, 5,
      {"x": "F", "wt": "R", "dw_w": "R", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})
dwss_row("dws_conv_stream-frame1-5x32x32x1", 5, 32, 32, 1, 5, 1,
      {"x": "S", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})
# T > 128: no scalar loader (x refused); DwStrideFlatEpilogue reads hist and res and writes y and hist_out word by word
# (gemm_epilogues.h: `hist[(bq * M + m) * r + j]`, `y[yo] = ... res[yo]`, `hist_out[...] = smem[...]`; its f32x4 reads are LDS)
dwss_row("dws_conv_stream-r4-3x16x32x160", 3, 16, 32, 160, 8, 4,
      {"x": "R", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "S", "hist_out": "S", "res": "S", "y": "S"})


def up_row(name, entry, B, K, M, Tin, r):
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
up_row("up_conv-2x32x16x6-r2", "hilc_up_conv", 2, 32, 16, 6, 2)
up_row("up_conv_stream-2x32x16x4-r4", "hilc_up_conv_stream", 2, 32, 16, 4, 4)
up_row("up_conv_expanded-2x48x24x4-r5", "hilc_up_conv_expanded", 2, 48, 24, 4, 5)


def stft_row(name, B, T, n_fft, hop, hist):
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


stft_row("stft_logmag-n16-T64-hist", 2, 64, 16, 1, True)      # the generic loader
stft_row("stft_logmag-n16-T512-seg", 1, 512, 16, 1, False)      # per-clip LDS segments (Tf >= 512)


def spec_row(name, pre, B=2, T=128):
    cls = {"wav": "S", "hist": "S", "dft_packed": "R", "nyq_sin": "S", "pw_packed": "R", "bias": "S", "y": "R"}
    cls.update({"pre_w": "S", "pre_b": "S"} if pre else {"x": "R"})

    @row(name, 2e-4, cls)
    def _():
        N = 64

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
            return {"y": A.ref_spec_block(a["wav"], a["hist"], a["basis_t"], a["wt"], a["bias"], x, N, 1, -4.0, 2.8, 1, 0.37)}
        return build, ref


spec_row("spec_block-n64-T128", False)
spec_row("spec_block_conv_pre-n64-T128", True)


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


ref_blocks = A.ref_blocks          # (the compositions live in tests/alignment.py: tests/large_families.py shares them)


def resblock_row(name, B, C, T, streaming):
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


resblock_row("resblock-64x8x2", 2, 64, 8, False)
resblock_row("resblock_stream-64x8x3", 3, 64, 8, True)


def chain_row(name, B, C, T, n, streaming):
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


chain_row("resblock_chain-64x8x2-offline", 2, 64, 8, 2, False)
chain_row("resblock_chain-64x8x3-stream", 3, 64, 8, 2, True)


def enc_row(name, B, C, T, r, n, streaming, stage0=False):
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
enc_row("encoder_stage-128x8-r4-offline", 2, 128, 8, 4, 2, False)
enc_row("encoder_stage-128x8-r4-stream", 3, 128, 8, 4, 2, True)
enc_row("encoder_stage-512x8-r8-offline", 2, 512, 8, 8, 2, False)
enc_row("encoder_stage-512x8-r8-stream", 3, 512, 8, 8, 2, True)
enc_row("encoder_stage0-T8-offline", 2, 64, 8, 2, 2, False, stage0=True)
enc_row("encoder_stage0-T128-stream", 3, 64, 128, 2, 2, True, stage0=True)


def dec_row(name, B, C, Tin, r, n, streaming, post=False):
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
dec_row("decoder_stage-96-r2-Tin2-offline", 2, 96, 2, 2, 3, False)
dec_row("decoder_stage-96-r2-Tin2-stream", 3, 96, 2, 2, 3, True)
dec_row("decoder_stage-384-r5-Tin4-offline", 2, 384, 4, 5, 3, False)
dec_row("decoder_stage-384-r5-Tin4-stream", 3, 384, 4, 5, 3, True)
dec_row("decoder_stage_post-96-r2-Tin2-offline", 2, 96, 2, 2, 3, False, post=True)
dec_row("decoder_stage_post-96-r2-Tin2-stream", 3, 96, 2, 2, 3, True, post=True)


# ---- the remaining float entry points: every operand is read and written word by word (class S) --------------------------------------
def l2norm_row(name, B, C, T, seed):
    @row(name, 1e-6, {"x": "S", "y": "S"})
    def _():
        def build(e):
            ins = {"x": rnd(seed, B, C, T)}
            return Built(ins, {"y": (B, T, C)}, dict(ins), lambda p: e.lib.hilc_l2norm(p["x"], p["y"], B, C, T, 1e-12, 1.0, 1, e.stream()))
        return build, lambda a: {"y": A.ref_l2norm(a["x"], 1e-12, 1.0, True)}


l2norm_row("l2norm-3x128x5", 3, 128, 5, 1)


def tail_row(name, B, C, seeds):
    """the last 9 samples of a 10-sample history followed by 7 new ones"""
    @row(name, 0.0, {"x": "S", "hist": "S", "out": "S"})
    def _():
        def build(e):
            ins = {"x": rnd(seeds[0], B, C, 7), "hist": rnd(seeds[1], B, C, 10)}
            return Built(ins, {"out": (B, C, 9)}, dict(ins), lambda p: e.lib.hilc_tail(p["x"], p["hist"], p["out"], B * C, 7, 9, 10, e.stream()))
        return build, lambda a: {"out": torch.cat([a["hist"], a["x"]], dim=2)[:, :, -9:]}


tail_row("tail-2x3x7-pad9", 2, 3, (1, 2))


def rvq_tables(Nq, K, C):
    cb = rnd(5, Nq, K, C) * 0.3
    return cb, cb.transpose(1, 2).contiguous(), cb.pow(2).sum(-1)


def rvq_enc_row(name, B, T):
    # 8 192 frames and more: the matrix-pipe form reads codebooks_t and norms as 16-byte words and falls back to the VALU form (csrc/rvq.hip)
    @row(name, 1e-5, {"z": "S", "codebooks": "S", "codebooks_t": "F", "norms": "F", "indices": "S", "q": "S", "frame_err": "S"})
    def _():
        Nq, K, C, n = 3, 1024, 128, 2

        def build(e):
            cb, cbt, nrm = rvq_tables(Nq, K, C)
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


rvq_enc_row("rvq_encode-valu-2x128x9", 2, 9)
rvq_enc_row("rvq_encode-mfma-8x128x1024", 8, 1024)


def rvq_dec_row(name, B, T, seed):
    @row(name, 1e-6, {"indices": "S", "codebooks": "S", "q": "S"})
    def _():
        Nq, K, C, n = 3, 1024, 128, 3

        def build(e):
            cb = rvq_tables(Nq, K, C)[0]
            idx = torch.from_numpy(np.random.RandomState(seed).randint(0, K, size=(B, n, T))).to(torch.int64)
            ins = {"indices": idx, "codebooks": cb}
            return Built(ins, {"q": (B, C, T)}, dict(ins),
                         lambda p: e.lib.hilc_rvq_decode(p["indices"], p["codebooks"], p["q"], B, C, T, K, Nq, n, 0, 0, e.stream()))

        def ref(a):
            q = sum(a["codebooks"][s][a["indices"][:, s]] for s in range(n))          # [B, T, C]
            return {"q": q.transpose(1, 2)}
        return build, ref


rvq_dec_row("rvq_decode-2x128x9", 2, 9, 3)

BASE = list(ROWS)          # the rows of the alignment sweep


# ======================================================================================================================
# rows that cross the tile edges (same builders, same requirements: a float64 reference, tolerance >= 4 x its measured floor)
# ======================================================================================================================
# entry point(s): kernel, its tiles -> the rows that cross each tiled dimension and end ragged there ("BASE": one of the base rows)
#   pw_conv, dws_conv, dws_conv_stream, up_conv, up_conv_stream, up_conv_expanded: the GEMM cores (gemm_core.h, gemm_lin.h), BN = 128 columns
#     x BM = 32 * MB rows (MB = 1..4 picked per launch), K slices of BK
#       -> pw_conv-2x17x36x132 (M = 32 + 4, 264 columns = 2 tiles + 8, K = 17), pw_conv-1x16x132x8 (M = 128 + 4: ragged whatever MB is),
#          dws_conv-k5-1x16x128x260 (BASE: 2 tiles + 4), up_conv-3x32x36x22-r2 / up_conv_stream-3x32x36x11-r4 (132 columns, M = 32 + 4),
#          up_conv_expanded-3x48x24x12-r5 (180 columns), dws_conv_stream-k5-9x32x36x24 (216 columns of whole clips, M = 32 + 4),
#          dws_conv_stream-r5-5x16x32x40 (BASE: 200 columns), dws_conv_stream-r4-3x16x32x160 (BASE: per-clip tiles, T = 128 + 32);
#          pw_conv / dws_conv_stream with T = 1 (frame1.hip): 32 streams per workgroup -> the frame1 rows of BASE (5 streams: one ragged
#          workgroup; more than 32 streams only repeats it)
#   stft_logmag: the same cores; the generic loader walks B * Tf flat columns, the segment form (no hist, Tf >= 512) per-clip tiles of 128
#       -> stft_logmag-n16-T132-hist (264 columns = 2 tiles + 8), stft_logmag-n16-T516-seg (4 tiles + 4); M = n_fft + 2 = 18 rows: ragged
#   spec_block, spec_block_conv_pre (spec.hip): TF = 128 frames per tile; flat over B * Tf for 32 <= Tf < 512 (spec_block only), else per clip
#       -> spec_block-n64-T132 (flat: 264 frames = 2 tiles + 8), spec_block-n64-T516 (per clip: 4 tiles + 4),
#          spec_block_conv_pre-n64-T132 (per clip: 1 tile + 4)
#   dw_conv, conv_pre (dwconv.hip): flat, 256 outputs (k = 5, T % 4 == 0: 256 groups of 4) per workgroup
#       -> every such row of BASE ends in a ragged workgroup after a full one (432 groups; 320 outputs); dw_conv-16x38-k8s4-hist: T = 38 is
#          no multiple of the stride 4
#   dw_convtr: flat, 256 outputs per workgroup -> dw_convtr-16x13-r4 (1664 = 6 x 256 + 128; the row of BASE is 6 x 256 exactly)
#   tail, and every hist_out of dw_conv / dw_convtr / conv_post (hist_out_kernel): flat, 256 elements per workgroup -> tail-2x15x7-pad9 (270)
#   conv_post: 256 samples of one clip per workgroup -> conv_post-8x260-k5-hist (T = 256 + 4)
#   l2norm: 64 frames per workgroup, 16 channels per round -> l2norm-5x36x13 (65 frames, C = 32 + 4)
#   rvq_encode, rvq_encode_mixed (rvq.hip): VALU form 16 frames per workgroup -> rvq_encode-valu-2x128x9 (BASE: 18 frames), rvq_encode_mixed-3x128x9
#     (27); matrix-pipe form (8192 frames and more) 32 frames per workgroup -> rvq_encode-mfma-8x128x1025 (8200 = 256 x 32 + 8)
#   rvq_decode, rvq_decode_mixed: flat, 256 elements per workgroup -> rvq_decode-3x128x3 (1152 = 4 x 256 + 128; the row of BASE is 9 x 256
#     exactly), rvq_decode_mixed-3x128x9 (3456 = 13 x 256 + 128)
#   resblock, resblock_balanced, resblock_chain, encoder_stage, encoder_stage0, decoder_stage, decoder_stage_post: the stage kernel
#     (resblock_cfg.h).  C <= 192: NCOL = 128 columns per tile, a lane owns a 4-column group; offline: carries from tile to tile
#       -> resblock-64x132x2, resblock_balanced-64x132x2-offline, resblock_chain-64x132x2-offline, encoder_stage-128x132-r4-offline,
#          encoder_stage0-T132-offline, decoder_stage-96-r2-Tin66-offline, decoder_stage_post-96-r2-Tin66-offline (T = 128 + 4)
#     streaming, one block: TO = 120 columns of the flat column space (8-column halo)
#       -> resblock_stream-64x160x5, resblock_balanced-64x160x5-stream (800 columns = 6 tiles + 80)
#     streaming, chain / stage: runs of whole streams, T = 160: 5 tiles = 4 streams
#       -> resblock_chain-64x160x5-stream, encoder_stage-128x160-r4-stream, encoder_stage0-T160-stream, decoder_stage-96-r2-Tin80-stream,
#          decoder_stage_post-96-r2-Tin80-stream (5 streams = one run + 1)
#     C >= 256: 32- / 64-column tiles of whole streams -> encoder_stage-512x8-r8-*, decoder_stage-384-r5-Tin4-* (BASE: 2 / 3 streams of 8 /
#       20 columns, a ragged tile; a second tile only repeats the first, whole streams never straddle one)
#   the channel dimension of the stage kernel is not tiled (C is a template parameter), nor is K of the RVQ (1024) or n_fft of spec_block
# resblock_balanced and the two *_mixed RVQ entry points are rows the base table does not have (the caller's two scheduler words; an
# int32 row of per-clip stage counts, unused index rows hold -1)
def rvq_mixed_row(name, encode):
    """the mixed-bitrate forms: clip b uses its first n_per_clip[b] stages (int32 [B] on the device)"""
    B, T, Nq, K, C, n = 3, 9, 3, 1024, 128, 3
    n_b = [2, 3, 1]
    cls = {"z": "S", "codebooks": "S", "codebooks_t": "F", "norms": "F", "n_per_clip": "S", "indices": "S", "q": "S", "frame_err": "S"} if encode else \
        {"indices": "S", "codebooks": "S", "n_per_clip": "S", "q": "S"}

    @row(name, 1e-6, cls)
    def _():
        def build(e):
            cb, cbt, nrm = rvq_tables(Nq, K, C)
            clip = torch.tensor(n_b, dtype=torch.int32)
            if encode:
                ins = {"z": rnd(7, B, C, T) * 0.4, "codebooks": cb, "codebooks_t": cbt, "norms": nrm, "n_per_clip": clip}

                def call(p):
                    return e.lib.hilc_rvq_encode_mixed(p["z"], p["codebooks"], p["codebooks_t"], p["norms"], p["n_per_clip"], p["indices"], p["q"],
                                                       p["frame_err"], B, C, T, K, Nq, n, 0, 0, 0, e.stream())
                return Built(ins, {"indices": ((B, n, T), torch.int64), "q": (B, C, T), "frame_err": (B * T,)}, dict(ins), call)
            idx = torch.from_numpy(np.random.RandomState(4).randint(0, K, size=(B, n, T))).to(torch.int64)
            for b, nb in enumerate(n_b):
                idx[b, nb:] = -1                                  # what hilc_rvq_encode_mixed writes there: ignored
            ins = {"indices": idx, "codebooks": cb, "n_per_clip": clip}
            return Built(ins, {"q": (B, C, T)}, dict(ins),
                         lambda p: e.lib.hilc_rvq_decode_mixed(p["indices"], p["codebooks"], p["n_per_clip"], p["q"], B, C, T, K, Nq, n, 0, 0, e.stream()))

        def ref(a):
            if encode:
                return {}                                         # like the RVQ encode rows of the alignment sweep: equality with the aligned call
            q = torch.stack([sum(a["codebooks"][s][a["indices"][b, s]] for s in range(n_b[b])) for b in range(B)])       # [B, T, C]
            return {"q": q.transpose(1, 2)}
        return build, ref


def balanced_row(name, B, C, T, streaming):
    """hilc_resblock / hilc_resblock_stream with the caller-owned tile scheduler: `sched`, two ints that are zero at the launch and zero
    again at its end — an input as far as a row is concerned (the sweep asserts it is unchanged), and one the kernel writes between"""
    cls = {"x": "R", "y": "R", "sched": "S"}
    cls.update(block_cls(1, streaming))

    @row(name, 2e-5, cls)
    def _():
        raw = raw_blocks(C, 1)

        def build(e):
            ins, outs, aux = {"x": rnd(C + T, B, C, T), "sched": torch.zeros(2, dtype=torch.int32)}, {"y": (B, C, T)}, {}
            aux["x"] = ins["x"]
            block_operands(e, raw, B, C, streaming, e.ops.resblock_pack, ins, outs, aux)

            def call(p):
                w = [p[f"b0.{nm}"] for nm in BLK]
                caches = [p.get(f"b0.{nm}") for nm in ("hist1", "hist2", "hist1_out", "hist2_out")]
                return e.lib.hilc_resblock_balanced(p["x"], *w, *caches, p["y"], p["sched"], int(streaming), B, C, T, float(raw[0][6]),
                                                    float(raw[0][7]), e.stream())
            return Built(ins, outs, aux, call)

        def ref(a):
            out = {}
            out["y"] = ref_blocks(a, a["x"], streaming, out)
            return out
        return build, ref


pw_row("pw_conv-2x17x36x132", 2, 17, 36, 132)
pw_row("pw_conv-1x16x132x8", 1, 16, 132, 8)
dwc_row("dw_conv-16x38-k8s4-hist", 2, 16, 38, 8, 4, True, False)
up_row("up_conv-3x32x36x22-r2", "hilc_up_conv", 3, 32, 36, 22, 2)
up_row("up_conv_stream-3x32x36x11-r4", "hilc_up_conv_stream", 3, 32, 36, 11, 4)
up_row("up_conv_expanded-3x48x24x12-r5", "hilc_up_conv_expanded", 3, 48, 24, 12, 5)
dwss_row("dws_conv_stream-k5-9x32x36x24", 9, 32, 36, 24, 5, 1,
         {"x": "F", "wt": "R", "dw_w": "S", "dw_b": "S", "hist": "F", "hist_out": "F", "res": "F", "y": "F"})
resblock_row("resblock-64x132x2", 2, 64, 132, False)
resblock_row("resblock_stream-64x160x5", 5, 64, 160, True)
chain_row("resblock_chain-64x132x2-offline", 2, 64, 132, 2, False)
chain_row("resblock_chain-64x160x5-stream", 5, 64, 160, 2, True)
enc_row("encoder_stage-128x132-r4-offline", 2, 128, 132, 4, 2, False)
enc_row("encoder_stage-128x160-r4-stream", 5, 128, 160, 4, 2, True)
dec_row("decoder_stage-96-r2-Tin66-offline", 2, 96, 66, 2, 3, False)
dec_row("decoder_stage-96-r2-Tin80-stream", 5, 96, 80, 2, 3, True)
enc_row("encoder_stage0-T132-offline", 2, 64, 132, 2, 2, False, stage0=True)
enc_row("encoder_stage0-T160-stream", 5, 64, 160, 2, 2, True, stage0=True)
dec_row("decoder_stage_post-96-r2-Tin66-offline", 2, 96, 66, 2, 3, False, post=True)
dec_row("decoder_stage_post-96-r2-Tin80-stream", 5, 96, 80, 2, 3, True, post=True)
stft_row("stft_logmag-n16-T132-hist", 2, 132, 16, 1, True)
stft_row("stft_logmag-n16-T516-seg", 1, 516, 16, 1, False)
rvq_enc_row("rvq_encode-mfma-8x128x1025", 8, 1025)
spec_row("spec_block-n64-T132", False, 2, 132)
spec_row("spec_block-n64-T516", False, 1, 516)
spec_row("spec_block_conv_pre-n64-T132", True, 2, 132)
dw_convtr_row("dw_convtr-16x13-r4", 2, 16, 13, 4, (31, 32, 33))
tail_row("tail-2x15x7-pad9", 2, 15, (41, 42))
rvq_dec_row("rvq_decode-3x128x3", 3, 3, 6)
conv_post_row("conv_post-8x260-k5-hist", 2, 8, 260, (19, 18, 13, 14))
l2norm_row("l2norm-5x36x13", 5, 36, 13, 21)
balanced_row("resblock_balanced-64x132x2-offline", 2, 64, 132, False)
balanced_row("resblock_balanced-64x160x5-stream", 5, 64, 160, True)
rvq_mixed_row("rvq_encode_mixed-3x128x9", True)
rvq_mixed_row("rvq_decode_mixed-3x128x9", False)

ALL_ROWS = list(ROWS)          # base, then edge
EDGE = ALL_ROWS[len(BASE):]
for _name in EDGE:
    ROWS[_name].edge = True

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
    # the edge rows
    "pw_conv-2x17x36x132": 2.68e-07,
    "pw_conv-1x16x132x8": 2.82e-07,
    "dw_conv-16x38-k8s4-hist": 1.72e-07,
    "up_conv-3x32x36x22-r2": 1.99e-07,
    "up_conv_stream-3x32x36x11-r4": 1.92e-07,
    "up_conv_expanded-3x48x24x12-r5": 3.74e-07,
    "dws_conv_stream-k5-9x32x36x24": 5.17e-07,
    "resblock-64x132x2": 4.26e-07,
    "resblock_stream-64x160x5": 8.46e-07,
    "resblock_chain-64x132x2-offline": 5.86e-07,
    "resblock_chain-64x160x5-stream": 8.86e-07,
    "encoder_stage-128x132-r4-offline": 8.55e-07,
    "encoder_stage-128x160-r4-stream": 1.10e-06,
    "decoder_stage-96-r2-Tin66-offline": 7.41e-07,
    "decoder_stage-96-r2-Tin80-stream": 8.20e-07,
    "conv_post-8x260-k5-hist": 7.84e-08,
    "l2norm-5x36x13": 4.45e-08,
    "resblock_balanced-64x132x2-offline": 4.26e-07,          # the operands and the reference of resblock-64x132x2 / resblock_stream-64x160x5
    "resblock_balanced-64x160x5-stream": 8.46e-07,
    "rvq_encode_mixed-3x128x9": 0.0,         # integers and equality, like the RVQ encode rows of the alignment sweep
    "rvq_decode_mixed-3x128x9": 8.94e-08,
    "encoder_stage0-T132-offline": 1.07e-06,
    "encoder_stage0-T160-stream": 1.41e-06,
    "decoder_stage_post-96-r2-Tin66-offline": 9.97e-08,
    "decoder_stage_post-96-r2-Tin80-stream": 5.78e-07,
    "stft_logmag-n16-T132-hist": 1.49e-07,
    "stft_logmag-n16-T516-seg": 1.31e-07,
    "rvq_encode-mfma-8x128x1025": 0.0,
    "spec_block-n64-T132": 2.26e-06,
    "spec_block-n64-T516": 4.07e-06,
    "spec_block_conv_pre-n64-T132": 2.28e-06,
    "dw_convtr-16x13-r4": 2.92e-07,
    "tail-2x15x7-pad9": 0.0,
    "rvq_decode-3x128x3": 8.94e-08,
}
EDGE_FLOORS = {name: FLOORS[name] for name in EDGE}

def entry_of(name):
    """the entry point a row calls: the row's name up to its first `-`"""
    return name.split("-")[0]


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
