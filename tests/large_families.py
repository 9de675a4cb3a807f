"""The operand families of the large-tensor rows (no tests here; tests/test_gpu_large.py launches them on the device,
tests/test_large_cpu.py runs each at a small size with its float32 reference as the "kernel").

A family builds, for one row of `tests/large.py: CASES` at one size, the periodic operands (`Operands`), the call of the C entry
point, the float64 reference of three periods, the predicate of the fast form, the `hilcodec_amd.ops` mirror and the fall-back the
engine takes behind a refusal."""
import types
from fractions import Fraction

import numpy as np
import torch

from hilcodec_amd import synth
from tests import alignment as A
from tests import large as L
from tests.entry_rows import BLK, RS, block_structs, cast, raw_blocks, rnd, void

F1 = Fraction(1)


class Operands:
    """the operands of one case at one size: periodic tensors on the device, their three-period twins on the CPU for the reference"""

    def __init__(self, e, c, d):
        self.e, self.c, self.d = e, c, d
        self.B, self.T, self.P = d["B"], d["T"], c.P
        self.Lr = self.T if self.T <= 3 * self.P else 3 * self.P + self.T % self.P
        self.ins, self.outs, self.aux, self.rates, self.dev, self.full = {}, {}, {}, {}, {}, {}

    def _n(self, n, rate):
        v = n * rate
        assert v.denominator == 1, (n, rate)
        return int(v)

    def per(self, name, seed, rows, rate=F1, scale=1.0, aux=None, pat=None):
        pat = L.pattern(seed, rows, self._n(self.P, rate), scale) if pat is None else pat
        self.ins[name] = L.periodic(pat, self._n(self.T, rate), self.B, self.e.dev)
        self.aux[aux or name] = L.periodic(pat, self._n(self.Lr, rate), L.NPAT)
        self.full[aux or name] = self.ins[name]

    def full_aux(self):
        """what the reference takes, with every clip at its full length: the reference itself as the "kernel" (tests/test_large_cpu.py)"""
        return {**self.aux, **self.full}

    def wav(self, name, seed, aux=None):
        self.per(name, seed, 1, aux=aux, pat=synth.synth_clips(L.NPAT, self.P, seed=seed))

    def hist(self, name, seed, rows, n, scale=0.7, aux=None, wav=False):
        h = synth.synth_clips(L.NPAT, n, seed=seed) if wav else rnd(seed, L.NPAT, rows, n) * scale
        self.ins[name] = h.to(self.e.dev)[torch.arange(self.B, device=self.e.dev) % L.NPAT].contiguous()
        self.aux[aux or name] = h
        self.full[aux or name] = self.ins[name]

    def weight(self, name, t, aux=None, dev=None):
        """t: the CPU tensor the reference uses; dev: what the launch takes in its place (a packed layout)"""
        self.dev[name] = t.to(self.e.dev)
        self.ins[name] = self.dev[name] if dev is None else dev(self.dev[name])
        self.aux[aux or name] = t

    def out(self, name, shape, rate=None, dtype=torch.float32):
        self.outs[name] = (tuple(shape), dtype)
        if rate is not None:
            self.rates[name] = rate


def blocks(o, C, n, streaming, pack):
    raw = raw_blocks(C, n)
    o.aux["blocks"], o.aux["caches"], o.full["caches"] = [tuple(b) for b in raw], [], []
    for j, b in enumerate(raw):
        for nm, t in zip(BLK, b[:6]):
            o.weight(f"b{j}.{nm}", t, dev=pack if nm in ("w1t", "w2t") else None)
        if streaming:
            o.hist(f"b{j}.hist1", 7 + j, C, 4)
            o.hist(f"b{j}.hist2", 8 + j, C, 4)
            o.aux["caches"].append((o.aux.pop(f"b{j}.hist1"), o.aux.pop(f"b{j}.hist2")))
            o.full["caches"].append((o.full.pop(f"b{j}.hist1"), o.full.pop(f"b{j}.hist2")))
            o.out(f"b{j}.hist1_out", (o.B, C, 4))
            o.out(f"b{j}.hist2_out", (o.B, C, 4))
    return raw


def take(o, name):
    """an input the fall-back consumes: the operand set lets go of it, so that it is freed as soon as the fall-back has read it"""
    o.full = {k: v for k, v in o.full.items() if v is not o.ins[name]}
    return o.ins.pop(name)


def fb_blocks(e, o, xs, raw, streaming):
    """the lowest rung of the engine's ladder for a residual block: pointwise GEMM + depthwise launch, twice (engine._resblock).
    xs: [x] — popped, so that nothing but this function holds the blocks' input (three tensors of its size are alive at a time)"""
    ops, got = e.ops, {}
    x = xs.pop()
    for j, b in enumerate(raw):
        w = {nm: o.dev[f"b{j}.{nm}"] for nm in BLK}
        h1, h2 = (o.ins[f"b{j}.hist1"], o.ins[f"b{j}.hist2"]) if streaming else (None, None)
        h = ops.pw_conv(x, w["w1t"], in_scale=float(b[6]), in_elu=True)
        g, c1 = ops.dw_conv(h, w["dw1_w"], w["dw1_b"], hist=h1, want_hist=True, out_elu=True)
        del h
        h = ops.pw_conv(g, w["w2t"])
        del g
        x, c2 = ops.dw_conv(h, w["dw2_w"], w["dw2_b"], res=x, hist=h2, want_hist=True, out_scale=float(b[7]))
        del h
        if streaming:
            got[f"b{j}.hist1_out"], got[f"b{j}.hist2_out"] = c1, c2
    return x, got


# ======================================================================================================================
# the families: build(e, c, d) -> namespace(o = Operands, call(p) -> rc, ref(aux) -> {output: [NPAT, ...]}, fast() -> (bool, str),
#                                          mirror() -> bool or None, fallback() -> {output: tensor} or None)
# ======================================================================================================================
def fam_pw(e, c, d):
    B, K, M, T = d["B"], d["K"], d["M"], d["T"]
    res = bool(c.kw.get("res"))
    o = Operands(e, c, d)
    o.per("x", 100 + K, K)
    o.weight("wt", rnd(K + M, K, M) / K ** 0.5)
    o.weight("bias", rnd(M, M) * 0.1)
    if res:
        o.per("res", 3, M)
    o.out("y", (B, M, T), F1)

    def call(p):
        return e.lib.hilc_pw_conv(p["x"], p["wt"], p["bias"], p.get("res"), p["y"], B, K, M, T, 0.77, 1, 0.61, e.stream())

    def ref(a):
        return {"y": A.ref_pw_conv(a["x"], a["wt"], a["bias"], a.get("res"), 0.77, True, 0.61)}
    lin = L.lin_ok(B, K, T) and T % 4 == 0
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (lin, "linear core" if lin else "generic core"), mirror=lambda: None,
                                 fallback=lambda: {"y": e.ops.pw_conv(o.ins["x"], o.ins["wt"], o.ins["bias"], o.ins.get("res"), 0.77, True, 0.61)})


def fam_dws(e, c, d):
    B, K, M, T, r = d["B"], d["K"], d["M"], d["T"], d["r"]
    k5 = r == 1
    k, To = (5 if k5 else 2 * r), -(-T // r)
    o = Operands(e, c, d)
    o.per("x", 200 + K + r, K)
    o.weight("wt", rnd(K + M, K, M) / K ** 0.5)
    o.weight("dw_w", rnd(M + k, M, k) * 0.5)
    o.weight("dw_b", rnd(M, M) * 0.1)
    o.out("y", (B, M, To), Fraction(1, r))
    os_ = 0.37 if k5 else 1.0

    def call(p):
        return e.lib.hilc_dws_conv(p["x"], p["wt"], p["dw_w"], p["dw_b"], None, p["y"], B, K, M, T, k, r, 0.86, 1, os_, 0, e.stream())

    def ref(a):
        return {"y": A.ref_dws(a["x"], a["wt"], a["dw_w"], a["dw_b"], None, None, r, 0.86, True, os_, False)[0]}
    lin = L.lin_ok(B, K, T) and T % 4 == 0 and T >= 4
    form = ("linear core, " + ("wave-row tiles" if k5 and e.lib.hilc_dws_conv_wave_row(B, M, T, 0) else "column-block tiles")) if lin else "generic core"
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (lin, form), mirror=lambda: None,
                                 fallback=lambda: {"y": e.ops.dws_conv(o.ins["x"], o.ins["wt"], o.ins["dw_w"], o.ins["dw_b"], None, r, 0.86, True, os_, False)})


def fam_dwss(e, c, d):
    """hilc_dws_conv_stream on a hop longer than one tile (T > 128, k = 2 r): flat tiles, cache in, cache out, shortcut"""
    B, K, M, T, r = d["B"], d["K"], d["M"], d["T"], d["r"]
    k, pad = 2 * r, r
    o = Operands(e, c, d)
    o.per("x", 600 + K + r, K)
    o.weight("wt", rnd(K + M, K, M) / K ** 0.5)
    o.weight("dw_w", rnd(M + k, M, k) * 0.5)
    o.weight("dw_b", rnd(M, M) * 0.1)
    o.hist("hist", 12, M, pad)
    o.per("res", 11, M, Fraction(1, r))
    o.out("y", (B, M, T // r), Fraction(1, r))
    o.out("hist_out", (B, M, pad))

    def call(p):
        return e.lib.hilc_dws_conv_stream(p["x"], p["wt"], p["dw_w"], p["dw_b"], p["hist"], p["hist_out"], p["res"], p["y"], B, K, M, T, k, r, 0.86, 1,
                                          1.0, 0, e.stream())

    def ref(a):
        y, h = A.ref_dws(a["x"], a["wt"], a["dw_w"], a["dw_b"], a["hist"], a["res"], r, 0.86, True, 1.0, False)
        return {"y": y, "hist_out": h}

    def fallback():          # engine._dws_layer, not fused: pointwise GEMM + cached depthwise launch
        h = e.ops.pw_conv(take(o, "x"), o.ins["wt"], in_scale=0.86, in_elu=True)
        y, hc = e.ops.dw_conv(h, o.ins["dw_w"], o.ins["dw_b"], res=o.ins["res"], stride=r, hist=o.ins["hist"], want_hist=True)
        return {"y": y, "hist_out": hc}
    mirror = lambda: e.ops.dws_conv_stream_supported(T, k, r, True, B, M, K)          # noqa: E731
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (mirror() and L.lin_ok(B, K, T), "linear core, flat tiles"), mirror=mirror,
                                 fallback=fallback)


def fam_l2(e, c, d):
    B, C, T = d["B"], d["C"], d["T"]
    o = Operands(e, c, d)
    o.per("x", 700 + C, C)
    o.out("y", (B, C, T), F1)
    return types.SimpleNamespace(o=o, call=lambda p: e.lib.hilc_l2norm(p["x"], p["y"], B, C, T, 1e-12, 1.0, 0, e.stream()),
                                 ref=lambda a: {"y": A.ref_l2norm(a["x"], 1e-12, 1.0, False)}, fast=lambda: (True, "the one kernel"),
                                 mirror=lambda: None, fallback=lambda: None)


def fam_up(e, c, d):
    B, K, M, Tin, r = d["B"], d["K"], d["M"], d["T"], d["r"]
    o = Operands(e, c, d)
    o.per("x", 100 + K, K)
    o.weight("tr_w", rnd(80, K, 2 * r) * 0.3)
    o.weight("wt", rnd(81, K, M) / K ** 0.5)
    o.weight("bias", rnd(82, M) * 0.1)
    o.out("y", (B, M, Tin * r), Fraction(r))

    def call(p):
        return e.lib.hilc_up_conv(p["x"], p["tr_w"], p["wt"], p["bias"], p["y"], B, K, M, Tin, r, 0.7071, 1, e.stream())

    def ref(a):
        return {"y": A.ref_up_conv(a["x"], None, a["tr_w"], a["wt"], a["bias"], r, 0.7071, True)[0]}
    lin = L.lin_ok(B, K, Tin) and B * Tin * r < (1 << 31)
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (lin, "linear core" if lin else "generic core"), mirror=lambda: None,
                                 fallback=lambda: {"y": e.ops.up_conv(o.ins["x"], o.ins["tr_w"], o.ins["wt"], o.ins["bias"], r, 0.7071, True)})


def fam_dw(e, c, d):
    B, C, T, k, s, hist = d["B"], d["C"], d["T"], d["k"], d["s"], d["hist"]
    pad, To = k - s, -(-T // s)
    o = Operands(e, c, d)
    o.per("x", 300 + C + k, C)
    o.weight("w", rnd(C + k, C, k))
    o.weight("bias", rnd(C, C) * 0.1)
    if hist:
        o.hist("hist", 5, C, pad)
        o.out("hist_out", (B, C, pad))
    o.out("y", (B, C, To), Fraction(1, s))

    def call(p):
        return e.lib.hilc_dw_conv(p["x"], p.get("hist"), p["w"], p["bias"], None, p["y"], p.get("hist_out"), B, C, T, k, s, 0.9, 1, 0.4, 1, e.stream())

    def ref(a):
        y, h = A.ref_dw_conv(a["x"], a.get("hist"), a["w"], a["bias"], None, s, 0.9, True, 0.4, True)
        return {"y": y, "hist_out": h} if hist else {"y": y}
    vec = k == 5 and s == 1 and T % 4 == 0
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (True, "4-sample kernel" if vec else "generic kernel"), mirror=lambda: None,
                                 fallback=lambda: None)


def fam_dwtr(e, c, d):
    B, C, T, r = d["B"], d["C"], d["T"], d["r"]
    o = Operands(e, c, d)
    o.per("x", 400 + C, C)
    o.hist("hist", 2, C, 1, 0.5)
    o.weight("w", rnd(3, C, 2 * r))
    o.out("y", (B, C, T * r), Fraction(r))
    o.out("hist_out", (B, C, 1))

    def call(p):
        return e.lib.hilc_dw_convtr(p["x"], p["hist"], p["w"], p["y"], p["hist_out"], B, C, T, r, 0.7, 1, e.stream())

    def ref(a):
        y, h = A.ref_dw_convtr(a["x"], a["hist"], a["w"], r, 0.7, True)
        return {"y": y, "hist_out": h}
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (True, "the one kernel"), mirror=lambda: None, fallback=lambda: None)


def fam_pre(e, c, d):
    B, C, T, k, HL = d["B"], d["C"], d["T"], 5, 6
    o = Operands(e, c, d)
    o.wav("wav", 5)
    o.hist("hist", 6, 1, HL, wav=True)
    o.weight("w", rnd(1, C, k))
    o.weight("bias", rnd(2, C) * 0.1)
    o.out("y", (B, C, T), F1)

    def call(p):
        return e.lib.hilc_conv_pre(p["wav"], p["hist"], HL, p["w"], p["bias"], p["y"], B, C, T, k, 1 / 0.1122080159, e.stream())
    return types.SimpleNamespace(o=o, call=call, ref=lambda a: {"y": A.ref_conv_pre(a["wav"], a["hist"], a["w"], a["bias"], 1 / 0.1122080159)},
                                 fast=lambda: (T % 4 == 0, "4-sample kernel"), mirror=lambda: None, fallback=lambda: None)


def fam_post(e, c, d):
    B, C, T, k = d["B"], d["C"], d["T"], 5
    o = Operands(e, c, d)
    o.per("x", 500 + C, C)
    o.hist("hist", 8, C, 4, 0.6)
    o.weight("w", rnd(3, C, k) / 20)
    o.weight("bias", rnd(4, 1) * 0.1)
    o.out("y", (B, 1, T), F1)
    o.out("hist_out", (B, C, 4))

    def call(p):
        return e.lib.hilc_conv_post(p["x"], p["hist"], p["w"], p["bias"], p["y"], p["hist_out"], B, C, T, k, 0.707, 1, 0.1122080159, 1, e.stream())

    def ref(a):
        y, h = A.ref_conv_post(a["x"], a["hist"], a["w"], a["bias"], 0.707, True, 0.1122080159, True)
        return {"y": y, "hist_out": h}
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (T % 4 == 0, "eight-class kernel"), mirror=lambda: None, fallback=lambda: None)


def fam_stft(e, c, d):
    B, T, N = d["B"], d["T"], 64
    o = Operands(e, c, d)
    o.wav("wav", N)
    o.weight("basis_t", e.fold.stft_basis_layout(synth.stft_basis(N)))
    o.out("spec", (B, N // 2 + 1, T), F1)

    def call(p):
        return e.lib.hilc_stft_logmag(p["wav"], None, 0, p["basis_t"], p["spec"], B, T, N, 1, 0.0, 1.0, 2, e.stream())
    return types.SimpleNamespace(o=o, call=call, ref=lambda a: {"spec": A.ref_stft(a["wav"], None, a["basis_t"], N, 1, 0.0, 1.0, 2)},
                                 fast=lambda: (T >= 512, "per-clip LDS segments"), mirror=lambda: None, fallback=lambda: None)


# The waveform of the SpecBlock rows.  log(max(|STFT|, 1e-5)) magnifies the rounding of a bin whose magnitude is nearly cancelled, and
# over thousands of frames some seed always has one: the references in float32 and in float64 then differ by up to 1.4e-4 (seeds 77 / 71,
# min |STFT| 4e-6 / 2e-5), more than the row's whole tolerance.  Seed 21 keeps every magnitude of its three patterns above 9.8e-5 and the
# two references within 3.5e-6 of each other (measured on the CPU; asserted again as `tolerance >= 4 x floor` where the rows run).
SPEC_WAV_SEED = 21


def spec_operands(e, o, N, C, hist):
    bt = e.fold.stft_basis_layout(synth.stft_basis(N))
    wt = rnd(N + 1, N // 2 + 1, C) / (N // 2 + 1) ** 0.5
    dft_p, nyq, pw_p = e.ops.spec_block_tables(bt.to(e.dev), wt.to(e.dev), N)          # layout only
    o.ins.update({"spec.dft_packed": dft_p, "spec.nyq_sin": nyq, "spec.pw_packed": pw_p})
    o.dev.update({"basis_t": bt.to(e.dev), "swt": wt.to(e.dev)})
    o.aux.update({"basis_t": bt, "swt": wt})
    o.wav("spec.wav", SPEC_WAV_SEED, aux="wav")
    o.weight("spec.bias", rnd(N + 2, C) * 0.1, aux="sbias")
    o.aux["whist"] = None
    if hist:
        o.hist("spec.hist", 9, 1, N - 1, aux="whist", wav=True)


def fam_spec(e, c, d):
    B, T, N = d["B"], d["T"], 64
    o = Operands(e, c, d)
    spec_operands(e, o, N, N, True)
    o.per("x", 9, N)
    o.out("y", (B, N, T), F1)

    def call(p):
        return e.lib.hilc_spec_block(p["spec.wav"], p["spec.hist"], N - 1, p["spec.dft_packed"], p["spec.nyq_sin"], p["spec.pw_packed"], p["spec.bias"],
                                     p["x"], p["y"], B, T, N, 1, -4.0, 2.8, 1, 0.37, e.stream())

    def ref(a):
        return {"y": A.ref_spec_block(a["wav"], a["whist"], a["basis_t"], a["swt"], a["sbias"], a["x"], N, 1, -4.0, 2.8, 1, 0.37)}
    ok = bool(e.lib.hilc_spec_block_supported(N, 1, N, T)) and e.ops.spec_block_supported(N, 1, N, T)
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (ok, "one-launch SpecBlock"), mirror=lambda: None, fallback=lambda: None)


def fam_res(e, c, d):
    B, C, T, streaming = d["B"], d["C"], d["T"], c.kw["streaming"]
    o = Operands(e, c, d)
    o.per("x", C + 1, C)
    raw = blocks(o, C, 1, streaming, e.ops.resblock_pack)
    o.out("y", (B, C, T), F1)

    def call(p):
        w = [p[f"b0.{nm}"] for nm in BLK]
        if not streaming:
            return e.lib.hilc_resblock(p["x"], *w, p["y"], B, C, T, float(raw[0][6]), float(raw[0][7]), e.stream())
        return e.lib.hilc_resblock_stream(p["x"], *w, p["b0.hist1"], p["b0.hist2"], p["b0.hist1_out"], p["b0.hist2_out"], p["y"], B, C, T,
                                          float(raw[0][6]), float(raw[0][7]), e.stream())

    def ref(a):
        out = {}
        out["y"] = A.ref_blocks(a, a["x"], streaming, out)
        return out

    def fallback():
        y, got = fb_blocks(e, o, [take(o, "x")], raw, streaming)
        got["y"] = y
        return got
    q = e.lib.hilc_resblock_stream_supported(C, T) if streaming else e.lib.hilc_resblock_supported(C, T)
    mirror = lambda: e.ops.resblock_supported(C, T, B, streaming)          # noqa: E731
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (bool(q) and mirror(), "fused residual block"), mirror=mirror, fallback=fallback)


def fam_chain(e, c, d):
    B, C, T, n, streaming = d["B"], d["C"], d["T"], d["n"], c.kw["streaming"]
    o = Operands(e, c, d)
    o.per("x", C + 2, C)
    raw = blocks(o, C, n, streaming, lambda w: e.ops.resblock_chain_pack(w, streaming))
    o.out("y", (B, C, T), F1)

    def call(p):
        return e.lib.hilc_resblock_chain(p["x"], p["y"], void(block_structs(e, p, raw, streaming)), n, int(streaming), B, C, T, e.stream())

    def ref(a):
        out = {}
        out["y"] = A.ref_blocks(a, a["x"], streaming, out)
        return out

    def fallback():
        y, got = fb_blocks(e, o, [take(o, "x")], raw, streaming)
        got["y"] = y
        return got
    q = e.lib.hilc_resblock_chain_supported(C, T, n, int(streaming))
    mirror = lambda: e.ops.resblock_chain_supported(C, T, n, B, streaming)          # noqa: E731
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (bool(q) and mirror(), "chain launch"), mirror=mirror, fallback=fallback)


def fam_enc(e, c, d):
    B, C, T, r, n, streaming, stage0 = d["B"], d["C"], d["T"], d["r"], d["n"], c.kw["streaming"], bool(c.kw.get("stage0"))
    in_scale, N = (1 + n * RS ** 2) ** -0.5, 64
    o = Operands(e, c, d)
    pack = lambda w: e.ops.resblock_chain_pack(w, streaming)          # noqa: E731
    if stage0:
        spec_operands(e, o, N, C, streaming)
        o.weight("spec.pre_w", rnd(71, C, 5) * 0.5, aux="pre_w")
        o.weight("spec.pre_b", rnd(72, C) * 0.1, aux="pre_b")
    else:
        o.per("x", C + r, C)
    raw = blocks(o, C, n, streaming, pack)
    wd = rnd(70, C, 2 * C) / C ** 0.5                               # k-major [C, 2C]
    o.aux["wd"], o.dev["wd"] = wd, wd.to(e.dev)
    o.ins["down.w_lo"], o.ins["down.w_hi"] = pack(wd[:, :C].contiguous().to(e.dev)), pack(wd[:, C:].contiguous().to(e.dev))
    o.weight("down.dw_w", rnd(73, 2 * C, 2 * r) * 0.3, aux="ddw")
    o.weight("down.dw_b", rnd(74, 2 * C) * 0.1, aux="ddb")
    o.per("down.res", 75, 2 * C, Fraction(1, r), 0.5, aux="dres")
    o.aux["dhist"] = None
    if streaming:
        o.hist("down.hist", 30, 2 * C, r, 0.6, aux="dhist")
        o.out("down.hist_out", (B, 2 * C, r))
    o.out("down.y", (B, 2 * C, T // r), Fraction(1, r))

    def call(p):
        down = e.L.DownParams(p["down.w_lo"], p["down.w_hi"], p["down.dw_w"], p["down.dw_b"], p.get("down.hist"), p.get("down.hist_out"),
                              p["down.res"], p["down.y"], in_scale, r)
        blk = block_structs(e, p, raw, streaming)
        if stage0:
            spec = e.L.Spec0Params(p["spec.wav"], p["spec.dft_packed"], p["spec.nyq_sin"], p["spec.pw_packed"], p["spec.bias"], p["spec.pre_w"],
                                   p["spec.pre_b"], p.get("spec.hist"), N - 1 if streaming else 0, 1 / 0.1122080159, -4.0, 2.8, 0.37, 1, N, 1, 5)
            return e.lib.hilc_encoder_stage0(void(spec), void(blk), n, void(down), int(streaming), B, T, e.stream())
        return e.lib.hilc_encoder_stage(p["x"], void(blk), n, void(down), int(streaming), B, C, T, e.stream())

    def fallback():
        ops = e.ops
        if stage0:
            wh = o.ins.get("spec.hist")
            x = ops.conv_pre(o.ins["spec.wav"], o.ins["spec.pre_w"], o.ins["spec.pre_b"], 1 / 0.1122080159, hist=wh)
            s = ops.stft_logmag(o.ins["spec.wav"], o.dev["basis_t"], N, 1, -4.0, 2.8, 1, hist=wh)
            xs = [ops.pw_conv(s, o.dev["swt"], o.ins["spec.bias"], res=x, out_scale=0.37)]
            del s, x
        else:
            xs = [take(o, "x")]
        x, got = fb_blocks(e, o, xs, raw, streaming)
        h = ops.pw_conv(x, o.dev["wd"], in_scale=in_scale, in_elu=True)
        del x
        got["down.y"], hc = ops.dw_conv(h, o.ins["down.dw_w"], o.ins["down.dw_b"], res=o.ins["down.res"], stride=r, hist=o.ins.get("down.hist"),
                                       want_hist=True)
        if streaming:
            got["down.hist_out"] = hc
        return got
    if stage0:
        q = e.lib.hilc_encoder_stage0_supported(T, n, r, N, 1, 5, int(streaming))
        mirror = lambda: e.ops.encoder_stage0_supported(T, n, r, N, 1, 5, B, streaming)          # noqa: E731
    else:
        q = e.lib.hilc_encoder_stage_supported(C, T, n, r, int(streaming))
        mirror = lambda: e.ops.encoder_stage_supported(C, T, n, r, B, streaming)          # noqa: E731
    return types.SimpleNamespace(o=o, call=call, ref=lambda a: A.ref_encoder_stage(a, streaming, stage0, r, in_scale, N),
                                 fast=lambda: (bool(q) and mirror(), "stage launch"), mirror=mirror, fallback=fallback)


def fam_dec(e, c, d):
    B, C, T, r, n, streaming, post = d["B"], d["C"], d["T"], d["r"], d["n"], c.kw["streaming"], bool(c.kw.get("post"))
    o = Operands(e, c, d)
    pack = lambda w: e.ops.resblock_chain_pack(w, streaming)          # noqa: E731
    o.per("up.x", 100 + C, 2 * C, Fraction(1, r), aux="xin")
    o.weight("up.tr_w", rnd(80, 2 * C, 2 * r) * 0.3, aux="tw")
    wu = rnd(81, 2 * C, C) / (2 * C) ** 0.5
    o.aux["wu"], o.dev["wu"] = wu, wu.to(e.dev)
    o.ins["up.w_lo"], o.ins["up.w_hi"] = pack(wu[:C].contiguous().to(e.dev)), pack(wu[C:].contiguous().to(e.dev))
    o.weight("up.bias", rnd(82, C) * 0.1, aux="bu")
    o.aux["uhist"] = o.aux["phist"] = None
    if streaming:
        o.hist("up.hist", 30, 2 * C, 1, 0.6, aux="uhist")
        o.out("up.hist_out", (B, 2 * C, 1))
    raw = blocks(o, C, n, streaming, pack)
    if post:
        o.weight("post.w", rnd(83, C, 5) * 0.2, aux="pw")
        o.weight("post.bias", rnd(84, 1) * 0.1, aux="pb")
        o.out("post.wav", (B, 1, T), F1)
        if streaming:
            o.hist("post.hist", 31, C, 4, 0.6, aux="phist")
            o.out("post.hist_out", (B, C, 4))
    else:
        o.out("y", (B, C, T), F1)

    def call(p):
        up = e.L.UpParams(p["up.x"], p["up.tr_w"], p["up.w_lo"], p["up.w_hi"], p["up.bias"], p.get("up.hist"), p.get("up.hist_out"), 0.7071, r)
        blk = block_structs(e, p, raw, streaming)
        if post:
            ps = e.L.PostParams(p["post.w"], p["post.bias"], p["post.wav"], p.get("post.hist"), p.get("post.hist_out"), 0.5, 0.1122, 1, 5)
            return e.lib.hilc_decoder_stage_post(void(up), void(blk), n, void(ps), int(streaming), B, C, T, e.stream())
        return e.lib.hilc_decoder_stage(void(up), void(blk), n, p["y"], int(streaming), B, C, T, e.stream())

    def fallback():
        ops, got = e.ops, {}
        y, uh = ops.up_conv(take(o, "up.x"), o.ins["up.tr_w"], o.dev["wu"], o.ins["up.bias"], r, in_scale=0.7071, in_elu=True, hist=o.ins.get("up.hist"),
                            want_hist=True)
        if streaming:
            got["up.hist_out"] = uh
        ys = [y]
        del y
        y, g2 = fb_blocks(e, o, ys, raw, streaming)
        got.update(g2)
        if post:
            got["post.wav"], ph = ops.conv_post(y, o.ins["post.w"], o.ins["post.bias"], in_scale=0.5, in_elu=True, out_scale=0.1122, do_tanh=True,
                                                hist=o.ins.get("post.hist"), want_hist=True)
            if streaming:
                got["post.hist_out"] = ph
        else:
            got["y"] = y
        return got
    q = e.lib.hilc_decoder_stage_supported(C, T, n, r, int(streaming)) and (not post or e.lib.hilc_decoder_stage_post_supported(C, T, n, r, 5))
    mirror = lambda: (e.ops.decoder_stage_supported(C, T, n, r, B, streaming)          # noqa: E731
                      and (not post or e.ops.decoder_stage_post_supported(C, T, n, r, 5)))
    return types.SimpleNamespace(o=o, call=call, ref=lambda a: A.ref_decoder_stage(a, streaming, post, r),
                                 fast=lambda: (bool(q) and mirror(), "stage launch"), mirror=mirror, fallback=fallback)


RVQ = types.SimpleNamespace(Nq=3, K=1024, C=128, n=2, min_gap=1e-3)


def rvq_tables():
    cb = rnd(5, RVQ.Nq, RVQ.K, RVQ.C) * 0.3
    return cb, cb.transpose(1, 2).contiguous(), cb.pow(2).sum(-1)


def rvq_ref(z, cb):
    """z [npat, C, L] float64 -> (indices [npat, n, L], q [npat, C, L], the smallest best-to-second gap of any argmin)"""
    r = z.transpose(1, 2).clone()                                    # [npat, L, C]
    q, idx, gap = torch.zeros_like(r), [], float("inf")
    for s in range(RVQ.n):
        dist = cb[s].pow(2).sum(-1) - 2 * r @ cb[s].t()              # [npat, L, K]
        two = dist.topk(2, dim=-1, largest=False).values
        gap = min(gap, float((two[..., 1] - two[..., 0]).min()))
        k = dist.argmin(-1)
        idx.append(k)
        r = r - cb[s][k]
        q = q + cb[s][k]
    return torch.stack(idx, 1), q.transpose(1, 2).contiguous(), gap


def fam_rvq_enc(e, c, d):
    B, T = d["B"], d["T"]
    o = Operands(e, c, d)
    cb, cbt, nrm = rvq_tables()
    o.per("z", 7, RVQ.C, scale=0.4)
    o.weight("codebooks", cb)
    o.weight("codebooks_t", cbt)
    o.weight("norms", nrm)
    o.out("indices", (B, RVQ.n, T), F1, torch.int64)
    o.out("q", (B, RVQ.C, T), F1)

    def call(p):
        return e.lib.hilc_rvq_encode(p["z"], p["codebooks"], p["codebooks_t"], p["norms"], p["indices"], p["q"], None, B, RVQ.C, T, RVQ.K, RVQ.Nq,
                                     RVQ.n, 0, 0, c.kw["flags"], e.stream())

    def ref(a):
        """float64 arg-mins; no frame of the patterns is a near-tie (the project's bar for one is a gap under 1e-4), so the kernel's fp32
        scores must give these indices exactly, and q = the sum of their code words"""
        idx, q, gap = rvq_ref(a["z"], a["codebooks"])
        assert a["z"].dtype != torch.float64 or gap > RVQ.min_gap, f"a frame of the patterns is a near-tie (gap {gap:.2e}): pick another seed"
        return {"indices": idx.to(a["z"].dtype), "q": q}
    mfma = c.kw["flags"] == 0 and B * T >= 8192
    return types.SimpleNamespace(o=o, call=call, ref=ref, fast=lambda: (True, "matrix pipe" if mfma else "VALU"), mirror=lambda: None,
                                 fallback=lambda: None)


def fam_rvq_dec(e, c, d):
    B, T = d["B"], d["T"]
    o = Operands(e, c, d)
    cb = rvq_tables()[0]
    pat = torch.from_numpy(np.random.RandomState(3).randint(0, RVQ.K, size=(L.NPAT, RVQ.n, c.P))).to(torch.int64)
    o.per("indices", 0, RVQ.n, pat=pat)
    o.weight("codebooks", cb)
    o.out("q", (B, RVQ.C, T), F1)

    def ref(a):
        q = sum(a["codebooks"][s][a["indices"][:, s]] for s in range(RVQ.n))          # [npat, L, C]
        return {"q": q.transpose(1, 2).contiguous()}
    return types.SimpleNamespace(o=o, call=lambda p: e.lib.hilc_rvq_decode(p["indices"], p["codebooks"], p["q"], B, RVQ.C, T, RVQ.K, RVQ.Nq, RVQ.n, 0, 0,
                                                                           e.stream()),
                                 ref=ref, fast=lambda: (True, "the one kernel"), mirror=lambda: None, fallback=lambda: None)


FAMILIES = {"dwss": fam_dwss, "l2": fam_l2, "pw": fam_pw, "dws": fam_dws, "up": fam_up, "dw": fam_dw, "dwtr": fam_dwtr, "pre": fam_pre, "post": fam_post, "stft": fam_stft,
            "spec": fam_spec, "res": fam_res, "chain": fam_chain, "enc": fam_enc, "dec": fam_dec, "rvq_enc": fam_rvq_enc, "rvq_dec": fam_rvq_dec}


def references(f):
    """float64 reference of the three periods (and the clip's end) and the floor under the tolerance: the same reference in float32"""
    a = {k: v for k, v in f.o.aux.items()}
    r64 = f.ref(cast(a, torch.float64))
    r32 = f.ref(cast(a, torch.float32))
    floor = max([float((r32[k].double() - r64[k].double()).abs().max()) for k in r64] + [0.0])
    return {k: v.double() for k, v in r64.items()}, floor
