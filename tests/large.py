"""Helpers of the large-tensor tests (tests/test_large_cpu.py, tests/test_gpu_large.py): entry points on activation tensors just
below and at 4 GiB, where byte offsets stop fitting 32 bits ("Large tensors").  The cases are here; what builds a case's
operands, call and reference is in tests/large_families.py.

The method.  Every entry point is causal with a short receptive field, so an input that is periodic in time with period P gives, after
the receptive field, an output that is periodic with P (times the op's rate).  A float64 reference of THREE periods then stands for
a multi-GiB output: period 0 carries the zero / cache history, period 1 is the first one the history no longer reaches (P >= 2 x the
receptive field), period 2 stands for every later one.  Clips cycle through `NPAT` distinct patterns (clip b = pattern b % NPAT), rows
of a pattern differ pairwise, and no power of two of elements is a multiple of P — an offset that wraps at 2 / 4 / 8 GiB, a clip base
taken from another clip or a row read from its neighbour all land on other values.  `compare_periodic` walks the WHOLE output on the
device in chunks of at most 256 MiB.

No GPU import at module level: the table of cases (`CASES`) and its arithmetic are checked on the CPU."""
import math
import types
from fractions import Fraction

import torch

from hilcodec_amd import synth

LIMIT = 1 << 32                  # bytes: the first size whose byte offsets no longer fit 32 bits
CHUNK_BYTES = 256 << 20          # the whole-tensor compare touches at most this much of an output at a time
NPAT = 3
WRAPS = (29, 30, 31)             # 2^k ELEMENTS = a 2 / 4 / 8 GiB wrap of a float offset
MEMORY_CAP = 25 << 30            # a case needs less than this (the file's peak on the device)


def bytes_of(shape, itemsize=4) -> int:
    n = itemsize
    for s in shape:
        n *= int(s)
    return n


# ---- receptive field and the conditions on P ------------------------------------------------------------------------------------------
def receptive_field(layers) -> int:
    """Input samples (at the rate of the FIRST layer's input) that one output sample of a chain of causal layers looks back over, itself
    included.  layers: ("conv", k, stride) — k taps, also a strided / depthwise / STFT window (k = n_fft, stride = hop); ("convtr", r) —
    the transposed conv k = 2r stride r (an output reads two input frames); ("pw",) — 1 x 1.  Rates below the input's are fractions."""
    rf, jump = Fraction(1), Fraction(1)
    for layer in layers:
        if layer[0] == "conv":
            rf += (layer[1] - 1) * jump
            jump *= layer[2]
        elif layer[0] == "convtr":
            rf += jump
            jump /= layer[1]
        else:
            assert layer[0] == "pw", layer
    return math.ceil(rf)


RESBLOCK = [("pw",), ("conv", 5, 1), ("pw",), ("conv", 5, 1)]


def model_receptive_field(mk) -> int:
    """hil_speech / hil_music, waveform in -> waveform out, in samples: the longest of the sequential path and the paths that enter
    through a SpecBlock (an STFT window of 64 * 2^s samples at hop = the stage's rate)"""
    ratios = list(reversed(mk["strides"]))
    k, kl, kr = mk["kernel_size"], mk["last_kernel_size"], mk["residual_kernel_size"]
    block = [("pw",), ("conv", kr, 1), ("pw",), ("conv", kr, 1)]

    def tail_of_encoder(s):          # what follows stage s's SpecBlock
        out = []
        for r in ratios[s:]:
            out += block * mk["n_residual_enc"] + [("pw",), ("conv", 2 * r, r)]
        return out + [("conv", kl, 1), ("pw",)]

    dec = [("pw",), ("conv", k, 1)]
    for r in mk["strides"]:
        dec += [("convtr", r), ("pw",)] + block * mk["n_residual_dec"]
    dec += [("conv", kl, 1)]
    paths = [[("conv", k, 1)] + tail_of_encoder(0) + dec]
    hop = 1
    for s in range(len(ratios) + 1):
        n_fft = mk["n_fft_base"] * 2 ** s
        rest = tail_of_encoder(s) if s < len(ratios) else [("conv", kl, 1), ("pw",)]
        # the window is n_fft samples at the waveform's rate; what follows runs at 1 / hop of it
        rf = n_fft + (receptive_field(rest + dec) - 1) * hop
        paths.append(rf)
        if s < len(ratios):
            hop *= ratios[s]
    return max(p if isinstance(p, int) else receptive_field(p) for p in paths)


def wraps_visible(P: int, ks=WRAPS) -> bool:
    """an offset that loses 2^k elements lands on another phase of the period"""
    return all((1 << k) % P != 0 for k in ks)


def check_period(P: int, rf: int, ks=WRAPS) -> None:
    assert wraps_visible(P, ks), f"P = {P}: a wrap of 2^k elements, k in {ks}, lands on the same phase"
    assert P >= 2 * rf, f"P = {P} is shorter than twice the receptive field {rf}"


def pattern(seed: int, rows: int, P: int, scale: float = 1.0, npat: int = NPAT) -> torch.Tensor:
    """`[npat, rows, P]` float32 on the CPU from `synth.normalish`; rows and patterns differ pairwise (asserted)"""
    t = torch.from_numpy(synth.normalish(seed, npat * rows * P)).view(npat, rows, P) * scale
    flat = t.reshape(npat * rows, P)
    if flat.shape[0] <= 4096:
        d = torch.cdist(flat.double(), flat.double())
        d.fill_diagonal_(1.0)
        assert float(d.min()) > 0.0, "two rows of the patterns are equal"
    else:
        assert torch.unique(flat, dim=0).shape[0] == flat.shape[0], "two rows of the patterns are equal"
    return t


def periodic(pat: torch.Tensor, T: int, B: int = 1, device=None, hist: torch.Tensor = None):
    """pat `[npat, R, P]` (CPU) -> `[B, R, T]` on `device`, clip b = pat[b % npat] repeated along time (tiled on the device: the copy
    reads an expanded view, nothing of T elements exists on the host).  hist `[npat, R, L]`: the history operand of the same clips ->
    (x, `[B, R, L]`)."""
    npat, R, P = pat.shape
    dev = torch.device("cpu") if device is None else device
    pd = pat.to(dev)
    x = torch.empty(B, R, T, dtype=pat.dtype, device=dev)
    n, rest = T // P, T % P
    for b in range(min(B, npat)):
        src = pd[b]
        if n:
            x[b][:, :n * P].unflatten(1, (n, P)).copy_(src.unsqueeze(1).expand(R, n, P))
        if rest:
            x[b][:, n * P:].copy_(src[:, :rest])
    # the remaining clips repeat the first npat, a chunk of whole cycles at a time
    cycles = max(1, CHUNK_BYTES // max(1, npat * R * T * x.element_size()))
    for b0 in range(npat, B, npat * cycles):
        b1 = min(B, b0 + npat * cycles)
        x[b0:b1].copy_(x[:npat].repeat(cycles, 1, 1)[:b1 - b0])
    if hist is None:
        return x
    h = hist.to(dev)[torch.arange(B, device=dev) % npat].contiguous()
    return x, h


def ref_index(t0: int, t1: int, P: int, first_from_ref0: bool, device=None, T: int = 0, tail: int = 0) -> torch.Tensor:
    """where output time t in [t0, t1) of T stands in the reference: itself while t < 2 P, else the same phase of period 2; the last
    `tail` outputs stand at the reference's own end, `tail` = what it holds beyond three periods (the end of a clip is not periodic: a
    strided window there runs into the zeros behind the last sample).  not first_from_ref0 (a history that continues the periodic
    signal): every earlier period is period 2"""
    t = torch.arange(t0, t1, device=device)
    late = 2 * P + t % P
    idx = late if not first_from_ref0 else torch.where(t < 2 * P, t, late)
    if tail:
        idx = torch.where(t >= T - tail, 3 * P + tail - (T - t), idx)
    return idx


def compare_periodic(y: torch.Tensor, ref3: torch.Tensor, P: int, first_from_ref0: bool = True, chunk_bytes: int = CHUNK_BYTES):
    """max |y - ref| over the WHOLE of y `[B, R, T]` (any device) against ref3 `[npat, R, L]` (float64), clip b against pattern
    b % npat, in chunks of at most chunk_bytes of y.  L = T where T <= 3 P; else 3 P, or 3 P + T % P: the reference of an input of
    three periods and the last, partial one of the clip (`ref_index`).  -> namespace(err, clip, row, t, byte_offset, finite): the largest
    error and where it sits (NaN counts as infinite: finite = False)."""
    B, R, T = y.shape
    npat = ref3.shape[0]
    assert ref3.shape[1] == R and ref3.dtype == torch.float64, (y.shape, ref3.shape, P)
    tail = ref3.shape[2] - 3 * P if T > 3 * P else 0
    assert ref3.shape[2] == T if T <= 3 * P else tail in (0, T % P), (y.shape, ref3.shape, P)
    ref = ref3.to(y.device)
    per_col = R * y.element_size()
    tc = max(1, min(T, chunk_bytes // per_col))
    nb = max(1, chunk_bytes // (per_col * tc))
    best = types.SimpleNamespace(err=-1.0, clip=0, row=0, t=0, byte_offset=0, finite=True)
    for t0 in range(0, T, tc):
        t1 = min(T, t0 + tc)
        rc = ref[:, :, ref_index(t0, t1, P, first_from_ref0, y.device, T, tail)]               # [npat, R, t1 - t0]
        for b0 in range(0, B, nb):
            b1 = min(B, b0 + nb)
            sel = rc if (b0 % npat == 0 and b1 - b0 == npat) else rc[torch.arange(b0, b1, device=y.device) % npat]
            d = (y[b0:b1, :, t0:t1].double() - sel).abs()
            if not bool(torch.isfinite(d).all()):
                best.finite = False
                d = torch.nan_to_num(d, nan=float("inf"), posinf=float("inf"))
            m = float(d.max())
            if m > best.err:
                i = int(d.reshape(-1).argmax())
                cb, rem = divmod(i, R * (t1 - t0))
                row, tt = divmod(rem, t1 - t0)
                best.err, best.clip, best.row, best.t = m, b0 + cb, row, t0 + tt
            del d, sel
    best.byte_offset = ((best.clip * R + best.row) * T + best.t) * y.element_size()
    return best


def identical_clips_equal(y: torch.Tensor, npat: int = NPAT, chunk_bytes: int = CHUNK_BYTES) -> bool:
    """clips that carry the same pattern (b and b % npat) are `torch.equal` — batch invariance, bit for bit.  Vacuous for B <= npat."""
    B = y.shape[0]
    per = max(1, chunk_bytes // max(1, y[0].numel() * y.element_size())) * npat
    for b0 in range(npat, B, per):
        b1 = min(B, b0 + per)
        if not torch.equal(y[b0:b1], y[torch.arange(b0, b1, device=y.device) % npat]):
            return False
    return True


# ---- mirrors of launch-path predicates that have no query of their own ------------------------------------------------------------------
def lin_ok(B: int, K: int, T: int) -> bool:
    """csrc/gemm_epilogues.h `lin_ok`: the linear-addressing GEMM cores take an x of fewer than 2^32 bytes"""
    return B * K * T * 4 < LIMIT


# ---- the table of cases -----------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, family, tolrow, P, layers, below, at, b3=None, exact=True, stream_guard=None, **kw):
    """family: the builder of tests/large_families.py; tolrow: the row of tests/entry_rows.py whose tolerance the case uses;
    layers: for `receptive_field`; below / at / b3: the dimensions of the sizes; exact: "below" and "at" promise the same bits;
    stream_guard: the product (in bytes) a streaming form's launch path refuses from 2^32 on — None: an offline / flat form"""
    sizes = {"below": dict(below), "at": dict(at)}
    if b3 is not None:
        sizes["b3"] = dict(b3)
    CASES[name] = types.SimpleNamespace(name=name, family=family, tolrow=tolrow, P=P, layers=layers, sizes=sizes, exact=exact,
                                        stream_guard=stream_guard, kw=kw)


def tensors(c, d) -> dict:
    """every activation tensor (shape) a launch of case c at dimensions d reads or writes; weights and caches of a few KB left out"""
    f, B = c.family, d["B"]
    if f == "pw":
        t = {"x": (B, d["K"], d["T"]), "y": (B, d["M"], d["T"])}
        if c.kw.get("res"):
            t["res"] = t["y"]
        return t
    if f == "dws":
        return {"x": (B, d["K"], d["T"]), "y": (B, d["M"], -(-d["T"] // d["r"]))}
    if f == "up":
        return {"x": (B, d["K"], d["T"]), "y": (B, d["M"], d["T"] * d["r"])}
    if f == "dwss":
        return {"x": (B, d["K"], d["T"]), "y": (B, d["M"], d["T"] // d["r"]), "res": (B, d["M"], d["T"] // d["r"])}
    if f == "l2":
        return {"x": (B, d["C"], d["T"]), "y": (B, d["C"], d["T"])}
    if f == "dw":
        return {"x": (B, d["C"], d["T"]), "y": (B, d["C"], -(-d["T"] // d["s"]))}
    if f == "dwtr":
        return {"x": (B, d["C"], d["T"]), "y": (B, d["C"], d["T"] * d["r"])}
    if f == "pre":
        return {"wav": (B, 1, d["T"]), "y": (B, d["C"], d["T"])}
    if f == "post":
        return {"x": (B, d["C"], d["T"]), "y": (B, 1, d["T"])}
    if f == "stft":
        return {"wav": (B, 1, d["T"]), "spec": (B, 33, d["T"])}
    if f == "spec":
        return {"wav": (B, 1, d["T"]), "x": (B, 64, d["T"]), "y": (B, 64, d["T"])}
    if f in ("res", "chain"):
        return {"x": (B, d["C"], d["T"]), "y": (B, d["C"], d["T"])}
    if f == "enc":
        t = {"down.y": (B, 2 * d["C"], d["T"] // d["r"]), "down.res": (B, 2 * d["C"], d["T"] // d["r"])}
        t.update({"spec.wav": (B, 1, d["T"])} if c.kw.get("stage0") else {"x": (B, d["C"], d["T"])})
        return t
    if f == "dec":
        t = {"up.x": (B, 2 * d["C"], d["T"] // d["r"])}
        t.update({"post.wav": (B, 1, d["T"])} if c.kw.get("post") else {"y": (B, d["C"], d["T"])})
        return t
    if f == "rvq_enc":
        return {"z": (B, 128, d["T"]), "q": (B, 128, d["T"]), "indices": (B, 2 * 2, d["T"])}          # int64 = two words
    assert f == "rvq_dec", f
    return {"indices": (B, 2 * 2, d["T"]), "q": (B, 128, d["T"])}


def governing_bytes(c, d) -> int:
    """the largest activation of the launch — or, for a streaming form, the product its guard uses"""
    if c.stream_guard is not None:
        return c.stream_guard(d)
    return max(bytes_of(s) for s in tensors(c, d).values())


def need_bytes(c, size: str) -> int:
    """device memory a case may take: its operands, the "below" outputs the "at" case is compared with, the compare's chunks (float64
    copies of two chunks and their difference) — and, for a streaming form that is refused, the intermediates of the fall-back
    (at most two tensors of the governing size alive at once beside its input and output)"""
    d = c.sizes[size]
    t = tensors(c, d)
    total = sum(bytes_of(s) for s in t.values()) + 8 * CHUNK_BYTES + (1 << 30)
    if size == "at":
        total += max(bytes_of(s) for k, s in tensors(c, c.sizes["below"]).items() if k in OUTPUTS[c.family])
    if c.stream_guard is not None and size == "at":
        total += 2 * governing_bytes(c, d)
    return total


OUTPUTS = {"dwss": ("y",), "l2": ("y",), "pw": ("y",), "dws": ("y",), "up": ("y",), "dw": ("y",), "dwtr": ("y",), "pre": ("y",), "post": ("y",), "stft": ("spec",),
           "spec": ("y",), "res": ("y",), "chain": ("y",), "enc": ("down.y",), "dec": ("y", "post.wav"), "rvq_enc": ("q", "indices"),
           "rvq_dec": ("q",)}

T26, T25, T24, T23 = 1 << 26, 1 << 25, 1 << 24, 1 << 23
PW = [("pw",)]

# pointwise conv: x governs (the linear core below, the generic core at), y governs (the linear core writes past 4 GiB), B = 3 ragged
case("pw_conv-x", "pw", "pw_conv-2x17x64x132", 300, PW, dict(B=1, K=16, M=16, T=T26 - 4), dict(B=1, K=16, M=16, T=T26))
case("pw_conv-y", "pw", "pw_conv-2x17x64x132", 300, PW, dict(B=1, K=16, M=64, T=T24 - 4), dict(B=1, K=16, M=64, T=T24))
case("pw_conv-b3-ragged", "pw", "pw_conv-2x17x64x132", 300, PW, dict(B=3, K=16, M=4, T=22369620), dict(B=3, K=16, M=4, T=22369624), res=True)
# pointwise -> depthwise: k5 and the strided form (k = 8, r = 4)
case("dws_conv-k5", "dws", "dws_conv-k5-1x16x128x260", 300, [("pw",), ("conv", 5, 1)], dict(B=1, K=32, M=32, T=T25 - 4, r=1),
     dict(B=1, K=32, M=32, T=T25, r=1), b3=dict(B=3, K=32, M=32, T=T24 + 4, r=1))
case("dws_conv-r4", "dws", "dws_conv-r4-2x16x32x64", 300, [("pw",), ("conv", 8, 4)], dict(B=1, K=32, M=32, T=T25 - 4, r=4),
     dict(B=1, K=32, M=32, T=T25, r=4))
# up-sampling: x [B,32,Tin] and y [B,16,2 Tin] are the same size
case("up_conv-r2", "up", "up_conv-2x32x16x6-r2", 300, [("convtr", 2), ("pw",)], dict(B=1, K=32, M=16, T=T25 - 2, r=2),
     dict(B=1, K=32, M=16, T=T25, r=2), b3=dict(B=3, K=32, M=16, T=T24 + 2, r=2))
# depthwise
case("dw_conv-k5", "dw", "dw_conv-24x36-k5", 300, [("conv", 5, 1)], dict(B=1, C=16, T=T26 - 4, k=5, s=1, hist=False),
     dict(B=1, C=16, T=T26, k=5, s=1, hist=False), b3=dict(B=3, C=16, T=T25 + 4, k=5, s=1, hist=False))
case("dw_conv-k8s4-hist", "dw", "dw_conv-16x40-k8s4-hist", 300, [("conv", 8, 4)], dict(B=1, C=16, T=T26 - 1, k=8, s=4, hist=True),
     dict(B=1, C=16, T=T26, k=8, s=4, hist=True))
case("dw_convtr-r4", "dwtr", "dw_convtr-16x12-r4", 300, [("convtr", 4)], dict(B=1, C=16, T=T24 - 1, r=4), dict(B=1, C=16, T=T24, r=4))
# first / last conv: the output / the input governs
case("conv_pre", "pre", "conv_pre-24x36-k5", 300, [("conv", 5, 1)], dict(B=1, C=64, T=T24 - 4), dict(B=1, C=64, T=T24))
case("conv_post", "post", "conv_post-24x36-k5-hist", 300, [("conv", 5, 1)], dict(B=1, C=96, T=11184808), dict(B=1, C=96, T=11184812),
     b3=dict(B=3, C=96, T=5592408))
# STFT (spec [B,33,T] governs) and the one-launch SpecBlock (x [B,64,T])
case("stft_logmag-n64", "stft", "stft_logmag-n16-T512-seg", 1500, [("conv", 64, 1)], dict(B=1, T=32537628), dict(B=1, T=32537632))
case("spec_block-n64", "spec", "spec_block-n64-T128", 1500, [("conv", 64, 1), ("pw",)], dict(B=1, T=T24 - 4), dict(B=1, T=T24),
     b3=dict(B=3, T=T23 + 4))
# the fused residual block, the chain and the stage launches: offline
case("resblock-64-offline", "res", "resblock-64x8x2", 300, RESBLOCK, dict(B=1, C=64, T=T24 - 4), dict(B=1, C=64, T=T24),
     b3=dict(B=3, C=64, T=T23 + 4), streaming=False)
case("resblock-768-offline", "res", "resblock-64x8x2", 60, RESBLOCK, dict(B=1, C=768, T=1398100), dict(B=1, C=768, T=1398104), streaming=False)
case("resblock_chain-64x2-offline", "chain", "resblock_chain-64x8x2-offline", 300, RESBLOCK * 2, dict(B=1, C=64, T=T24 - 4, n=2),
     dict(B=1, C=64, T=T24, n=2), b3=dict(B=3, C=64, T=T23 + 4, n=2), streaming=False)
case("resblock_chain-96x3-offline", "chain", "resblock_chain-64x8x2-offline", 300, RESBLOCK * 3, dict(B=1, C=96, T=11184808, n=3),
     dict(B=1, C=96, T=11184812, n=3), streaming=False)
ENC = RESBLOCK * 2 + [("pw",), ("conv", 4, 2)]
case("encoder_stage-64-r2-offline", "enc", "encoder_stage-128x8-r4-offline", 300, ENC, dict(B=1, C=64, T=T24 - 4, r=2, n=2),
     dict(B=1, C=64, T=T24, r=2, n=2), b3=dict(B=3, C=64, T=T23 + 4, r=2, n=2), streaming=False)
case("encoder_stage0-offline", "enc", "encoder_stage0-T8-offline", 1500, [("conv", 64, 1), ("pw",)] + ENC, dict(B=1, C=64, T=T24 - 4, r=2, n=2),
     dict(B=1, C=64, T=T24, r=2, n=2), streaming=False, stage0=True)
DEC = [("convtr", 2), ("pw",)] + RESBLOCK * 3
case("decoder_stage-96-r2-offline", "dec", "decoder_stage-96-r2-Tin2-offline", 300, DEC, dict(B=1, C=96, T=11184808, r=2, n=3),
     dict(B=1, C=96, T=11184812, r=2, n=3), b3=dict(B=3, C=96, T=5592408, r=2, n=3), streaming=False)
case("decoder_stage_post-offline", "dec", "decoder_stage_post-96-r2-Tin2-offline", 300, DEC + [("conv", 5, 1)], dict(B=1, C=96, T=11184808, r=2, n=3),
     dict(B=1, C=96, T=11184812, r=2, n=3), streaming=False, post=True)
# the streaming forms: one hop of 320 samples, B at the boundary of the product their launch path guards
HOP = 320
case("resblock-64-stream", "res", "resblock_stream-64x8x3", HOP, RESBLOCK, dict(B=52428, C=64, T=HOP), dict(B=52429, C=64, T=HOP),
     streaming=True, stream_guard=lambda d: d["B"] * d["C"] * d["T"] * 4)
case("resblock_chain-64x2-stream", "chain", "resblock_chain-64x8x3-stream", HOP, RESBLOCK * 2, dict(B=52428, C=64, T=HOP, n=2),
     dict(B=52429, C=64, T=HOP, n=2), streaming=True, stream_guard=lambda d: d["B"] * d["C"] * d["T"] * 4)
case("encoder_stage-64-r2-stream", "enc", "encoder_stage-128x8-r4-stream", HOP, ENC, dict(B=26214, C=64, T=HOP, r=2, n=2),
     dict(B=26215, C=64, T=HOP, r=2, n=2), streaming=True, stream_guard=lambda d: d["B"] * 2 * d["C"] * d["T"] * 4)
case("encoder_stage0-stream", "enc", "encoder_stage0-T128-stream", HOP, [("conv", 64, 1), ("pw",)] + ENC, dict(B=26214, C=64, T=HOP, r=2, n=2),
     dict(B=26215, C=64, T=HOP, r=2, n=2), streaming=True, stage0=True, stream_guard=lambda d: d["B"] * 128 * d["T"] * 4)
case("decoder_stage-96-r2-stream", "dec", "decoder_stage-96-r2-Tin2-stream", HOP, DEC, dict(B=34952, C=96, T=HOP, r=2, n=3),
     dict(B=34953, C=96, T=HOP, r=2, n=3), streaming=True, stream_guard=lambda d: d["B"] * d["C"] * d["T"] * 4)
case("decoder_stage_post-stream", "dec", "decoder_stage_post-96-r2-Tin2-stream", HOP, DEC + [("conv", 5, 1)], dict(B=34952, C=96, T=HOP, r=2, n=3),
     dict(B=34953, C=96, T=HOP, r=2, n=3), streaming=True, post=True, stream_guard=lambda d: d["B"] * d["C"] * d["T"] * 4)
# the long hop of the fused down-sampling layer (T > 128: the linear core only): its launch path refuses an x of 2^32 bytes
case("dws_conv_stream-r4-long", "dwss", "dws_conv_stream-r4-3x16x32x160", 160, [("pw",), ("conv", 8, 4)], dict(B=419430, K=16, M=32, T=160, r=4),
     dict(B=419431, K=16, M=32, T=160, r=4), streaming=True, stream_guard=lambda d: d["B"] * d["K"] * d["T"] * 4)
# L2 normalisation over the channels
case("l2norm", "l2", "l2norm-3x128x5", 60, PW, dict(B=1, C=128, T=T23 - 1), dict(B=1, C=128, T=T23))
# residual VQ: z / q [B,128,T]; both forms of the encoder through `flags`
case("rvq_encode-mfma", "rvq_enc", "rvq_encode-mfma-8x128x1024", 60, PW, dict(B=1, T=T23 - 1), dict(B=1, T=T23), b3=dict(B=3, T=(1 << 22) + 1), flags=0)
case("rvq_encode-valu", "rvq_enc", "rvq_encode-mfma-8x128x1024", 60, PW, dict(B=1, T=T23 - 1), dict(B=1, T=T23), flags=1)
case("rvq_decode", "rvq_dec", "rvq_decode-2x128x9", 60, PW, dict(B=1, T=T23 - 1), dict(B=1, T=T23))


def legal(c, d) -> bool:
    """the dimensions are ones the form takes (the header's conditions: T % 4, T % stride, whole streams)"""
    f, T = c.family, d["T"]
    if f == "dwss":
        return T % 4 == 0 and T % d["r"] == 0 and T > 128
    if f in ("pw", "dws", "spec", "res", "chain", "pre", "post") or (f == "dw" and d["k"] == 5):
        return T % 4 == 0 and (f != "dws" or T % d["r"] == 0)
    if f in ("enc", "dec"):
        return T % 4 == 0 and T % d["r"] == 0
    if f == "up":
        return (T * d["r"]) % 4 == 0 and d["M"] % 4 == 0
    if f == "stft":
        return T % 4 == 0          # (any T is legal; the per-clip segment form wants whole 4-frame groups of the neighbours it is compared with)
    return T > 0


def step(c) -> int:
    """the distance between two legal sizes of the case's governing dimension (T, or B for a streaming form)"""
    if c.stream_guard is not None:
        return 1
    d = c.sizes["at"]
    if c.family == "up":
        return 2
    if c.family in ("rvq_enc", "rvq_dec", "dwtr", "l2") or (c.family == "dw" and d["k"] != 5):
        return 1
    return 4


# ---- the long clip through the model ------------------------------------------------------------------------------------------------------
MODEL_P = 12800                       # 40 frames of 320 samples
MODEL_T_AT = 11185920                 # 34 956 frames: the fewest whole 4-frame groups whose decoder activation [1, 96, T] reaches 4 GiB
MODEL_T_BELOW = 11184640              # 34 952 frames: one group less, the longest such clip below the limit


def model_pattern(seed: int = 99) -> torch.Tensor:
    """one period `[1, 1, MODEL_P]` of the long clip, as `synth.synth_clips` makes audio (clamped to +-1)"""
    return synth.synth_clips(1, MODEL_P, seed=seed)
