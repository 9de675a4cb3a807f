"""PyTorch-ROCm custom ops (`torch.ops.hilcodec.*`) over the C ABI of `include/hilcodec_amd.h`.

Every entry point of the hot path is registered with the dispatcher through `torch.library`:
  * schema + a CUDA(HIP) implementation = torch tensors -> device pointers -> the hand-written gfx950 kernels
    (ctypes launch on the current HIP stream; PyTorch supplies memory and the stream, no arithmetic);
  * a CPU implementation that raises (there is deliberately no fallback path);
  * a fake (meta) implementation = the op's shape function,
so the module classes are ordinary traceable `nn.Module`s like the reference's (`torch.compile(fullgraph=True)`,
`torch.export`, HIP-graph capture all see plain ops).  All ops are functional (outputs are fresh tensors) except where
a caller hands in persistent streaming state to be overwritten (`hist_out` arguments, declared as mutated).

The public functions below are what `engine.py` and the module classes call; they only normalise arguments and
dispatch through `torch.ops.hilcodec`.  All tensors must be fp32 (indices int64), contiguous, on a GPU."""
from __future__ import annotations

import contextlib
import contextvars
import ctypes
import numbers
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ._lib import DownParams, PostParams, ResblockParams, Spec0Params, UpParams, check, lib
from .audio_level import SP_WORDS
from .downlink import DL_WORDS, DS_WORDS
from .downlink import bucket as downlink_bucket
from .bwe import BW_WORDS, CP_WORDS
from .bwe import bits as bwe_bits
from .dtx import LEVELS, state_words
from .forward import LR_WORDS, SD_WORDS
from .forward_srtp import RT_WORDS as FSRTP_RT_WORDS
from .jitter import AD_WORDS, ST_WORDS
from .report import FA_WORDS, RP_WORDS
from .rate import RC_WORDS, bucket
from .rtx import NK_WORDS, RX_WORDS
from .srtp import KEY_WORDS as SRTP_KEY_WORDS
from .srtp import RX_WORDS as SRTP_RX_WORDS
from .srtp import TX_WORDS as SRTP_TX_WORDS
from .resample import HOP
from .wire import CAP_BYTES, CONCEAL_CODES, NACK_BYTES, REPORT_BYTES, SRTP_TAG_BYTES, TRANSPORT_HEADER, packet_bytes

_LIB = torch.library.Library("hilcodec", "DEF")


def _ptr(t: Optional[Tensor], dtype=torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("hilcodec_amd ops need GPU tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    return t.data_ptr()


def _al16(t: Optional[Tensor]) -> Optional[Tensor]:
    """An input operand the library refuses unless it is 16-byte aligned ("Pointer alignment", class R): a contiguous
    tensor may start at any float of its storage (`rec[:, :, k:k + T]` with B = 1, a cache kept as a view), so such a view is
    copied to a fresh allocation first.  The aligned tensor is returned as it is: no allocation, no launch.  The caller keeps the
    result in a local until the launch is enqueued."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def _al16_out(op: str, **outs: Optional[Tensor]) -> None:
    """Caller-owned outputs of the same class cannot be copied: a misaligned one is an error that names the operand."""
    for name, t in outs.items():
        for i, u in enumerate(t if isinstance(t, (list, tuple)) else [t]):
            if u is not None and u.data_ptr() % 16 != 0:
                which = f"{name}[{i}]" if isinstance(t, (list, tuple)) else name
                raise RuntimeError(f"{op}: `{which}` must be 16-byte aligned (data_ptr() % 16 == {u.data_ptr() % 16}): the kernel writes "
                                   "it as 16-byte words and the caller owns it, so it cannot be copied")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _new(ref: Tensor, *shape, dtype=torch.float32) -> Tensor:
    return torch.empty(shape, device=ref.device, dtype=dtype)


class LaunchTimer:
    """Optional per-launch HIP-event timing on the stream the kernels are launched on (bench.py).
    `work` is the algorithmic work of the launch (flops for the GEMMs, bytes for the HBM-bound ops)."""

    def __init__(self):
        self.records = []          # (kind, work, start_event, end_event, tag)

    def totals(self):
        out = {}
        for kind, work, e0, e1, _tag in self.records:
            t = out.setdefault(kind, [0, 0.0, 0.0])
            t[0] += 1
            t[1] += float(work)
            t[2] += e0.elapsed_time(e1) * 1e-3
        return out                 # kind -> [launches, work, seconds]


_TIMER: contextvars.ContextVar = contextvars.ContextVar("hilcodec_launch_timer", default=None)


@contextlib.contextmanager
def timed_launches(timer: Optional[LaunchTimer] = None):
    """`with ops.timed_launches() as t:` — every launch issued by THIS context (thread / task) inside the block is
    bracketed by HIP events on its launch stream and recorded in `t`.  A context variable, not a module global: another
    thread's launches are neither timed nor slowed down."""
    t = timer if timer is not None else LaunchTimer()
    token = _TIMER.set(t)
    try:
        yield t
    finally:
        _TIMER.reset(token)


class _timed:
    def __init__(self, kind: str, work: float, tag: str = ""):
        self.kind, self.work, self.tag = kind, work, tag
        self.timer = _TIMER.get()

    def __enter__(self):
        if self.timer is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.timer is not None:
            self.e1.record()
            self.timer.records.append((self.kind, self.work, self.e0, self.e1, self.tag))
        return False


def _no_cpu(*_a, **_k):
    raise RuntimeError("hilcodec_amd ops need GPU tensors (no CPU fallback)")


def _register(name: str, schema: str, impl, fake) -> None:
    _LIB.define(f"{name}{schema}")
    _LIB.impl(name, impl, "CUDA")
    _LIB.impl(name, _no_cpu, "CPU")
    torch.library.register_fake(f"hilcodec::{name}", fake, lib=_LIB)


# ======================================================================================================
# GEMM family
# ======================================================================================================
def _pw_conv(x, wt, bias, res, in_scale, in_elu, out_scale):
    B, K, T = x.shape
    M = wt.shape[1]
    if wt.shape[0] != K:
        raise RuntimeError(f"pw_conv: weight rows {wt.shape[0]} != input channels {K}")
    wt = _al16(wt)
    y = _new(x, B, M, T)
    with _timed("pw_conv", 2.0 * B * T * K * M, f"K{K} M{M} T{T}"):
        check(lib.hilc_pw_conv(_ptr(x), _ptr(wt), _ptr(bias), _ptr(res), _ptr(y), B, K, M, T,
                               in_scale, int(in_elu), out_scale, _stream()), "hilc_pw_conv")
    return y


_register("pw_conv", "(Tensor x, Tensor wt, Tensor? bias, Tensor? res, float in_scale, bool in_elu, float out_scale)"
          " -> Tensor", _pw_conv,
          lambda x, wt, bias, res, in_scale, in_elu, out_scale: x.new_empty(x.shape[0], wt.shape[1], x.shape[2]))


def _dws_conv(x, wt, dw_w, dw_b, res, stride, in_scale, in_elu, out_scale, out_elu):
    B, K, T = x.shape
    M, k = wt.shape[1], dw_w.shape[1]
    To = (T + stride - 1) // stride
    wt = _al16(wt)
    y = _new(x, B, M, To)
    with _timed("dws_conv", 2.0 * B * T * K * M, f"K{K} M{M} T{T} k{k} s{stride}"):
        check(lib.hilc_dws_conv(_ptr(x), _ptr(wt), _ptr(dw_w), _ptr(dw_b), _ptr(res), _ptr(y), B, K, M, T, k,
                                stride, in_scale, int(in_elu), out_scale, int(out_elu), _stream()), "hilc_dws_conv")
    return y


_register("dws_conv", "(Tensor x, Tensor wt, Tensor dw_w, Tensor? dw_b, Tensor? res, int stride, float in_scale, "
          "bool in_elu, float out_scale, bool out_elu) -> Tensor", _dws_conv,
          lambda x, wt, dw_w, dw_b, res, stride, in_scale, in_elu, out_scale, out_elu:
          x.new_empty(x.shape[0], wt.shape[1], (x.shape[2] + stride - 1) // stride))


def _dws_conv_stream(x, wt, dw_w, dw_b, hist, hist_out, res, stride, in_scale, in_elu, out_scale, out_elu):
    B, K, T = x.shape
    M, k = wt.shape[1], dw_w.shape[1]
    pad = k - stride
    for h in (hist, hist_out):
        if h is not None and tuple(h.shape) != (B, M, pad):
            raise RuntimeError(f"cache must be [{B},{M},{pad}], got {tuple(h.shape)}")
    wt = _al16(wt)
    if T > 128:                      # hops longer than one tile have no scalar loader
        x = _al16(x)
    elif (k, stride) in ((16, 8), (10, 5)):      # the two shapes whose taps are read as 16- / 8-byte words per row
        dw_w = _al16(dw_w)
    y = _new(x, B, M, T // stride)
    with _timed("dws_conv", 2.0 * B * T * K * M, f"K{K} M{M} T{T} k{k} s{stride} stream"):
        check(lib.hilc_dws_conv_stream(_ptr(x), _ptr(wt), _ptr(dw_w), _ptr(dw_b), _ptr(hist), _ptr(hist_out),
                                       _ptr(res), _ptr(y), B, K, M, T, k, stride, in_scale, int(in_elu), out_scale,
                                       int(out_elu), _stream()), "hilc_dws_conv_stream")
    return y


_register("dws_conv_stream", "(Tensor x, Tensor wt, Tensor dw_w, Tensor? dw_b, Tensor? hist, Tensor(a!) hist_out, "
          "Tensor? res, int stride, float in_scale, bool in_elu, float out_scale, bool out_elu) -> Tensor",
          _dws_conv_stream,
          lambda x, wt, dw_w, dw_b, hist, hist_out, res, stride, in_scale, in_elu, out_scale, out_elu:
          x.new_empty(x.shape[0], wt.shape[1], x.shape[2] // stride))


def _up_conv_expand_taps(tr_w, stride):
    K = tr_w.shape[0]
    out = _new(tr_w, K * stride * 8)
    check(lib.hilc_up_conv_expand_taps(_ptr(tr_w), _ptr(out), K, stride, _stream()), "hilc_up_conv_expand_taps")
    return out


_register("up_conv_expand_taps", "(Tensor tr_w, int stride) -> Tensor", _up_conv_expand_taps,
          lambda tr_w, stride: tr_w.new_empty(tr_w.shape[0] * stride * 8))


def _up_conv(x, hist, hist_out, tr_w, taps, wt, bias, stride, in_scale, in_elu):
    B, K, Tin = x.shape
    M = wt.shape[1]
    for h in (hist, hist_out):
        if h is not None and h.numel() != B * K:
            raise RuntimeError(f"cache must be [{B},{K},1], got {tuple(h.shape)}")
    wt = _al16(wt)
    y = _new(x, B, M, Tin * stride)
    with _timed("up_conv", 2.0 * B * Tin * stride * K * M,
                f"K{K} M{M} Tin{Tin} r{stride}" + (" stream" if hist is not None or hist_out is not None else "")):
        check(lib.hilc_up_conv_expanded(_ptr(x), _ptr(hist), _ptr(hist_out), _ptr(tr_w), _ptr(taps), _ptr(wt),
                                        _ptr(bias), _ptr(y), B, K, M, Tin, stride, in_scale, int(in_elu), _stream()),
              "hilc_up_conv")
    return y


_register("up_conv", "(Tensor x, Tensor? hist, Tensor(a!)? hist_out, Tensor tr_w, Tensor? taps, Tensor wt, Tensor? bias, "
          "int stride, float in_scale, bool in_elu) -> Tensor", _up_conv,
          lambda x, hist, hist_out, tr_w, taps, wt, bias, stride, in_scale, in_elu:
          x.new_empty(x.shape[0], wt.shape[1], x.shape[2] * stride))


def _resblock_pack(wt):
    Cc = wt.shape[0]
    out = _new(wt, Cc * Cc)
    check(lib.hilc_resblock_pack_weights(_ptr(wt), _ptr(out), Cc, _stream()), "hilc_resblock_pack_weights")
    return out


_register("resblock_pack", "(Tensor wt) -> Tensor", _resblock_pack, lambda wt: wt.new_empty(wt.shape[0] * wt.shape[0]))

_SCHED = {}


class SchedWorkspace:
    """Ticket words of the residual-block kernel's tile scheduler (two ints per launch, zero at launch, re-armed by the
    kernel itself) owned by ONE schedule object (graph_step.GraphedHop / PipelinedHop): allocated outside graph capture,
    one slot per launch in call order, so that (i) no allocation or memset node lands inside a capture, (ii) launches that
    run concurrently — the two branches of a pipelined hop, two graphs replayed on different streams — never share a
    ticket (shared words would hand out duplicate or skipped tiles)."""

    def __init__(self, device, slots: int = 64):
        self.words = torch.zeros(2 * slots, dtype=torch.int32, device=device)
        self.slots, self.next = slots, 0

    def take(self) -> Tensor:
        if self.next >= self.slots:
            raise RuntimeError("SchedWorkspace: more residual-block launches than slots")
        w = self.words[2 * self.next:2 * self.next + 2]
        self.next += 1
        return w


_SCHED_WS: contextvars.ContextVar = contextvars.ContextVar("hilcodec_sched_workspace", default=None)


@contextlib.contextmanager
def sched_workspace(ws: Optional[SchedWorkspace]):
    """the residual-block launches of this block take their ticket words from `ws`, slot 0 first"""
    if ws is not None:
        ws.next = 0
    token = _SCHED_WS.set(ws)
    try:
        yield ws
    finally:
        _SCHED_WS.reset(token)


def _sched_buffer(device) -> Tensor:
    """Two zeroed ints for the residual-block kernel's ticket scheduler; the kernel re-arms them itself, so a buffer is
    written by the host only once.  Inside `sched_workspace(...)`: the owner's next slot.  Otherwise one buffer per
    (device, stream): launches on one stream are ordered, so they may share; eager launches only — a captured graph must
    bring its own workspace (allocating here during capture would put a memset node and the buffer into that graph)."""
    ws = _SCHED_WS.get()
    if ws is not None:
        return ws.take()
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("residual-block launch inside a graph capture without ops.sched_workspace(...): "
                           "the ticket words must be allocated by the owner of the graph, outside the capture")
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _SCHED.get(key)
    if buf is None:
        buf = torch.zeros(2, dtype=torch.int32, device=device)
        _SCHED[key] = buf
    return buf


def _resblock(x, w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, hist1, hist2, hist1_out, hist2_out, pre_scale, out_scale):
    B, Cc, T = x.shape
    streaming = hist1_out is not None or hist1 is not None
    for h in (hist1, hist2, hist1_out, hist2_out):
        if h is not None and tuple(h.shape) != (B, Cc, 4):
            raise RuntimeError(f"resblock caches must be [{B},{Cc},4], got {tuple(h.shape)}")
    x, w1p, w2p, hist1, hist2 = _al16(x), _al16(w1p), _al16(w2p), _al16(hist1), _al16(hist2)
    _al16_out("resblock", hist1_out=hist1_out, hist2_out=hist2_out)
    y = torch.empty_like(x)
    with _timed("resblock", 4.0 * B * T * Cc * Cc, f"C{Cc} T{T}" + (" stream" if streaming else "")):
        check(lib.hilc_resblock_balanced(_ptr(x), _ptr(w1p), _ptr(dw1_w), _ptr(dw1_b), _ptr(w2p), _ptr(dw2_w),
                                         _ptr(dw2_b), _ptr(hist1), _ptr(hist2), _ptr(hist1_out), _ptr(hist2_out),
                                         _ptr(y), _ptr(_sched_buffer(x.device), torch.int32), int(streaming), B, Cc, T,
                                         pre_scale, out_scale, _stream()), "hilc_resblock")
    return y


_register("resblock", "(Tensor x, Tensor w1p, Tensor dw1_w, Tensor dw1_b, Tensor w2p, Tensor dw2_w, Tensor dw2_b, "
          "Tensor? hist1, Tensor? hist2, Tensor(a!)? hist1_out, Tensor(b!)? hist2_out, float pre_scale, float out_scale)"
          " -> Tensor", _resblock,
          lambda x, w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, hist1, hist2, hist1_out, hist2_out, pre_scale, out_scale:
          torch.empty_like(x))


def _void(obj):
    """a ctypes struct, or an array of them, as a `const void *` argument of the C ABI"""
    return ctypes.cast(ctypes.pointer(obj), ctypes.c_void_p)


def _al16_blocks(op, params, hist_in, hist_out):
    """The blocks' operands a stage launch refuses unless 16-byte aligned: the two packed matrices of each block (parameters 0 and 3
    of every 6) and the caches.  Inputs are copied where they are not (`_al16`), caches the caller owns as outputs raise."""
    _al16_out(op, hist_out=list(hist_out))
    return [_al16(t) if i % 3 == 0 else t for i, t in enumerate(params)], [_al16(h) for h in hist_in]


def _block_params(op, B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales):
    """The `hilc_resblock_params` array of a stage launch from the flat lists of the op schemas: 6 parameter tensors per block and
    (streaming) 2 caches in + 2 caches out per block, each `[B, C, 4]`; offline no cache at all.  The lists are checked as a whole
    before the first pointer is taken: a kernel indexes them by block and trusts the shapes."""
    n = len(pre_scales)
    if len(params) != 6 * n or len(out_scales) != n or len(hist_in) != (2 * n if streaming else 0) or len(hist_out) != len(hist_in):
        raise RuntimeError(f"{op}: 6 parameter tensors per block, and (streaming) 2 caches in and 2 caches out per block")
    for h in list(hist_in) + list(hist_out):
        if tuple(h.shape) != (B, Cc, 4):
            raise RuntimeError(f"{op}: resblock caches must be [{B},{Cc},4], got {tuple(h.shape)}")
    blocks = (ResblockParams * n)()
    for i in range(n):
        caches = list(hist_in[2 * i:2 * i + 2]) + list(hist_out[2 * i:2 * i + 2]) if streaming else [None] * 4
        blocks[i] = ResblockParams(*[_ptr(t) for t in list(params[6 * i:6 * i + 6]) + caches], float(pre_scales[i]), float(out_scales[i]))
    return blocks


def _down_params(op, y, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride):
    """`hilc_down_params`: the down-sampling layer behind the blocks of an encoder stage launch, writing y `[B, 2C, T / stride]`"""
    B, C2, To = y.shape
    for t, shape in ((dhist, (B, C2, stride)), (dhist_out, (B, C2, stride)), (dres, (B, C2, To))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"{op}: expected {shape}, got {tuple(t.shape)}")
    return DownParams(_ptr(w_lo), _ptr(w_hi), _ptr(ddw_w), _ptr(ddw_b), _ptr(dhist), _ptr(dhist_out), _ptr(dres), _ptr(y),
                      float(in_scale), int(stride))


def _up_params(op, xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride):
    """`hilc_up_params`: the up-sampling layer in front of the blocks of a decoder stage launch, reading xin `[B, 2C, T / stride]`"""
    B, K2, _ = xin.shape
    for h in (uhist, uhist_out):
        if h is not None and h.numel() != B * K2:
            raise RuntimeError(f"{op}: the up-sampling cache must be [{B},{K2},1], got {tuple(h.shape)}")
    return UpParams(_ptr(xin), _ptr(tr_w), _ptr(w_lo), _ptr(w_hi), _ptr(bias), _ptr(uhist), _ptr(uhist_out), float(in_scale), int(stride))


def _resblock_chain(x, params, hist_in, hist_out, pre_scales, out_scales):
    B, Cc, T = x.shape
    streaming = len(hist_in) > 0                   # no caches: the offline causal model (zero padding in front of every clip)
    x = _al16(x)
    params, hist_in = _al16_blocks("resblock_chain", params, hist_in, hist_out)
    blocks = _block_params("resblock_chain", B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales)
    n = len(blocks)
    y = torch.empty_like(x)
    with _timed("resblock", 4.0 * n * B * T * Cc * Cc, f"C{Cc} T{T}" + (" stream" if streaming else "") + f" chain x{n}"):
        check(lib.hilc_resblock_chain(_ptr(x), _ptr(y), _void(blocks), n, int(streaming), B, Cc, T, _stream()), "hilc_resblock_chain")
    return y


_register("resblock_chain", "(Tensor x, Tensor[] params, Tensor[] hist_in, Tensor(a!)[] hist_out, float[] pre_scales, "
          "float[] out_scales) -> Tensor", _resblock_chain,
          lambda x, params, hist_in, hist_out, pre_scales, out_scales: torch.empty_like(x))


def _encoder_stage(x, params, hist_in, hist_out, pre_scales, out_scales, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale,
                   stride):
    B, Cc, T = x.shape
    streaming = dhist_out is not None
    if T % stride != 0:
        raise RuntimeError("encoder_stage: T must be a multiple of the stride")
    x, w_lo, w_hi, dhist, dres = _al16(x), _al16(w_lo), _al16(w_hi), _al16(dhist), _al16(dres)
    if Cc >= 256:                    # the wide stages read a row's taps as 16- / 8-byte words
        ddw_w = _al16(ddw_w)
    params, hist_in = _al16_blocks("encoder_stage", params, hist_in, hist_out)
    _al16_out("encoder_stage", dhist_out=dhist_out)
    blocks = _block_params("encoder_stage", B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales)
    n = len(blocks)
    y = torch.empty(B, 2 * Cc, T // stride, device=x.device, dtype=torch.float32)
    down = _down_params("encoder_stage", y, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride)
    tag = f"C{Cc} T{T}" + (" stream" if streaming else "")
    with _timed("resblock", 4.0 * n * B * T * Cc * Cc + 4.0 * B * T * Cc * Cc, tag + f" stage x{n} + down s{stride}"):
        check(lib.hilc_encoder_stage(_ptr(x), _void(blocks), n, _void(down), int(streaming), B, Cc, T, _stream()), "hilc_encoder_stage")
    return y


_register("encoder_stage", "(Tensor x, Tensor[] params, Tensor[] hist_in, Tensor(a!)[] hist_out, float[] pre_scales, float[] out_scales, "
          "Tensor w_lo, Tensor w_hi, Tensor ddw_w, Tensor ddw_b, Tensor? dhist, Tensor(b!)? dhist_out, Tensor? dres, float in_scale, "
          "int stride) -> Tensor", _encoder_stage,
          lambda x, params, hist_in, hist_out, pre_scales, out_scales, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride:
          x.new_empty(x.shape[0], 2 * x.shape[1], x.shape[2] // stride))


def _decoder_stage(xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride, params, hist_in, hist_out, pre_scales, out_scales):
    B, K2, Tin = xin.shape
    Cc, T = K2 // 2, Tin * stride
    streaming = len(hist_in) > 0 or uhist_out is not None        # no caches at all: the offline causal model
    tr_w, w_lo, w_hi = _al16(tr_w), _al16(w_lo), _al16(w_hi)
    params, hist_in = _al16_blocks("decoder_stage", params, hist_in, hist_out)
    blocks = _block_params("decoder_stage", B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales)
    n = len(blocks)
    up = _up_params("decoder_stage", xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride)
    y = torch.empty(B, Cc, T, device=xin.device, dtype=torch.float32)
    with _timed("resblock", 4.0 * n * B * T * Cc * Cc + 4.0 * B * T * Cc * Cc, f"C{Cc} T{T}" + (" stream" if streaming else "") + f" up r{stride} + stage x{n}"):
        check(lib.hilc_decoder_stage(_void(up), _void(blocks), n, _ptr(y), int(streaming), B, Cc, T, _stream()), "hilc_decoder_stage")
    return y


_register("decoder_stage", "(Tensor xin, Tensor tr_w, Tensor w_lo, Tensor w_hi, Tensor? bias, Tensor? uhist, Tensor(a!)? uhist_out, "
          "float in_scale, int stride, Tensor[] params, Tensor[] hist_in, Tensor(b!)[] hist_out, float[] pre_scales, float[] out_scales) "
          "-> Tensor", _decoder_stage,
          lambda xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride, params, hist_in, hist_out, pre_scales, out_scales:
          xin.new_empty(xin.shape[0], xin.shape[1] // 2, xin.shape[2] * stride))


def _encoder_stage0(wav, wav_hist, dft_packed, nyq_sin, pw_packed, bias, pre_w, pre_b, pre_in_scale, mean, std, normalize, out_scale, params, hist_in,
                    hist_out, pre_scales, out_scales, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride):
    B, one, T = wav.shape
    Cc, k = pre_w.shape
    streaming = dhist_out is not None
    if one != 1 or Cc != 64 or T % stride != 0:
        raise RuntimeError("encoder_stage0: wav [B,1,T], a 64-channel first conv, T a multiple of the stride")
    if wav_hist is not None and (wav_hist.shape[0] != B or wav_hist.numel() // B < 63):
        raise RuntimeError(f"encoder_stage0: the waveform history must be [{B},1,>=63], got {tuple(wav_hist.shape)}")
    dft_packed, pw_packed, w_lo, w_hi, dhist, dres = _al16(dft_packed), _al16(pw_packed), _al16(w_lo), _al16(w_hi), _al16(dhist), _al16(dres)
    params, hist_in = _al16_blocks("encoder_stage0", params, hist_in, hist_out)
    _al16_out("encoder_stage0", dhist_out=dhist_out)
    blocks = _block_params("encoder_stage0", B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales)
    n = len(blocks)
    y = torch.empty(B, 2 * Cc, T // stride, device=wav.device, dtype=torch.float32)
    down = _down_params("encoder_stage0", y, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride)
    wh = wav_hist.reshape(B, -1) if wav_hist is not None else None
    spec = Spec0Params(_ptr(wav), _ptr(dft_packed), _ptr(nyq_sin), _ptr(pw_packed), _ptr(bias), _ptr(pre_w), _ptr(pre_b),
                       _ptr(wh), int(wh.shape[1]) if wh is not None else 0, float(pre_in_scale),
                       float(mean), float(std), float(out_scale), int(normalize), 64, 1, int(pre_w.shape[1]))
    work = 2.0 * B * T * 64 * (64 + 1 + 32 + 1) + 2.0 * B * T * Cc * k + 4.0 * n * B * T * Cc * Cc + 4.0 * B * T * Cc * Cc
    with _timed("resblock", work, f"C{Cc} T{T}" + (" stream" if streaming else "") + f" conv_pre + spec N64 + stage x{n} + down s{stride}"):
        check(lib.hilc_encoder_stage0(_void(spec), _void(blocks), n, _void(down), int(streaming), B, T, _stream()), "hilc_encoder_stage0")
    return y


_register("encoder_stage0", "(Tensor wav, Tensor? wav_hist, Tensor dft_packed, Tensor nyq_sin, Tensor pw_packed, Tensor? bias, Tensor pre_w, Tensor? pre_b, "
          "float pre_in_scale, float mean, float std, int normalize, float out_scale, Tensor[] params, Tensor[] hist_in, Tensor(a!)[] hist_out, "
          "float[] pre_scales, float[] out_scales, Tensor w_lo, Tensor w_hi, Tensor ddw_w, Tensor ddw_b, Tensor? dhist, Tensor(b!)? dhist_out, "
          "Tensor? dres, float in_scale, int stride) -> Tensor", _encoder_stage0,
          lambda wav, wav_hist, dft_packed, nyq_sin, pw_packed, bias, pre_w, pre_b, pre_in_scale, mean, std, normalize, out_scale, params, hist_in,
          hist_out, pre_scales, out_scales, w_lo, w_hi, ddw_w, ddw_b, dhist, dhist_out, dres, in_scale, stride:
          wav.new_empty(wav.shape[0], 2 * pre_w.shape[0], wav.shape[2] // stride))


def _decoder_stage_post(xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride, params, hist_in, hist_out, pre_scales, out_scales,
                        post_w, post_b, post_hist, post_hist_out, post_in_scale, post_out_scale, do_tanh):
    B, K2, Tin = xin.shape
    Cc, T = K2 // 2, Tin * stride
    streaming = len(hist_in) > 0 or uhist_out is not None or post_hist_out is not None      # no caches at all: the offline causal model
    if post_w.dim() != 2 or post_w.shape[0] != Cc:
        raise RuntimeError(f"decoder_stage_post: the closing conv's taps must be [{Cc}, k], got {tuple(post_w.shape)}")
    for h in (post_hist, post_hist_out):
        if h is not None and tuple(h.shape) != (B, Cc, post_w.shape[1] - 1):
            raise RuntimeError(f"decoder_stage_post: the closing conv's cache must be [{B},{Cc},{post_w.shape[1] - 1}], got {tuple(h.shape)}")
    tr_w, w_lo, w_hi, post_hist = _al16(tr_w), _al16(w_lo), _al16(w_hi), _al16(post_hist)
    params, hist_in = _al16_blocks("decoder_stage_post", params, hist_in, hist_out)
    _al16_out("decoder_stage_post", post_hist_out=post_hist_out)
    blocks = _block_params("decoder_stage_post", B, Cc, streaming, params, hist_in, hist_out, pre_scales, out_scales)
    n = len(blocks)
    up = _up_params("decoder_stage_post", xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride)
    wav = torch.empty(B, 1, T, device=xin.device, dtype=torch.float32)
    post = PostParams(_ptr(post_w), _ptr(post_b), _ptr(wav), _ptr(post_hist), _ptr(post_hist_out), float(post_in_scale), float(post_out_scale),
                      int(do_tanh), int(post_w.shape[1]))
    with _timed("resblock", 4.0 * n * B * T * Cc * Cc + 4.0 * B * T * Cc * Cc, f"C{Cc} T{T}" + (" stream" if streaming else "") + f" up r{stride} + stage x{n} + conv_post"):
        check(lib.hilc_decoder_stage_post(_void(up), _void(blocks), n, _void(post), int(streaming), B, Cc, T, _stream()), "hilc_decoder_stage_post")
    return wav


_register("decoder_stage_post", "(Tensor xin, Tensor tr_w, Tensor w_lo, Tensor w_hi, Tensor? bias, Tensor? uhist, Tensor(a!)? uhist_out, float in_scale, "
          "int stride, Tensor[] params, Tensor[] hist_in, Tensor(b!)[] hist_out, float[] pre_scales, float[] out_scales, Tensor post_w, Tensor? post_b, "
          "Tensor? post_hist, Tensor(c!)? post_hist_out, float post_in_scale, float post_out_scale, bool do_tanh) -> Tensor",
          _decoder_stage_post,
          lambda xin, tr_w, w_lo, w_hi, bias, uhist, uhist_out, in_scale, stride, params, hist_in, hist_out, pre_scales, out_scales, post_w, post_b,
          post_hist, post_hist_out, post_in_scale, post_out_scale, do_tanh: xin.new_empty(xin.shape[0], 1, xin.shape[2] * stride))


def _resblock_pack_rc(wt, row_classes):
    Cc = wt.shape[0]
    out = torch.empty(Cc * Cc, device=wt.device, dtype=torch.float32)
    check(lib.hilc_resblock_pack_weights_rc(_ptr(wt), _ptr(out), Cc, int(row_classes), _stream()), "hilc_resblock_pack_weights_rc")
    return out


_register("resblock_pack_rc", "(Tensor wt, int row_classes) -> Tensor", _resblock_pack_rc,
          lambda wt, row_classes: wt.new_empty(wt.shape[0] * wt.shape[0]))


# ======================================================================================================
# HBM-bound element-wise ops
# ======================================================================================================
def _dw_conv(x, hist, w, bias, res, hist_out, stride, in_scale, in_elu, out_scale, out_elu):
    B, Cc, T = x.shape
    k = w.shape[1]
    To = (T + stride - 1) // stride
    y = _new(x, B, Cc, To)
    with _timed("dw_conv", 4.0 * B * Cc * (T + To * (2 if res is not None else 1)), f"C{Cc} T{T} k{k} s{stride}"):
        check(lib.hilc_dw_conv(_ptr(x), _ptr(hist), _ptr(w), _ptr(bias), _ptr(res), _ptr(y), _ptr(hist_out),
                               B, Cc, T, k, stride, in_scale, int(in_elu), out_scale, int(out_elu), _stream()),
              "hilc_dw_conv")
    return y


_register("dw_conv", "(Tensor x, Tensor? hist, Tensor w, Tensor? bias, Tensor? res, Tensor(a!)? hist_out, int stride, "
          "float in_scale, bool in_elu, float out_scale, bool out_elu) -> Tensor", _dw_conv,
          lambda x, hist, w, bias, res, hist_out, stride, in_scale, in_elu, out_scale, out_elu:
          x.new_empty(x.shape[0], x.shape[1], (x.shape[2] + stride - 1) // stride))


def _dw_convtr(x, hist, w, hist_out, stride, in_scale, in_elu):
    B, Cc, T = x.shape
    if w.shape[1] != 2 * stride:
        raise RuntimeError("dw_convtr: kernel size must be 2 * stride")
    y = _new(x, B, Cc, T * stride)
    with _timed("dw_convtr", 4.0 * B * Cc * T * (1 + stride), f"C{Cc} T{T} r{stride}"):
        check(lib.hilc_dw_convtr(_ptr(x), _ptr(hist), _ptr(w), _ptr(y), _ptr(hist_out), B, Cc, T, stride,
                                 in_scale, int(in_elu), _stream()), "hilc_dw_convtr")
    return y


_register("dw_convtr", "(Tensor x, Tensor? hist, Tensor w, Tensor(a!)? hist_out, int stride, float in_scale, bool in_elu)"
          " -> Tensor", _dw_convtr,
          lambda x, hist, w, hist_out, stride, in_scale, in_elu: x.new_empty(x.shape[0], x.shape[1], x.shape[2] * stride))


def _conv_pre(wav, hist, w, bias, in_scale):
    B, one, T = wav.shape
    if one != 1:
        raise RuntimeError("conv_pre expects a [B,1,T] waveform")
    Cc, k = w.shape
    y = _new(wav, B, Cc, T)
    hl = hist.shape[-1] if hist is not None else 0
    with _timed("conv_pre", 4.0 * B * T * (1 + Cc)):
        check(lib.hilc_conv_pre(_ptr(wav), _ptr(hist), hl, _ptr(w), _ptr(bias), _ptr(y), B, Cc, T, k,
                                in_scale, _stream()), "hilc_conv_pre")
    return y


_register("conv_pre", "(Tensor wav, Tensor? hist, Tensor w, Tensor? bias, float in_scale) -> Tensor", _conv_pre,
          lambda wav, hist, w, bias, in_scale: wav.new_empty(wav.shape[0], w.shape[0], wav.shape[2]))


def _conv_post(x, hist, w, bias, hist_out, in_scale, in_elu, out_scale, do_tanh):
    B, Cc, T = x.shape
    k = w.shape[1]
    # not refused, but the one fall-back that is not bit-identical: the generic kernel sums the channels in sequence, the 16-byte path
    # in eight classes (include/hilcodec_amd.h).  The model's waveform must not depend on where a view starts: copy, keep the class order.
    x, hist = _al16(x), _al16(hist)
    y = _new(x, B, 1, T)
    with _timed("conv_post", 4.0 * B * T * (1 + Cc)):
        check(lib.hilc_conv_post(_ptr(x), _ptr(hist), _ptr(w), _ptr(bias), _ptr(y), _ptr(hist_out), B, Cc, T, k,
                                 in_scale, int(in_elu), out_scale, int(do_tanh), _stream()), "hilc_conv_post")
    return y


_register("conv_post", "(Tensor x, Tensor? hist, Tensor w, Tensor? bias, Tensor(a!)? hist_out, float in_scale, "
          "bool in_elu, float out_scale, bool do_tanh) -> Tensor", _conv_post,
          lambda x, hist, w, bias, hist_out, in_scale, in_elu, out_scale, do_tanh: x.new_empty(x.shape[0], 1, x.shape[2]))


def _stft_logmag(wav, hist, basis_t, n_fft, hop, mean, std, normalize):
    B, one, T = wav.shape
    Tf = (T - 1) // hop + 1
    basis_t = _al16(basis_t)
    spec = _new(wav, B, n_fft // 2 + 1, Tf)
    hl = hist.shape[-1] if hist is not None else 0
    with _timed("stft", 2.0 * B * Tf * n_fft * (n_fft + 2), f"N{n_fft} hop{hop}"):
        check(lib.hilc_stft_logmag(_ptr(wav), _ptr(hist), hl, _ptr(basis_t), _ptr(spec), B, T, n_fft, hop,
                                   mean, std, normalize, _stream()), "hilc_stft_logmag")
    return spec


_register("stft_logmag", "(Tensor wav, Tensor? hist, Tensor basis_t, int n_fft, int hop, float mean, float std, "
          "int normalize) -> Tensor", _stft_logmag,
          lambda wav, hist, basis_t, n_fft, hop, mean, std, normalize:
          wav.new_empty(wav.shape[0], n_fft // 2 + 1, (wav.shape[2] - 1) // hop + 1))


def _spec_block_pack(w, n_fft, which):
    out = _new(w, lib.hilc_spec_block_packed_floats(n_fft, which))
    check(lib.hilc_spec_block_pack(_ptr(w), _ptr(out), w.shape[0], n_fft, which, _stream()), "hilc_spec_block_pack")
    return out


_register("spec_block_pack", "(Tensor w, int n_fft, int which) -> Tensor", _spec_block_pack,
          lambda w, n_fft, which: w.new_empty(lib.hilc_spec_block_packed_floats(n_fft, which)))


def _spec_block(wav, hist, dft_packed, nyq_sin, pw_packed, bias, x, n_fft, hop, mean, std, normalize, out_scale):
    B, one, T = wav.shape
    hl = hist.shape[-1] if hist is not None else 0
    Tf = (T - 1) // hop + 1
    if x is not None and tuple(x.shape) != (B, n_fft, Tf):
        raise RuntimeError(f"spec_block: x must be [{B},{n_fft},{Tf}], got {tuple(x.shape)}")
    x, dft_packed, pw_packed = _al16(x), _al16(dft_packed), _al16(pw_packed)
    y = torch.empty(B, n_fft, Tf, device=wav.device, dtype=torch.float32)
    with _timed("spec_block", 2.0 * B * Tf * n_fft * (n_fft + 1 + n_fft // 2 + 1), f"N{n_fft} hop{hop}"):
        check(lib.hilc_spec_block(_ptr(wav), _ptr(hist), hl, _ptr(dft_packed), _ptr(nyq_sin), _ptr(pw_packed), _ptr(bias), _ptr(x), _ptr(y),
                                  B, T, n_fft, hop, mean, std, normalize, out_scale, _stream()), "hilc_spec_block")
    return y


_register("spec_block", "(Tensor wav, Tensor? hist, Tensor dft_packed, Tensor nyq_sin, Tensor pw_packed, Tensor? bias, Tensor? x, "
          "int n_fft, int hop, float mean, float std, int normalize, float out_scale) -> Tensor", _spec_block,
          lambda wav, hist, dft_packed, nyq_sin, pw_packed, bias, x, n_fft, hop, mean, std, normalize, out_scale:
          wav.new_empty(wav.shape[0], n_fft, (wav.shape[2] - 1) // hop + 1))


def _spec_block_conv_pre(wav, hist, dft_packed, nyq_sin, pw_packed, bias, pre_w, pre_b, pre_in_scale, n_fft, hop, mean, std,
                         normalize, out_scale):
    B, one, T = wav.shape
    hl = hist.shape[-1] if hist is not None else 0
    Cc, k = pre_w.shape
    dft_packed, pw_packed = _al16(dft_packed), _al16(pw_packed)
    y = _new(wav, B, Cc, T)
    with _timed("spec_block", 2.0 * B * T * n_fft * (n_fft + 1 + n_fft // 2 + 1) + 2.0 * B * T * Cc * k,
                f"N{n_fft} hop{hop} +conv_pre"):
        check(lib.hilc_spec_block_conv_pre(_ptr(wav), _ptr(hist), hl, _ptr(dft_packed), _ptr(nyq_sin), _ptr(pw_packed), _ptr(bias),
                                           _ptr(pre_w), _ptr(pre_b), pre_in_scale, _ptr(y), B, T, n_fft, hop, k, mean, std,
                                           normalize, out_scale, _stream()), "hilc_spec_block_conv_pre")
    return y


_register("spec_block_conv_pre", "(Tensor wav, Tensor? hist, Tensor dft_packed, Tensor nyq_sin, Tensor pw_packed, Tensor? bias, "
          "Tensor pre_w, Tensor? pre_b, float pre_in_scale, int n_fft, int hop, float mean, float std, int normalize, "
          "float out_scale) -> Tensor", _spec_block_conv_pre,
          lambda wav, hist, dft_packed, nyq_sin, pw_packed, bias, pre_w, pre_b, pre_in_scale, n_fft, hop, mean, std, normalize,
          out_scale: wav.new_empty(wav.shape[0], pre_w.shape[0], wav.shape[2]))


def _tail(x, hist, out):
    B, Cc, T = x.shape
    pad = out.shape[-1]
    hl = hist.shape[-1] if hist is not None else 0
    check(lib.hilc_tail(_ptr(x), _ptr(hist), _ptr(out), B * Cc, T, pad, hl, _stream()), "hilc_tail")


_register("tail", "(Tensor x, Tensor? hist, Tensor(a!) out) -> ()", _tail, lambda x, hist, out: None)


def _l2norm(x, eps, scale, channel_last_out):
    B, Cc, T = x.shape
    y = _new(x, *((B, T, Cc) if channel_last_out else (B, Cc, T)))
    check(lib.hilc_l2norm(_ptr(x), _ptr(y), B, Cc, T, eps, scale, int(channel_last_out), _stream()), "hilc_l2norm")
    return y


_register("l2norm", "(Tensor x, float eps, float scale, bool channel_last_out) -> Tensor", _l2norm,
          lambda x, eps, scale, channel_last_out:
          x.new_empty(*((x.shape[0], x.shape[2], x.shape[1]) if channel_last_out else x.shape)))


# ======================================================================================================
# residual VQ
# ======================================================================================================
def _zct(z, channel_last):
    if channel_last:
        B, T, Cc = z.shape
    else:
        B, Cc, T = z.shape
    return B, Cc, T


RVQ_VALU_ONLY = 1      # include/hilcodec_amd.h: HILC_RVQ_VALU_ONLY


def _rvq_encode(z, codebooks, codebooks_t, norms, n_clip, n, channel_last, stage_major, want_q, want_loss, flags):
    B, Cc, T = _zct(z, channel_last)
    Nq, K, _ = codebooks.shape
    rows = max(1, min(n, Nq))
    idx = _new(z, *((rows, B, T) if stage_major else (B, rows, T)), dtype=torch.int64)
    q = torch.empty_like(z) if want_q else None
    ferr = _new(z, B * T) if want_loss else None
    with _timed("rvq_encode", 2.0 * B * T * K * Cc * rows):
        check(lib.hilc_rvq_encode_mixed(_ptr(z), _ptr(codebooks), _ptr(codebooks_t), _ptr(norms),
                                        _ptr(n_clip, torch.int32), _ptr(idx, torch.int64), _ptr(q), _ptr(ferr),
                                        B, Cc, T, K, Nq, n, int(channel_last), int(stage_major), int(flags), _stream()),
              "hilc_rvq_encode")
    loss = None
    if want_loss:
        loss = _new(z)
        check(lib.hilc_mse_finalize(_ptr(ferr), _ptr(loss), B * T, float(B) * T * Cc, _stream()), "hilc_mse_finalize")
    # the dispatcher wants real tensors for every declared output
    return idx, (q if q is not None else _new(z, 0)), (loss if loss is not None else _new(z, 0))


def _rvq_encode_fake(z, codebooks, codebooks_t, norms, n_clip, n, channel_last, stage_major, want_q, want_loss, flags):
    B, Cc, T = _zct(z, channel_last)
    rows = max(1, min(n, codebooks.shape[0]))
    idx = z.new_empty(*((rows, B, T) if stage_major else (B, rows, T)), dtype=torch.int64)
    return idx, (torch.empty_like(z) if want_q else z.new_empty(0)), (z.new_empty(()) if want_loss else z.new_empty(0))


_register("rvq_encode", "(Tensor z, Tensor codebooks, Tensor codebooks_t, Tensor norms, Tensor? n_clip, int n, "
          "bool channel_last, bool stage_major, bool want_q, bool want_loss, int flags) -> (Tensor, Tensor, Tensor)",
          _rvq_encode, _rvq_encode_fake)


def _rvq_decode(indices, codebooks, n_clip, n, channel_last, stage_major):
    if stage_major:
        _, B, T = indices.shape
    else:
        B, _, T = indices.shape
    Nq, K, Cc = codebooks.shape
    q = _new(codebooks, *((B, T, Cc) if channel_last else (B, Cc, T)))
    check(lib.hilc_rvq_decode_mixed(_ptr(indices, torch.int64), _ptr(codebooks), _ptr(n_clip, torch.int32), _ptr(q),
                                    B, Cc, T, K, Nq, n, int(channel_last), int(stage_major), _stream()),
          "hilc_rvq_decode")
    return q


def _rvq_decode_fake(indices, codebooks, n_clip, n, channel_last, stage_major):
    B, T = (indices.shape[1], indices.shape[2]) if stage_major else (indices.shape[0], indices.shape[2])
    Cc = codebooks.shape[2]
    return codebooks.new_empty(*((B, T, Cc) if channel_last else (B, Cc, T)))


_register("rvq_decode", "(Tensor indices, Tensor codebooks, Tensor? n_clip, int n, bool channel_last, bool stage_major)"
          " -> Tensor", _rvq_decode, _rvq_decode_fake)


def _rvq_ema_stats(z, codebooks, indices, n, channel_last, stage_major):
    B, Cc, T = _zct(z, channel_last)
    Nq, K, _ = codebooks.shape
    rows = indices.shape[0] if stage_major else indices.shape[1]
    bucket = _new(z, n, K + K * Cc)
    with _timed("rvq_ema_stats", 4.0 * B * T * Cc * n):
        check(lib.hilc_rvq_ema_stats(_ptr(z), _ptr(codebooks), _ptr(indices, torch.int64), _ptr(bucket), B, Cc, T, K,
                                     n, rows, int(channel_last), int(stage_major), _stream()), "hilc_rvq_ema_stats")
    return bucket


_register("rvq_ema_stats", "(Tensor z, Tensor codebooks, Tensor indices, int n, bool channel_last, bool stage_major)"
          " -> Tensor", _rvq_ema_stats,
          lambda z, codebooks, indices, n, channel_last, stage_major:
          z.new_empty(n, codebooks.shape[1] * (1 + codebooks.shape[2])))


def _rvq_ema_update(embed, ema_num, ema_embed, bucket, decay):
    n, K, Cc = embed.shape
    if tuple(ema_num.shape) != (n, K) or tuple(ema_embed.shape) != (n, K, Cc) or tuple(bucket.shape) != (n, K + K * Cc):
        raise RuntimeError("rvq_ema_update: inconsistent shapes")
    check(lib.hilc_rvq_ema_update(_ptr(embed), _ptr(ema_num), _ptr(ema_embed), _ptr(bucket), float(decay), K, Cc, n,
                                  _stream()), "hilc_rvq_ema_update")


_register("rvq_ema_update", "(Tensor(a!) embed, Tensor(b!) ema_num, Tensor(c!) ema_embed, Tensor bucket, float decay)"
          " -> ()", _rvq_ema_update, lambda embed, ema_num, ema_embed, bucket, decay: None)

# ======================================================================================================
# per-stream session state (graph_step.GraphedHop(sessions=True))
# ======================================================================================================
class StateLayout:
    """Where every stream's part of every cache lies in one state block (graph_step.StateBlock; the layout of
    hilc_state_slots_apply / _gather): cache k, a `[streams, C, L]` tensor, starts at float `off[k]` (16-B aligned) and stream
    b's part of it is the `lens[k]` = C*L floats at `off[k] + b * lens[k]`.  A record is one stream's parts concatenated in
    order (`record_len` floats).  Host-only (no device needed); `tables(device)` gives the kernels' device arrays."""

    def __init__(self, shapes: Sequence[Sequence[int]], n_enc: int):
        """shapes: the `[streams, C, L]` shape of every cache in the reference's order, the first `n_enc` the encoder's"""
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.n_enc = int(n_enc)
        self.streams = self.shapes[0][0]
        if any(len(s) != 3 or s[0] != self.streams for s in self.shapes):
            raise ValueError("StateLayout: every cache must be [streams, C, L] with the same streams")
        self.off: List[int] = []
        self.lens: List[int] = []
        total = 0
        for s in self.shapes:
            self.off.append(total)
            self.lens.append(s[1] * s[2])
            total += (s[0] * s[1] * s[2] + 3) // 4 * 4
        self.total = total                       # floats of the block
        self.record_len = sum(self.lens)
        self._tables = {}

    def tables(self, device) -> Tuple[Tensor, Tensor]:
        """(slice_off int64, slice_len int32) on `device`, built once (before a graph capture: the first hop warms them)"""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = (torch.tensor(self.off, dtype=torch.int64, device=device),
                                 torch.tensor(self.lens, dtype=torch.int32, device=device))
        return self._tables[key]

    def record(self, cache_enc: Sequence[Tensor], cache_dec: Sequence[Tensor]) -> Tensor:
        """one stream's caches (B = 1 tensors, the format of `wire.load_cache_npz(..., batch=1)`) -> its flat fp32 record, on
        the first cache's device; ValueError if a count or a shape does not match"""
        caches = list(cache_enc) + list(cache_dec)
        if len(cache_enc) != self.n_enc or len(caches) != len(self.shapes):
            raise ValueError(f"expected {self.n_enc} + {len(self.shapes) - self.n_enc} caches, got {len(cache_enc)} + {len(cache_dec)}")
        for k, (c, s) in enumerate(zip(caches, self.shapes)):
            if tuple(c.shape) != (1,) + s[1:]:
                raise ValueError(f"cache {k}: expected shape {(1,) + s[1:]}, got {tuple(c.shape)}")
        dev = caches[0].device
        return torch.cat([c.detach().reshape(-1).to(dev, torch.float32) for c in caches])

    def split(self, record: Tensor) -> Tuple[List[Tensor], List[Tensor]]:
        """a flat record -> (encoder caches, decoder caches) as B = 1 views of it"""
        out, o = [], 0
        for s, n in zip(self.shapes, self.lens):
            out.append(record[o:o + n].view(1, s[1], s[2]))
            o += n
        return out[:self.n_enc], out[self.n_enc:]


def _state_slots_apply(block, slice_off, slice_len, action, records):
    if slice_len.numel() != slice_off.numel():
        raise RuntimeError("state_slots_apply: slice_off and slice_len differ in length")
    nrec = 0 if records is None else records.shape[0]
    check(lib.hilc_state_slots_apply(_ptr(block), _ptr(slice_off, torch.int64), _ptr(slice_len, torch.int32), slice_off.numel(),
                                     action.numel(), _ptr(action, torch.int32), _ptr(records), nrec, _stream()),
          "hilc_state_slots_apply")


_register("state_slots_apply", "(Tensor(a!) block, Tensor slice_off, Tensor slice_len, Tensor action, Tensor? records) -> ()",
          _state_slots_apply, lambda block, slice_off, slice_len, action, records: None)


def _state_slots_gather(block, slice_off, slice_len, slots, streams, record_len):
    if slice_len.numel() != slice_off.numel():
        raise RuntimeError("state_slots_gather: slice_off and slice_len differ in length")
    rec = _new(block, slots.numel(), record_len)
    check(lib.hilc_state_slots_gather(_ptr(block), _ptr(slice_off, torch.int64), _ptr(slice_len, torch.int32), slice_off.numel(),
                                      streams, _ptr(slots, torch.int32), slots.numel(), _ptr(rec), _stream()),
          "hilc_state_slots_gather")
    return rec


_register("state_slots_gather", "(Tensor block, Tensor slice_off, Tensor slice_len, Tensor slots, int streams, int record_len)"
          " -> Tensor", _state_slots_gather,
          lambda block, slice_off, slice_len, slots, streams, record_len: block.new_empty(slots.shape[0], record_len))


def _state_slots_hold(src, dst, slice_off, slice_len, hold, wav, indices, packets, nbytes):
    if slice_len.numel() != slice_off.numel():
        raise RuntimeError("state_slots_hold: slice_off and slice_len differ in length")
    B = hold.numel()
    n_max, frames = (0, 0) if indices is None else (indices.shape[0], indices.shape[2])
    check(lib.hilc_state_slots_hold(_ptr(src), _ptr(dst), _ptr(slice_off, torch.int64), _ptr(slice_len, torch.int32),
                                    slice_off.numel(), B, _ptr(hold, torch.int32), _ptr(wav), 0 if wav is None else wav.numel() // B,
                                    _ptr(indices, torch.int64), n_max, frames, _ptr(packets, torch.uint8),
                                    0 if packets is None else packets.shape[1], _ptr(nbytes, torch.int32), _stream()),
          "hilc_state_slots_hold")


_register("state_slots_hold", "(Tensor src, Tensor(a!) dst, Tensor slice_off, Tensor slice_len, Tensor hold, Tensor(b!)? wav, "
          "Tensor(c!)? indices, Tensor(d!)? packets, Tensor(e!)? nbytes) -> ()", _state_slots_hold,
          lambda src, dst, slice_off, slice_len, hold, wav, indices, packets, nbytes: None)


# ======================================================================================================
# per-stream 10-bit packets (graph_step.GraphedEncodeHop / GraphedDecodeHop; format: wire.packet_bytes)
# ======================================================================================================
def _rows(op: str, B: int, **rows) -> None:
    """the optional per-slot rows of a side kernel: each one given has B entries"""
    for name, row in rows.items():
        if row is not None and row.numel() != B:
            raise RuntimeError(f"{op}: {name} needs {B} entries")


def _pack_codes_10bit(indices, n_clip):
    n, B, T = indices.shape
    packets = _new(indices, B, packet_bytes(n, T), dtype=torch.uint8)
    nbytes = _new(indices, B, dtype=torch.int32)
    check(lib.hilc_pack_codes_10bit(_ptr(indices, torch.int64), _ptr(n_clip, torch.int32), _ptr(packets, torch.uint8),
                                    _ptr(nbytes, torch.int32), B, T, n, _stream()), "hilc_pack_codes_10bit")
    return packets, nbytes


def _pack_codes_10bit_fake(indices, n_clip):
    n, B, T = indices.shape
    return indices.new_empty(B, packet_bytes(n, T), dtype=torch.uint8), indices.new_empty(B, dtype=torch.int32)


_register("pack_codes_10bit", "(Tensor indices, Tensor? n_clip) -> (Tensor, Tensor)", _pack_codes_10bit, _pack_codes_10bit_fake)


def _rvq_decode_packed(packets, n_clip, codebooks, n, frames):
    B = packets.shape[0]
    Nq, K, Cc = codebooks.shape
    if packets.dim() != 2 or packets.shape[1] != packet_bytes(n, frames):
        raise RuntimeError(f"rvq_decode_packed: packets must be [B, {packet_bytes(n, frames)}] for n = {n}, {frames} frames")
    q = _new(codebooks, B, frames, Cc)
    check(lib.hilc_rvq_decode_packed(_ptr(packets, torch.uint8), _ptr(n_clip, torch.int32), _ptr(codebooks), _ptr(q), B, Cc, frames, K,
                                     Nq, n, _stream()), "hilc_rvq_decode_packed")
    return q


_register("rvq_decode_packed", "(Tensor packets, Tensor? n_clip, Tensor codebooks, int n, int frames) -> Tensor", _rvq_decode_packed,
          lambda packets, n_clip, codebooks, n, frames: codebooks.new_empty(packets.shape[0], frames, codebooks.shape[2]))


# ======================================================================================================
# loss concealment of the receiver (graph_step.GraphedDecodeHop(conceal=True); semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _conceal_prepare(state, action, hold, lost, n_slot, packets, frames, fade_hops):
    B = action.numel()
    if state.dim() != 2 or state.shape[0] != B or hold.numel() != B or lost.numel() != B or n_slot.numel() != B:
        raise RuntimeError(f"conceal_prepare: state must be [{B}, n_max + {CONCEAL_CODES}] and hold, lost, n_slot [{B}]")
    n_max = state.shape[1] - CONCEAL_CODES
    if packets.dim() != 2 or packets.shape[0] != B or packets.shape[1] != packet_bytes(max(n_max, 0), frames):
        raise RuntimeError(f"conceal_prepare: packets must be [{B}, {packet_bytes(max(n_max, 0), frames)}]")
    ramp = _new(state, B, dtype=torch.int32)
    check(lib.hilc_conceal_prepare(_ptr(state, torch.int32), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(lost, torch.int32),
                                   _ptr(n_slot, torch.int32), _ptr(packets, torch.uint8), _ptr(ramp, torch.int32), B, frames, n_max,
                                   fade_hops, _stream()), "hilc_conceal_prepare")
    return ramp


_register("conceal_prepare", "(Tensor(a!) state, Tensor action, Tensor(b!) hold, Tensor lost, Tensor(c!) n_slot, Tensor(d!) packets, "
          "int frames, int fade_hops) -> Tensor", _conceal_prepare,
          lambda state, action, hold, lost, n_slot, packets, frames, fade_hops: state.new_empty(action.shape[0], dtype=torch.int32))


def _conceal_gain(wav, ramp, gains, weights):
    B = ramp.numel()
    if wav.shape[0] != B or wav.numel() == 0 or weights.numel() * B != wav.numel() or gains.numel() < 2:
        raise RuntimeError(f"conceal_gain: wav must be [{B}, ...] with weights.numel() samples per row, gains [fade_hops + 1]")
    check(lib.hilc_conceal_gain(_ptr(wav), _ptr(ramp, torch.int32), _ptr(gains), _ptr(weights), B, weights.numel(), gains.numel() - 1,
                                _stream()), "hilc_conceal_gain")


_register("conceal_gain", "(Tensor(a!) wav, Tensor ramp, Tensor gains, Tensor weights) -> ()", _conceal_gain,
          lambda wav, ramp, gains, weights: None)

# ======================================================================================================
# sample-rate conversion at the codec's input and output (hilcodec_amd/resample.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _resample_len(T, L, M):
    return (T * L + M - 1) // M


def _resample_poly(x, hist_in, hist_out, taps, L, M):
    if x.dim() != 3 or x.shape[1] != 1 or x.shape[2] < 1 or taps.dim() != 2 or taps.shape[0] != L:
        raise RuntimeError(f"resample_poly: x must be [B, 1, T >= 1] and taps [L = {L}, Q]")
    B, _, T = x.shape
    Q = taps.shape[1]
    for name, h in (("hist_in", hist_in), ("hist_out", hist_out)):
        if h is not None and h.numel() != B * (Q - 1):
            raise RuntimeError(f"resample_poly: {name} must be [{B}, 1, {Q - 1}]")
    y = _new(x, B, 1, _resample_len(T, L, M))
    check(lib.hilc_resample_poly(_ptr(x), _ptr(hist_in), _ptr(hist_out), _ptr(y), _ptr(taps), B, T, L, M, Q, _stream()),
          "hilc_resample_poly")
    return y


_register("resample_poly", "(Tensor x, Tensor? hist_in, Tensor(a!)? hist_out, Tensor taps, int L, int M) -> Tensor", _resample_poly,
          lambda x, hist_in, hist_out, taps, L, M: x.new_empty(x.shape[0], 1, _resample_len(x.shape[2], L, M)))

# ======================================================================================================
# in-band forward error correction of the sender / receiver (graph_step.GraphedEncodeHop / GraphedDecodeHop(fec_stages=m);
# format: wire.fec_packet_bytes; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _pack_codes_10bit_fec(indices, n_clip, prev_in, prev_out, action, hold, m):
    n, B, T = indices.shape
    W = 1 + m * T
    if prev_in.shape != (B, W) or prev_out.shape != (B, W) or prev_in.dtype != torch.int32 or prev_out.dtype != torch.int32:
        raise RuntimeError(f"pack_codes_10bit_fec: prev_in and prev_out must be int32 [{B}, {W}]")
    _rows("pack_codes_10bit_fec", B, n_clip=n_clip, action=action, hold=hold)
    packets = _new(indices, B, packet_bytes(n + m, T), dtype=torch.uint8)
    nbytes = _new(indices, B, dtype=torch.int32)
    check(lib.hilc_pack_codes_10bit_fec(_ptr(indices, torch.int64), _ptr(n_clip, torch.int32), _ptr(prev_in, torch.int32),
                                        _ptr(prev_out, torch.int32), _ptr(action, torch.int32), _ptr(hold, torch.int32),
                                        _ptr(packets, torch.uint8), _ptr(nbytes, torch.int32), B, T, n, m, _stream()),
          "hilc_pack_codes_10bit_fec")
    return packets, nbytes


def _pack_codes_10bit_fec_fake(indices, n_clip, prev_in, prev_out, action, hold, m):
    n, B, T = indices.shape
    return indices.new_empty(B, packet_bytes(n + m, T), dtype=torch.uint8), indices.new_empty(B, dtype=torch.int32)


_register("pack_codes_10bit_fec", "(Tensor indices, Tensor? n_clip, Tensor prev_in, Tensor(a!) prev_out, Tensor? action, "
          "Tensor? hold, int m) -> (Tensor, Tensor)", _pack_codes_10bit_fec, _pack_codes_10bit_fec_fake)


def _fec_select(packets, fec, n_slot, n, m, frames):
    B = packets.shape[0]
    if packets.dim() != 2 or packets.shape[1] != packet_bytes(n + m, frames) or fec.numel() != B or n_slot.numel() != B:
        raise RuntimeError(f"fec_select: packets must be [B, {packet_bytes(n + m, frames)}] and fec, n_slot [B]")
    out = _new(packets, B, packet_bytes(n, frames), dtype=torch.uint8)
    check(lib.hilc_fec_select(_ptr(packets, torch.uint8), _ptr(fec, torch.int32), _ptr(n_slot, torch.int32), _ptr(out, torch.uint8),
                              B, frames, n, m, _stream()), "hilc_fec_select")
    return out


_register("fec_select", "(Tensor packets, Tensor fec, Tensor(a!) n_slot, int n, int m, int frames) -> Tensor", _fec_select,
          lambda packets, fec, n_slot, n, m, frames: packets.new_empty(packets.shape[0], packet_bytes(n, frames)))

# ======================================================================================================
# discontinuous transmission and comfort noise of the sender / receiver (graph_step.GraphedEncodeHop(dtx=),
# GraphedDecodeHop(cng_order=); definition: hilcodec_amd/dtx.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _dtx_encode(x, action, hold, run, packets, nbytes, indices, prev, level_thr, thr_vad, order, hangover, sid_interval):
    B = run.numel()
    if x.dim() != 3 or x.shape[0] != B or x.shape[1] != 1 or x.shape[2] % HOP or x.shape[2] == 0:
        raise RuntimeError(f"dtx_encode: x must be [{B}, 1, {HOP} T]")
    T = x.shape[2] // HOP
    if indices.dim() != 3 or indices.shape[1] != B or indices.shape[2] != T:
        raise RuntimeError(f"dtx_encode: indices must be [n, {B}, {T}]")
    if packets.dim() != 2 or packets.shape[0] != B or nbytes.numel() != B or level_thr.numel() != LEVELS - 1:
        raise RuntimeError(f"dtx_encode: packets must be [{B}, stride], nbytes [{B}], level_thr [{LEVELS - 1}]")
    _rows("dtx_encode", B, action=action, hold=hold)
    if prev is not None and (prev.dim() != 2 or prev.shape[0] != B):
        raise RuntimeError(f"dtx_encode: prev must be [{B}, words]")
    kind = _new(run, B, dtype=torch.int32)
    check(lib.hilc_dtx_encode(_ptr(x.contiguous()), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(run, torch.int32),
                              _ptr(kind, torch.int32), _ptr(packets, torch.uint8), _ptr(nbytes, torch.int32), _ptr(indices, torch.int64),
                              _ptr(prev, torch.int32), _ptr(level_thr, torch.float64), float(thr_vad), B, T, order, hangover,
                              sid_interval, indices.shape[0], packets.shape[1], 0 if prev is None else prev.shape[1], _stream()),
          "hilc_dtx_encode")
    return kind


_register("dtx_encode", "(Tensor x, Tensor? action, Tensor? hold, Tensor(a!) run, Tensor(b!) packets, Tensor(c!) nbytes, "
          "Tensor(d!) indices, Tensor(e!)? prev, Tensor level_thr, float thr_vad, int order, int hangover, int sid_interval) -> Tensor",
          _dtx_encode, lambda x, action, hold, run, packets, nbytes, indices, prev, level_thr, thr_vad, order, hangover, sid_interval:
          run.new_empty(run.shape[0], dtype=torch.int32))


def _cng_synth(packets, action, hold, state, wav, restore, gains, order):
    B = hold.numel()
    if wav.dim() != 3 or wav.shape[0] != B or wav.shape[1] != 1 or wav.shape[2] % HOP or wav.shape[2] == 0 or not wav.is_contiguous():
        raise RuntimeError(f"cng_synth: wav must be a contiguous [{B}, 1, {HOP} T]")
    if packets.dim() != 2 or packets.shape[0] != B or state.shape != (B, state_words(order)) or gains.numel() != LEVELS:
        raise RuntimeError(f"cng_synth: packets must be [{B}, stride], state [{B}, {state_words(order)}], gains [{LEVELS}]")
    _rows("cng_synth", B, action=action, restore=restore)
    check(lib.hilc_cng_synth(_ptr(packets, torch.uint8), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(state, torch.int32),
                             _ptr(wav), _ptr(restore, torch.int32), _ptr(gains), B, wav.shape[2] // HOP, order, packets.shape[1],
                             _stream()), "hilc_cng_synth")


_register("cng_synth", "(Tensor packets, Tensor? action, Tensor(a!) hold, Tensor(b!) state, Tensor(c!) wav, Tensor(d!)? restore, "
          "Tensor gains, int order) -> ()", _cng_synth, lambda packets, action, hold, state, wav, restore, gains, order: None)

# ======================================================================================================
# transport header of the sender and jitter buffer of the receiver (graph_step.GraphedEncodeHop(header=True),
# GraphedDecodeHop(jitter=); format: wire.pack_transport; definition: hilcodec_amd/jitter.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _packet_header(packets, nbytes, n_clip, kind, action, hold, ctr_in, ctr_out, n, m, frames):
    B = packets.shape[0]
    if packets.dim() != 2 or packets.shape[1] != packet_bytes(n + m, frames) or nbytes.numel() != B:
        raise RuntimeError(f"packet_header: packets must be [B, {packet_bytes(n + m, frames)}] and nbytes [B]")
    if ctr_in.numel() != B or ctr_out.numel() != B:
        raise RuntimeError(f"packet_header: the counter rows need {B} entries")
    _rows("packet_header", B, n_clip=n_clip, kind=kind, action=action, hold=hold)
    out = _new(packets, B, TRANSPORT_HEADER + packets.shape[1], dtype=torch.uint8)
    out_nbytes = _new(packets, B, dtype=torch.int32)
    check(lib.hilc_packet_header(_ptr(packets, torch.uint8), _ptr(nbytes, torch.int32), _ptr(n_clip, torch.int32), _ptr(kind, torch.int32),
                                 _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(ctr_in, torch.int32), _ptr(ctr_out, torch.int32),
                                 _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32), B, frames, n, m, _stream()), "hilc_packet_header")
    return out, out_nbytes


_register("packet_header", "(Tensor packets, Tensor nbytes, Tensor? n_clip, Tensor? kind, Tensor? action, Tensor? hold, Tensor ctr_in, "
          "Tensor(a!) ctr_out, int n, int m, int frames) -> (Tensor, Tensor)", _packet_header,
          lambda packets, nbytes, n_clip, kind, action, hold, ctr_in, ctr_out, n, m, frames:
          (packets.new_empty(packets.shape[0], TRANSPORT_HEADER + packets.shape[1]), packets.new_empty(packets.shape[0], dtype=torch.int32)))


def _jitter_args(op, arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, n, m, frames, order, depth, adapt=None):
    """the shape checks of a jitter step and the arguments both entry points begin with"""
    B = hold.numel()
    stride = packet_bytes(n + m, frames)
    aw = (TRANSPORT_HEADER + stride + 3) // 4
    if arrivals.dim() != 2 or arrivals.shape[1] != 1 + aw or offsets.numel() != B + 1:
        raise RuntimeError(f"{op}: arrivals must be [A, {1 + aw}] and offsets [{B + 1}]")
    if (packets.shape != (B, stride) or state.shape != (B, ST_WORDS) or (adapt is not None and adapt.shape != (B, AD_WORDS))
            or meta.dim() != 2 or meta.shape[0] != B):
        raise RuntimeError(f"{op}: packets must be [{B}, {stride}], state [{B}, {ST_WORDS}], "
                           + ("" if adapt is None else f"adapt [{B}, {AD_WORDS}], ") + f"meta [{B}, C]")
    C = meta.shape[1]
    if ring.shape != (B, C, (stride + 3) // 4):
        raise RuntimeError(f"{op}: ring must be [{B}, {C}, {(stride + 3) // 4}]")
    _rows(op, B, action=action, n_slot=n_slot, lost=lost, fec=fec)
    return (_ptr(arrivals, torch.int32), _ptr(offsets, torch.int32), arrivals.shape[0], _ptr(action, torch.int32), _ptr(hold, torch.int32),
            _ptr(n_slot, torch.int32), _ptr(lost, torch.int32), _ptr(fec, torch.int32), _ptr(packets, torch.uint8), _ptr(state, torch.int32),
            _ptr(meta, torch.int32), _ptr(ring, torch.int32), B, frames, n, m, order, int(lost is not None), depth, C)


def _jitter_step(arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, n, m, frames, order, depth):
    args = _jitter_args("jitter_step", arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, n, m, frames, order,
                        depth)
    check(lib.hilc_jitter_step(*args, _stream()), "hilc_jitter_step")


_register("jitter_step", "(Tensor arrivals, Tensor offsets, Tensor? action, Tensor(a!) hold, Tensor(b!) n_slot, Tensor(c!)? lost, "
          "Tensor(d!)? fec, Tensor(e!) packets, Tensor(f!) state, Tensor(g!) meta, Tensor(h!) ring, int n, int m, int frames, int order, "
          "int depth) -> ()", _jitter_step,
          lambda arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, n, m, frames, order, depth: None)


def _jitter_adapt_step(arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, adapt, n, m, frames, order, depth,
                       headroom, max_late, window, resync, force_windows):
    args = _jitter_args("jitter_adapt_step", arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, n, m, frames,
                        order, depth, adapt)
    check(lib.hilc_jitter_adapt_step(*args, _ptr(adapt, torch.int32), headroom, max_late, window, resync, force_windows, _stream()),
          "hilc_jitter_adapt_step")


_register("jitter_adapt_step", "(Tensor arrivals, Tensor offsets, Tensor? action, Tensor(a!) hold, Tensor(b!) n_slot, Tensor(c!)? lost, "
          "Tensor(d!)? fec, Tensor(e!) packets, Tensor(f!) state, Tensor(g!) meta, Tensor(h!) ring, Tensor(i!) adapt, int n, int m, "
          "int frames, int order, int depth, int headroom, int max_late, int window, int resync, int force_windows) -> ()",
          _jitter_adapt_step,
          lambda arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, adapt, n, m, frames, order, depth,
          headroom, max_late, window, resync, force_windows: None)

# ======================================================================================================
# per-room mixing of the receiver's output (graph_step.GraphedDecodeHop(mix=); definition: hilcodec_amd/mixer.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _mix_rows(name, wav):
    if wav.dim() != 3 or wav.shape[1] != 1 or wav.shape[0] < 1 or wav.shape[2] < 1 or not wav.is_contiguous():
        raise RuntimeError(f"{name}: wav must be a contiguous [B, 1, L >= 1]")
    return wav.shape[0], wav.shape[2]


def _mix_levels(wav, score, action):
    B, L = _mix_rows("mix_levels", wav)
    if score.shape != (B,) or (action is not None and action.numel() != B):
        raise RuntimeError(f"mix_levels: score must be float64 [{B}] and action int32 [{B}]")
    check(lib.hilc_mix_levels(_ptr(wav), _ptr(score, torch.float64), _ptr(action, torch.int32), B, L, _stream()), "hilc_mix_levels")


_register("mix_levels", "(Tensor wav, Tensor(a!) score, Tensor? action) -> ()", _mix_levels, lambda wav, score, action: None)


def _mix_rooms(wav, room, score, top_k, mixed, speakers):
    B, L = _mix_rows("mix_rooms", wav)
    if room.shape != (B,) or score.shape != (B,) or speakers.shape != (B,):
        raise RuntimeError(f"mix_rooms: room, score and speakers must be [{B}]")
    if mixed.shape != wav.shape or mixed.data_ptr() == wav.data_ptr():
        raise RuntimeError(f"mix_rooms: mixed must be [{B}, 1, {L}] and a buffer other than wav")
    check(lib.hilc_mix_rooms(_ptr(wav), _ptr(room, torch.int32), _ptr(score, torch.float64), top_k, _ptr(mixed),
                             _ptr(speakers, torch.int32), B, L, _stream()), "hilc_mix_rooms")


_register("mix_rooms", "(Tensor wav, Tensor room, Tensor score, int top_k, Tensor(a!) mixed, Tensor(b!) speakers) -> ()", _mix_rooms,
          lambda wav, room, score, top_k, mixed, speakers: None)


def _mix_gains(wav, gains, power, action, gate2, lo, hi, up, down, min_gain, max_gain, smooth):
    B, L = _mix_rows("mix_gains", wav)
    if gains.shape != (B, 2) or power.shape != (B,) or (action is not None and action.numel() != B):
        raise RuntimeError(f"mix_gains: gains must be float64 [{B}, 2], power float64 [{B}] and action int32 [{B}]")
    check(lib.hilc_mix_gains(_ptr(wav), _ptr(gains, torch.float64), _ptr(power, torch.float64), _ptr(action, torch.int32), gate2, lo,
                             hi, up, down, min_gain, max_gain, smooth, B, L, _stream()), "hilc_mix_gains")


_register("mix_gains", "(Tensor wav, Tensor(a!) gains, Tensor(b!) power, Tensor? action, float gate2, float lo, float hi, float up, "
          "float down, float min_gain, float max_gain, float smooth) -> ()", _mix_gains,
          lambda wav, gains, power, action, gate2, lo, hi, up, down, min_gain, max_gain, smooth: None)


def _mix_rooms_dyn(wav, room, score, top_k, gains, limiter, ceiling, release, sub, action, mixed, speakers):
    B, L = _mix_rows("mix_rooms_dyn", wav)
    if room.shape != (B,) or score.shape != (B,) or speakers.shape != (B,) or (action is not None and action.numel() != B):
        raise RuntimeError(f"mix_rooms_dyn: room, score, speakers and action must be [{B}]")
    if (gains is not None and gains.shape != (B, 2)) or (limiter is not None and limiter.shape != (B, 2)):
        raise RuntimeError(f"mix_rooms_dyn: gains and limiter must be float64 [{B}, 2]")
    if mixed.shape != wav.shape or mixed.data_ptr() == wav.data_ptr():
        raise RuntimeError(f"mix_rooms_dyn: mixed must be [{B}, 1, {L}] and a buffer other than wav")
    check(lib.hilc_mix_rooms_dyn(_ptr(wav), _ptr(room, torch.int32), _ptr(score, torch.float64), top_k, _ptr(gains, torch.float64),
                                 _ptr(limiter, torch.float64), ceiling, release, sub, _ptr(action, torch.int32), _ptr(mixed),
                                 _ptr(speakers, torch.int32), B, L, _stream()), "hilc_mix_rooms_dyn")


_register("mix_rooms_dyn", "(Tensor wav, Tensor room, Tensor score, int top_k, Tensor? gains, Tensor(a!)? limiter, float ceiling, "
          "float release, int sub, Tensor? action, Tensor(b!) mixed, Tensor(c!) speakers) -> ()", _mix_rooms_dyn,
          lambda wav, room, score, top_k, gains, limiter, ceiling, release, sub, action, mixed, speakers: None)

# ======================================================================================================
# quality-targeted variable bitrate of the sender (graph_step.GraphedEncodeHop(vbr=); definition: hilcodec_amd/vbr.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _vbr_select(z, indices, codebooks, n_clip, action, hold, credit, n_lo, rho, stage_bits, rate_bits, burst_bits):
    if z.dim() != 3 or indices.dim() != 3 or codebooks.dim() != 3 or indices.shape[1:] != z.shape[:2] or codebooks.shape[2] != z.shape[2]:
        raise RuntimeError("vbr_select: z must be [B, T, C], indices [n, B, T] and codebooks [Nq, K, C]")
    B, T, Cc = z.shape
    n = indices.shape[0]
    Nq, K, _ = codebooks.shape
    _rows("vbr_select", B, n_clip=n_clip, action=action, hold=hold, credit=credit)
    n_eff = _new(z, B, dtype=torch.int32)
    distortion = _new(z, B, n + 1, dtype=torch.float64)
    check(lib.hilc_vbr_select(_ptr(z), _ptr(indices, torch.int64), _ptr(codebooks), _ptr(n_clip, torch.int32), _ptr(action, torch.int32),
                              _ptr(hold, torch.int32), _ptr(credit, torch.int32), _ptr(n_eff, torch.int32),
                              _ptr(distortion, torch.float64), B, T, Cc, K, Nq, n, n_lo, rho, stage_bits, rate_bits, burst_bits,
                              _stream()), "hilc_vbr_select")
    return n_eff, distortion


_register("vbr_select", "(Tensor z, Tensor(a!) indices, Tensor codebooks, Tensor? n_clip, Tensor? action, Tensor? hold, "
          "Tensor(b!)? credit, int n_lo, float rho, int stage_bits, int rate_bits, int burst_bits) -> (Tensor, Tensor)", _vbr_select,
          lambda z, indices, codebooks, n_clip, action, hold, credit, n_lo, rho, stage_bits, rate_bits, burst_bits:
          (z.new_empty(z.shape[0], dtype=torch.int32), z.new_empty(z.shape[0], indices.shape[0] + 1, dtype=torch.float64)))

# ======================================================================================================
# receiver reports and loss-adaptive FEC (graph_step.GraphedDecodeHop(report=), GraphedEncodeHop(fec_adapt=); definition:
# hilcodec_amd/report.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _rx_report(jitter_state, action, rows, reports, due, window, interval):
    B = due.numel()
    if jitter_state.shape != (B, ST_WORDS) or rows.shape != (B, RP_WORDS) or reports.shape != (B, REPORT_BYTES):
        raise RuntimeError(f"rx_report: jitter_state must be [{B}, {ST_WORDS}], rows [{B}, {RP_WORDS}] and reports [{B}, {REPORT_BYTES}]")
    _rows("rx_report", B, action=action)
    check(lib.hilc_rx_report(_ptr(jitter_state, torch.int32), _ptr(action, torch.int32), _ptr(rows, torch.int32),
                             _ptr(reports, torch.uint8), _ptr(due, torch.int32), B, window, interval, _stream()), "hilc_rx_report")


_register("rx_report", "(Tensor jitter_state, Tensor? action, Tensor(a!) rows, Tensor(b!) reports, Tensor(c!) due, int window, "
          "int interval) -> ()", _rx_report, lambda jitter_state, action, rows, reports, due, window, interval: None)


def _fec_adapt(report, action, hold, rows, prev, fec_on, m, frames, on_q8, off_q8, calm_reports, timeout_hops, initial_on):
    B = fec_on.numel()
    if rows.shape != (B, FA_WORDS) or prev.shape != (B, 1 + m * frames):
        raise RuntimeError(f"fec_adapt: rows must be [{B}, {FA_WORDS}] and prev [{B}, {1 + m * frames}]")
    _rows("fec_adapt", B, report=report, action=action, hold=hold)
    check(lib.hilc_fec_adapt(_ptr(report, torch.int32), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(rows, torch.int32),
                             _ptr(prev, torch.int32), _ptr(fec_on, torch.int32), B, frames, m, on_q8, off_q8, calm_reports,
                             timeout_hops, int(initial_on), _stream()), "hilc_fec_adapt")


_register("fec_adapt", "(Tensor? report, Tensor? action, Tensor? hold, Tensor(a!) rows, Tensor(b!) prev, Tensor(c!) fec_on, int m, "
          "int frames, int on_q8, int off_q8, int calm_reports, int timeout_hops, bool initial_on) -> ()", _fec_adapt,
          lambda report, action, hold, rows, prev, fec_on, m, frames, on_q8, off_q8, calm_reports, timeout_hops, initial_on: None)

# ======================================================================================================
# NACK and retransmission (graph_step.GraphedDecodeHop(nack=), GraphedEncodeHop(rtx=); definition: hilcodec_amd/rtx.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _nack_build(jitter_state, meta, action, rows, nacks, due, m, rtt_hops, retry_hops, max_requests, skip_fecable):
    B = due.numel()
    if jitter_state.shape != (B, ST_WORDS) or meta.dim() != 2 or meta.shape[0] != B or rows.shape != (B, NK_WORDS) or \
            nacks.shape != (B, NACK_BYTES):
        raise RuntimeError(f"nack_build: jitter_state must be [{B}, {ST_WORDS}], meta [{B}, capacity], rows [{B}, {NK_WORDS}] and nacks "
                           f"[{B}, {NACK_BYTES}]")
    _rows("nack_build", B, action=action)
    check(lib.hilc_nack_build(_ptr(jitter_state, torch.int32), _ptr(meta, torch.int32), _ptr(action, torch.int32), _ptr(rows, torch.int32),
                              _ptr(nacks, torch.uint8), _ptr(due, torch.int32), B, meta.shape[1], m, rtt_hops, retry_hops, max_requests,
                              int(skip_fecable), _stream()), "hilc_nack_build")


_register("nack_build", "(Tensor jitter_state, Tensor meta, Tensor? action, Tensor(a!) rows, Tensor(b!) nacks, Tensor(c!) due, int m, "
          "int rtt_hops, int retry_hops, int max_requests, bool skip_fecable) -> ()", _nack_build,
          lambda jitter_state, meta, action, rows, nacks, due, m, rtt_hops, retry_hops, max_requests, skip_fecable: None)


def _rtx_step(packets, nbytes, nack_base, nack_bitmap, action, tags, ring, rows, out, out_nbytes):
    if packets.dim() != 2 or tags.dim() != 2 or out.dim() != 3:
        raise RuntimeError("rtx_step: packets must be [B, row_bytes], tags [B, history] and out [B, per_hop, row_bytes]")
    B, tb = packets.shape
    R, P = tags.shape[1], out.shape[1]
    if nbytes.numel() != B or tags.shape[0] != B or ring.shape != (B, R, (tb + 3) // 4) or rows.shape != (B, RX_WORDS) or \
            out.shape != (B, P, tb) or out_nbytes.shape != (B, P):
        raise RuntimeError(f"rtx_step: nbytes must be [{B}], tags [{B}, {R}], ring [{B}, {R}, {(tb + 3) // 4}], rows [{B}, {RX_WORDS}], "
                           f"out [{B}, {P}, {tb}] and out_nbytes [{B}, {P}]")
    _rows("rtx_step", B, nack_base=nack_base, nack_bitmap=nack_bitmap, action=action)
    check(lib.hilc_rtx_step(_ptr(packets, torch.uint8), _ptr(nbytes, torch.int32), _ptr(nack_base, torch.int32),
                            _ptr(nack_bitmap, torch.int32), _ptr(action, torch.int32), _ptr(tags, torch.int32), _ptr(ring, torch.int32),
                            _ptr(rows, torch.int32), _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32), B, tb, R, P, _stream()),
          "hilc_rtx_step")


_register("rtx_step", "(Tensor packets, Tensor nbytes, Tensor? nack_base, Tensor? nack_bitmap, Tensor? action, Tensor(a!) tags, "
          "Tensor(b!) ring, Tensor(c!) rows, Tensor(d!) out, Tensor(e!) out_nbytes) -> ()", _rtx_step,
          lambda packets, nbytes, nack_base, nack_bitmap, action, tags, ring, rows, out, out_nbytes: None)

# ======================================================================================================
# report-driven rate control of the sender (graph_step.GraphedEncodeHop(rate=); definition: hilcodec_amd/rate.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _rate_ceiling(report, action, hold, n_clip, prev, rows, n_ceil, frames, n, m, header, min_bits, max_bits, start_bits, high_q8, low_q8,
                  increase_q8, burst_hops, timeout_hops):
    B = n_ceil.numel()
    if rows.shape != (B, RC_WORDS) or (prev is not None and prev.shape != (B, 1 + m * frames)):
        raise RuntimeError(f"rate_ceiling: rows must be [{B}, {RC_WORDS}] and prev [{B}, {1 + m * frames}]")
    _rows("rate_ceiling", B, report=report, action=action, hold=hold, n_clip=n_clip)
    check(lib.hilc_rate_ceiling(_ptr(report, torch.int32), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(n_clip, torch.int32),
                                _ptr(prev, torch.int32), _ptr(rows, torch.int32), _ptr(n_ceil, torch.int32), B, frames, n, m, int(header),
                                min_bits, max_bits, start_bits, high_q8, low_q8, increase_q8, burst_hops, timeout_hops, _stream()),
          "hilc_rate_ceiling")


_register("rate_ceiling", "(Tensor? report, Tensor? action, Tensor? hold, Tensor? n_clip, Tensor? prev, Tensor(a!) rows, Tensor(b!) n_ceil, "
          "int frames, int n, int m, bool header, int min_bits, int max_bits, int start_bits, int high_q8, int low_q8, int increase_q8, "
          "int burst_hops, int timeout_hops) -> ()", _rate_ceiling,
          lambda report, action, hold, n_clip, prev, rows, n_ceil, frames, n, m, header, min_bits, max_bits, start_bits, high_q8, low_q8,
          increase_q8, burst_hops, timeout_hops: None)


def _rate_charge(nbytes, rtx_nbytes, rows, burst_hops):
    B = nbytes.numel()
    if rows.shape != (B, RC_WORDS) or (rtx_nbytes is not None and (rtx_nbytes.dim() != 2 or rtx_nbytes.shape[0] != B)):
        raise RuntimeError(f"rate_charge: rows must be [{B}, {RC_WORDS}] and rtx_nbytes [{B}, per_hop]")
    check(lib.hilc_rate_charge(_ptr(nbytes, torch.int32), _ptr(rtx_nbytes, torch.int32), _ptr(rows, torch.int32), B,
                               0 if rtx_nbytes is None else rtx_nbytes.shape[1], burst_hops, _stream()), "hilc_rate_charge")


_register("rate_charge", "(Tensor nbytes, Tensor? rtx_nbytes, Tensor(a!) rows, int burst_hops) -> ()", _rate_charge,
          lambda nbytes, rtx_nbytes, rows, burst_hops: None)

# ======================================================================================================
# delay-based bandwidth estimate (graph_step.GraphedDecodeHop(bwe=) / GraphedEncodeHop(cap=); definition: hilcodec_amd/bwe.py;
# semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _rx_bwe(arrivals, offsets, times, action, rows, caps, due, n, m, frames, order, min_bits, max_bits, window, rate_window, alpha_q8,
            beta_q8, increase_q16, interval, reset_ticks):
    B = due.numel()
    aw = (TRANSPORT_HEADER + packet_bytes(n + m, frames) + 3) // 4
    if arrivals.dim() != 2 or arrivals.shape[1] != 1 + aw or offsets.numel() != B + 1 or times.numel() != arrivals.shape[0]:
        raise RuntimeError(f"rx_bwe: arrivals must be [A, {1 + aw}], offsets [{B + 1}] and times [A]")
    if rows.shape != (B, BW_WORDS) or caps.shape != (B, CAP_BYTES):
        raise RuntimeError(f"rx_bwe: rows must be [{B}, {BW_WORDS}] and caps [{B}, {CAP_BYTES}]")
    _rows("rx_bwe", B, action=action)
    check(lib.hilc_rx_bwe(_ptr(arrivals, torch.int32), _ptr(offsets, torch.int32), _ptr(times, torch.int32), arrivals.shape[0],
                          _ptr(action, torch.int32), _ptr(rows, torch.int32), _ptr(caps, torch.uint8), _ptr(due, torch.int32), B, frames,
                          n, m, order, min_bits, max_bits, window, rate_window, alpha_q8, beta_q8, increase_q16, interval, reset_ticks,
                          _stream()), "hilc_rx_bwe")


_register("rx_bwe", "(Tensor arrivals, Tensor offsets, Tensor times, Tensor? action, Tensor(a!) rows, Tensor(b!) caps, Tensor(c!) due, "
          "int n, int m, int frames, int order, int min_bits, int max_bits, int window, int rate_window, int alpha_q8, int beta_q8, "
          "int increase_q16, int interval, int reset_ticks) -> ()", _rx_bwe,
          lambda arrivals, offsets, times, action, rows, caps, due, n, m, frames, order, min_bits, max_bits, window, rate_window, alpha_q8,
          beta_q8, increase_q16, interval, reset_ticks: None)


def _rate_cap(cap, action, hold, rows, rate_rows, min_bits, max_bits, timeout_hops):
    B = rows.shape[0]
    if rows.shape != (B, CP_WORDS) or rate_rows.shape != (B, RC_WORDS):
        raise RuntimeError(f"rate_cap: rows must be [{B}, {CP_WORDS}] and rate_rows [{B}, {RC_WORDS}]")
    _rows("rate_cap", B, cap=cap, action=action, hold=hold)
    check(lib.hilc_rate_cap(_ptr(cap, torch.int32), _ptr(action, torch.int32), _ptr(hold, torch.int32), _ptr(rows, torch.int32),
                            _ptr(rate_rows, torch.int32), B, min_bits, max_bits, timeout_hops, _stream()), "hilc_rate_cap")


_register("rate_cap", "(Tensor? cap, Tensor? action, Tensor? hold, Tensor(a!) rows, Tensor(b!) rate_rows, int min_bits, int max_bits, "
          "int timeout_hops) -> ()", _rate_cap, lambda cap, action, hold, rows, rate_rows, min_bits, max_bits, timeout_hops: None)

# ======================================================================================================
# SRTP packet protection (graph_step.GraphedEncodeHop(srtp=) / GraphedDecodeHop(srtp=); definition: hilcodec_amd/srtp.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _srtp_protect(packets, nbytes, keys, rows, action, out, out_nbytes):
    if packets.dim() != 2:
        raise RuntimeError("srtp_protect: packets must be [B, row_bytes]")
    B, tb = packets.shape
    if nbytes.numel() != B or keys.shape != (B, SRTP_KEY_WORDS) or rows.shape != (B, SRTP_TX_WORDS) or \
            out.shape != (B, tb + SRTP_TAG_BYTES) or out_nbytes.numel() != B:
        raise RuntimeError(f"srtp_protect: nbytes must be [{B}], keys [{B}, {SRTP_KEY_WORDS}], rows [{B}, {SRTP_TX_WORDS}], "
                           f"out [{B}, {tb + SRTP_TAG_BYTES}] and out_nbytes [{B}]")
    _rows("srtp_protect", B, action=action)
    check(lib.hilc_srtp_protect(_ptr(packets, torch.uint8), _ptr(nbytes, torch.int32), _ptr(keys, torch.int32), _ptr(rows, torch.int32),
                                _ptr(action, torch.int32), _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32), B, tb, _stream()),
          "hilc_srtp_protect")


_register("srtp_protect", "(Tensor packets, Tensor nbytes, Tensor keys, Tensor(a!) rows, Tensor? action, Tensor(b!) out, "
          "Tensor(c!) out_nbytes) -> ()", _srtp_protect, lambda packets, nbytes, keys, rows, action, out, out_nbytes: None)


def _srtp_unprotect(arrivals, offsets, keys, rows, action, plain, row_bytes):
    B = rows.shape[0]
    pw, aw = (row_bytes + SRTP_TAG_BYTES + 3) // 4, (row_bytes + 3) // 4
    if arrivals.dim() != 2 or arrivals.shape[1] != 1 + pw or offsets.numel() != B + 1 or plain.shape != (arrivals.shape[0], 1 + aw):
        raise RuntimeError(f"srtp_unprotect: arrivals must be [A, {1 + pw}], offsets [{B + 1}] and plain [A, {1 + aw}]")
    if keys.shape != (B, SRTP_KEY_WORDS) or rows.shape != (B, SRTP_RX_WORDS):
        raise RuntimeError(f"srtp_unprotect: keys must be [{B}, {SRTP_KEY_WORDS}] and rows [{B}, {SRTP_RX_WORDS}]")
    _rows("srtp_unprotect", B, action=action)
    check(lib.hilc_srtp_unprotect(_ptr(arrivals, torch.int32), _ptr(offsets, torch.int32), arrivals.shape[0], _ptr(keys, torch.int32),
                                  _ptr(rows, torch.int32), _ptr(action, torch.int32), _ptr(plain, torch.int32), B, row_bytes, _stream()),
          "hilc_srtp_unprotect")


_register("srtp_unprotect", "(Tensor arrivals, Tensor offsets, Tensor keys, Tensor(a!) rows, Tensor? action, Tensor(b!) plain, "
          "int row_bytes) -> ()", _srtp_unprotect, lambda arrivals, offsets, keys, rows, action, plain, row_bytes: None)


# the forwarding hop's egress (graph_step.GraphedForwardHop(srtp=); definition: hilcodec_amd/forward_srtp.py)
def _srtp_protect_routes(rows, nbytes, routes, new_routes, action, rekey_up, rekey_down, keys, route_rows, out, out_nbytes):
    if rows.dim() != 4:
        raise RuntimeError("srtp_protect_routes: rows must be [B, fanout, burst, row_bytes]")
    B, F, P, tb = rows.shape
    if nbytes.shape != (B, F, P) or routes.shape != (B, F) or new_routes.shape != (B, F) or keys.shape != (B, SRTP_KEY_WORDS) or \
            route_rows.shape != (B, F, FSRTP_RT_WORDS) or out.shape != (B, F, P, tb + SRTP_TAG_BYTES) or out_nbytes.shape != (B, F, P):
        raise RuntimeError(f"srtp_protect_routes: nbytes must be [{B}, {F}, {P}], routes and new_routes [{B}, {F}], keys [{B}, "
                           f"{SRTP_KEY_WORDS}], route_rows [{B}, {F}, {FSRTP_RT_WORDS}], out [{B}, {F}, {P}, {tb + SRTP_TAG_BYTES}] and "
                           f"out_nbytes [{B}, {F}, {P}]")
    _rows("srtp_protect_routes", B, action=action, rekey_up=rekey_up, rekey_down=rekey_down)
    check(lib.hilc_srtp_protect_routes(_ptr(rows, torch.uint8), _ptr(nbytes, torch.int32), _ptr(routes, torch.int32),
                                       _ptr(new_routes, torch.int32), _ptr(action, torch.int32), _ptr(rekey_up, torch.int32),
                                       _ptr(rekey_down, torch.int32), _ptr(keys, torch.int32), _ptr(route_rows, torch.int32),
                                       _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32), B, F, P, tb, _stream()),
          "hilc_srtp_protect_routes")


_register("srtp_protect_routes", "(Tensor rows, Tensor nbytes, Tensor routes, Tensor new_routes, Tensor? action, Tensor? rekey_up, "
          "Tensor? rekey_down, Tensor keys, Tensor(a!) route_rows, Tensor(b!) out, Tensor(c!) out_nbytes) -> ()", _srtp_protect_routes,
          lambda rows, nbytes, routes, new_routes, action, rekey_up, rekey_down, keys, route_rows, out, out_nbytes: None)

# ======================================================================================================
# selective forwarding hop (graph_step.GraphedForwardHop; definition: hilcodec_amd/forward.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _forward_arrivals(op, arrivals, n, m, frames):
    """the arrival records of a forwarding op checked: int32 [max_arrivals, 1 + ceil(tb / 4)]; returns tb"""
    tb = TRANSPORT_HEADER + packet_bytes(n + m, frames)
    if arrivals.dim() != 2 or arrivals.shape[1] != 1 + (tb + 3) // 4:
        raise RuntimeError(f"{op}: arrivals must be int32 [max_arrivals, {1 + (tb + 3) // 4}] for n = {n}, m = {m}, frames = {frames}")
    return tb


def _forward_classify(arrivals, offsets, action, rows, pick, pick_count, n, m, frames, order, burst, hang_hops):
    B = pick_count.numel()
    _forward_arrivals("forward_classify", arrivals, n, m, frames)
    if offsets.shape != (B + 1,) or rows.shape != (B, SD_WORDS) or pick.shape != (B, burst):
        raise RuntimeError(f"forward_classify: offsets must be [{B + 1}], rows [{B}, {SD_WORDS}] and pick [{B}, {burst}]")
    _rows("forward_classify", B, action=action)
    check(lib.hilc_forward_classify(_ptr(arrivals, torch.int32), _ptr(offsets, torch.int32), arrivals.shape[0], _ptr(action, torch.int32),
                                    _ptr(rows, torch.int32), _ptr(pick, torch.int32), _ptr(pick_count, torch.int32), B, frames, n, m,
                                    order, burst, hang_hops, _stream()), "hilc_forward_classify")


_register("forward_classify", "(Tensor arrivals, Tensor offsets, Tensor? action, Tensor(a!) rows, Tensor(b!) pick, Tensor(c!) pick_count, "
          "int n, int m, int frames, int order, int burst, int hang_hops) -> ()", _forward_classify,
          lambda arrivals, offsets, action, rows, pick, pick_count, n, m, frames, order, burst, hang_hops: None)


def _forward_route(arrivals, action, room, layers, sender_rows, pick, pick_count, routes, new_routes, rows, out, out_nbytes, n, m, frames,
                   order, keep_fec):
    B = room.numel()
    tb = _forward_arrivals("forward_route", arrivals, n, m, frames)
    if out.dim() != 4 or out.shape[0] != B or out.shape[3] != tb:
        raise RuntimeError(f"forward_route: out must be uint8 [{B}, fanout, burst, {tb}]")
    F, P = out.shape[1], out.shape[2]
    if sender_rows.shape != (B, SD_WORDS) or pick.shape != (B, P) or routes.shape != (B, F) or new_routes.shape != (B, F) or \
            rows.shape != (B, LR_WORDS) or out_nbytes.shape != (B, F, P):
        raise RuntimeError(f"forward_route: sender_rows must be [{B}, {SD_WORDS}], pick [{B}, {P}], routes and new_routes [{B}, {F}], rows "
                           f"[{B}, {LR_WORDS}] and out_nbytes [{B}, {F}, {P}]")
    _rows("forward_route", B, action=action, layers=layers, pick_count=pick_count)
    check(lib.hilc_forward_route(_ptr(arrivals, torch.int32), arrivals.shape[0], _ptr(action, torch.int32), _ptr(room, torch.int32),
                                 _ptr(layers, torch.int32), _ptr(sender_rows, torch.int32), _ptr(pick, torch.int32),
                                 _ptr(pick_count, torch.int32), _ptr(routes, torch.int32), _ptr(new_routes, torch.int32),
                                 _ptr(rows, torch.int32), _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32), B, frames, n, m, order, F,
                                 P, int(keep_fec), _stream()), "hilc_forward_route")


_register("forward_route", "(Tensor arrivals, Tensor? action, Tensor room, Tensor layers, Tensor sender_rows, Tensor pick, Tensor pick_count, "
          "Tensor(a!) routes, Tensor(b!) new_routes, Tensor(c!) rows, Tensor(d!) out, Tensor(e!) out_nbytes, int n, int m, int frames, "
          "int order, bool keep_fec) -> ()", _forward_route,
          lambda arrivals, action, room, layers, sender_rows, pick, pick_count, routes, new_routes, rows, out, out_nbytes, n, m, frames,
          order, keep_fec: None)

# ======================================================================================================
# downlink control of the forwarding hop (graph_step.GraphedForwardHop(downlink=); definition: hilcodec_amd/downlink.py; semantics:
# include/hilcodec_amd.h)
# ======================================================================================================
def _downlink_store(arrivals, action, pick, pick_count, tags, ring, rows, n, m, frames):
    B = pick_count.numel()
    tb = _forward_arrivals("downlink_store", arrivals, n, m, frames)
    if pick.dim() != 2 or tags.dim() != 2:
        raise RuntimeError("downlink_store: pick must be [B, burst] and tags [B, history]")
    P, R = pick.shape[1], tags.shape[1]
    if pick.shape[0] != B or tags.shape[0] != B or ring.shape != (B, R, 1 + (tb + 3) // 4) or rows.shape != (B, DS_WORDS):
        raise RuntimeError(f"downlink_store: pick must be [{B}, {P}], tags [{B}, {R}], ring [{B}, {R}, {1 + (tb + 3) // 4}] and rows "
                           f"[{B}, {DS_WORDS}]")
    _rows("downlink_store", B, action=action)
    check(lib.hilc_downlink_store(_ptr(arrivals, torch.int32), arrivals.shape[0], _ptr(action, torch.int32), _ptr(pick, torch.int32),
                                  _ptr(pick_count, torch.int32), _ptr(tags, torch.int32), _ptr(ring, torch.int32), _ptr(rows, torch.int32),
                                  B, frames, n, m, P, R, _stream()), "hilc_downlink_store")


_register("downlink_store", "(Tensor arrivals, Tensor? action, Tensor pick, Tensor pick_count, Tensor(a!) tags, Tensor(b!) ring, "
          "Tensor(c!) rows, int n, int m, int frames) -> ()", _downlink_store,
          lambda arrivals, action, pick, pick_count, tags, ring, rows, n, m, frames: None)


def _downlink_step(routes, new_routes, packets, nbytes, layers, action, report, nack_base, nack_bitmap, tags, ring, rows, memory, eff_layers,
                   out, out_nbytes, rtx_out, rtx_nbytes, rtx_routes, n, m, frames, keep_fec, rate_on, min_bits, max_bits, start_bits, high_q8,
                   low_q8, increase_q8, burst_hops, timeout_hops):
    B = layers.numel()
    tb = TRANSPORT_HEADER + packet_bytes(n + m, frames)
    if packets.dim() != 4 or packets.shape[0] != B or packets.shape[3] != tb:
        raise RuntimeError(f"downlink_step: packets must be uint8 [{B}, fanout, burst, {tb}]")
    F, P = packets.shape[1], packets.shape[2]
    if routes.shape != (B, F) or new_routes.shape != (B, F) or nbytes.shape != (B, F, P) or rows.shape != (B, DL_WORDS) or \
            memory.shape != (B, F) or eff_layers.shape != (B,) or out.shape != (B, F, P, tb) or out_nbytes.shape != (B, F, P):
        raise RuntimeError(f"downlink_step: routes, new_routes and memory must be [{B}, {F}], nbytes and out_nbytes [{B}, {F}, {P}], rows "
                           f"[{B}, {DL_WORDS}], eff_layers [{B}] and out [{B}, {F}, {P}, {tb}]")
    for name, row in (("report", report), ("nack_base", nack_base), ("nack_bitmap", nack_bitmap)):
        if row is not None and row.shape != (B, F):
            raise RuntimeError(f"downlink_step: {name} must be [{B}, {F}]")
    history = [tags, ring, rtx_out, rtx_nbytes, rtx_routes]
    if any(t is None for t in history) and not all(t is None for t in history):
        raise RuntimeError("downlink_step: tags, ring, rtx_out, rtx_nbytes and rtx_routes come together or not at all")
    R = Q = 0
    if tags is not None:
        if tags.dim() != 2 or rtx_out.dim() != 3:
            raise RuntimeError("downlink_step: tags must be [B, history] and rtx_out [B, per_hop, row_bytes]")
        R, Q = tags.shape[1], rtx_out.shape[1]
        if tags.shape[0] != B or ring.shape != (B, R, 1 + (tb + 3) // 4) or rtx_out.shape != (B, Q, tb) or rtx_nbytes.shape != (B, Q) or \
                rtx_routes.shape != (B, Q):
            raise RuntimeError(f"downlink_step: tags must be [{B}, {R}], ring [{B}, {R}, {1 + (tb + 3) // 4}], rtx_out [{B}, {Q}, {tb}], "
                               f"rtx_nbytes and rtx_routes [{B}, {Q}]")
    _rows("downlink_step", B, action=action)
    check(lib.hilc_downlink_step(_ptr(routes, torch.int32), _ptr(new_routes, torch.int32), _ptr(packets, torch.uint8),
                                 _ptr(nbytes, torch.int32), _ptr(layers, torch.int32), _ptr(action, torch.int32),
                                 _ptr(report, torch.int32), _ptr(nack_base, torch.int32), _ptr(nack_bitmap, torch.int32),
                                 _ptr(tags, torch.int32), _ptr(ring, torch.int32), _ptr(rows, torch.int32), _ptr(memory, torch.int32),
                                 _ptr(eff_layers, torch.int32), _ptr(out, torch.uint8), _ptr(out_nbytes, torch.int32),
                                 _ptr(rtx_out, torch.uint8), _ptr(rtx_nbytes, torch.int32), _ptr(rtx_routes, torch.int32), B, frames, n, m,
                                 F, P, int(keep_fec), R, max(Q, 1), int(rate_on), min_bits, max_bits, start_bits, high_q8, low_q8,
                                 increase_q8, burst_hops, timeout_hops, _stream()), "hilc_downlink_step")


_register("downlink_step", "(Tensor routes, Tensor new_routes, Tensor packets, Tensor nbytes, Tensor layers, Tensor? action, Tensor? report, "
          "Tensor? nack_base, Tensor? nack_bitmap, Tensor? tags, Tensor? ring, Tensor(a!) rows, Tensor(b!) memory, Tensor(c!) eff_layers, "
          "Tensor(d!) out, Tensor(e!) out_nbytes, Tensor(f!)? rtx_out, Tensor(g!)? rtx_nbytes, Tensor(h!)? rtx_routes, int n, int m, "
          "int frames, bool keep_fec, bool rate_on, int min_bits, int max_bits, int start_bits, int high_q8, int low_q8, int increase_q8, "
          "int burst_hops, int timeout_hops) -> ()", _downlink_step,
          lambda routes, new_routes, packets, nbytes, layers, action, report, nack_base, nack_bitmap, tags, ring, rows, memory, eff_layers,
          out, out_nbytes, rtx_out, rtx_nbytes, rtx_routes, n, m, frames, keep_fec, rate_on, min_bits, max_bits, start_bits, high_q8, low_q8,
          increase_q8, burst_hops, timeout_hops: None)

# ======================================================================================================
# audio level and level-based speaker selection (graph_step.GraphedEncodeHop(audio_level=True), GraphedForwardHop(speakers=);
# definition: hilcodec_amd/audio_level.py; semantics: include/hilcodec_amd.h)
# ======================================================================================================
def _audio_level(x, thr, hold, level):
    B = level.numel()
    if x.dim() not in (2, 3) or x.shape[0] != B or x.numel() == 0 or thr.shape != (LEVELS - 1,):
        raise RuntimeError(f"audio_level: x must be fp32 [{B}, 1, L] or [{B}, L] and thr float64 [{LEVELS - 1}]")
    _rows("audio_level", B, hold=hold)
    check(lib.hilc_audio_level(_ptr(x), _ptr(thr, torch.float64), _ptr(hold, torch.int32), _ptr(level, torch.int32), B, x.numel() // B,
                               _stream()), "hilc_audio_level")


_register("audio_level", "(Tensor x, Tensor thr, Tensor? hold, Tensor(a!) level) -> ()", _audio_level, lambda x, thr, hold, level: None)


def _forward_rank(sender_rows, loud, room, action, shadow_prev, shadow, rows, fanout, hang_hops, floor_level, attack_shift, decay_q8,
                  margin_db):
    B = room.numel()
    if sender_rows.shape != (B, SD_WORDS) or shadow_prev.shape != (B, SD_WORDS) or shadow.shape != (B, SD_WORDS) or \
            rows.shape != (B, SP_WORDS):
        raise RuntimeError(f"forward_rank: sender_rows, shadow_prev and shadow must be [{B}, {SD_WORDS}] and rows [{B}, {SP_WORDS}]")
    _rows("forward_rank", B, loud=loud, action=action)
    check(lib.hilc_forward_rank(_ptr(sender_rows, torch.int32), _ptr(loud, torch.int32), _ptr(room, torch.int32), _ptr(action, torch.int32),
                                _ptr(shadow_prev, torch.int32), _ptr(shadow, torch.int32), _ptr(rows, torch.int32), B, fanout, hang_hops,
                                floor_level, attack_shift, decay_q8, margin_db, _stream()), "hilc_forward_rank")


_register("forward_rank", "(Tensor sender_rows, Tensor loud, Tensor room, Tensor? action, Tensor shadow_prev, Tensor(a!) shadow, "
          "Tensor(b!) rows, int fanout, int hang_hops, int floor_level, int attack_shift, int decay_q8, int margin_db) -> ()", _forward_rank,
          lambda sender_rows, loud, room, action, shadow_prev, shadow, rows, fanout, hang_hops, floor_level, attack_shift, decay_q8,
          margin_db: None)

_OPS = torch.ops.hilcodec


# ======================================================================================================
# public wrappers (traceable: arguments in, torch.ops.hilcodec.* out)
# ======================================================================================================
def pw_conv(x: Tensor, wt: Tensor, bias: Optional[Tensor] = None, res: Optional[Tensor] = None,
            in_scale: float = 1.0, in_elu: bool = False, out_scale: float = 1.0) -> Tensor:
    """x `[B,K,T]`, wt `[K,M]` -> `[B,M,T]`; see hilc_pw_conv."""
    return _OPS.pw_conv(x, wt, bias, res, float(in_scale), bool(in_elu), float(out_scale))


def dws_conv(x: Tensor, wt: Tensor, dw_w: Tensor, dw_b: Optional[Tensor] = None, res: Optional[Tensor] = None,
             stride: int = 1, in_scale: float = 1.0, in_elu: bool = False, out_scale: float = 1.0,
             out_elu: bool = False) -> Tensor:
    """Fused pointwise -> depthwise causal conv (offline): x `[B,K,T]`, wt `[K,M]`, dw_w `[M,k]` ->
    `[B,M,ceil(T/stride)]`; see hilc_dws_conv."""
    return _OPS.dws_conv(x, wt, dw_w, dw_b, res, int(stride), float(in_scale), bool(in_elu), float(out_scale),
                         bool(out_elu))


def dws_conv_stream_supported(T: int, k: int, stride: int, has_res: bool = False, B: int = 1, M: int = 1, K: int = 1) -> bool:
    """whole-clip tiles: a hop of at most 128 samples per stream, a multiple of the stride; longer hops for the
    down-sampling form (k = 2 * stride): per-clip tiles with a recomputed halo — the linear-addressing core only, so an x `[B,K,T]` of
    2^32 bytes or more is refused (csrc/gemm.hip: `lin_ok`) — which take a shortcut `res` only in their
    flat-tile form (csrc/gemm.hip: stride <= 8, fewer than 2^31 outputs, a tile holds at most two stream starts).  The byte bound needs the
    caller's B and K: with the defaults (1, 1) it never binds, and a long hop that the library then refuses raises from the wrapper."""
    if T > 128:
        if not (k == 2 * stride and stride <= 16 and T % 4 == 0 and T % stride == 0):
            return False
        if B * K * T * 4 >= (1 << 32):
            return False
        if not has_res:
            return True
        h = (stride + 3) // 4 * 4
        n_out = (128 - h - stride) // stride + 1
        while (n_out * stride) % 4 != 0:
            n_out -= 1
        to = T // stride
        return stride <= 8 and B * to + T < (1 << 31) and B * M * to < (1 << 31) and to * 2 >= n_out + 1
    return T % stride == 0 and stride <= k <= 32


def dws_conv_stream_profitable(T: int, k: int, stride: int, has_res: bool = False, B: int = 1, M: int = 1, K: int = 1) -> bool:
    """where the fused hop beats pointwise GEMM + cached depthwise conv (measured, tools/layer_profile.py
    --mode streaming): not for 2- or 3-sample hops of the tiled core, whose depthwise taps are nearly all cache reads."""
    if T == 1 and stride == 1:
        return k <= 32  # single-frame layers: the latency-bound 32 x 32-tile kernel (csrc/frame1.hip), taps in its epilogue
    return dws_conv_stream_supported(T, k, stride, has_res, B, M, K) and T // stride >= 1 and T >= 4


def _state_out(given: Optional[Tensor], like: Tensor, *shape) -> Tensor:
    """the next hop's cache: the caller's persistent buffer, or (reference protocol) a fresh tensor"""
    return given if given is not None else torch.empty(shape, device=like.device, dtype=torch.float32)


def dws_conv_stream(x: Tensor, wt: Tensor, dw_w: Tensor, dw_b: Optional[Tensor], hist: Optional[Tensor],
                    res: Optional[Tensor] = None, stride: int = 1, in_scale: float = 1.0, in_elu: bool = False,
                    out_scale: float = 1.0, out_elu: bool = False, hist_out: Optional[Tensor] = None):
    """Streaming hop of a depthwise-separable block (hilc_dws_conv_stream): x `[B,K,T]` (T <= 128, or any T % 4 == 0 for k = 2 * stride), cache
    `[B,M,k-stride]` (last pointwise outputs of the previous hop) -> (y `[B,M,T/stride]`, new cache)."""
    hout = _state_out(hist_out, x, x.shape[0], wt.shape[1], dw_w.shape[1] - stride)
    y = _OPS.dws_conv_stream(x, wt, dw_w, dw_b, hist, hout, res, int(stride), float(in_scale), bool(in_elu),
                             float(out_scale), bool(out_elu))
    return y, hout


def up_conv_taps(tr_w: Tensor, stride: int) -> Optional[Tensor]:
    """Expanded tap table for strides without a vector tap path (hilc_up_conv_expand_taps); built once per spec."""
    if stride in (2, 4, 8):
        return None
    return _OPS.up_conv_expand_taps(tr_w, int(stride))


def up_conv(x: Tensor, tr_w: Tensor, wt: Tensor, bias: Optional[Tensor], stride: int, in_scale: float = 1.0,
            in_elu: bool = True, hist: Optional[Tensor] = None, want_hist: bool = False,
            taps: Optional[Tensor] = None, hist_out: Optional[Tensor] = None):
    """Fused [Scale, ELU, depthwise transposed conv (k=2*stride), pointwise conv + bias]:
    x `[B,K,Tin]`, tr_w `[K,2*stride]`, wt `[K,M]` -> `[B,M,Tin*stride]`; see hilc_up_conv.
    Streaming: hist `[B,K,1]` = the activated last input frame of the previous hop -> (y, new cache)."""
    if taps is None and stride not in (2, 4, 8):
        taps = up_conv_taps(tr_w, stride)
    hout = _state_out(hist_out, x, x.shape[0], x.shape[1], 1) if want_hist else None
    y = _OPS.up_conv(x, hist, hout, tr_w, taps, wt, bias, int(stride), float(in_scale), bool(in_elu))
    return (y, hout) if want_hist else y


def resblock_supported(C: int, T: int, B: int = 1, streaming: bool = False) -> bool:
    """mirror of hilc_resblock_supported / hilc_resblock_stream_supported (plain Python so that a tracing compiler can
    evaluate it; the C entry points are checked against this in tests/test_api_cpu.py); the streaming form walks a flat
    32-bit column space and also takes the wide blocks of a hop (C = 256 / 384; C = 512 / 768 where whole streams tile 32
    columns)"""
    if T <= 0 or T % 4 != 0:
        return False
    if not streaming:
        return C in (64, 96, 128, 192, 256, 384, 512, 768)
    if B * C * T * 4 >= (1 << 32):
        return False
    return C in (64, 96, 128, 192, 256, 384) or (C in (512, 768) and 32 % T == 0)


def resblock_chain_supported(C: int, T: int, nblk: int, B: int = 1, streaming: bool = True) -> bool:
    """mirror of hilc_resblock_chain_supported: the blocks of one stage in one launch"""
    if nblk < 2 or nblk > (3 if C in (96, 192) or C == (768 if streaming else 384) else 2) or T <= 0 or T % 4 != 0:
        return False
    if not streaming:
        return C in (64, 96, 128, 192, 256, 384, 512)
    if B * C * T * 4 >= (1 << 32):
        return False
    return C in (64, 96, 128, 192) or (C in (512, 768) and 32 % T == 0)


def resblock_chain_row_classes(C: int, streaming: bool = True) -> int:
    """mirror of hilc_resblock_chain_row_classes(_offline): the row split of the packed weights a chain launch reads"""
    if not streaming:
        return 8 if C in (512, 768) else (4 if C in (256, 384) else (2 if C in (128, 192) else 1))
    return 8 if C >= 512 or C == 256 else (12 if C == 384 else (1 if C in (64, 96) else 2))


def resblock_chain_pack(wt: Tensor, streaming: bool = True) -> Tensor:
    """k-major `[C,C]` pointwise weights -> the packed layout of hilc_resblock_chain for this width"""
    return _OPS.resblock_pack_rc(wt, resblock_chain_row_classes(wt.shape[0], streaming))


def _flatten_blocks(x: Tensor, Cc: int, blocks: Sequence[Sequence], hist, hist_out):
    """The per-block arguments of a stage op -> the flat lists of its schema (params, hist_in, hist_out, pre_scales, out_scales):
    `blocks[i]` = (w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, pre_scale, out_scale), `hist[i]` = that block's two caches, `hist_out[i]` =
    where its new caches `[B, C, 4]` go (None: fresh tensors).  hist None, the offline model, leaves both cache lists empty."""
    B = x.shape[0]
    params, hin, hout, pre, out = [], [], [], [], []
    for i, blk in enumerate(blocks):
        if len(blk) != 8:
            raise RuntimeError("a block is (w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, pre_scale, out_scale)")
        params.extend(blk[:6])
        pre.append(float(blk[6]))
        out.append(float(blk[7]))
        if hist is not None:
            hin.extend(hist[i])
            given = hist_out[i] if hist_out is not None and hist_out[i] is not None else (None, None)
            hout.extend([_state_out(given[0], x, B, Cc, 4), _state_out(given[1], x, B, Cc, 4)])
    return params, hin, hout, pre, out


def resblock_chain(x: Tensor, blocks: Sequence[Sequence], hist: Optional[Sequence[Sequence[Tensor]]] = None,
                   hist_out: Optional[Sequence[Optional[Sequence[Tensor]]]] = None):
    """The residual blocks of ONE stage of a streaming hop in one launch (hilc_resblock_chain): `blocks[i]` =
    (w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, pre_scale, out_scale) with w1p / w2p packed by `resblock_chain_pack`, `hist[i]` =
    that block's two caches, `hist_out[i]` = where its new caches go (None: fresh tensors).  Returns (y, [new caches of block 0,
    of block 1, ...]) — equal, bit for bit, to the blocks launched one by one.  hist None: the offline model (w1p / w2p packed with
    `resblock_chain_pack(w, streaming=False)`) -> y only."""
    params, hin, hout, pre, post = _flatten_blocks(x, x.shape[1], blocks, hist, hist_out)
    y = _OPS.resblock_chain(x, params, hin, hout, pre, post)
    return y if hist is None else (y, hout)


def decoder_stage_supported(C: int, T: int, nblk: int, stride: int, B: int = 1, streaming: bool = True) -> bool:
    """mirror of hilc_decoder_stage_supported (C = output channels of the stage, T = its samples per stream / clip)"""
    if not 1 <= nblk <= 3 or T <= 0 or T % 4 != 0 or stride <= 0 or T % stride != 0 or (streaming and B * C * T * 4 >= (1 << 32)):
        return False
    if C == 768:
        return stride == 8 and (32 % T == 0 if streaming else nblk == 1)
    if C == 384:
        return stride == 5
    return (C == 192 and stride == 4) or (C == 96 and stride == 2)


def decoder_stage(xin: Tensor, up: Sequence, blocks: Sequence[Sequence], hist: Optional[Sequence[Sequence[Tensor]]] = None,
                  up_hist: Optional[Tensor] = None, hist_out: Optional[Sequence[Optional[Sequence[Tensor]]]] = None,
                  up_hist_out: Optional[Tensor] = None):
    """A decoder stage in ONE launch (hilc_decoder_stage): its up-sampling layer `up` = (tr_w `[2C,2r]` — stride 5: the EXPANDED table of
    `up_conv_taps` —, w_lo, w_hi,
    bias `[C]`, in_scale, stride) — w_lo / w_hi = the two ROW halves of the k-major `[2C,C]` pointwise weight packed with
    `resblock_chain_pack` — and its residual blocks (`blocks[i]`, `hist[i]`, `hist_out[i]` as in `resblock_chain`).
    xin `[B,2C,T/r]`, up_hist `[B,2C,1]` -> (y `[B,C,T]`, [block caches...], up-sampling cache); hist None: the offline model -> y."""
    B, K2, _ = xin.shape
    tr_w, w_lo, w_hi, bias, in_scale, stride = up
    streaming = hist is not None
    params, hin, hout, pre, post = _flatten_blocks(xin, K2 // 2, blocks, hist, hist_out)
    uout = _state_out(up_hist_out, xin, B, K2, 1) if streaming else None
    y = _OPS.decoder_stage(xin, tr_w, w_lo, w_hi, bias, up_hist if streaming else None, uout, float(in_scale), int(stride),
                           params, hin, hout, pre, post)
    return (y, hout, uout) if streaming else y


def encoder_stage0_supported(T: int, nblk: int, stride: int, n_fft: int, hop: int, pre_ksize: int, B: int = 1, streaming: bool = False) -> bool:
    """mirror of hilc_encoder_stage0_supported: the encoder's FIRST stage with the first conv and its SpecBlock in the same launch (a hop: T >= 128
    so that a tile holds at most one stream start, and the 32-bit offsets of the streaming form)"""
    if not (1 <= nblk <= 2 and stride == 2 and n_fft == 64 and hop == 1 and pre_ksize == 5 and T > 0 and T % 4 == 0):
        return False
    return not streaming or (T >= 128 and B * 128 * T * 4 < (1 << 32))


def encoder_stage0(wav: Tensor, spec: Sequence, blocks: Sequence[Sequence], down: Sequence, res: Optional[Tensor] = None,
                   hist: Optional[Sequence[Sequence[Tensor]]] = None, hist_out: Optional[Sequence[Optional[Sequence[Tensor]]]] = None,
                   down_hist: Optional[Tensor] = None, down_hist_out: Optional[Tensor] = None, wav_hist: Optional[Tensor] = None):
    """The encoder's first conv, stage-0 SpecBlock, residual blocks and down-sampling layer in ONE launch (hilc_encoder_stage0):
    `spec` = (dft_packed, nyq_sin, pw_packed, bias, pre_w `[64,5]`, pre_b, pre_in_scale, mean, std, normalize, out_scale) as given to
    `spec_block_conv_pre`; `blocks`, `down`, `res` as in `encoder_stage`.  Offline (hist None): wav `[B,1,T]` -> `[B,128,T/2]`, equal bit for
    bit to `encoder_stage(spec_block_conv_pre(wav, ...), blocks, down)`.  A streaming hop (round 6): `wav_hist` `[B,1,H >= 63]` = the waveform
    cache, `hist` / `hist_out` / `down_hist` / `down_hist_out` as in `encoder_stage` -> (y, [block caches...], down cache)."""
    dft, nyq, pw, bias, pre_w, pre_b, pre_in, mean, std, normalize, out_scale = spec
    w_lo, w_hi, ddw_w, ddw_b, in_scale, stride = down
    B, Cc = wav.shape[0], pre_w.shape[0]
    streaming = hist is not None
    params, hin, hout, pre, post = _flatten_blocks(wav, Cc, blocks, hist, hist_out)
    dout = _state_out(down_hist_out, wav, B, 2 * Cc, int(stride)) if streaming else None
    y = _OPS.encoder_stage0(wav, wav_hist if streaming else None, dft, nyq, pw, bias, pre_w, pre_b, float(pre_in), float(mean), float(std),
                            int(normalize), float(out_scale), params, hin, hout, pre, post, w_lo, w_hi, ddw_w, ddw_b,
                            down_hist if streaming else None, dout, res, float(in_scale), int(stride))
    return (y, hout, dout) if streaming else y


def decoder_stage_post_supported(C: int, T: int, nblk: int, stride: int, ksize: int) -> bool:
    """mirror of hilc_decoder_stage_post_supported: the offline decoder's LAST stage with the closing conv in the same launch"""
    return C == 96 and stride == 2 and nblk == 3 and ksize == 5 and T > 0 and T % 4 == 0


def decoder_stage_post(xin: Tensor, up: Sequence, blocks: Sequence[Sequence], post: Sequence, hist: Optional[Sequence[Sequence[Tensor]]] = None,
                       up_hist: Optional[Tensor] = None, post_hist: Optional[Tensor] = None,
                       hist_out: Optional[Sequence[Optional[Sequence[Tensor]]]] = None, up_hist_out: Optional[Tensor] = None,
                       post_hist_out: Optional[Tensor] = None):
    """The decoder's last stage AND its closing layer in ONE launch (hilc_decoder_stage_post): `up`, `blocks` as in `decoder_stage`,
    `post` = (w `[C,5]`, bias `[1]` or None, in_scale, out_scale, do_tanh) as given to `conv_post`.  Offline (hist None):
    xin `[B,2C,T/r]` -> wav `[B,1,T]`, equal bit for bit to `conv_post(decoder_stage(...))`.  Streaming hop (round 6): `hist` / `up_hist` /
    `hist_out` / `up_hist_out` as in `decoder_stage`, `post_hist` `[B,C,4]` = the closing conv's cache ->
    (wav, [block caches...], up-sampling cache, closing conv's cache), equal bit for bit to `decoder_stage` + `conv_post` with the same caches."""
    tr_w, w_lo, w_hi, bias, in_scale, stride = up
    pw, pb, p_in, p_out, p_tanh = post
    B, K2, _ = xin.shape
    Cc = K2 // 2
    streaming = hist is not None
    params, hin, hout, pre, post_s = _flatten_blocks(xin, Cc, blocks, hist, hist_out)
    uout = _state_out(up_hist_out, xin, B, K2, 1) if streaming else None
    pout = _state_out(post_hist_out, xin, B, Cc, pw.shape[1] - 1) if streaming else None
    wav = _OPS.decoder_stage_post(xin, tr_w, w_lo, w_hi, bias, up_hist if streaming else None, uout, float(in_scale), int(stride),
                                  params, hin, hout, pre, post_s, pw, pb, post_hist if streaming else None, pout,
                                  float(p_in), float(p_out), bool(p_tanh))
    return (wav, hout, uout, pout) if streaming else wav


def encoder_stage_supported(C: int, T: int, nblk: int, stride: int, B: int = 1, streaming: bool = True) -> bool:
    """mirror of hilc_encoder_stage_supported (+ the 32-bit offsets of the streaming form)"""
    if nblk < 1 or nblk > 2 or T <= 0 or T % 4 != 0 or stride <= 0 or T % stride != 0 or (streaming and B * 2 * C * T * 4 >= (1 << 32)):
        return False
    if (C == 64 and stride == 2) or (C == 128 and stride == 4):
        return True
    if not streaming:
        return (C == 256 and stride == 5) or (C == 512 and stride == 8)                      # the wide stages of the offline model
    return (C == 256 and stride == 5 and T % 40 == 0) or (C == 512 and stride == 8 and T % 8 == 0 and 32 % T == 0)   # ... of a hop


def encoder_stage(x: Tensor, blocks: Sequence[Sequence], down: Sequence, hist: Optional[Sequence[Sequence[Tensor]]] = None,
                  hist_out: Optional[Sequence[Optional[Sequence[Tensor]]]] = None, down_hist: Optional[Tensor] = None,
                  down_hist_out: Optional[Tensor] = None, res: Optional[Tensor] = None):
    """An encoder stage in ONE launch (hilc_encoder_stage): its residual blocks (`blocks[i]` as in `resblock_chain`) and its
    down-sampling layer `down` = (w_lo, w_hi, dw_w `[2C,2r]`, dw_b `[2C]`, in_scale, stride) — w_lo / w_hi = the two column halves
    of the k-major `[C,2C]` pointwise weight, packed with `resblock_chain_pack`.  Offline (hist None): -> y `[B,2C,T/r]`.
    Streaming: hist / hist_out per block as in `resblock_chain`, `down_hist` `[B,2C,r]` -> (y, [block caches...], down cache).
    `res` `[B,2C,T/r]` is added to the output (the next stage's SpecBlock branch)."""
    B, Cc, _ = x.shape
    w_lo, w_hi, ddw_w, ddw_b, in_scale, stride = down
    streaming = hist is not None
    params, hin, hout, pre, post = _flatten_blocks(x, Cc, blocks, hist, hist_out)
    dout = _state_out(down_hist_out, x, B, 2 * Cc, int(stride)) if streaming else None
    y = _OPS.encoder_stage(x, params, hin, hout, pre, post, w_lo, w_hi, ddw_w, ddw_b, down_hist if streaming else None, dout, res,
                           float(in_scale), int(stride))
    return (y, hout, dout) if streaming else y


def resblock_pack(wt: Tensor) -> Tensor:
    """k-major `[C,C]` pointwise weights -> the fused block's packed layout (hilc_resblock_pack_weights)."""
    return _OPS.resblock_pack(wt)


def resblock(x: Tensor, w1p: Tensor, dw1_w: Tensor, dw1_b: Tensor, w2p: Tensor, dw2_w: Tensor, dw2_b: Tensor,
             pre_scale: float, out_scale: float, hist: Optional[Sequence[Tensor]] = None,
             hist_out: Optional[Sequence[Tensor]] = None):
    """Fully fused residual block (hilc_resblock): x `[B,C,T]` -> new tensor `[B,C,T]`; w1p / w2p = PACKED
    pointwise weights (`resblock_pack`).  Streaming: hist = (cache of depthwise 1, cache of depthwise 2), each
    `[B,C,4]` -> (y, [new caches]).  k-major `[C,C]` matrices are accepted too and packed on the fly (tests, tools);
    the plans hold the packed form."""
    if w1p.dim() == 2:
        w1p, w2p = resblock_pack(w1p), resblock_pack(w2p)
    if hist is None:
        return _OPS.resblock(x, w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, None, None, None, None, float(pre_scale),
                             float(out_scale))
    B, Cc, _ = x.shape
    o1 = _state_out(hist_out[0] if hist_out is not None else None, x, B, Cc, 4)
    o2 = _state_out(hist_out[1] if hist_out is not None else None, x, B, Cc, 4)
    y = _OPS.resblock(x, w1p, dw1_w, dw1_b, w2p, dw2_w, dw2_b, hist[0], hist[1], o1, o2, float(pre_scale),
                      float(out_scale))
    return y, [o1, o2]


def dw_conv(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, res: Optional[Tensor] = None,
            stride: int = 1, hist: Optional[Tensor] = None, want_hist: bool = False,
            in_scale: float = 1.0, in_elu: bool = False, out_scale: float = 1.0, out_elu: bool = False,
            hist_out: Optional[Tensor] = None):
    """x `[B,C,T]`, w `[C,k]` -> `[B,C,ceil(T/stride)]` (+ new history `[B,C,k-stride]` if want_hist)."""
    hout = _state_out(hist_out, x, x.shape[0], x.shape[1], w.shape[1] - stride) if want_hist else None
    y = _OPS.dw_conv(x, hist, w, bias, res, hout, int(stride), float(in_scale), bool(in_elu), float(out_scale),
                     bool(out_elu))
    return (y, hout) if want_hist else y


def dw_convtr(x: Tensor, w: Tensor, stride: int, hist: Optional[Tensor] = None, want_hist: bool = False,
              in_scale: float = 1.0, in_elu: bool = False, hist_out: Optional[Tensor] = None):
    """x `[B,C,T]`, w `[C,2*stride]` -> `[B,C,T*stride]`."""
    hout = _state_out(hist_out, x, x.shape[0], x.shape[1], 1) if want_hist else None
    y = _OPS.dw_convtr(x, hist, w, hout, int(stride), float(in_scale), bool(in_elu))
    return (y, hout) if want_hist else y


def conv_pre(wav: Tensor, w: Tensor, bias: Optional[Tensor], in_scale: float = 1.0,
             hist: Optional[Tensor] = None) -> Tensor:
    """wav `[B,1,T]`, w `[C,k]` -> `[B,C,T]`; hist `[B,1,L]` (L >= k-1) = waveform history."""
    return _OPS.conv_pre(wav, hist, w, bias, float(in_scale))


def conv_post(x: Tensor, w: Tensor, bias: Optional[Tensor], in_scale: float = 1.0, in_elu: bool = True,
              out_scale: float = 1.0, do_tanh: bool = True, hist: Optional[Tensor] = None,
              want_hist: bool = False, hist_out: Optional[Tensor] = None):
    """x `[B,C,T]`, w `[C,k]` -> `[B,1,T]`."""
    hout = _state_out(hist_out, x, x.shape[0], x.shape[1], w.shape[1] - 1) if want_hist else None
    y = _OPS.conv_post(x, hist, w, bias, hout, float(in_scale), bool(in_elu), float(out_scale), bool(do_tanh))
    return (y, hout) if want_hist else y


def stft_logmag(wav: Tensor, basis_t: Tensor, n_fft: int, hop: int, mean: float = 0.0, std: float = 1.0,
                normalize=True, hist: Optional[Tensor] = None) -> Tensor:
    """wav `[B,1,T]` -> `[B, n_fft/2+1, (T-1)//hop+1]`; normalize: False/0 log-mag, True/1 (log-mag - mean)/std,
    2 plain magnitude."""
    return _OPS.stft_logmag(wav, hist, basis_t, int(n_fft), int(hop), float(mean), float(std), int(normalize))


def spec_block_supported(n_fft: int, hop: int, C: int, T: int) -> bool:
    """mirror of hilc_spec_block_supported (plain Python: traceable)"""
    if n_fft not in (64, 128, 256) or hop != {64: 1, 128: 2, 256: 8}[n_fft] or C != n_fft or T <= 0:
        return False
    return ((T - 1) // hop + 1) % 4 == 0


def spec_block_profitable(n_fft: int, hop: int, C: int, T: int) -> bool:
    """supported, and the launch fills its 128-frame tiles: clips of 32 ... 511 frames (a streaming hop: 40 frames per stream at n_fft = 256)
    walk the flat frame space, longer ones per-clip tiles that must be >= 60 % full"""
    if not spec_block_supported(n_fft, hop, C, T):
        return False
    tf = (T - 1) // hop + 1
    if 32 <= tf < 512:          # round 6: short clips (a streaming hop) tile the FLAT frame space — every tile full (csrc/spec.hip: FLAT)
        return True
    return tf * 10 >= ((tf + 127) // 128) * 128 * 6


def spec_block_tables(basis_t: Tensor, wt: Tensor, n_fft: int):
    """The fused SpecBlock's operands from the un-fused ones: basis_t `[n_fft][m_pad]` (interleaved cos_k, sin_k columns,
    k = 0..n_fft/2: hilc_stft_logmag's layout) -> packed DFT matrix with exactly n_fft rows + the sin_{n_fft/2} row;
    wt `[n_fft/2+1][C]` -> packed conv weight.  Pure column selection: no arithmetic touches the basis."""
    cols = [0, n_fft] + list(range(2, n_fft))              # cos_0, cos_{N/2}, then (cos_k, sin_k), k = 1..N/2-1
    dft = basis_t[:, cols].contiguous()
    nyq = basis_t[:, n_fft + 1].contiguous()
    return (_OPS.spec_block_pack(dft, int(n_fft), 0), nyq, _OPS.spec_block_pack(wt.contiguous(), int(n_fft), 1))


def spec_block(wav: Tensor, dft_packed: Tensor, nyq_sin: Tensor, pw_packed: Tensor, bias: Optional[Tensor], x: Optional[Tensor],
               n_fft: int, hop: int, mean: float = 0.0, std: float = 1.0, normalize=True, out_scale: float = 1.0,
               hist: Optional[Tensor] = None) -> Tensor:
    """One-launch SpecBlock (hilc_spec_block): wav `[B,1,T]`, x `[B,n_fft,T/hop]` -> x + out_scale * (W spec + bias);
    hist `[B,1,L]` (L >= n_fft-1) = the waveform before t = 0 (streaming hop).  x None: the branch alone."""
    return _OPS.spec_block(wav, hist, dft_packed, nyq_sin, pw_packed, bias, x, int(n_fft), int(hop), float(mean), float(std),
                           int(normalize), float(out_scale))


def spec_block_conv_pre(wav: Tensor, dft_packed: Tensor, nyq_sin: Tensor, pw_packed: Tensor, bias: Optional[Tensor],
                        pre_w: Tensor, pre_b: Optional[Tensor], pre_in_scale: float, n_fft: int, hop: int, mean: float = 0.0,
                        std: float = 1.0, normalize=True, out_scale: float = 1.0, hist: Optional[Tensor] = None) -> Tensor:
    """First encoder stage in one launch: conv_pre(wav) + SpecBlock branch (hilc_spec_block_conv_pre)."""
    return _OPS.spec_block_conv_pre(wav, hist, dft_packed, nyq_sin, pw_packed, bias, pre_w, pre_b, float(pre_in_scale), int(n_fft),
                                    int(hop), float(mean), float(std), int(normalize), float(out_scale))


def tail(x: Tensor, hist: Optional[Tensor], pad: int, out: Optional[Tensor] = None) -> Tensor:
    """Last `pad` samples of cat([hist, x], -1) along time; x `[B,C,T]`, hist `[B,C,L]`."""
    out = _state_out(out, x, x.shape[0], x.shape[1], pad)
    _OPS.tail(x, hist, out)
    return out


def l2norm(x: Tensor, eps: float = 1e-12, scale: float = 1.0, channel_last_out: bool = False) -> Tensor:
    return _OPS.l2norm(x, float(eps), float(scale), bool(channel_last_out))


def is_scalar_n(n) -> bool:
    """anything integer-like (python / numpy ints, 0-dim arrays and tensors) is ONE n for the whole batch"""
    return isinstance(n, numbers.Integral) or (isinstance(n, (Tensor, np.ndarray)) and n.ndim == 0)


def per_clip_n(n, B: int, Nq: int, device):
    """`n` as the reference takes it (one int for the whole batch) or one int per clip (mixed-bitrate batch).
    Returns (rows, int32 [B] device tensor or None).  Every entry obeys the reference's assert
    (`models/hilcodec/vector_quantize.py:213-214`)."""
    if is_scalar_n(n):
        return int(n), None
    host = torch.as_tensor(n).detach().to("cpu", torch.int64).reshape(-1)
    if host.numel() != B:
        raise RuntimeError(f"per-clip n needs {B} entries, got {host.numel()}")
    lo, hi = int(host.min()), int(host.max())
    assert 1 <= lo and hi <= Nq, f"'n' must be in range of 1 <= n <= {Nq}"
    return hi, host.to(torch.int32).to(device)


def _device_n(n, n_clip: Tensor, B: int):
    """the device-resident per-clip form: `n` = rows of the indices, `n_clip` int32 `[B]` on the GPU, entries in [1, n] (the
    kernels clamp to that range).  Neither copied to the host nor range-checked per call: the caller validates (a graphed hop
    uploads the entries it has checked)."""
    if n_clip.numel() != B:
        raise RuntimeError(f"n_clip needs {B} entries, got {n_clip.numel()}")
    return int(n), n_clip


def rvq_encode(z: Tensor, codebooks: Tensor, codebooks_t: Tensor, norms: Tensor, n,
               channel_last: bool = False, stage_major: bool = False, want_q: bool = True,
               want_loss: bool = False, valu_only: bool = False, n_clip: Optional[Tensor] = None):
    """Returns (indices int64, q or None, loss 0-d or None).  `n`: int, or one int per clip (rows of `indices`
    beyond a clip's own n hold -1).  `valu_only` (HILC_RVQ_VALU_ONLY of the C ABI): keep batches of 8 192 frames and more on the
    VALU form instead of the matrix pipe — same fmaf chains, same bits; the quantiser modules pass their `rvq_valu_only` attribute.
    `n_clip`: the per-clip n as an int32 device tensor `[B]` with `n` (int) the rows — see `_device_n`."""
    B = z.shape[0]
    n, n_clip = per_clip_n(n, B, codebooks.shape[0], z.device) if n_clip is None else _device_n(n, n_clip, B)
    idx, q, loss = _OPS.rvq_encode(z, codebooks, codebooks_t, norms, n_clip, n, bool(channel_last), bool(stage_major),
                                   bool(want_q), bool(want_loss), RVQ_VALU_ONLY if valu_only else 0)
    return idx, (q if want_q else None), (loss if want_loss else None)


def rvq_decode(indices: Tensor, codebooks: Tensor, n, channel_last: bool = True,
               stage_major: bool = True, n_clip: Optional[Tensor] = None) -> Tensor:
    """`n`: int or one int per clip; or `n_clip` = int32 device tensor `[B]` with `n` the rows (`_device_n`)"""
    B = indices.shape[1] if stage_major else indices.shape[0]
    n, n_clip = per_clip_n(n, B, codebooks.shape[0], indices.device) if n_clip is None else _device_n(n, n_clip, B)
    return _OPS.rvq_decode(indices, codebooks, n_clip, n, bool(channel_last), bool(stage_major))


def rvq_ema_stats(z: Tensor, codebooks: Tensor, indices: Tensor, n: int, channel_last: bool = False,
                  stage_major: bool = False) -> Tensor:
    """Training-side cluster statistics of the first n stages: bucket `[n, K + K*C]` (counts | residual sums),
    the reference's per-stage all-reduce payload (`vector_quantize.py:155-162`) for all stages at once."""
    return _OPS.rvq_ema_stats(z, codebooks, indices, int(n), bool(channel_last), bool(stage_major))


def rvq_ema_update(embed: Tensor, ema_num: Tensor, ema_embed: Tensor, bucket: Tensor, decay: float) -> None:
    """In place on stacked `[n,K,C]` / `[n,K]` tensors: EMA of counts and sums, embed = ema_embed / ema_num."""
    _OPS.rvq_ema_update(embed, ema_num, ema_embed, bucket, float(decay))


def state_slots_apply(block: Tensor, layout: StateLayout, action: Tensor, records: Optional[Tensor] = None) -> None:
    """In place on a state block (`layout`): stream b zeroed where action[b] == -1, loaded from row r-1 of `records`
    `[R, layout.record_len]` where action[b] == r >= 1, kept otherwise; `action` int32 `[layout.streams]` on the device."""
    if block.numel() < layout.total or action.numel() != layout.streams:
        raise RuntimeError("state_slots_apply: block or action does not match the layout")
    if records is not None and (records.dim() != 2 or records.shape[1] != layout.record_len):
        raise RuntimeError(f"state_slots_apply: records must be [R, {layout.record_len}]")
    off, lens = layout.tables(block.device)
    _OPS.state_slots_apply(block, off, lens, action, records)


def state_slots_gather(block: Tensor, layout: StateLayout, slots: Tensor) -> Tensor:
    """records `[len(slots), layout.record_len]` of the streams `slots` (int32, device) of a state block"""
    if block.numel() < layout.total:
        raise RuntimeError("state_slots_gather: block does not match the layout")
    off, lens = layout.tables(block.device)
    return _OPS.state_slots_gather(block, off, lens, slots, layout.streams, layout.record_len)


def state_slots_hold(src: Tensor, dst: Tensor, layout: StateLayout, hold: Tensor, wav: Optional[Tensor] = None,
                     indices: Optional[Tensor] = None, packets: Optional[Tensor] = None, nbytes: Optional[Tensor] = None,
                     slices: Optional[int] = None) -> None:
    """Streams b with hold[b] != 0 (int32 `[layout.streams]` on the device) do not advance: their parts of `dst` (the block a hop
    wrote) are copied back from `src` (the block it read), their `wav` rows (`[streams, ...]` fp32) are set to 0, their `indices`
    (`[n, streams, T]` int64) to -1, their `packets` rows (`[streams, stride]` uint8) and `nbytes` (`[streams]` int32) to 0.
    Every output is optional; in place.  `slices`: only the layout's first `slices` slices (None: all of them)."""
    B = layout.streams
    if src.numel() < layout.total or dst.numel() < layout.total or hold.numel() != B:
        raise RuntimeError("state_slots_hold: src, dst or hold does not match the layout")
    if wav is not None and (wav.shape[0] != B or wav.numel() == 0):
        raise RuntimeError(f"state_slots_hold: wav must be [{B}, ...]")
    if indices is not None and (indices.dim() != 3 or indices.shape[1] != B):
        raise RuntimeError(f"state_slots_hold: indices must be [n, {B}, T]")
    if packets is not None and (packets.dim() != 2 or packets.shape[0] != B):
        raise RuntimeError(f"state_slots_hold: packets must be [{B}, stride]")
    if nbytes is not None and nbytes.numel() != B:
        raise RuntimeError(f"state_slots_hold: nbytes must have {B} entries")
    off, lens = layout.tables(src.device)
    if slices is not None:
        off, lens = off[:slices], lens[:slices]
    _OPS.state_slots_hold(src, dst, off, lens, hold, wav, indices, packets, nbytes)


def pack_codes_10bit(indices: Tensor, n_clip: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """stage-major indices `[n, B, T]` -> (packets uint8 `[B, wire.packet_bytes(n, T)]`, nbytes int32 `[B]`): stream b's first
    n_b stages (`n_clip` int32 device `[B]`, clamped to [1, n]; None = n) in the wire format of `wire.pack_stream_packet`, the row
    zero past its length.  Codes outside [0, 1024) are clamped into it."""
    if indices.dim() != 3:
        raise RuntimeError("pack_codes_10bit: indices must be [n, B, T]")
    if n_clip is not None and n_clip.numel() != indices.shape[1]:
        raise RuntimeError(f"n_clip needs {indices.shape[1]} entries, got {n_clip.numel()}")
    return _OPS.pack_codes_10bit(indices, n_clip)


def rvq_decode_packed(packets: Tensor, codebooks: Tensor, n: int, frames: int, n_clip: Optional[Tensor] = None) -> Tensor:
    """packets `[B, wire.packet_bytes(n, frames)]` -> q `[B, frames, C]` (channel-last), bit-identical to `rvq_decode` of the
    unpacked indices with the same per-stream n (`n_clip` int32 device `[B]`, clamped to [1, n]; None = n)"""
    if n_clip is not None and n_clip.numel() != packets.shape[0]:
        raise RuntimeError(f"n_clip needs {packets.shape[0]} entries, got {n_clip.numel()}")
    return _OPS.rvq_decode_packed(packets, n_clip, codebooks, int(n), int(frames))


def conceal_prepare(state: Tensor, action: Tensor, hold: Tensor, lost: Tensor, n_slot: Tensor, packets: Tensor, frames: int,
                    fade_hops: int) -> Tensor:
    """The receiver's concealment step before its packed dequantiser, in place on its per-hop control rows (int32 `[B]` device
    rows `action`, `hold`, `lost`, `n_slot`; `packets` uint8 `[B, wire.packet_bytes(n_max, frames)]`) and the concealment state
    (int32 `[B, n_max + 3]`): received slots store their last frame, concealed slots get the substitute packet and n, slots with
    nothing to repeat are held.  Returns the per-slot ramp word (int32 `[B]`) that `conceal_gain` reads."""
    return _OPS.conceal_prepare(state, action, hold, lost, n_slot, packets, int(frames), int(fade_hops))


def conceal_gain(wav: Tensor, ramp: Tensor, gains: Tensor, weights: Tensor) -> None:
    """wav `[B, ...]` (fp32, `weights.numel()` samples per row) times the fade ramp of each row with a ramp word (`conceal_prepare`):
    gain = G[a] + (G[c] - G[a]) * W[s], each operation rounded on its own in fp32; `gains` = G `[F + 1]`, `weights` = W
    (`wire.conceal_tables`).  Rows without a ramp are not touched; in place."""
    _OPS.conceal_gain(wav, ramp, gains, weights)


def pack_codes_10bit_fec(indices: Tensor, prev_in: Tensor, prev_out: Tensor, m: int, n_clip: Optional[Tensor] = None,
                         action: Optional[Tensor] = None, hold: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The FEC sender's packets: stage-major indices `[n, B, T]` -> (packets uint8 `[B, wire.packet_bytes(n + m, T)]`, nbytes int32
    `[B]`).  Stream b's packet is `wire.pack_fec_packet` of its first n_b stages (`n_clip`, clamped to [m, n]; None = n) and, when
    its previous-codes row in `prev_in` (int32 `[B, 1 + m T]`: valid, then the m x T codes) is valid, those codes.  `prev_out`
    (distinct from `prev_in`) receives this hop's first m stages, in place.  `action` / `hold` (int32 `[B]`, optional): a slot
    with an action has no previous hop; a held slot keeps its row and sends nothing (row 0, nbytes 0)."""
    if indices.dim() != 3:
        raise RuntimeError("pack_codes_10bit_fec: indices must be [n, B, T]")
    if prev_in is prev_out:
        raise RuntimeError("pack_codes_10bit_fec: prev_in and prev_out must be distinct buffers")
    return _OPS.pack_codes_10bit_fec(indices, n_clip, prev_in, prev_out, action, hold, int(m))


def fec_select(packets: Tensor, fec: Tensor, n_slot: Tensor, n: int, m: int, frames: int) -> Tensor:
    """The FEC receiver's compaction: wide rows uint8 `[B, wire.packet_bytes(n + m, frames)]` -> rows `[B, wire.packet_bytes(n,
    frames)]`: `wire.fec_primary` of each row, or `wire.fec_redundant` where `fec` (int32 `[B]`) is set, whose `n_slot` entry
    (int32 `[B]`, in place: the row's primary n on entry) becomes m."""
    return _OPS.fec_select(packets, fec, n_slot, int(n), int(m), int(frames))


def dtx_encode(x: Tensor, run: Tensor, packets: Tensor, nbytes: Tensor, indices: Tensor, level_thr: Tensor, thr_vad: float, order: int,
               hangover: int, sid_interval: int, action: Optional[Tensor] = None, hold: Optional[Tensor] = None,
               prev: Optional[Tensor] = None) -> Tensor:
    """The DTX sender's step after its packer (dtx.encode_model): the 24 kHz hop `x` fp32 `[B, 1, 320 T]` is analysed per stream,
    `run` (int32 `[B]`) advances in place, SID and SILENT hops rewrite their `packets` row (uint8 `[B, stride >= 1 + order]`),
    `nbytes` (int32 `[B]`) and `indices` (int64 `[n, B, T]`) in place, and clear word 0 of their `prev` row (the FEC packer's
    int32 `[B, 1 + m T]` output, optional).  `level_thr`: float64 `[127]` (dtx.level_table) on the device.  `action` / `hold`
    (int32 `[B]`, optional): the session rows.  Returns each stream's kind (int32 `[B]`: dtx.HELD / SPEECH / SID / SILENT)."""
    return _OPS.dtx_encode(x, action, hold, run, packets, nbytes, indices, prev, level_thr, float(thr_vad), int(order), int(hangover),
                           int(sid_interval))


def cng_synth(packets: Tensor, hold: Tensor, state: Tensor, wav: Tensor, gains: Tensor, order: int, action: Optional[Tensor] = None,
              restore: Optional[Tensor] = None) -> None:
    """The CN receiver's step after its decoder (dtx.cng_model), in place: per slot, `hold` (int32 `[B]`) 2 = a SID is in its
    `packets` row (uint8 `[B, stride >= 1 + order]`), 3 = silent, 0 = decoded this hop, else held.  Slots that produce noise get
    their `wav` row (fp32 contiguous `[B, 1, 320 T]`) overwritten, hold 0 and `restore` 1; a silent slot without a SID gets hold 1.
    `state`: int32 `[B, 3 + 2 order]` (dtx.state_words); `gains`: fp32 `[128]` (dtx.gain_table) on the device."""
    _OPS.cng_synth(packets, action, hold, state, wav, restore, gains, int(order))


def packet_header(packets: Tensor, nbytes: Tensor, ctr_in: Tensor, ctr_out: Tensor, n: int, m: int, frames: int,
                  n_clip: Optional[Tensor] = None, kind: Optional[Tensor] = None, action: Optional[Tensor] = None,
                  hold: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The headed sender's last step: packets uint8 `[B, wire.packet_bytes(n + m, frames)]` and nbytes int32 `[B]` -> (rows uint8
    `[B, wire.transport_bytes(n, m, frames)]`, byte counts int32 `[B]`, 0 = nothing to send): each sent row is
    `wire.pack_transport(c_b, packet, n_b, sid, fec)` with c_b the slot's hop counter from `ctr_in` (int32 `[B]`); `ctr_out` (distinct)
    receives the next counters, in place.  `n_clip`, `kind` (dtx kinds), `action`, `hold`: optional int32 `[B]` session rows."""
    if ctr_in is ctr_out:
        raise RuntimeError("packet_header: ctr_in and ctr_out must be distinct buffers")
    return _OPS.packet_header(packets, nbytes, n_clip, kind, action, hold, ctr_in, ctr_out, int(n), int(m), int(frames))


def jitter_step(arrivals: Tensor, offsets: Tensor, hold: Tensor, n_slot: Tensor, packets: Tensor, state: Tensor, meta: Tensor,
                ring: Tensor, n: int, m: int, frames: int, order: Optional[int], depth: int, action: Optional[Tensor] = None,
                lost: Optional[Tensor] = None, fec: Optional[Tensor] = None) -> None:
    """The jitter receiver's first step (jitter.JitterModel), in place: this hop's arrivals (int32 `[A, 1 + ceil((3 + stride) / 4)]`:
    byte count, then the headed packet; grouped by slot, `offsets` int32 `[B + 1]`) go into each slot's ring (`meta` int32 `[B, C]`,
    `ring` int32 `[B, C, ceil(stride / 4)]`) and state row (`state` int32 `[B, 14]`), and the slot's play decision is written to the
    `hold` (in: the host's holds), `n_slot`, `lost` (conceal only), `fec` (m >= 1 only) rows and `packets` (uint8 `[B, stride]`),
    stride = wire.packet_bytes(n + m, frames).  `order`: the comfort-noise order (None: a SID is malformed)."""
    _OPS.jitter_step(arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, int(n), int(m), int(frames),
                     -1 if order is None else int(order), int(depth))


def jitter_adapt_step(arrivals: Tensor, offsets: Tensor, hold: Tensor, n_slot: Tensor, packets: Tensor, state: Tensor, meta: Tensor,
                      ring: Tensor, adapt: Tensor, n: int, m: int, frames: int, order: Optional[int], cfg,
                      action: Optional[Tensor] = None, lost: Optional[Tensor] = None, fec: Optional[Tensor] = None) -> None:
    """`jitter_step` with an adaptive playout clock (jitter.JitterModel with cfg.adapt), in place: the same arguments, and `adapt`
    (int32 `[B, jitter.AD_WORDS]`), each slot's adapt row.  `cfg`: the jitter.JitterConfig, its `adapt` set (depth and the
    AdaptConfig's parameters; the capacity is `meta`'s width)."""
    a = cfg.adapt
    _OPS.jitter_adapt_step(arrivals, offsets, action, hold, n_slot, lost, fec, packets, state, meta, ring, adapt, int(n), int(m),
                           int(frames), -1 if order is None else int(order), int(cfg.depth), int(a.headroom),
                           a.max_late_for(meta.shape[1]), int(a.window), int(a.resync), int(a.force_windows))


def resample_poly(x: Tensor, taps: Tensor, L: int, M: int, hist: Optional[Tensor] = None, hist_out: Optional[Tensor] = None) -> Tensor:
    """x fp32 `[B, 1, T]` -> y `[B, 1, ceil(T L / M)]`: the polyphase conversion of hilcodec_amd/resample.py with the phase-major tap
    table `taps` `[L, Q]` (resample.device_taps).  `hist` `[B, 1, Q - 1]`: the input samples before x (None: zeros); `hist_out`
    (distinct from `hist`): receives the last Q - 1 samples of hist || x, in place, in the style of `cache_out=`."""
    if hist is not None and hist is hist_out:
        raise RuntimeError("resample_poly: hist and hist_out must be distinct buffers (the kernel refuses one shared pointer too)")
    return _OPS.resample_poly(x, hist, hist_out, taps, int(L), int(M))


def mix_levels(wav: Tensor, score: Tensor, action: Optional[Tensor] = None) -> None:
    """The mixer's first step (mixer.py), in place: `score` (float64 `[B]`) becomes max(E, score / 2) with E the float64 energy of the
    slot's `wav` row (fp32 contiguous `[B, 1, L]`); a slot with an `action` (int32 `[B]`, optional) starts from score 0."""
    _OPS.mix_levels(wav, score, action)


def mix_rooms(wav: Tensor, room: Tensor, score: Tensor, top_k: int, mixed: Tensor, speakers: Tensor) -> None:
    """The mixer's second step (mixer.py), in place: per slot of `room` (int32 `[B]`, -1 = none) the clamped fp32 sum of the rows of
    its room's `top_k` highest-scoring other members -> `mixed` (fp32 `[B, 1, L]`, not `wav`), and `speakers` (int32 `[B]`): 1 for the
    slots that are among their room's top_k.  `score`: float64 `[B]` as `mix_levels` left it."""
    _OPS.mix_rooms(wav, room, score, int(top_k), mixed, speakers)


def mix_gains(wav: Tensor, gains: Tensor, power: Tensor, level, action: Optional[Tensor] = None) -> None:
    """The mixer's levelling step (mixer.py, "Gain"), in place: per slot `gains` (float64 `[B, 2]`) becomes (the previous hop-end gain,
    this hop's end gain) and `power` (float64 `[B]`) the smoothed power, by the rule of `level` (a mixer.LevelConfig) on the energy of
    the slot's `wav` row; a slot with an `action` starts from gains (1, 1) and power 0."""
    _OPS.mix_gains(wav, gains, power, action, level.gate2, level.lo, level.hi, float(level.up), float(level.down),
                   float(level.min_gain), float(level.max_gain), float(level.smooth))


def mix_rooms_dyn(wav: Tensor, room: Tensor, score: Tensor, top_k: int, mixed: Tensor, speakers: Tensor, gains: Optional[Tensor] = None,
                  limiter: Optional[Tensor] = None, limit=None, action: Optional[Tensor] = None) -> None:
    """`mix_rooms` with levelled terms (`gains` float64 `[B, 2]` as `mix_gains` left it) and / or the limiter of `limit` (a
    mixer.LimitConfig; its state `limiter` float64 `[B, 2]`, in place) instead of the clamp (mixer.py, "Mix" and "Limit"); a slot with an
    `action` starts from limiter (0, 1).  Neither row: `mix_rooms`."""
    if (limiter is None) != (limit is None):
        raise RuntimeError("mix_rooms_dyn: limiter (the state row) and limit (its LimitConfig) come together")
    ceiling, release, sub = (1.0, 0.5, 16) if limit is None else (float(limit.ceiling), float(limit.release), int(limit.sub))
    _OPS.mix_rooms_dyn(wav, room, score, int(top_k), gains, limiter, ceiling, release, sub, action, mixed, speakers)


def room_mix(wav: Tensor, room: Tensor, score: Optional[Tensor] = None, top_k: int = 3,
             dynamics=None) -> Tuple[Tensor, Tensor, Tensor]:
    """`hilcodec_amd.mix_rooms`: one hop of the room mixer for callers without a graph (two launches, three with levelling;
    mixer.MixModel bit for bit).  wav fp32 `[B, 1, L]` and room int32 `[B]` on the GPU; `score` float64 `[B]`: the state returned by the
    previous call (updated in place; None: a fresh one); `dynamics`: a mixer.Dynamics for B slots on wav's device, whose levelling and
    limiter rows are updated in place (None: the plain clamped sum).  Returns (mixed fp32 `[B, 1, L]`, speakers int32 `[B]`, score)."""
    from .mixer import Dynamics, MixConfig
    top_k = int(MixConfig(top_k).top_k)
    if dynamics is not None and not isinstance(dynamics, Dynamics):
        raise ValueError(f"mix_rooms: dynamics must be a mixer.Dynamics or None, got {dynamics!r}")
    wav = wav.contiguous()
    B = wav.shape[0]
    if dynamics is not None and (dynamics.batch != B or dynamics.device.type != wav.device.type
                                 or (dynamics.device.index is not None and dynamics.device.index != wav.device.index)):
        raise ValueError(f"mix_rooms: dynamics holds {dynamics.batch} slots on {dynamics.device}, wav has {B} on {wav.device}")
    if score is None:
        score = torch.zeros(B, dtype=torch.float64, device=wav.device)
    mixed = torch.empty_like(wav)
    speakers = torch.empty(B, dtype=torch.int32, device=wav.device)
    mix_levels(wav, score)
    if dynamics is None or (dynamics.level is None and dynamics.limit is None):
        mix_rooms(wav, room, score, top_k, mixed, speakers)
        return mixed, speakers, score
    if dynamics.level is not None:
        mix_gains(wav, dynamics.gains, dynamics.power, dynamics.level)
    mix_rooms_dyn(wav, room, score, top_k, mixed, speakers, dynamics.gains, dynamics.limiter, dynamics.limit)
    return mixed, speakers, score


def vbr_select(z: Tensor, indices: Tensor, codebooks: Tensor, n_lo: int, rho: float, stage_bits: int = 0, rate_bits: int = 0,
               burst_bits: int = 0, n_clip: Optional[Tensor] = None, action: Optional[Tensor] = None, hold: Optional[Tensor] = None,
               credit: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The VBR sender's step between its quantiser and its packer (vbr.VbrModel): `z` fp32 `[B, T, C]` (the quantiser's input),
    `indices` int64 `[n, B, T]` (in place: rows >= a slot's n_eff become -1), `codebooks` fp32 `[Nq, K, C]` -> (n_eff int32 `[B]`,
    distortion float64 `[B, n + 1]`).  `n_clip` (int32 `[B]`, optional): each slot's ceiling; `action` / `hold` (int32 `[B]`, optional):
    the session rows; `credit` (int32 `[B]`, in place, optional): the token bucket of a capped sender, with vbr.bucket_bits' three
    numbers (without it `rate_bits` must be 0)."""
    return _OPS.vbr_select(z, indices, codebooks, n_clip, action, hold, credit, int(n_lo), float(rho), int(stage_bits), int(rate_bits),
                           int(burst_bits))


def rx_report(jitter_state: Tensor, rows: Tensor, reports: Tensor, due: Tensor, cfg, action: Optional[Tensor] = None) -> None:
    """The reporting receiver's step after its jitter step (report.ReportModel), in place: `jitter_state` (int32 `[B, 14]`, read only)
    -> `rows` (int32 `[B, report.RP_WORDS]`), `reports` (uint8 `[B, 3]`: each slot's latest report, written when one is emitted) and
    `due` (int32 `[B]`: 1 where one was emitted on this hop).  `cfg`: the report.ReportConfig; `action` (int32 `[B]`, optional): the
    session row, a start clears the slot."""
    _OPS.rx_report(jitter_state, action, rows, reports, due, int(cfg.window), int(cfg.interval))


def fec_adapt(prev: Tensor, rows: Tensor, fec_on: Tensor, m: int, frames: int, cfg, report: Optional[Tensor] = None,
              action: Optional[Tensor] = None, hold: Optional[Tensor] = None) -> None:
    """The adaptive sender's step ahead of its packer (report.FecAdaptModel), in place: `rows` (int32 `[B, report.FA_WORDS]`) take this
    hop's `report` words (int32 `[B]`, report.report_word, 0: none; optional), word 0 of `prev` (int32 `[B, 1 + m frames]`, the
    previous-codes rows the packer reads) is cleared for the slots that are off and not held, and `fec_on` (int32 `[B]`) is each slot's
    switch.  `cfg`: the report.FecAdaptConfig; `action` / `hold` (int32 `[B]`, optional): the session rows."""
    _OPS.fec_adapt(report, action, hold, rows, prev, fec_on, int(m), int(frames), int(cfg.on_q8), int(cfg.off_q8), int(cfg.calm_reports),
                   int(cfg.timeout_hops), bool(cfg.initial_on))


def nack_build(jitter_state: Tensor, meta: Tensor, rows: Tensor, nacks: Tensor, due: Tensor, cfg, m: int = 0,
               action: Optional[Tensor] = None) -> None:
    """The NACKing receiver's step after its jitter step (rtx.NackModel), in place: `jitter_state` (int32 `[B, 14]`) and `meta` (int32
    `[B, capacity]`, the ring's meta words), both read only -> `rows` (int32 `[B, rtx.NK_WORDS]`), `nacks` (uint8 `[B, 4]`: each slot's
    latest NACK, wire.pack_nack, written when one is emitted) and `due` (int32 `[B]`: 1 where one was emitted on this hop).  `cfg`: the
    rtx.NackConfig; `m`: the receiver's fec_stages; `action` (int32 `[B]`, optional): the session row, a start clears the slot."""
    _OPS.nack_build(jitter_state, meta, action, rows, nacks, due, int(m), int(cfg.rtt_hops), int(cfg.retry_hops), int(cfg.max_requests),
                    bool(cfg.skip_fecable))


def rtx_step(packets: Tensor, nbytes: Tensor, tags: Tensor, ring: Tensor, rows: Tensor, out: Tensor, out_nbytes: Tensor,
             nack_base: Optional[Tensor] = None, nack_bitmap: Optional[Tensor] = None, action: Optional[Tensor] = None) -> None:
    """The retransmitting sender's step behind its header (rtx.RtxModel), in place: this hop's headed `packets` (uint8 `[B,
    row_bytes]`) and `nbytes` (int32 `[B]`) enter the history — `tags` (int32 `[B, history]`), `ring` (int32 `[B, history, ceil(row_bytes
    / 4)]`) — and the hops that this hop's NACKs ask for (`nack_base` / `nack_bitmap`, int32 `[B]` each: rtx.nack_words, 0: none; both or
    neither) are copied to `out` (uint8 `[B, per_hop, row_bytes]`) with `out_nbytes` (int32 `[B, per_hop]`); `rows` (int32 `[B,
    rtx.RX_WORDS]`) count.  `action` (int32 `[B]`, optional): the session row, a start empties the slot's history."""
    _OPS.rtx_step(packets, nbytes, nack_base, nack_bitmap, action, tags, ring, rows, out, out_nbytes)


def rate_ceiling(rows: Tensor, n_ceil: Tensor, n: int, frames: int, m: int, header: bool, cfg, report: Optional[Tensor] = None,
                 action: Optional[Tensor] = None, hold: Optional[Tensor] = None, n_clip: Optional[Tensor] = None,
                 prev: Optional[Tensor] = None) -> None:
    """The rate-controlled sender's step in front of its quantiser (rate.RateModel.ceiling), in place: `rows` (int32 `[B, rate.RC_WORDS]`)
    take this hop's `report` words (int32 `[B]`, report.report_word, 0: none; optional), each slot's rate moves and its bucket fills, and
    `n_ceil` (int32 `[B]`) is the most stages the bucket pays for.  `cfg`: the rate.RateConfig of a sender with `n` stages, `frames`
    frames, `m` redundant stages and the transport header or not (rate.bucket checks it); `action` / `hold` (int32 `[B]`, optional): the
    session rows; `n_clip` (int32 `[B]`, optional): each slot's own ceiling; `prev` (int32 `[B, 1 + m frames]`, optional, read only): the
    previous-codes rows the packer reads on this hop."""
    bits = bucket(cfg, frames, m, header)
    _OPS.rate_ceiling(report, action, hold, n_clip, prev, rows, n_ceil, int(frames), int(n), int(m), bool(header), bits.min_bits,
                      bits.max_bits, bits.start_bits, int(cfg.high_q8), int(cfg.low_q8), int(cfg.increase_q8), int(cfg.burst_hops),
                      int(cfg.timeout_hops))


def rate_charge(nbytes: Tensor, rows: Tensor, cfg, rtx_nbytes: Optional[Tensor] = None) -> None:
    """The rate-controlled sender's last step (rate.RateModel.charge), in place: the credit of `rows` (int32 `[B, rate.RC_WORDS]`) pays
    for this hop's `nbytes` (int32 `[B]`, the packets as sent) and `rtx_nbytes` (int32 `[B, per_hop]`, optional: its retransmissions),
    down to a debt of cfg.burst_hops hops of the slot's rate."""
    _OPS.rate_charge(nbytes, rtx_nbytes, rows, int(cfg.burst_hops))


def rx_bwe(arrivals: Tensor, offsets: Tensor, times: Tensor, rows: Tensor, caps: Tensor, due: Tensor, cfg, n: int, frames: int,
           m: int = 0, order: Optional[int] = None, action: Optional[Tensor] = None) -> None:
    """The estimating receiver's step after its jitter step (bwe.BweModel), in place: one hop's `arrivals` (int32 `[max_arrivals, 1 +
    ceil(tb / 4)]` records grouped by slot, tb = wire.transport_bytes(n, m, frames)), `offsets` (int32 `[B + 1]`) and the records'
    arrival ticks `times` (int32 `[max_arrivals]`, 1/24000 s mod 2^32), all read only -> `rows` (int32 `[B, bwe.BW_WORDS]`), `caps`
    (uint8 `[B, 3]`: each slot's latest cap, wire.pack_cap, written when one is emitted) and `due` (int32 `[B]`: 1 where one was emitted
    on this hop).  `cfg`: the bwe.BweConfig (bwe.bits checks it against `frames`); `order`: the comfort-noise order of the SIDs accepted
    (None: a SID is malformed); `action` (int32 `[B]`, optional): the session row, a start clears the slot."""
    lo, hi = bwe_bits(cfg, frames)
    _OPS.rx_bwe(arrivals, offsets, times, action, rows, caps, due, int(n), int(m), int(frames), -1 if order is None else int(order), lo, hi,
                int(cfg.window), int(cfg.rate_window), int(cfg.alpha_q8), int(cfg.beta_q8), cfg.increase(frames), int(cfg.interval),
                int(cfg.reset_ticks))


def rate_cap(rows: Tensor, rate_rows: Tensor, cfg, min_bits: int, max_bits: int, cap: Optional[Tensor] = None,
             action: Optional[Tensor] = None, hold: Optional[Tensor] = None) -> None:
    """The capped sender's step directly in front of rate_ceiling (bwe.CapModel), in place: `rows` (int32 `[B, bwe.CP_WORDS]`) take this
    hop's `cap` words (int32 `[B]`, bwe.cap_word, 0: none; optional) and RC_RATE_Q8 of `rate_rows` (int32 `[B, rate.RC_WORDS]`) is kept
    at or below the slot's cap.  `cfg`: the bwe.CapConfig; `min_bits` / `max_bits`: the bounds of the sender's rate (its rate.bucket);
    `action` / `hold` (int32 `[B]`, optional): the session rows."""
    _OPS.rate_cap(cap, action, hold, rows, rate_rows, int(min_bits), int(max_bits), int(cfg.timeout_hops))


def srtp_protect(packets: Tensor, nbytes: Tensor, keys: Tensor, rows: Tensor, out: Optional[Tensor] = None,
                 out_nbytes: Optional[Tensor] = None, action: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The protecting sender's step behind packet_header (srtp.SenderModel), outside a graph on any rows and state: `packets` (uint8
    `[B, row_bytes]`) and `nbytes` (int32 `[B]`), read only, under `keys` (int32 `[B, srtp.KEY_WORDS]`, srtp.key_row per slot, zero: no
    key) and the TX `rows` (int32 `[B, srtp.TX_WORDS]`, in place) -> (`out` uint8 `[B, row_bytes + 10]`, `out_nbytes` int32 `[B]`),
    allocated when not given.  `action` (int32 `[B]`, optional): the session row, a start clears the slot's row.  A byte tensor may be
    any contiguous view: rows that are not word-aligned are read and written byte by byte."""
    if packets.dim() != 2:
        raise RuntimeError("srtp_protect: packets must be [B, row_bytes]")
    B, tb = packets.shape
    if out is None:
        out = _new(packets, B, tb + SRTP_TAG_BYTES, dtype=torch.uint8)
    if out_nbytes is None:
        out_nbytes = _new(packets, B, dtype=torch.int32)
    _OPS.srtp_protect(packets, nbytes, keys, rows, action, out, out_nbytes)
    return out, out_nbytes


def srtp_unprotect(arrivals: Tensor, offsets: Tensor, keys: Tensor, rows: Tensor, row_bytes: int, plain: Optional[Tensor] = None,
                   action: Optional[Tensor] = None) -> Tensor:
    """The protected receiver's step in front of its jitter step (srtp.ReceiverModel), outside a graph on any rows and state: one hop's
    protected `arrivals` (int32 `[max_arrivals, 1 + ceil((row_bytes + 10) / 4)]` records grouped by slot) and `offsets` (int32 `[B +
    1]`), read only, under `keys` (int32 `[B, srtp.KEY_WORDS]`) and the RX `rows` (int32 `[B, srtp.RX_WORDS]`, in place) -> `plain`
    (int32 `[max_arrivals, 1 + ceil(row_bytes / 4)]`, zeros when not given): the records jitter_step takes, a rejected arrival as a
    record of 0 bytes; records outside every slot's range are left as they are.  `row_bytes`: wire.transport_bytes(n, m, frames)."""
    if plain is None:
        plain = torch.zeros(arrivals.shape[0], 1 + (int(row_bytes) + 3) // 4, device=arrivals.device, dtype=torch.int32)
    _OPS.srtp_unprotect(arrivals, offsets, keys, rows, action, plain, int(row_bytes))
    return plain


def srtp_protect_routes(rows: Tensor, nbytes: Tensor, routes: Tensor, new_routes: Tensor, keys: Tensor, route_rows: Tensor,
                        out: Optional[Tensor] = None, out_nbytes: Optional[Tensor] = None, action: Optional[Tensor] = None,
                        rekey_up: Optional[Tensor] = None, rekey_down: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The protected forwarder's last step (forward_srtp.RouteModel), outside a graph on any rows and state: a hop's final `rows` (uint8
    `[B, fanout, burst, row_bytes]`) and `nbytes` (int32 `[B, fanout, burst]`) with the `routes` and `new_routes` (int32 `[B, fanout]`)
    of the route launch, read only, under the listeners' downlink `keys` (int32 `[B, srtp.KEY_WORDS]`) and the `route_rows` (int32 `[B,
    fanout, forward_srtp.RT_WORDS]`, in place) -> (`out` uint8 `[B, fanout, burst, row_bytes + 10]`, `out_nbytes` int32 `[B, fanout,
    burst]`), allocated when not given.  `action`, `rekey_up`, `rekey_down` (int32 `[B]`, optional): the slots joined, given an uplink
    key, given a downlink key on this hop; each restarts the routes it touches.  A byte tensor may be any contiguous view: rows that
    are not word-aligned are read and written byte by byte."""
    if rows.dim() != 4:
        raise RuntimeError("srtp_protect_routes: rows must be [B, fanout, burst, row_bytes]")
    B, F, P, tb = rows.shape
    if out is None:
        out = _new(rows, B, F, P, tb + SRTP_TAG_BYTES, dtype=torch.uint8)
    if out_nbytes is None:
        out_nbytes = _new(rows, B, F, P, dtype=torch.int32)
    _OPS.srtp_protect_routes(rows, nbytes, routes, new_routes, action, rekey_up, rekey_down, keys, route_rows, out, out_nbytes)
    return out, out_nbytes


def forward_classify(arrivals: Tensor, offsets: Tensor, rows: Tensor, pick: Tensor, pick_count: Tensor, cfg, n: int, frames: int,
                     m: int = 0, order: Optional[int] = None, action: Optional[Tensor] = None) -> None:
    """The forwarding hop's first launch (forward.SenderModel), in place: one hop's `arrivals` (int32 `[max_arrivals, 1 + ceil(tb / 4)]`
    records grouped by slot, tb = wire.transport_bytes(n, m, frames)) and `offsets` (int32 `[B + 1]`), as GraphedDecodeHop.play stages
    them -> each slot's sender row (`rows`, int32 `[B, forward.SD_WORDS]`), the record indices of its first cfg.burst valid arrivals
    (`pick`, int32 `[B, burst]`, -1 behind `pick_count`, int32 `[B]`).  `cfg`: the forward.ForwardConfig; `order`: the comfort-noise
    order of the SIDs accepted (None: a SID is malformed); `action` (int32 `[B]`, optional): non-zero clears the slot's row."""
    _OPS.forward_classify(arrivals, offsets, action, rows, pick, pick_count, int(n), int(m), int(frames), -1 if order is None else int(order),
                          int(cfg.burst), int(cfg.hang_hops))


def forward_route(arrivals: Tensor, room: Tensor, layers: Tensor, sender_rows: Tensor, pick: Tensor, pick_count: Tensor, routes: Tensor,
                  new_routes: Tensor, rows: Tensor, out: Tensor, out_nbytes: Tensor, cfg, n: int, frames: int, m: int = 0,
                  order: Optional[int] = None, action: Optional[Tensor] = None) -> None:
    """The forwarding hop's second launch (forward.ListenerModel), in place: with `sender_rows`, `pick` and `pick_count` as
    forward_classify left them on this hop, `room` and `layers` (int32 `[B]` each) -> each listener's `routes` (int32 `[B, fanout]`: the
    owners, -1 when free), `new_routes` (1 where a route's owner changed), listener row (`rows`, int32 `[B, forward.LR_WORDS]`) and the
    forwarded packets `out` (uint8 `[B, fanout, burst, tb]`, each cut to the listener's layers: forward.trim_packet) with `out_nbytes`
    (int32 `[B, fanout, burst]`, 0: an empty row).  fanout and burst are read from `out`'s shape; `cfg.keep_fec` decides whether a
    redundant section is kept."""
    _OPS.forward_route(arrivals, action, room, layers, sender_rows, pick, pick_count, routes, new_routes, rows, out, out_nbytes, int(n), int(m),
                       int(frames), -1 if order is None else int(order), bool(cfg.keep_fec))


def downlink_store(arrivals: Tensor, pick: Tensor, pick_count: Tensor, tags: Tensor, ring: Tensor, rows: Tensor, n: int, frames: int,
                   m: int = 0, action: Optional[Tensor] = None) -> None:
    """The forwarding hop's third launch (downlink.DownlinkModel.store), in place: the arrivals that forward_classify picked on this hop
    (`arrivals`, `pick` int32 `[B, burst]`, `pick_count` int32 `[B]`) enter each sender slot's history — `tags` (int32 `[B, history]`),
    `ring` (int32 `[B, history, 1 + ceil(tb / 4)]`: arrival records) — and `rows` (int32 `[B, downlink.DS_WORDS]`) count.  burst and
    history are read from the shapes; `action` (int32 `[B]`, optional): non-zero empties the slot's history."""
    _OPS.downlink_store(arrivals, action, pick, pick_count, tags, ring, rows, int(n), int(m), int(frames))


def downlink_step(routes: Tensor, new_routes: Tensor, packets: Tensor, nbytes: Tensor, layers: Tensor, rows: Tensor, memory: Tensor,
                  eff_layers: Tensor, out: Tensor, out_nbytes: Tensor, cfg, fcfg, n: int, frames: int, m: int = 0,
                  action: Optional[Tensor] = None, report: Optional[Tensor] = None, nack_base: Optional[Tensor] = None,
                  nack_bitmap: Optional[Tensor] = None, tags: Optional[Tensor] = None, ring: Optional[Tensor] = None,
                  rtx_out: Optional[Tensor] = None, rtx_nbytes: Optional[Tensor] = None, rtx_routes: Optional[Tensor] = None) -> None:
    """The forwarding hop's fourth launch (downlink.DownlinkModel.step), in place: with `routes`, `new_routes`, `packets` (uint8 `[B,
    fanout, burst, tb]`) and `nbytes` as forward_route left them on this hop, `layers` (int32 `[B]`) and this hop's feedback (`report`,
    `nack_base`, `nack_bitmap`: int32 `[B, fanout]` each, downlink.feedback_rows; optional) -> each listener's row (`rows`, int32 `[B,
    downlink.DL_WORDS]`), its routes' `memory` (int32 `[B, fanout]`), `eff_layers` (int32 `[B]`), the rows cut to them (`out`,
    `out_nbytes`, the shapes of `packets`, `nbytes`) and, with cfg.history, the retransmissions answered from `tags` and `ring`
    (downlink_store): `rtx_out` (uint8 `[B, per_hop, tb]`), `rtx_nbytes` and `rtx_routes` (int32 `[B, per_hop]`).  `cfg`: the
    downlink.DownlinkConfig (downlink.bucket checks it), `fcfg`: the forward.ForwardConfig."""
    bits = downlink_bucket(cfg, frames, m, packets.shape[1] if packets.dim() == 4 else fcfg.fanout, fcfg.keep_fec)
    if (cfg.history > 0) != (tags is not None):
        raise RuntimeError("downlink_step: tags, ring and the rtx rows are given exactly with cfg.history > 0")
    if tags is not None and (tags.dim() != 2 or tags.shape[1] != cfg.history or rtx_out is None or rtx_out.dim() != 3 or
                             rtx_out.shape[1] != cfg.per_hop):
        raise RuntimeError(f"downlink_step: tags must be [B, {cfg.history}] and rtx_out [B, {cfg.per_hop}, row_bytes]")
    r = cfg.rate
    _OPS.downlink_step(routes, new_routes, packets, nbytes, layers, action, report, nack_base, nack_bitmap, tags, ring, rows, memory,
                       eff_layers, out, out_nbytes, rtx_out, rtx_nbytes, rtx_routes, int(n), int(m), int(frames), bool(fcfg.keep_fec),
                       r is not None, bits.min_bits, bits.max_bits, bits.start_bits, *((int(r.high_q8), int(r.low_q8), int(r.increase_q8),
                       int(r.burst_hops), int(r.timeout_hops)) if r is not None else (0, 0, 0, 1, 0)))


def audio_level(x: Tensor, thr: Tensor, level: Optional[Tensor] = None, hold: Optional[Tensor] = None) -> Tensor:
    """The sender's level launch (audio_level.hop_level): `x` (fp32 `[B, 1, L]` or `[B, L]`, the 24 kHz hop the encoder reads) -> `level`
    (int32 `[B]`, written in place when given, else new): each row's -dBov in 1 dB steps, 0..127.  `thr`: dtx.level_table() on the device
    (float64 `[127]`); `hold` (int32 `[B]`, optional): a non-zero entry gives 127 and its row is not read."""
    if level is None:
        level = _new(x, x.shape[0], dtype=torch.int32)
    _OPS.audio_level(x, thr, hold, level)
    return level


def forward_rank(sender_rows: Tensor, loud: Tensor, room: Tensor, shadow_prev: Tensor, shadow: Tensor, rows: Tensor, cfg, speakers,
                 action: Optional[Tensor] = None) -> None:
    """The forwarding hop's launch between forward_classify and forward_route (audio_level.RankModel): with `sender_rows` (int32 `[B,
    forward.SD_WORDS]`) as forward_classify left them on this hop, the one-hop row `loud` (int32 `[B]`: 128 - level, 0: none;
    audio_level.loud_row), `room` (int32 `[B]`) and `shadow_prev`, the shadow rows of the previous hop -> this hop's `shadow` rows (int32
    `[B, forward.SD_WORDS]`, another tensor than `shadow_prev`: forward_route takes them as its sender_rows) and the speaker rows (`rows`,
    int32 `[B, audio_level.SP_WORDS]`, in place).  `cfg`: the forward.ForwardConfig, `speakers`: the audio_level.SpeakerConfig; `action`
    (int32 `[B]`, optional): non-zero clears the slot's row."""
    _OPS.forward_rank(sender_rows, loud, room, action, shadow_prev, shadow, rows, int(cfg.fanout), int(cfg.hang_hops),
                      int(speakers.floor_level), int(speakers.attack_shift), int(speakers.decay_q8), int(speakers.margin_db))
