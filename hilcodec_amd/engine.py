"""Execution plans for the HILCodec hot path on MI355X.

A *spec* is the folded, device-resident description of one sub-network (encoder / decoder / RVQ):
plain fp32 weights in kernel layouts plus the handful of scalars the reference applies around them.
`run_encoder` / `run_decoder` walk a spec and enqueue the hand-written gfx950 kernels (`ops.py` ->
C ABI) on the current HIP stream; with `caches=None` they compute the offline causal model
(`models/hilcodec/modules/seanet.py:368-378,477-479`), with a cache list they compute one streaming
step with the reference's cache protocol (`models/hilcodec/streaming.py:482-517,619-648`).  Both
behaviours of the reference's two decoders are data in the spec (per-block
`pre_scale`, where wav_std is applied), not code forks.
"""
from __future__ import annotations

import contextlib
import contextvars
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops

# offline path: fuse every pointwise->depthwise pair into one launch (hilc_dws_conv).  The unfused
# kernels remain the streaming path (per-hop tiles are a few samples wide) and a debugging aid.
FUSE_DWS = True
# narrow layers (C <= 192) are HBM-bound unless the whole residual block is one launch (hilc_resblock)
FUSE_UPSAMPLE = True      # decoder up-sampling: transposed conv computed inside the pointwise GEMM's loader
FUSE_RESBLOCK = True
FUSE_STREAM = True        # streaming hops: cache-aware fused kernels instead of pointwise GEMM + depthwise launches
FUSE_RESBLOCK_MAX_C = 192


@dataclass
class ExecOptions:
    """Launch structure of ONE model's encoder or decoder (held by the module, passed to run_encoder / run_decoder): two models
    in one process may run different schedules side by side — nothing here is process-global.  Every setting computes the SAME
    bits (tests pin each against the others); the defaults are the fastest measured.  The arithmetic is the reference's fp32
    throughout: the split-bf16 decoder mode of rounds 2-4 and the launch variants that were measured slower (batched cache
    updates, four-wave C = 256 chains, the 256-column lockstep shape) are gone from the library (round 5; `profiles/r05_experiments.md`).

    stage_launches: a whole stage per launch — its residual blocks back to back per tile and its down-sampling (encoder) /
      up-sampling (decoder) layer as the last / first phase (`hilc_encoder_stage`, `hilc_decoder_stage`, `hilc_resblock_chain`).
      False: one launch per residual block and per layer (round 3's structure).
    wide_blocks: the residual blocks with C >= 256 in the fused kernel (one launch per block or stage); False: two
      depthwise-separable GEMM launches per block with the mid tensor in HBM (round 3's structure).
    decoder_stage_narrow: (with stage_launches) the decoder stages that run ONE long workgroup per CU — C = 192 / 96, and the
      form that holds one block behind the up-sampling phase (offline C = 768) — take their up-sampling layer into the launch
      (C = 96: and the closing conv).  False: up-sampling launch + chain (round 4's structure for those stages; `PipelinedHop`
      captured with it until round 6, when one launch per stage made it the slower choice there too).
    stream_defer_spec: streaming hop: the SpecBlock branches of stages >= 1 computed alone and added by the down-sampling
      epilogue in front (False: in-line, as in round 3)."""
    stage_launches: bool = True
    wide_blocks: bool = True
    decoder_stage_narrow: bool = True
    stream_defer_spec: bool = True


_DEFAULT_OPTIONS = ExecOptions()

# The HIP stream that takes the STFT front halves of the un-fused SpecBlocks while a hop is warmed up / captured
# (graph_step).  A context variable like ops._TIMER / ops._SCHED_WS: it belongs to the schedule being built on THIS thread,
# not to the model — two schedules built concurrently on one model from different threads do not see each other's stream.
_SIDE_STREAM: contextvars.ContextVar = contextvars.ContextVar("hilcodec_side_stream", default=None)


# Per-schedule overrides of a model's ExecOptions (a schedule object that wants another launch structure for ITS capture —
# PipelinedHop — says so here instead of writing into the module's options: context-local, like the side stream)
_OPT_OVERRIDES: contextvars.ContextVar = contextvars.ContextVar("hilcodec_exec_overrides", default=None)


@contextlib.contextmanager
def exec_overrides(**fields):
    token = _OPT_OVERRIDES.set(dict(_OPT_OVERRIDES.get() or {}, **fields))
    try:
        yield
    finally:
        _OPT_OVERRIDES.reset(token)


def _effective(opts: "ExecOptions") -> "ExecOptions":
    over = None if torch.compiler.is_compiling() else _OPT_OVERRIDES.get()
    if not over:
        return opts
    import dataclasses
    return dataclasses.replace(opts, **over)


@contextlib.contextmanager
def spectra_side_stream(stream):
    token = _SIDE_STREAM.set(stream)
    try:
        yield
    finally:
        _SIDE_STREAM.reset(token)


FUSE_SPECBLOCK = True     # long encoder stages (n_fft <= 256): STFT -> log-mag -> 1x1 conv -> += in one launch
STREAM_STAGE0 = True      # streaming hop: first conv + stage-0 SpecBlock as the opening phase of the first stage launch (hilc_encoder_stage0)


@dataclass
class ResBlockSpec:
    pw1_wt: Tensor
    dw1_w: Tensor
    dw1_b: Optional[Tensor]
    pw2_wt: Tensor
    dw2_w: Tensor
    dw2_b: Optional[Tensor]
    pre_scale: float        # (1 + idx*res_scale^2)^-1/2  (seanet.py:84), 1.0 in the streaming decoder
    out_scale: float        # res_scale * res_scale_param (seanet.py:144-148); 1.0 when merged into dw2
    pw1_packed: Optional[Tensor] = None   # MFMA-lane-order copies for the fused block (finalize_spec): C = 64 ... 768
    pw2_packed: Optional[Tensor] = None
    pw1_chain: Optional[Tensor] = None    # the same for a chain launch (streaming plans; another row split below C = 192, else the tensors above)
    pw2_chain: Optional[Tensor] = None

    @property
    def chain_args(self) -> tuple:
        """this block as `ops.resblock_chain` and the stage ops take it"""
        return (self.pw1_chain, self.dw1_w, self.dw1_b, self.pw2_chain, self.dw2_w, self.dw2_b, self.pre_scale, self.out_scale)


@dataclass
class SpecBlockSpec:
    basis_t: Tensor
    n_fft: int
    hop: int
    mean: float
    std: float
    normalize: bool         # False when (y-mean)/std is merged into the layer (streaming.py:321-344)
    wt: Tensor              # [n_fft/2+1, C]
    bias: Optional[Tensor]
    out_scale: float        # res_scale * scale_param; 1.0 when merged
    fused: Optional[tuple] = None   # (dft_packed, nyq_sin, pw_packed) of the one-launch kernel (finalize_spec)


@dataclass
class EncStageSpec:
    spec: SpecBlockSpec
    blocks: List[ResBlockSpec]
    down_in_scale: float    # (1 + n_res*res_scale^2)^-1/2
    down_pw_wt: Tensor
    down_dw_w: Tensor
    down_dw_b: Optional[Tensor]
    ratio: int
    down_lo: Optional[Tensor] = None      # the two column halves of down_pw_wt packed for the one-launch stage (finalize_spec; C = 64 / 128)
    down_hi: Optional[Tensor] = None


@dataclass
class EncoderSpec:
    pre_w: Tensor
    pre_b: Optional[Tensor]
    pre_in_scale: float     # 1/wav_std, or 1.0 when merged into pre_w (streaming.py:472-480)
    stages: List[EncStageSpec]
    spec_post: SpecBlockSpec
    post_dw_w: Tensor
    post_pw_wt: Tensor
    post_pw_b: Optional[Tensor]
    l2norm: bool
    dim: int
    wav_cache_len: int      # n_fft of spec_post - 1


@dataclass
class DecStageSpec:
    in_scale: float         # 1.0 for the first stage, (1 + n_res*res_scale^2)^-1/2 after
    tr_w: Tensor
    ratio: int
    pw_wt: Tensor
    pw_b: Optional[Tensor]
    blocks: List[ResBlockSpec]
    taps: Optional[Tensor] = None         # expanded tap table for strides without a vector tap path (finalize_spec)
    up_lo: Optional[Tensor] = None        # the two row halves of pw_wt packed for the one-launch stage (C = 192 / 96; streaming plans also C = 768)
    up_hi: Optional[Tensor] = None


@dataclass
class DecoderSpec:
    pre_pw_wt: Tensor
    pre_dw_w: Tensor
    pre_dw_b: Optional[Tensor]
    stages: List[DecStageSpec]
    post_in_scale: float
    post_w: Tensor
    post_b: Optional[Tensor]
    post_out_scale: float   # wav_std (offline: scales conv AND bias, seanet.py:464-466); 1.0 if merged into post_w
    tanh: bool


@dataclass
class RvqSpec:
    codebooks: Tensor       # [Nq, K, C]
    codebooks_t: Tensor     # [Nq, C, K]
    norms: Tensor           # [Nq, K]

    @property
    def num_quantizers(self) -> int:
        return self.codebooks.shape[0]


STREAM_WIDE_C = (256, 384, 512, 768)     # the wide blocks (csrc/resblock_kernel.h: NARROW shapes)


def finalize_block(rb: "ResBlockSpec", streaming: bool = False) -> "ResBlockSpec":
    c = rb.pw1_wt.shape[0]
    narrow = c <= FUSE_RESBLOCK_MAX_C and ops.resblock_supported(c, 4)
    if (rb.pw1_packed is None and rb.pw1_wt.device.type in ("cuda", "meta") and rb.pw1_wt.shape[1] == c
            and (narrow or c in STREAM_WIDE_C)):
        rb.pw1_packed = ops.resblock_pack(rb.pw1_wt)
        rb.pw2_packed = ops.resblock_pack(rb.pw2_wt)
    if rb.pw1_packed is not None and rb.pw1_chain is None and (c <= FUSE_RESBLOCK_MAX_C or c in STREAM_WIDE_C):
        same = ops.resblock_chain_row_classes(c, streaming) == (8 if c >= 512 else (4 if c >= 256 else (2 if c == 192 else 1)))     # hilc_resblock_pack_weights' own split
        rb.pw1_chain = rb.pw1_packed if same else ops.resblock_chain_pack(rb.pw1_wt, streaming)
        rb.pw2_chain = rb.pw2_packed if same else ops.resblock_chain_pack(rb.pw2_wt, streaming)
    return rb


def finalize_spec(spec, streaming: bool = False):
    """Device-side, one-off derived tables of an Encoder/DecoderSpec whose tensors already live on the GPU: packed
    pointwise weights of the fused residual blocks, expanded up-sampling taps.  (They used to be hidden caches keyed
    by data_ptr inside the op wrappers; as part of the spec they are plain graph inputs for torch.compile.)"""
    for st in spec.stages:
        sb = getattr(st, "spec", None)
        if (isinstance(sb, SpecBlockSpec) and sb.fused is None and sb.basis_t.device.type in ("cuda", "meta")
                and sb.n_fft in (64, 128, 256) and sb.wt.shape[1] == sb.n_fft):
            sb.fused = ops.spec_block_tables(sb.basis_t, sb.wt, sb.n_fft)
        for rb in st.blocks:
            finalize_block(rb, streaming)
        if (isinstance(st, EncStageSpec) and st.down_lo is None and st.down_pw_wt.device.type in ("cuda", "meta")
                and st.down_pw_wt.shape[0] in (64, 128, 256, 512) and st.down_pw_wt.shape[1] == 2 * st.down_pw_wt.shape[0]
                and all(rb.pw1_chain is not None for rb in st.blocks)):
            c = st.down_pw_wt.shape[0]
            st.down_lo = ops.resblock_chain_pack(st.down_pw_wt[:, :c].contiguous(), streaming)
            st.down_hi = ops.resblock_chain_pack(st.down_pw_wt[:, c:].contiguous(), streaming)
        if isinstance(st, DecStageSpec) and st.tr_w.device.type in ("cuda", "meta"):
            st.taps = ops.up_conv_taps(st.tr_w, st.ratio)
            c = st.pw_wt.shape[1]
            if (st.up_lo is None and st.pw_wt.shape[0] == 2 * c and {768: 8, 384: 5, 192: 4, 96: 2}.get(c, 0) == st.ratio
                    and all(rb.pw1_chain is not None for rb in st.blocks)):
                st.up_lo = ops.resblock_chain_pack(st.pw_wt[:c].contiguous(), streaming)
                st.up_hi = ops.resblock_chain_pack(st.pw_wt[c:].contiguous(), streaming)
    return spec


def spec_to(spec, device):
    """Copy of a spec (any of the dataclasses above, nested) with every tensor moved to `device`."""
    import dataclasses
    if isinstance(spec, Tensor):
        return spec.to(device)
    if isinstance(spec, (list, tuple)):
        return type(spec)(spec_to(v, device) for v in spec)
    if dataclasses.is_dataclass(spec):
        return type(spec)(**{f.name: spec_to(getattr(spec, f.name), device) for f in dataclasses.fields(spec)})
    return spec


def _to(dev, *ts):
    return [None if t is None else t.to(device=dev, dtype=torch.float32).contiguous() for t in ts]


# --------------------------------------------------------------------------------------
# building blocks
# --------------------------------------------------------------------------------------
def _fusable(rb: ResBlockSpec, x: Tensor, streaming: bool = False, wide: Optional[bool] = None) -> bool:
    if wide is None:
        wide = streaming
    return (FUSE_RESBLOCK and rb.pw1_packed is not None and rb.dw1_w.shape[1] == 5 and rb.dw2_w.shape[1] == 5
            and rb.dw1_b is not None and rb.dw2_b is not None
            and (x.shape[1] <= FUSE_RESBLOCK_MAX_C or wide)
            and ops.resblock_supported(x.shape[1], x.shape[2], x.shape[0], streaming))


def _chainable(blocks: Sequence[ResBlockSpec]) -> bool:
    """what every chain / stage kernel assumes of its blocks: weights packed for it, 5-tap depthwise convs with a bias"""
    return all(rb.pw1_chain is not None and rb.dw1_w.shape[1] == 5 and rb.dw2_w.shape[1] == 5 and rb.dw1_b is not None
               and rb.dw2_b is not None for rb in blocks)


class _Caches:
    """The cursor over one streaming step's cache list (order of `encoder_cache_shapes` / `decoder_cache_shapes`): hands out each
    layer's cache with the place of its successor — `caches_out[i]`, or None = a fresh tensor, the reference's protocol — and takes
    back what the op returned, so the new list grows in the order the old one is read.  Offline (`caches` None) it hands out None
    and passes results through: one call site serves both modes."""

    def __init__(self, caches: Optional[Sequence[Tensor]] = None, caches_out: Optional[Sequence[Tensor]] = None, expected: int = 0):
        self.streaming = caches is not None
        self.i = 0                  # caches handed out so far
        self.new: List[Tensor] = []
        self.out = caches_out if self.streaming else None
        if self.streaming:
            for name, seq in (("caches", caches), ("caches_out", self.out)):
                if seq is not None and len(seq) != expected:
                    raise RuntimeError(f"expected {expected} {name}, got {len(seq)}")
            self.caches = [c.contiguous() for c in caches]

    def next(self) -> tuple:
        """(hist, hist_out) of the next layer"""
        if not self.streaming:
            return None, None
        i = self.i
        self.i = i + 1
        return self.caches[i], (None if self.out is None else self.out[i])

    def block(self) -> tuple:
        """(hist, hist_out) of the next residual block: its two depthwise caches"""
        if not self.streaming:
            return None, None
        i = self.i
        self.i = i + 2
        return self.caches[i:i + 2], (None if self.out is None else self.out[i:i + 2])

    def blocks(self, n: int) -> tuple:
        """the same for the next n blocks, as `ops.resblock_chain` and the stage ops take them"""
        if not self.streaming:
            return None, None
        i = self.i
        self.i = i + 2 * n
        return ([self.caches[j:j + 2] for j in range(i, i + 2 * n, 2)],
                None if self.out is None else [self.out[j:j + 2] for j in range(i, i + 2 * n, 2)])

    def take(self, r, layer_first: bool = False):
        """What an op returned -> y.  Streaming it is (y, new cache), (y, [block caches]) or a stage op's (y, [block caches], layer
        cache[, closing conv's cache]); `layer_first`: the layer's cache stands in FRONT of the blocks' in the list (decoder stages).
        The new caches are the successors of everything handed out since the last call, in that order."""
        if not self.streaming:
            return r
        if layer_first:
            self.new.append(r[2])
            self.new.extend(r[1])
            self.new.extend(r[3:])
        elif isinstance(r[1], Tensor):
            self.new.append(r[1])
        else:
            self.new.extend(r[1])
            self.new.extend(r[2:])
        if len(self.new) != self.i:
            raise RuntimeError(f"internal error: {len(self.new)} new caches kept after cache {self.i - 1} was handed out")
        return r[0]

    def done(self, y):
        """y offline, (y, new caches) streaming"""
        if not self.streaming:
            return y
        if self.i != len(self.caches):
            raise RuntimeError(f"internal error: the step read {self.i} of {len(self.caches)} caches")
        if self.out is not None:
            for i in range(self.i):
                if self.new[i] is not self.out[i]:
                    raise RuntimeError(f"internal error: new cache {i} is not caches_out[{i}]")
        return y, self.new


# the argument tuples of the stage ops (`ops.encoder_stage0`, `ops.encoder_stage`, `ops.decoder_stage`, `ops.decoder_stage_post`)
def _spec0_args(es: "EncoderSpec") -> tuple:
    sb = es.stages[0].spec
    return (sb.fused[0], sb.fused[1], sb.fused[2], sb.bias, es.pre_w, es.pre_b, es.pre_in_scale, sb.mean, sb.std, sb.normalize, sb.out_scale)


def _down_args(st: "EncStageSpec") -> tuple:
    return (st.down_lo, st.down_hi, st.down_dw_w, st.down_dw_b, st.down_in_scale, st.ratio)


def _up_args(st: "DecStageSpec") -> tuple:
    return (st.tr_w if st.taps is None else st.taps, st.up_lo, st.up_hi, st.pw_b, st.in_scale, st.ratio)


def _post_args(ds: "DecoderSpec") -> tuple:
    return (ds.post_w, ds.post_b, ds.post_in_scale, ds.post_out_scale, ds.tanh)


def _dws_layer(cur: _Caches, fused: bool, x: Tensor, pw_wt: Tensor, dw_w: Tensor, dw_b: Optional[Tensor], res=None, stride: int = 1,
               in_scale: float = 1.0, in_elu: bool = False, out_scale: float = 1.0, out_elu: bool = False) -> Tensor:
    """Pointwise conv -> causal depthwise conv (with the next cache of `cur`, streaming).  `fused`: one launch, the pointwise outputs
    never leave LDS (a hop: whole-clip tiles, the cache read and written in the epilogue); else pointwise GEMM + depthwise launch.
    `res` is added to the output; a function in its place is called where the tensor is needed, behind the pointwise launch."""
    hist, hist_out = cur.next()
    if fused:
        res = res() if callable(res) else res
        if cur.streaming:
            return cur.take(ops.dws_conv_stream(x, pw_wt, dw_w, dw_b, hist, res=res, stride=stride, in_scale=in_scale, in_elu=in_elu,
                                                out_scale=out_scale, out_elu=out_elu, hist_out=hist_out))
        return ops.dws_conv(x, pw_wt, dw_w, dw_b, res=res, stride=stride, in_scale=in_scale, in_elu=in_elu, out_scale=out_scale, out_elu=out_elu)
    h = ops.pw_conv(x, pw_wt, in_scale=in_scale, in_elu=in_elu)
    return cur.take(ops.dw_conv(h, dw_w, dw_b, res=res() if callable(res) else res, stride=stride, hist=hist, want_hist=cur.streaming,
                                out_scale=out_scale, out_elu=out_elu, hist_out=hist_out))


def _up_layer(cur: _Caches, st: "DecStageSpec", x: Tensor) -> Tensor:
    """A decoder stage's up-sampling layer as a launch of its own: [Scale, ELU, depthwise transposed conv, pointwise conv + bias]"""
    hist, hist_out = cur.next()
    if (FUSE_STREAM if cur.streaming else FUSE_UPSAMPLE) and (x.shape[2] * st.ratio) % 4 == 0:
        # the up-sampled tensor only exists inside the GEMM's loader
        return cur.take(ops.up_conv(x, st.tr_w, st.pw_wt, st.pw_b, st.ratio, in_scale=st.in_scale, in_elu=True, hist=hist,
                                    want_hist=cur.streaming, taps=st.taps, hist_out=hist_out))
    u = cur.take(ops.dw_convtr(x, st.tr_w, st.ratio, hist=hist, want_hist=cur.streaming, in_scale=st.in_scale, in_elu=True, hist_out=hist_out))
    return ops.pw_conv(u, st.pw_wt, st.pw_b)


def _resblock(rb: ResBlockSpec, x: Tensor, cur: _Caches, opts: ExecOptions = _DEFAULT_OPTIONS) -> Tensor:
    """One residual block; streaming: with the next two caches of `cur`."""
    k1, k2 = rb.dw1_w.shape[1], rb.dw2_w.shape[1]
    if (not cur.streaming or x.shape[2] >= 4) and _fusable(rb, x, cur.streaming, opts.wide_blocks):
        # one launch per block: x is read once, y written once, everything else stays in LDS.  A streaming hop: same kernel, the two
        # depthwise caches patch the first tile's halo columns; the wide blocks of a hop (C = 256 ... 768) take its narrow-tile shapes
        hist, hist_out = cur.block()
        return cur.take(ops.resblock(x, rb.pw1_packed, rb.dw1_w, rb.dw1_b, rb.pw2_packed, rb.dw2_w, rb.dw2_b, rb.pre_scale, rb.out_scale,
                                     hist=hist, hist_out=hist_out))
    if cur.streaming:       # wide layers of a streaming hop (T <= 128)
        fused = FUSE_STREAM and ops.dws_conv_stream_profitable(x.shape[2], k1, 1) and ops.dws_conv_stream_profitable(x.shape[2], k2, 1)
    else:
        fused = FUSE_DWS and k1 == 5 and k2 == 5
    # two layers: [ELU, pw, dw] and [pw, dw, *scale + shortcut]; the ELU between them in the epilogue of a fused first launch, else in
    # the second pointwise GEMM's loader
    g = _dws_layer(cur, fused, x, rb.pw1_wt, rb.dw1_w, rb.dw1_b, in_scale=rb.pre_scale, in_elu=True, out_elu=fused)
    return _dws_layer(cur, fused, g, rb.pw2_wt, rb.dw2_w, rb.dw2_b, res=x, in_elu=not fused, out_scale=rb.out_scale)


def _stage_blocks(blocks: Sequence[ResBlockSpec], x: Tensor, cur: _Caches, opts: ExecOptions) -> Tensor:
    """The residual blocks of one stage: ONE chain launch where the kernel exists (the blocks run back to back per tile, the
    activations between them stay in registers: `ops.resblock_chain`); otherwise block by block."""
    n = len(blocks)
    chain = FUSE_RESBLOCK and opts.stage_launches and n >= 2
    if cur.streaming:
        chain = (chain and FUSE_STREAM and x.shape[2] >= 4 and _chainable(blocks) and (x.shape[1] <= FUSE_RESBLOCK_MAX_C or opts.wide_blocks)
                 and ops.resblock_chain_supported(x.shape[1], x.shape[2], n, x.shape[0]))
    else:
        chain = (chain and all(rb.pw1_chain is not None and _fusable(rb, x, False, opts.wide_blocks) for rb in blocks)
                 and ops.resblock_chain_supported(x.shape[1], x.shape[2], n, x.shape[0], streaming=False))
    if chain:
        hist, hist_out = cur.blocks(n)
        return cur.take(ops.resblock_chain(x, [rb.chain_args for rb in blocks], hist, hist_out))
    for rb in blocks:
        x = _resblock(rb, x, cur, opts)
    return x


def _stage_fusable_blocks(st: "DecStageSpec", x: Tensor, streaming: bool, partial: bool = True) -> int:
    """How many of a decoder stage's residual blocks run in ONE launch with its up-sampling layer (`ops.decoder_stage`): all of them, the
    first one (where LDS holds the carry slots / the halo form of one block only), or 0 = no stage launch for this shape."""
    if st.up_lo is None or st.pw_b is None or not st.blocks:
        return 0
    if not _chainable(st.blocks):
        return 0
    c, t = st.pw_wt.shape[1], x.shape[2] * st.ratio
    for nb in ((len(st.blocks), 1) if partial else (len(st.blocks),)):
        if ops.decoder_stage_supported(c, t, nb, st.ratio, x.shape[0], streaming=streaming):
            return nb
    return 0


def _pre_fusable(es: "EncoderSpec", wav: Tensor, wav_hist: Optional[Tensor]) -> bool:
    """the first conv and the stage-0 SpecBlock in one launch (`ops.spec_block_conv_pre`, or as the opening phase of `ops.encoder_stage0`)"""
    sb0 = es.stages[0].spec
    return bool(FUSE_SPECBLOCK and sb0.fused is not None and sb0.n_fft == 64 and sb0.hop == 1
                and es.pre_w.shape == (64, 5) and ops.spec_block_supported(64, 1, 64, wav.shape[2])
                and (wav_hist is None or wav_hist.shape[-1] >= 63))


def _stage_launchable(st: "EncStageSpec", t: int, streaming: bool, opts: ExecOptions) -> bool:
    """what both one-launch forms of an encoder stage ask of the schedule and of the spec, at t samples per clip / stream"""
    return (FUSE_RESBLOCK and opts.stage_launches and (not streaming or FUSE_STREAM) and st.down_lo is not None and st.down_dw_b is not None
            and st.down_dw_w.shape[1] == 2 * st.ratio and t % st.ratio == 0 and _chainable(st.blocks))


def _stage0_fusable(es: "EncoderSpec", wav: Tensor, streaming: bool, opts: ExecOptions) -> bool:
    """(where `_pre_fusable`) the whole first stage behind the first conv and its SpecBlock: `ops.encoder_stage0`"""
    st0 = es.stages[0]
    return bool((not streaming or STREAM_STAGE0) and _stage_launchable(st0, wav.shape[2], streaming, opts)
                and ops.encoder_stage0_supported(wav.shape[2], len(st0.blocks), st0.ratio, 64, 1, es.pre_w.shape[1], wav.shape[0], streaming))


def _enc_stage_fusable(st: "EncStageSpec", x: Tensor, streaming: bool, opts: ExecOptions) -> bool:
    """an encoder stage, residual blocks and down-sampling layer, as one launch: `ops.encoder_stage`"""
    return bool(_stage_launchable(st, x.shape[2], streaming, opts) and (x.shape[1] <= FUSE_RESBLOCK_MAX_C or opts.wide_blocks)
                and ops.encoder_stage_supported(x.shape[1], x.shape[2], len(st.blocks), st.ratio, x.shape[0], streaming))


def _spec_fused(sb: SpecBlockSpec, wav: Tensor, wav_hist: Optional[Tensor]) -> bool:
    return bool(FUSE_SPECBLOCK and sb.fused is not None and (wav_hist is None or wav_hist.shape[-1] >= sb.n_fft - 1)
                and ops.spec_block_profitable(sb.n_fft, sb.hop, sb.wt.shape[1], wav.shape[2]))


def _spec_block(sb: SpecBlockSpec, x: Optional[Tensor], wav: Tensor, wav_hist: Optional[Tensor]) -> Tensor:
    """x + out_scale * (W logspec(wav) + bias) `[B, C, T_f]` (`seanet.py:220-246`; streaming, merged: `streaming.py:346-366`); x None:
    the branch ALONE — what `x.add_()` adds.  It depends on the waveform only."""
    if _spec_fused(sb, wav, wav_hist):
        return ops.spec_block(wav, sb.fused[0], sb.fused[1], sb.fused[2], sb.bias, x, sb.n_fft, sb.hop, sb.mean, sb.std,
                              sb.normalize, sb.out_scale, hist=wav_hist)
    s = ops.stft_logmag(wav, sb.basis_t, sb.n_fft, sb.hop, sb.mean, sb.std, sb.normalize, hist=wav_hist)
    return ops.pw_conv(s, sb.wt, sb.bias, res=x, out_scale=sb.out_scale)


def _early_branches(todo: Sequence[SpecBlockSpec], wav: Tensor, wav_hist: Optional[Tensor], side) -> Optional[dict]:
    """Streaming hop inside a captured graph: the SpecBlock branches of the later stages depend on the waveform only, so they
    are computed on `side` (`spectra_side_stream`) beside the first encoder stages (their launches fill idle CUs instead of
    standing in the chain); the consumer waits for each one's event.  Same launches, same results."""
    if side is None or torch.compiler.is_compiling() or not wav.is_cuda or not todo:
        return None
    main = torch.cuda.current_stream(wav.device)
    capturing = torch.cuda.is_current_stream_capturing()
    early = {}
    side.wait_stream(main)
    with torch.cuda.stream(side):
        for sb in todo:
            r = _spec_block(sb, None, wav, wav_hist)
            if not capturing:
                r.record_stream(main)
            done = torch.cuda.Event()
            done.record(side)
            early[id(sb)] = (r, done)
    return early


# The linear-addressing GEMM cores address an activation tensor with 32-bit byte offsets (csrc/gemm_epilogues.h: lin_ok): with an
# x of 4 GiB or more hilc_pw_conv / hilc_dws_conv / hilc_up_conv silently take the generic core (10-20 % slower, same bits).  Clips
# are independent and results batch-invariant bit for bit (tests/test_gpu_fullsize.py), so an offline batch whose LARGEST activation
# would reach the limit is run as equal clip chunks that each stay below it.  The fused OFFLINE block, chain and stage launches have no
# such limit (64-bit offsets; only their streaming forms refuse 4 GiB), so a single clip above it — which cannot be chunked — still
# runs them; a mono clip of 466 s has its 4 GiB tensors only inside and between the last two decoder stage launches, a launch outside
# them that met one would take the generic core (DESIGN.md "Large tensors", tests/test_gpu_large.py).
OFFSET_LIMIT_BYTES = 1 << 32


def _clip_chunks(batch: int, per_clip_elems: int) -> List[Tuple[int, int]]:
    """[(lo, hi)] — one range if the whole batch fits 32-bit byte offsets, else the fewest equal chunks that do"""
    most = max(1, (OFFSET_LIMIT_BYTES - 1) // (4 * max(1, per_clip_elems)))
    if batch <= most:
        return [(0, batch)]
    n = -(-batch // most)
    size = -(-batch // n)
    return [(lo, min(batch, lo + size)) for lo in range(0, batch, size)]


def _encoder_clip_elems(es: "EncoderSpec", T: int) -> int:
    """largest [C, T_s] activation of one clip that a launch of the offline encoder reads or writes"""
    best, t = es.pre_w.shape[0] * T, T
    for st in es.stages:
        best = max(best, st.down_pw_wt.shape[0] * t)
        t = -(-t // st.ratio)
        best = max(best, st.down_dw_w.shape[0] * t)
    return best


def _decoder_clip_elems(ds: "DecoderSpec", F: int) -> int:
    best, t = ds.pre_dw_w.shape[0] * F, F
    for st in ds.stages:
        best = max(best, st.tr_w.shape[0] * t)
        t *= st.ratio
        best = max(best, st.pw_wt.shape[1] * t)
    return best


def _cache_count(spec) -> int:
    """len(encoder_cache_shapes(spec)) or len(decoder_cache_shapes(spec)) without reading a shape (every hop asks): one cache in front,
    one behind, and per stage its layer's and two per residual block"""
    return 2 + sum(1 + 2 * len(st.blocks) for st in spec.stages)


def _begin(x: Tensor, opts: ExecOptions, offline: bool, clip_elems, spec) -> tuple:
    """how run_encoder and run_decoder open: (contiguous fp32 input, the options in force, the clip ranges of an offline batch that
    has to run in chunks — else None)"""
    x = x.contiguous().float()
    chunks = None
    if offline and not torch.compiler.is_compiling():
        chunks = _clip_chunks(x.shape[0], clip_elems(spec, x.shape[2]))
    return x, _effective(opts), (chunks if chunks is not None and len(chunks) > 1 else None)


def run_encoder(es: EncoderSpec, wav: Tensor, caches: Optional[Sequence[Tensor]] = None,
                channel_last_out: bool = False, caches_out: Optional[Sequence[Tensor]] = None,
                opts: ExecOptions = _DEFAULT_OPTIONS):
    """wav `[B,1,T]` -> z `[B,dim,ceil(T/hop)]` (or `[B,T',dim]`), and the new cache list if streaming.
    `caches_out` (streaming, optional): persistent buffers, same shapes as `caches` and distinct from them, that
    receive the next hop's caches (ping-pong state block); without it every cache is a fresh tensor, which is the
    reference's protocol (`streaming.py:482-517`: cache_out never aliases cache_in)."""
    if wav.dim() != 3 or wav.shape[1] != 1:
        raise RuntimeError(f"expected [B,1,T] waveform, got {tuple(wav.shape)}")
    wav, opts, chunks = _begin(wav, opts, caches is None, _encoder_clip_elems, es)
    if chunks:
        return torch.cat([run_encoder(es, wav[lo:hi], None, channel_last_out, None, opts) for lo, hi in chunks], dim=0)
    cur = _Caches(caches, caches_out, _cache_count(es))
    streaming = cur.streaming
    wav_hist, tail_out = cur.next()
    if streaming:
        cur.take((None, ops.tail(wav, wav_hist, es.wav_cache_len, out=tail_out)))
    sb0 = es.stages[0].spec
    fuse_pre = _pre_fusable(es, wav, wav_hist)
    fuse_stage0 = fuse_pre and _stage0_fusable(es, wav, streaming, opts)
    if fuse_stage0:
        x = None      # first conv + first SpecBlock + the whole first stage in one launch: the first turn of the stage loop below
    elif fuse_pre:
        # first conv + first SpecBlock in one launch: the [64 x T] tensor between them never exists
        x = ops.spec_block_conv_pre(wav, sb0.fused[0], sb0.fused[1], sb0.fused[2], sb0.bias, es.pre_w, es.pre_b,
                                    es.pre_in_scale, 64, 1, sb0.mean, sb0.std, sb0.normalize, sb0.out_scale, hist=wav_hist)
    else:
        x = ops.conv_pre(wav, es.pre_w, es.pre_b, in_scale=es.pre_in_scale, hist=wav_hist)
    # Streaming hop: the SpecBlock branch of stage s + 1 (and spec_post's) is `x.add_(branch)` right after stage s's
    # down-sampling layer (`streaming.py:497-511`), and the branch depends on the waveform only.  It is computed on its own —
    # inside a captured graph beside the earlier stages, on the side stream — and ADDED BY THE DOWN-SAMPLING LAYER'S EPILOGUE
    # (`res`): one launch and one read + write of x less per stage on the critical path, the same two roundings in the same
    # order (`fadd(down, branch)`), bit-identical to the in-line form.
    later = [st.spec for st in es.stages[1:]] + [es.spec_post]
    # (offline the same deferral was measured in round 5: 73.8 -> 75.2 ms per step, same box — the branch-only launches write what the
    #  in-line ones read-modify-write, and the stage launches gain a `res` read: kept in-line)
    defer = streaming and FUSE_STREAM and opts.stream_defer_spec
    side = None if torch.compiler.is_compiling() else _SIDE_STREAM.get()          # (a tracing compiler cannot read a ContextVar; it never forks streams)
    early = _early_branches(later, wav, wav_hist, side) if defer else None

    def branch_of(sb):
        if early is not None and id(sb) in early:
            r, done = early[id(sb)]
            torch.cuda.current_stream(wav.device).wait_event(done)
            return r
        return _spec_block(sb, None, wav, wav_hist)

    for si, st in enumerate(es.stages):
        stage0 = fuse_stage0 and si == 0
        if not (fuse_pre and si == 0) and not (defer and si > 0):
            x = _spec_block(st.spec, x, wav, wav_hist)
        nxt = later[si]
        if stage0 or _enc_stage_fusable(st, x, streaming, opts):
            # the whole stage — its residual blocks and its down-sampling layer — is one launch; the stage's output never reaches HBM.
            # Stage 0 with the first conv and its SpecBlock in front (offline: seanet.py:368-378; a hop: streaming.py:490-511, with the
            # waveform cache in front of every stream's t = 0): neither the [64 x T] tensor in front of the stage nor the one behind its
            # blocks ever exists.  A hop launches it here, not above, so that the side branches have been forked by now.
            blocks, down = [rb.chain_args for rb in st.blocks], _down_args(st)
            res = branch_of(nxt) if defer else None
            hist, hist_out = cur.blocks(len(st.blocks))
            down_hist, down_hist_out = cur.next()
            state = dict(res=res, hist=hist, hist_out=hist_out, down_hist=down_hist, down_hist_out=down_hist_out)
            if stage0:
                x = cur.take(ops.encoder_stage0(wav, _spec0_args(es), blocks, down, wav_hist=wav_hist, **state))
            else:
                x = cur.take(ops.encoder_stage(x, blocks, down, **state))
            continue
        x = _stage_blocks(st.blocks, x, cur, opts)
        k = st.down_dw_w.shape[1]
        # (a shortcut the fused layer cannot take — a long hop at a stride above 8 — or a long hop whose x reaches 4 GiB falls through to pointwise GEMM + depthwise conv)
        if streaming:
            fused = FUSE_STREAM and ops.dws_conv_stream_profitable(x.shape[2], k, st.ratio, defer, x.shape[0], st.down_dw_w.shape[0], x.shape[1])
        else:
            fused = FUSE_DWS and k == 2 * st.ratio
        x = _dws_layer(cur, fused, x, st.down_pw_wt, st.down_dw_w, st.down_dw_b, res=(lambda: branch_of(nxt)) if defer else None,
                       stride=st.ratio, in_scale=st.down_in_scale, in_elu=True)
    if not defer:
        x = _spec_block(es.spec_post, x, wav, wav_hist)
    hist, hist_out = cur.next()
    h = cur.take(ops.dw_conv(x, es.post_dw_w, None, in_elu=True, hist=hist, want_hist=streaming, hist_out=hist_out))
    h = ops.pw_conv(h, es.post_pw_wt, es.post_pw_b)
    if es.l2norm:
        z = ops.l2norm(h, eps=1e-12, scale=float(es.dim) ** 0.5, channel_last_out=channel_last_out)
    else:
        z = h.transpose(1, 2).contiguous() if channel_last_out else h
    return cur.done(z)


def run_decoder(ds: DecoderSpec, q: Tensor, caches: Optional[Sequence[Tensor]] = None,
                caches_out: Optional[Sequence[Tensor]] = None, opts: ExecOptions = _DEFAULT_OPTIONS):
    """q `[B,dim,F]` (channel-major) -> wav `[B,1,F*hop]`, and the new cache list if streaming (`caches_out` as in
    run_encoder)."""
    q, opts, chunks = _begin(q, opts, caches is None, _decoder_clip_elems, ds)
    if chunks:
        return torch.cat([run_decoder(ds, q[lo:hi], None, None, opts) for lo, hi in chunks], dim=0)
    cur = _Caches(caches, caches_out, _cache_count(ds))
    streaming = cur.streaming
    k = ds.pre_dw_w.shape[1]
    if streaming:
        fused = FUSE_STREAM and ops.dws_conv_stream_profitable(q.shape[2], k, 1)
    else:
        fused = FUSE_DWS and k == 5
    x = _dws_layer(cur, fused, q, ds.pre_pw_wt, ds.pre_dw_w, ds.pre_dw_b)
    for st in ds.stages:
        width, t = st.pw_wt.shape[1], x.shape[2] * st.ratio
        nb = 0
        if ((FUSE_STREAM if streaming else FUSE_UPSAMPLE) and FUSE_RESBLOCK and opts.stage_launches
                and (opts.decoder_stage_narrow if width <= FUSE_RESBLOCK_MAX_C else opts.wide_blocks)):
            nb = _stage_fusable_blocks(st, x, streaming, opts.decoder_stage_narrow)
        if nb == 0:
            x = _stage_blocks(st.blocks, _up_layer(cur, st, x), cur, opts)
            continue
        # the stage — up-sampling layer and residual blocks — is one launch; the tensor between them never exists.  Where LDS holds
        # one block only behind the up-sampling phase (a hop's C = 384, the offline model's C = 768) the other blocks follow as
        # launches of their own.
        up, blocks = _up_args(st), [rb.chain_args for rb in st.blocks[:nb]]
        up_hist, up_hist_out = cur.next()
        hist, hist_out = cur.blocks(nb)
        if (st is ds.stages[-1] and nb == len(st.blocks) and ds.post_w.dim() == 2 and ds.post_w.shape[0] == width
                and ops.decoder_stage_post_supported(width, t, nb, st.ratio, ds.post_w.shape[1])):
            # the LAST stage and the closing conv (seanet.py:453-476, streaming.py:639-648) in one launch: the stage's [B, C, T] output
            # — the step's largest tensor — is neither written nor read; a hop reads the conv's cache at a stream's t = 0 and
            # writes it from its last column group
            post_hist, post_hist_out = cur.next()
            return cur.done(cur.take(ops.decoder_stage_post(x, up, blocks, _post_args(ds), hist, up_hist, post_hist, hist_out, up_hist_out,
                                                            post_hist_out), layer_first=True))
        x = cur.take(ops.decoder_stage(x, up, blocks, hist, up_hist, hist_out, up_hist_out), layer_first=True)
        if nb < len(st.blocks):
            x = _stage_blocks(st.blocks[nb:], x, cur, opts)
    hist, hist_out = cur.next()
    return cur.done(cur.take(ops.conv_post(x, ds.post_w, ds.post_b, in_scale=ds.post_in_scale, in_elu=True, out_scale=ds.post_out_scale,
                                           do_tanh=ds.tanh, hist=hist, want_hist=streaming, hist_out=hist_out)))


def encoder_cache_shapes(es: EncoderSpec) -> List[Tuple[int, int]]:
    """(channels, length) per cache, order of `Encoder.initialize_cache` (streaming.py:458-470)."""
    out = [(1, es.wav_cache_len)]
    for st in es.stages:
        for rb in st.blocks:
            c = rb.dw1_w.shape[0]
            out += [(c, rb.dw1_w.shape[1] - 1), (c, rb.dw2_w.shape[1] - 1)]
        out.append((st.down_dw_w.shape[0], st.down_dw_w.shape[1] - st.ratio))
    out.append((es.post_dw_w.shape[0], es.post_dw_w.shape[1] - 1))
    return out


def decoder_cache_shapes(ds: DecoderSpec) -> List[Tuple[int, int]]:
    """Order of `Decoder.initialize_cache` (streaming.py:599-607)."""
    out = [(ds.pre_dw_w.shape[0], ds.pre_dw_w.shape[1] - 1)]
    for st in ds.stages:
        out.append((st.tr_w.shape[0], 1))
        for rb in st.blocks:
            c = rb.dw1_w.shape[0]
            out += [(c, rb.dw1_w.shape[1] - 1), (c, rb.dw2_w.shape[1] - 1)]
    out.append((ds.post_w.shape[0], ds.post_w.shape[1] - 1))
    return out
