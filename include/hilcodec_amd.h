/* hilcodec_amd.h — C ABI of the MI355X-native HILCodec encode -> RVQ -> decode hot path.
 *
 * The reference (aask1357/hilcodec) is pure Python/PyTorch and has NO FFI: its hot path sits behind
 * nn.Module classes and bottoms out in ATen calls.  This header therefore declares the entry points
 * a binding of that path would need: one per arithmetic step of the folded graph (SURVEY.md
 * Appendix A).  Each entry cites the reference code it replaces (paths relative to the reference
 * checkout).  INTEGRATION.md shows the ctypes stub that binds them from the reference's modules.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's allocator in this repo);
 *    the library allocates nothing, keeps no mutable global state (only a per-device cache of immutable
 *    occupancy facts), and is re-entrant;
 *  - tensors are dense fp32, channel-major `[B][C][T]` (time contiguous) unless stated;
 *  - `stream` is a `hipStream_t` passed as `void*`; all work is enqueued on it, nothing syncs;
 *  - return value: HILC_OK (0) or a negative HILC_ERR_* code; nothing is launched on error;
 *  - "hist" arguments are the streaming caches of `models/hilcodec/causal_layers.py:147-188`
 *    (the samples *before* t = 0 of the layer's input); NULL means zero history, which is the
 *    causal zero padding of the offline model (`models/hilcodec/modules/conv.py:222-236`).
 *  - alignment: a float operand needs the 4 bytes of a float unless its entry says otherwise.  Where an entry names operands that
 *    "must be 16-byte aligned for the fast path", a 4-byte-aligned view of one switches the launch to a path that reads and writes
 *    it word by word, with the same results bit for bit (the one exception is stated at hilc_conv_post); where it names operands
 *    that are "refused", a pointer that is not 16-byte aligned returns HILC_ERR_UNSUPPORTED in front of the first launch.  The
 *    table of every (entry, operand) pair is DESIGN.md, "Pointer alignment".
 *  - size: an entry's "Size:" line says what it does with an activation tensor of 4 GiB or more (byte offsets that no longer fit 32 bits):
 *    the same kernel, another core with the same results bit for bit, or HILC_ERR_UNSUPPORTED in front of the first launch with nothing
 *    written.  Dimensions themselves are ints: B, C, T and T * stride stay below 2^31.  DESIGN.md, "Large tensors".
 *  - prologue  pro(v) = in_elu ? ELU(v * in_scale) : v * in_scale   (Scale + ELU modules,
 *    `models/hilcodec/modules/seanet.py:165-178`, torch.nn.ELU(alpha=1));
 *    it is applied to `x` only — histories hold already-activated samples, as the reference's
 *    caches do.
 */
#ifndef HILCODEC_AMD_H
#define HILCODEC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HILC_OK 0
#define HILC_ERR_SHAPE (-1)       /* a dimension is <= 0 or inconsistent            */
#define HILC_ERR_NULL (-2)        /* a required pointer is NULL                     */
#define HILC_ERR_LAUNCH (-3)      /* hipGetLastError() != hipSuccess after launch   */
#define HILC_ERR_UNSUPPORTED (-4) /* configuration outside what the kernels cover   */
#define HILC_ERR_RANGE (-5)       /* n outside 1..Nq (reference: AssertionError)    */

#define HILC_ABI_VERSION 16   /* 2: packed residual-block weights; 3: hilc_spec_block; 4: hilc_spec_block_conv_pre; 5: waveform history in both; 6-7: *_x3 (experimental; REMOVED in 14); 8: hilc_dws_conv_wave_row; 9: hilc_resblock_stream_supported (wide blocks in hilc_resblock_stream); 10: hilc_resblock_chain; 11: hilc_encoder_stage; 12: batched cache updates (REMOVED in 14); 13: hilc_decoder_stage; 14: the entry points that only served rejected experiments are gone (split-bf16 decoder GEMMs, batched cache updates); hilc_decoder_stage_post, hilc_encoder_stage0; 15: hilc_rvq_encode[_mixed] take `flags` (HILC_RVQ_VALU_ONLY replaces the HILC_RVQ_VALU environment variable); 16: per-stream sessions of a graphed hop, two new entry points — int hilc_state_slots_apply(float* block, const int64_t* slice_off, const int* slice_len, int nslices, int streams, const int* action, const float* records, int nrecords, void* stream) and int hilc_state_slots_gather(const float* block, const int64_t* slice_off, const int* slice_len, int nslices, int streams, const int* slots, int nslots, float* records, void* stream); no struct changes; additive under 16 (no version bump): hilc_state_slots_hold, hilc_pack_codes_10bit, hilc_rvq_decode_packed, and the receiver's loss concealment int hilc_conceal_prepare(int* state, const int* action, int* hold, const int* lost, int* n_per_stream, uint8_t* packets, int* ramp, int B, int T, int n_max, int fade_hops, void* stream) and int hilc_conceal_gain(float* wav, const int* ramp, const float* gains, const float* weights, int B, int samples, int fade_hops, void* stream); and the polyphase sample-rate converter int hilc_resample_poly(const float* x, const float* hist_in, float* hist_out, float* y, const float* taps, int B, int T_in, int L, int M, int Q, void* stream); and in-band forward error correction int hilc_pack_codes_10bit_fec(const int64_t* indices, const int* n_per_stream, const int* prev_in, int* prev_out, const int* action, const int* hold, uint8_t* packets, int* nbytes, int B, int T, int n_max, int m, void* stream) and int hilc_fec_select(const uint8_t* packets, const int* fec, int* n_per_stream, uint8_t* out, int B, int T, int n_max, int m, void* stream); and discontinuous transmission with comfort noise int hilc_dtx_encode(const float* x, const int* action, const int* hold, int* run, int* kind, uint8_t* packets, int* nbytes, int64_t* indices, int* prev, const double* level_thr, double thr_vad, int B, int T, int order, int hangover, int sid_interval, int n_max, int stride, int prev_words, void* stream) and int hilc_cng_synth(const uint8_t* packets, const int* action, int* hold, int* state, float* wav, int* restore, const float* gains, int B, int T, int order, int stride, void* stream); and the transport header and jitter buffer int hilc_packet_header(const uint8_t* packets, const int* nbytes, const int* n_per_stream, const int* kind, const int* action, const int* hold, const int* counter_in, int* counter_out, uint8_t* out, int* out_nbytes, int B, int T, int n_max, int m, void* stream) and int hilc_jitter_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold, int* n_per_stream, int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B, int T, int n_max, int m, int order, int conceal, int depth, int capacity, void* stream) with its adaptive form int hilc_jitter_adapt_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold, int* n_per_stream, int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B, int T, int n_max, int m, int order, int conceal, int depth, int capacity, int* adapt, int headroom, int max_late, int window, int resync, int force_windows, void* stream); and per-room mixing of the receiver's output int hilc_mix_levels(const float* wav, double* score, const int* action, int B, int L, void* stream) and int hilc_mix_rooms(const float* wav, const int* room, const double* score, int top_k, float* mixed, int* speakers, int B, int L, void* stream) with per-speaker levelling and a limiter int hilc_mix_gains(const float* wav, double* gains, double* power, const int* action, double gate2, double lo, double hi, double up, double down, double min_gain, double max_gain, double smooth, int B, int L, void* stream) and int hilc_mix_rooms_dyn(const float* wav, const int* room, const double* score, int top_k, const double* gains, double* limiter, double ceiling, double release, int sub, const int* action, float* mixed, int* speakers, int B, int L, void* stream); and quality-targeted variable bitrate of the sender int hilc_vbr_select(const float* z, int64_t* indices, const float* codebooks, const int* n_per_stream, const int* action, const int* hold, int* credit, int* n_eff, double* distortion, int B, int T, int C, int K, int Nq, int n, int n_lo, double rho, int stage_bits, int rate_bits, int burst_bits, void* stream); and receiver reports with loss-adaptive FEC int hilc_rx_report(const int* jitter_state, const int* action, int* rows, uint8_t* reports, int* due, int B, int window, int interval, void* stream) and int hilc_fec_adapt(const int* report, const int* action, const int* hold, int* rows, int* prev, int* fec_on, int B, int T, int m, int on_q8, int off_q8, int calm_reports, int timeout_hops, int initial_on, void* stream); and NACK with retransmission int hilc_nack_build(const int* jitter_state, const int* meta, const int* action, int* rows, uint8_t* nacks, int* due, int B, int capacity, int m, int rtt_hops, int retry_hops, int max_requests, int skip_fecable, void* stream) and int hilc_rtx_step(const uint8_t* packets, const int* nbytes, const int* nack_base, const int* nack_bitmap, const int* action, int* tags, int* ring, int* rows, uint8_t* out, int* out_nbytes, int B, int row_bytes, int history, int per_hop, void* stream); and report-driven rate control of the sender int hilc_rate_ceiling(const int* report, const int* action, const int* hold, const int* n_per_stream, const int* prev, int* rows, int* n_ceil, int B, int T, int n_max, int m, int header, int min_bits, int max_bits, int start_bits, int high_q8, int low_q8, int increase_q8, int burst_hops, int timeout_hops, void* stream) and int hilc_rate_charge(const int* nbytes, const int* rtx_nbytes, int* rows, int B, int per_hop, int burst_hops, void* stream); and the selective forwarding hop int hilc_forward_classify(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* rows, int* pick, int* pick_count, int B, int T, int n_max, int m, int order, int burst, int hang_hops, void* stream) and int hilc_forward_route(const int* arrivals, int max_arrivals, const int* action, const int* room, const int* layers, const int* sender_rows, const int* pick, const int* pick_count, int* routes, int* new_routes, int* rows, uint8_t* out, int* out_nbytes, int B, int T, int n_max, int m, int order, int fanout, int burst, int keep_fec, void* stream); and its downlink control int hilc_downlink_store(const int* arrivals, int max_arrivals, const int* action, const int* pick, const int* pick_count, int* tags, int* ring, int* rows, int B, int T, int n_max, int m, int burst, int history, void* stream) and int hilc_downlink_step(const int* routes, const int* new_routes, const uint8_t* in, const int* in_nbytes, const int* layers, const int* action, const int* report, const int* nack_base, const int* nack_bitmap, const int* tags, const int* ring, int* rows, int* memory, int* eff_layers, uint8_t* out, int* out_nbytes, uint8_t* rtx_out, int* rtx_nbytes, int* rtx_routes, int B, int T, int n_max, int m, int fanout, int burst, int keep_fec, int history, int per_hop, int rate_on, int min_bits, int max_bits, int start_bits, int high_q8, int low_q8, int increase_q8, int burst_hops, int timeout_hops, void* stream); and the audio level with level-based speaker selection int hilc_audio_level(const float* x, const double* thr, const int* hold, int* level, int B, int L, void* stream) and int hilc_forward_rank(const int* sd, const int* loud, const int* room, const int* action, const int* shadow_prev, int* shadow, int* rows, int B, int fanout, int hang_hops, int floor_level, int attack_shift, int decay_q8, int margin_db, void* stream); and the delay-based bandwidth estimate int hilc_rx_bwe(const int* arrivals, const int* offsets, const int* times, int max_arrivals, const int* action, int* rows, uint8_t* caps, int* due, int B, int T, int n_max, int m, int order, int min_bits, int max_bits, int window, int rate_window, int alpha_q8, int beta_q8, int increase_q16, int interval, int reset_ticks, void* stream) and int hilc_rate_cap(const int* cap, const int* action, const int* hold, int* rows, int* rate_rows, int B, int min_bits, int max_bits, int timeout_hops, void* stream); and SRTP packet protection int hilc_srtp_protect(const uint8_t* packets, const int* nbytes, const int* keys, int* rows, const int* action, uint8_t* out, int* out_nbytes, int B, int row_bytes, void* stream) and int hilc_srtp_unprotect(const int* arrivals, const int* offsets, int max_arrivals, const int* keys, int* rows, const int* action, int* plain, int B, int row_bytes, void* stream); and SRTP on the forwarding hop's routes int hilc_srtp_protect_routes(const uint8_t* rows, const int* nbytes, const int* routes, const int* new_routes, const int* action, const int* rekey_up, const int* rekey_down, const int* keys, int* route_rows, uint8_t* out, int* out_nbytes, int B, int fanout, int burst, int row_bytes, void* stream) */

int hilc_abi_version(void);
const char* hilc_error_string(int code);
/* text of the hipError_t behind the calling thread's most recent HILC_ERR_LAUNCH */
const char* hilc_last_hip_error(void);

/* ---- pointwise (1x1) convolution: fp32-MFMA GEMM with fused prologue / epilogue ----------------
 * y[b,m,t] = (sum_k wt[k][m] * pro(x[b,k,t]) + bias[m]) * out_scale + res[b,m,t]
 * Replaces: nn.Conv1d(k=1) inside SConv1d/NormConv1d (`models/hilcodec/modules/conv.py:115-134,
 * 202-236`) plus the ELU / Scale in front of it (`seanet.py:26-52,322-340`) and, with `res`, the
 * `x.add_(y.mul_(scale))` of SpecBlock (`seanet.py:241-246`).
 * wt is the folded weight TRANSPOSED to `[K][M]` (k-major).  bias, res may be NULL.  res may alias y.
 * Alignment: x, y and res must be 16-byte aligned for the fast path; wt is refused unless it is; bias needs only the 4 bytes of a float.
 * Size: x of 4 GiB or more takes the generic core (same fmaf chains, same bits); y / res of 4 GiB or more with a smaller x keep the fast path. */
int hilc_pw_conv(const float* x, const float* wt, const float* bias, const float* res, float* y,
                 int B, int K, int M, int T, float in_scale, int in_elu, float out_scale, void* stream);

/* ---- fused depthwise-separable block: pointwise conv -> depthwise causal conv through LDS ----------
 * h[b,m,t] = sum_k wt[k][m] * pro(x[b,k,t])                       (no bias: seanet.py:33-37)
 * y[b,m,o] = post((sum_j dw_w[m][j] * h[b,m,o*stride - pad + j] + dw_b[m]) * out_scale + res[b,m,o])
 * with h(t<0) = h(t>=T) = 0, pad = (ksize-1)-(stride-1), T_out = ceil(T/stride).  Supported: ksize 5 /
 * stride 1 (residual-block halves, `seanet.py:26-52,129-148`; decoder/encoder pre/post pairs) and
 * ksize = 2*stride (encoder down-sampling, `seanet.py:322-340`; res/out_elu/out_scale unused there).
 * The [M x T] intermediate h lives only in LDS: one HBM read of x and one write of y per block half.
 * Alignment: x, and for ksize 5 y and res, must be 16-byte aligned for the fast path; wt is refused unless it is; dw_w, dw_b (and y of the
 * strided form) need only the 4 bytes of a float.
 * Size: x of 4 GiB or more takes the generic core (same bits), for both kernel shapes. */
int hilc_dws_conv(const float* x, const float* wt, const float* dw_w, const float* dw_b, const float* res,
                  float* y, int B, int K, int M, int T, int ksize, int stride, float in_scale, int in_elu,
                  float out_scale, int out_elu, void* stream);

/* 1 if hilc_dws_conv (ksize 5, stride 1) runs this shape in the wave-row tile form (depthwise taps on the accumulator
 * registers), 0 for the column-block form with the LDS epilogue.  Both give the same bits; a pure function of the shape and the
 * device's CU count (diagnostics and tests). */
int hilc_dws_conv_wave_row(int B, int M, int T, int has_res);

/* ---- fused up-sampling stage: [Scale, ELU,] depthwise transposed conv (k = 2*stride) -> pointwise conv ---
 * u[b,k,q*stride+p] = tr_w[k][p] * pro(x[b,k,q]) + tr_w[k][p+stride] * pro(x[b,k,q-1])      (x[-1] = 0)
 * y[b,m,t] = sum_k wt[k][m] * u[b,k,t] + bias[m],   t < Tin*stride
 * The up-sampled tensor u only exists as the GEMM's B operand (computed in the loader).
 * Replaces: `seanet.py:424-441` (Scale, ELU, SConvTranspose1d, SConv1d k=1 with bias). Requires
 * (Tin*stride) % 4 == 0 and M % 4 == 0 (else HILC_ERR_UNSUPPORTED: use hilc_dw_convtr + hilc_pw_conv).
 * Alignment (the three entry points of this stage): tr_w, tr_w_expanded and y must be 16-byte aligned for the fast path; wt is refused
 * unless it is, before anything is written; x, hist, hist_out and bias need only the 4 bytes of a float.
 * Size (the three entry points): x of 4 GiB or more, or 2^31 output columns B * Tin * stride, take the generic core (same bits). */
int hilc_up_conv(const float* x, const float* tr_w, const float* wt, const float* bias, float* y,
                 int B, int K, int M, int Tin, int stride, float in_scale, int in_elu, void* stream);

/* Streaming hop of the same stage (`streaming.py:520-648` Decoder.forward, `causal_layers.py:168-188`): hist `[B][K]` =
 * pro(x[b,k,-1]) of the previous hop (the transposed conv's cache holds ACTIVATED samples, like hilc_dw_convtr's),
 * hist_out receives pro(x[b,k,Tin-1]).  Both optional; must not alias. */
int hilc_up_conv_stream(const float* x, const float* hist, float* hist_out, const float* tr_w, const float* wt,
                        const float* bias, float* y, int B, int K, int M, int Tin, int stride, float in_scale,
                        int in_elu, void* stream);

/* Strides other than 2 / 4 / 8 (the codec's 5): with `tr_w_expanded` = the table written by hilc_up_conv_expand_taps
 * (`[K][stride][8]` floats, 16-B aligned: for each phase p0 = t mod stride of a 4-column group its eight taps as two
 * 16-B words) the loader issues two vector tap loads per row instead of eight scalar ones.  hist / hist_out /
 * tr_w_expanded may be NULL (then this is hilc_up_conv_stream). */
int hilc_up_conv_expand_taps(const float* tr_w, float* expanded, int K, int stride, void* stream);
int hilc_up_conv_expanded(const float* x, const float* hist, float* hist_out, const float* tr_w,
                          const float* tr_w_expanded, const float* wt, const float* bias, float* y, int B, int K,
                          int M, int Tin, int stride, float in_scale, int in_elu, void* stream);

/* Streaming hop of hilc_dws_conv for the wide layers (DWSBlock.forward `streaming.py:160-192`, CausalConv1d
 * `causal_layers.py:147-165`): T <= 128 samples per stream and call, T % stride == 0, any ksize >= stride; longer
 * hops (T % 4 == 0; per-clip tiles with a recomputed halo) for ksize == 2 * stride.
 * hist `[B][M][ksize-stride]` = the last pointwise outputs of the previous hop (NULL = zeros), hist_out receives
 * the new cache (must not alias hist).  A tile holds whole clips, so nothing is recomputed.
 * Alignment: T <= 128: x, and for ksize 5 y, res, hist and hist_out, must be 16-byte aligned for the fast path; wt is refused unless it
 * is, and so is dw_w for ksize 16 / stride 8 and ksize 10 / stride 5 (a row's taps are read as 16- / 8-byte words).  T > 128: x and wt
 * are refused unless 16-byte aligned.  Everything else needs only the 4 bytes of a float.
 * Size: T > 128: an x of 4 GiB or more is HILC_ERR_UNSUPPORTED, nothing written (that form has the linear core only; fall back to hilc_pw_conv +
 * hilc_dw_conv, same bits).  T <= 128: it takes the generic core (from the launcher; not run at 4 GiB by the tests). */
int hilc_dws_conv_stream(const float* x, const float* wt, const float* dw_w, const float* dw_b, const float* hist,
                         float* hist_out, const float* res, float* y, int B, int K, int M, int T, int ksize,
                         int stride, float in_scale, int in_elu, float out_scale, int out_elu, void* stream);

/* ---- fully fused residual block (C in {64, 96, 128, 192} and — narrow-tile shapes — {256, 384, 512, 768}; T % 4 == 0) --------
 * y = x + out_scale * (dw2(pw2(ELU(dw1(pw1(ELU(pre_scale * x))) + dw1_b))) + dw2_b)
 * One HBM read of x and one write of y per block; both pointwise outputs and the mid activation
 * stay in LDS.  w1t / w2t are the two `[C][C]` pointwise matrices in the PACKED layout written by
 * hilc_resblock_pack_weights (below), dw*_w `[C][5]`.  y must not alias x.
 * Replaces: SEANetResnetBlock.forward (`seanet.py:129-148`) with skip='identity', kernel 5.
 * hilc_resblock_supported(C, T) tells the caller whether this specialisation exists.
 * Alignment (hilc_resblock, _stream, _balanced): x, y, w1t, w2t and the four caches are refused unless 16-byte aligned; the depthwise
 * taps and biases need only the 4 bytes of a float.
 * Size: hilc_resblock (and hilc_resblock_balanced with streaming = 0) takes any size, 64-bit offsets.  hilc_resblock_stream (and streaming = 1)
 * walks a flat 32-bit column space: B * C * T * 4 >= 2^32 is HILC_ERR_UNSUPPORTED (fall back to two hilc_dws_conv_stream or to hilc_pw_conv +
 * hilc_dw_conv launches per half). */
int hilc_resblock(const float* x, const float* w1t, const float* dw1_w, const float* dw1_b, const float* w2t,
                  const float* dw2_w, const float* dw2_b, float* y, int B, int C, int T, float pre_scale,
                  float out_scale, void* stream);
int hilc_resblock_supported(int C, int T);

/* One-off (per checkpoint) re-layout of a k-major `[C][C]` pointwise matrix (wt[k][m], the layout hilc_pw_conv
 * takes) into "MFMA lane order": the operands one lane feeds to the matrix pipe for a 16-deep K slice become
 * consecutive 16-B words, so the fused block streams its weights with a quarter of the load instructions.
 * packed: `C*C` floats, must not alias wt.  C in {64, 96, 128, 192}, and {256, 384, 512, 768} for the streaming form. */
int hilc_resblock_pack_weights(const float* wt, float* packed, int C, void* stream);

/* Streaming form of the same block (`streaming.py:195-276` ResBlock with two DWSBlock caches,
 * `causal_layers.py:147-167`): hist1 / hist2 `[B][C][4]` = the last 4 samples of the two depthwise convs'
 * inputs (the pointwise outputs) from the previous hop, hist*_out receive the new caches.  All four are
 * optional (NULL = zero history / no cache written); outputs must not alias inputs.
 * Besides the offline widths the streaming form takes the WIDE blocks of a hop, where a stream contributes 8 or 40
 * frames: C = 256 / 384 (64-column tiles over the flat stream-major column space) and C = 512 / 768 (32-column tiles of
 * whole streams, T in {4, 8, 16, 32}: no halo) — both GEMMs and the activation between them in one launch instead of two
 * hilc_dws_conv_stream launches; same products in the same order, bit-identical.  hilc_resblock_stream_supported(C, T)
 * tells the caller whether the specialisation exists (else HILC_ERR_UNSUPPORTED: fall back to two launches). */
int hilc_resblock_stream_supported(int C, int T);
int hilc_resblock_stream(const float* x, const float* w1t, const float* dw1_w, const float* dw1_b,
                         const float* w2t, const float* dw2_w, const float* dw2_b, const float* hist1,
                         const float* hist2, float* hist1_out, float* hist2_out, float* y, int B, int C, int T,
                         float pre_scale, float out_scale, void* stream);

/* Same kernels with a caller-owned dynamic tile scheduler: `sched` = two ints in device memory that are ZERO at
 * launch; the kernel leaves them zero again (the last workgroup re-arms them), so one buffer per stream can be
 * reused by every call on that stream.  Workgroups take tiles by ticket instead of from static lists — the
 * workgroups that share a CU are not served equally, and static lists leave a third of the kernel at half
 * occupancy.  streaming = 0: hilc_resblock semantics (hist* ignored and may be NULL); 1: hilc_resblock_stream.
 * sched == NULL: static lists. */
int hilc_resblock_balanced(const float* x, const float* w1t, const float* dw1_w, const float* dw1_b,
                           const float* w2t, const float* dw2_w, const float* dw2_b, const float* hist1,
                           const float* hist2, float* hist1_out, float* hist2_out, float* y, int* sched,
                           int streaming, int B, int C, int T, float pre_scale, float out_scale, void* stream);

/* ---- the residual blocks of ONE STAGE in one launch (ABI 10) --------------------------------------------------------
 * The reference runs a stage's blocks one after the other: encoder `seanet.py:316-330` (`self.blocks[i]`, 2 per stage),
 * decoder `seanet.py:437-452` (3 after each up-sampling layer); streaming `streaming.py:497-503` / `:633-639` with two
 * caches per block.  hilc_resblock_chain(x, y, blocks, nblk, ...) == nblk calls of hilc_resblock_stream with the output of
 * one as the input of the next, bit for bit — but per tile the blocks run back to back and a block's output stays in
 * registers as the next block's input and shortcut: the activations between the blocks never reach HBM and the stage is one
 * launch instead of nblk (a streaming hop of 1024 streams is 5-10 tiles per workgroup and launch).
 * blocks[i]: that block's parameters; w1t / w2t PACKED by hilc_resblock_pack_weights_rc(.., C, hilc_resblock_chain_row_classes(C))
 * (the chain's 8-wave shapes split the rows in two classes also below C = 192, so the layout differs from hilc_resblock's);
 * hist* as in hilc_resblock_stream (each optional; ignored with streaming = 0: the offline causal model, hilc_resblock).
 * hilc_resblock_chain_supported tells whether the specialisation exists: C in {64, 96, 128, 192} any T % 4 == 0;
 * streaming: C in {512, 768} with whole streams tiling 32 columns, and C = 256 (32-column tiles, four waves, runs of whole streams:
 * measured slower inside a 1024-stream hop than one launch per block, so the engine leaves it off); offline: C in {256, 384, 512} (C = 768: one block per launch,
 * the carry slots of a second do not fit LDS); nblk = 2, or 3 at the decoder's widths (96, 192, streaming 768, offline 384).
 * Else HILC_ERR_UNSUPPORTED: launch the blocks one by one.
 * Alignment: x, y and of every block w1t, w2t and (streaming) the four caches are refused unless 16-byte aligned; the depthwise taps and
 * biases need only the 4 bytes of a float.
 * Size: streaming = 0 takes any size; streaming = 1 refuses B * C * T * 4 >= 2^32 (HILC_ERR_UNSUPPORTED; hilc_resblock_chain_supported knows no
 * batch size and cannot say so: launch the blocks one by one). */
typedef struct hilc_resblock_params {
  const float* w1t; const float* dw1_w; const float* dw1_b;
  const float* w2t; const float* dw2_w; const float* dw2_b;
  const float* hist1; const float* hist2; float* hist1_out; float* hist2_out;
  float pre_scale, out_scale;
} hilc_resblock_params;
int hilc_resblock_chain_supported(int C, int T, int nblk, int streaming);
int hilc_resblock_chain_row_classes(int C);           /* streaming form */
int hilc_resblock_chain_row_classes_offline(int C);   /* offline form (streaming = 0: hilc_resblock semantics, C in {64 ... 768}) */
int hilc_resblock_pack_weights_rc(const float* wt, float* packed, int C, int row_classes, void* stream);
int hilc_resblock_chain(const float* x, float* y, const hilc_resblock_params* blocks, int nblk, int streaming,
                        int B, int C, int T, void* stream);

/* ---- a DECODER STAGE of a streaming hop in one launch (ABI 13): its up-sampling layer and its residual blocks -----------------
 * `seanet.py:431-452` ([Scale, ELU, depthwise SConvTranspose1d k = 2r stride r, 1x1 conv 2C -> C + bias], then the stage's
 * SEANetResnetBlocks); streaming `streaming.py:629-639`, the transposed conv's cache `[B][2C][1]` = its last ACTIVATED input frame
 * (`causal_layers.py:168-188`).  Equals hilc_up_conv_stream followed by hilc_resblock_chain bit for bit; the `[B][C][T]` tensor
 * between them never exists.  x `[B][2C][T/r]`, tr_w `[2C][2r]`, w_lo / w_hi: rows [0, C) / [C, 2C) of the k-major `[2C][C]`
 * pointwise weight, each packed with hilc_resblock_pack_weights_rc(.., C, hilc_resblock_chain_row_classes(C)).
 * Stages: C = 768 with r = 8 (streaming: whole streams per 32-column tile, T in {8, 16, 32}, nblk 1..3; offline: nblk = 1 — the
 * up-sampling layer and the stage's FIRST block, the carry slots of a second do not fit LDS), C = 384 with r = 5 (tr_w = the EXPANDED
 * tap table `[2C][r][8]` of hilc_up_conv_expand_taps; nblk 1..3; a streaming hop (ABI 15) on 32-column carry tiles, runs of whole
 * streams, twelve waves — rounds 4-5: nblk = 1 on 64-column halo tiles),
 * C = 192 with r = 4 and C = 96 with r = 2 (streaming hops and, with streaming = 0, the offline model: hist* ignored); nblk 1..3.
 * Alignment: y, up->tr_w, up->w_lo, up->w_hi and the blocks' operands named at hilc_resblock_chain are refused unless 16-byte aligned;
 * up->x, up->hist, up->hist_out, up->bias and the blocks' taps and biases need only the 4 bytes of a float.
 * Size (hilc_decoder_stage and hilc_decoder_stage_post): streaming = 0 takes any size; streaming = 1 refuses B * C * T * 4 >= 2^32
 * (HILC_ERR_UNSUPPORTED in front of the launch). */
typedef struct hilc_up_params {
  const float* x; const float* tr_w; const float* w_lo; const float* w_hi; const float* bias;
  const float* hist; float* hist_out;
  float in_scale; int stride;
} hilc_up_params;
int hilc_decoder_stage_supported(int C, int T, int nblk, int stride, int streaming);
int hilc_decoder_stage(const hilc_up_params* up, const hilc_resblock_params* blocks, int nblk, float* y, int streaming,
                       int B, int C, int T, void* stream);

/* ---- the decoder's LAST stage AND its closing layer in one launch (ABI 14) --------------------------------------------------
 * `seanet.py:453-476`: `[Scale, ELU, SConv1d(C, 1, k = 5, bias)]`, then the model's final scale / tanh — hilc_conv_post — as the closing
 * phase of the hilc_decoder_stage launch of the offline model's last stage (C = 96, r = 2, three blocks): the last block leaves
 * ELU(in_scale * y) in the LDS tile, the launch stores `wav` `[B][1][T]`; the stage's `[B][C][T]` output never reaches HBM.  Equals
 * hilc_decoder_stage followed by hilc_conv_post bit for bit (same row classes c mod 8, same order of the partial sums).  streaming = 0:
 * the offline model (`up->hist`, the blocks' caches and `post->hist` are ignored).  streaming = 1 (ABI 15): a hop (`streaming.py:639-648`) on the
 * carry form's runs of whole streams, with every cache of hilc_decoder_stage plus the closing conv's — equal, bit for bit, to
 * hilc_decoder_stage(streaming) followed by hilc_conv_post with the same caches.  hilc_decoder_stage_post_supported names the shapes;
 * everything else: HILC_ERR_UNSUPPORTED.
 * Alignment: as hilc_decoder_stage; post->wav, post->hist and post->hist_out are refused unless 16-byte aligned; post->w and post->bias
 * need only the 4 bytes of a float. */
typedef struct hilc_post_params {
  const float* w;      /* [C][ksize] */
  const float* bias;   /* [1] or NULL */
  float* wav;          /* [B][1][T] */
  const float* hist;   /* streaming (ABI 15): [B][C][ksize-1] the conv's cache = hilc_conv_post's (activated samples; NULL = zeros) */
  float* hist_out;     /* streaming: receives the next hop's cache (may be NULL) */
  float in_scale, out_scale;
  int do_tanh, ksize;
} hilc_post_params;
int hilc_decoder_stage_post_supported(int C, int T, int nblk, int stride, int ksize);
int hilc_decoder_stage_post(const hilc_up_params* up, const hilc_resblock_params* blocks, int nblk, const hilc_post_params* post,
                            int streaming, int B, int C, int T, void* stream);

/* ---- an ENCODER STAGE in one launch (ABI 11): its residual blocks and its down-sampling layer ------------------------------
 * `seanet.py:316-339` (`self.blocks[i]`, then `self.downsample[i]` = [Scale, ELU, 1x1 conv C -> 2C without bias, depthwise conv
 * k = 2r stride r with bias]); streaming `streaming.py:497-511` with the layer's cache `[B][2C][r]`.  Equals hilc_resblock_chain
 * followed by hilc_dws_conv / hilc_dws_conv_stream (stride r, in_scale, in_elu = 1, `res`) bit for bit; the stage's output
 * `[B][C][T]` never reaches HBM.  w_lo / w_hi: columns [0, C) / [C, 2C) of the k-major `[C][2C]` pointwise weight, each packed
 * like a block's matrix (hilc_resblock_pack_weights_rc with the row classes of the chain form in use).  res (optional): added to
 * the output, e.g. the next stage's SpecBlock branch.  Stages: C = 64 with r = 2, C = 128 with r = 4, and the wide stages C = 256 with
 * r = 5 and C = 512 with r = 8 — offline in the carry form of the narrow-tile shapes; a streaming hop (ABI 15): C = 256 on 32-column carry
 * tiles (runs of whole streams; T % 40 == 0, i.e. whole frames of the hop), C = 512 on whole-stream tiles (T in {8, 16, 32}); nblk 1..2;
 * T % 4 == 0, T % r == 0.  hilc_encoder_stage_supported names the shapes; everything else HILC_ERR_UNSUPPORTED (callers launch the
 * blocks and hilc_dws_conv[_stream] instead).
 * Alignment: x, down->w_lo, w_hi, res, y, hist, hist_out, the blocks' operands named at hilc_resblock_chain and, for C = 256 / 512,
 * down->dw_w are refused unless 16-byte aligned; down->dw_b, down->dw_w of the narrow stages and the blocks' taps and biases need only the
 * 4 bytes of a float.
 * Size: streaming = 0 takes any size; streaming = 1 refuses B * 2C * T * 4 >= 2^32 (HILC_ERR_UNSUPPORTED in front of the launch). */
typedef struct hilc_down_params {
  const float* w_lo; const float* w_hi; const float* dw_w; const float* dw_b;
  const float* hist; float* hist_out; const float* res; float* y;
  float in_scale; int stride;
} hilc_down_params;
int hilc_encoder_stage_supported(int C, int T, int nblk, int stride, int streaming);
int hilc_encoder_stage(const float* x, const hilc_resblock_params* blocks, int nblk, const hilc_down_params* down, int streaming,
                       int B, int C, int T, void* stream);

/* ---- the encoder's FIRST stage with its input computed in the launch (ABI 14; a streaming hop: ABI 15) ------------------------
 * `seanet.py:280-286` (first conv k = 5, 1 -> 64), `:220-246` (stage 0's SpecBlock: STFT n_fft 64 hop 1 -> log-magnitude -> 1x1 conv),
 * `:316-339` (the stage's residual blocks and down-sampling layer): hilc_spec_block_conv_pre's arithmetic as the opening phase of the
 * hilc_encoder_stage launch for C = 64, r = 2 — equal to the two launches bit for bit; the `[B][64][T]` tensor between them never
 * reaches HBM.  `spec`: the arguments of hilc_spec_block_conv_pre (packed tables from hilc_spec_block_pack).  streaming = 0: the offline
 * model (`spec->hist`, the blocks' caches and `down->hist` are ignored).  streaming = 1 (ABI 15, `streaming.py:490-511`): a hop on runs of whole
 * streams, T >= 128 (a 128-column tile then holds at most one stream start: its waveform segment is staged as two pieces, each with the 63
 * samples in front of it — a stream's history at t = 0), with every cache of hilc_encoder_stage(streaming).
 * Alignment: spec->dft_packed, spec->pw_packed, down->w_lo, w_hi, res, y, hist, hist_out and the blocks' operands named at
 * hilc_resblock_chain are refused unless 16-byte aligned; spec->wav, spec->hist and every other operand need only the 4 bytes of a float.
 * Size: streaming = 0 takes any size; streaming = 1 refuses B * 128 * T * 4 >= 2^32 (HILC_ERR_UNSUPPORTED in front of the launch). */
typedef struct hilc_spec0_params {
  const float* wav;         /* [B][T] */
  const float* dft_packed; const float* nyq_sin; const float* pw_packed; const float* bias;
  const float* pre_w;       /* [64][5] */
  const float* pre_b;       /* [64] or NULL */
  const float* hist;        /* streaming (ABI 15): [B][hist_len] waveform history, as hilc_spec_block_conv_pre's (NULL = zeros) */
  int hist_len;
  float pre_in_scale, mean, std, out_scale;
  int normalize, n_fft, hop, pre_ksize;
} hilc_spec0_params;
int hilc_encoder_stage0_supported(int T, int nblk, int stride, int n_fft, int hop, int pre_ksize, int streaming);
int hilc_encoder_stage0(const hilc_spec0_params* spec, const hilc_resblock_params* blocks, int nblk, const hilc_down_params* down,
                        int streaming, int B, int T, void* stream);

/* ---- depthwise causal convolution, kernel `ksize`, stride `stride` ----------------------------
 * pad = (ksize-1) - (stride-1);  T_out = ceil(T / stride)
 * y[b,c,o] = post((sum_j w[c][j] * xe[b,c,o*stride - pad + j] + bias[c]) * out_scale + res[b,c,o])
 * xe(t) = t < 0 ? hist[b,c,pad+t] (0 if hist NULL) : t < T ? pro(x[b,c,t]) : 0 ; post = ELU if out_elu.
 * hist_out (optional) receives the last `pad` samples of [hist | pro(x)]  -> next call's hist.
 * Replaces: depthwise SConv1d (`conv.py:202-236`, groups=C: `seanet.py:42-51,330-339,352-355,
 * 417-419`), CausalConv1d (`causal_layers.py:147-165`) and the residual tail of
 * SEANetResnetBlock.forward (`seanet.py:144-148`). res may alias y.
 * Alignment: x and y must be 16-byte aligned for the fast path (ksize 5, stride 1, T % 4 == 0); everything else needs only the 4 bytes
 * of a float.
 * Size: any (64-bit offsets), as for hilc_dw_convtr, hilc_conv_pre, hilc_conv_post and hilc_l2norm below — and, from its launcher only (not run at
 * 4 GiB by the tests), hilc_tail. */
int hilc_dw_conv(const float* x, const float* hist, const float* w, const float* bias, const float* res,
                 float* y, float* hist_out, int B, int C, int T, int ksize, int stride,
                 float in_scale, int in_elu, float out_scale, int out_elu, void* stream);

/* ---- depthwise causal transposed convolution, kernel 2*stride, stride `stride` -----------------
 * y[b,c,q*stride+p] = w[c][p] * xe[q] + w[c][p+stride] * xe[q-1],  T_out = T*stride,
 * xe(-1) = hist[b,c,0] (0 if NULL).  hist_out (optional) receives pro(x[b,c,T-1]).
 * Replaces: SConvTranspose1d (`conv.py:239-282`, right-trim k-s) and CausalConvTranspose1d
 * (`causal_layers.py:168-188`) for groups=C, k=2s, plus the Scale+ELU in front (`seanet.py:424-441`).
 * Alignment: every operand needs only the 4 bytes of a float. */
int hilc_dw_convtr(const float* x, const float* hist, const float* w, float* y, float* hist_out,
                   int B, int C, int T, int stride, float in_scale, int in_elu, void* stream);

/* ---- first encoder conv: Conv1d(1 -> C, ksize, causal, bias) on the waveform --------------------
 * y[b,c,t] = sum_j w[c][j] * (in_scale * we[b, t-(ksize-1)+j]) + bias[c];  we(t<0) = hist[b, hist_len+t] or 0.
 * Replaces: `seanet.py:280-286` (Scale(1/wav_std) + SConv1d) / `streaming.py:490`.
 * Alignment: wav and y must be 16-byte aligned for the fast path (ksize 5, T % 4 == 0); everything else needs only the 4 bytes of a float. */
int hilc_conv_pre(const float* wav, const float* hist, int hist_len, const float* w, const float* bias,
                  float* y, int B, int C, int T, int ksize, float in_scale, void* stream);

/* ---- last decoder conv: [Scale, ELU,] Conv1d(C -> 1, ksize, causal, bias), * out_scale, tanh -----
 * y[b,0,t] = act((sum_c sum_j w[c][j] * xe[b,c,t-(ksize-1)+j] + bias[0]) * out_scale), act = tanh if do_tanh.
 * Replaces: `seanet.py:457-473` / `streaming.py:643-647`. hist/hist_out as in hilc_dw_conv.
 * Order of the channel sum (ksize 5, T % 4 == 0, 16-B aligned x): eight classes c mod 8, each an fmaf chain over (c, tap) ascending, the
 * classes added in ascending order — the order of hilc_decoder_stage_post's closing phase.
 * Alignment: x and hist must be 16-byte aligned for that fast path; a 4-byte-aligned view of either takes the generic kernel, which sums
 * the channels in sequence (c ascending, then taps): the one fall-back whose bits differ.  w, bias, y and hist_out need only the 4 bytes
 * of a float. */
int hilc_conv_post(const float* x, const float* hist, const float* w, const float* bias, float* y,
                   float* hist_out, int B, int C, int T, int ksize, float in_scale, int in_elu,
                   float out_scale, int do_tanh, void* stream);

/* ---- causal STFT magnitude -> log -> normalise (the front half of a SpecBlock) ------------------
 * frame f covers we[b, f*hop-(n_fft-1) .. f*hop];  T_f = (T-1)/hop + 1;
 * mag = sqrt(max(re^2+im^2,1e-12));  spec[b,k,f] = normalize==2 ? mag : log(max(mag,1e-5)), then
 * (. - mean)/std if normalize==1 (0: plain log-magnitude, streaming model with merged normalisation)
 * basis_t: `[n_fft][m_pad]` fp32, row n holds (cos_0, sin_0, cos_1, sin_1, ...)*hann for sample n,
 *          m_pad = round_up(n_fft+2, 32), zero padded (host-built from the reference's basis).
 * Replaces: CausalSTFT (`conv.py:285-358`, `causal_layers.py:72-144`) + `seanet.py:224-236`.
 * Alignment: basis_t is refused unless 16-byte aligned; wav, hist and spec need only the 4 bytes of a float.
 * Size: any (64-bit offsets; both the flat and the per-clip segment form). */
int hilc_stft_logmag(const float* wav, const float* hist, int hist_len, const float* basis_t, float* spec,
                     int B, int T, int n_fft, int hop, float mean, float std, int normalize, void* stream);

/* ---- one-launch SpecBlock (long encoder stages: n_fft 64 / 128 / 256 with the codec's hops 1 / 2 / 8, C == n_fft) ---
 * y[b,m,f] = x[b,m,f] + out_scale * (sum_k pw[k][m] * spec[b,k,f] + bias[m]),  spec as in hilc_stft_logmag: `hist`
 * `[B][hist_len]` (hist_len >= n_fft-1) = the waveform before t = 0 for a streaming hop (`streaming.py:482-490`), NULL = zeros
 * i.e. SpecBlock.forward (`models/hilcodec/modules/seanet.py:220-246`: CausalSTFT `conv.py:329-358`, log / normalise,
 * 1x1 conv, `x.add_(y.mul_(scale))`) without the [n_fft/2+1 x T_f] tensor ever reaching HBM.  Bit-identical to
 * hilc_stft_logmag + hilc_pw_conv(res = x).  T_f = (T-1)/hop + 1 must be a multiple of 4; x, y 16-B aligned, y != x.
 * x == NULL: the branch alone, y = out_scale * (W spec + bias) — it depends on the waveform only, so a streaming hop computes it
 * beside the previous stage and the down-sampling layer in front adds it as its `res` (same two roundings, same result).
 * dft_packed / pw_packed: hilc_spec_block_pack of
 *   which = 0: the k-major `[n_fft][n_fft]` DFT matrix whose columns are (cos_0, cos_{N/2}, cos_1, sin_1, cos_2, sin_2, ...,
 *              cos_{N/2-1}, sin_{N/2-1}) * hann — the reference basis without the all-zero sin_0 row and without sin_{N/2};
 *   which = 1: the k-major `[n_fft/2+1][C]` conv weight (hilc_pw_conv's layout);
 * nyq_sin `[n_fft]`: the sin_{N/2} row of the reference basis (|.| <= 1.4e-4, evaluated as a scalar chain).
 * hilc_spec_block_packed_floats(n_fft, which) = size of a packed operand.
 * Alignment (hilc_spec_block and hilc_spec_block_conv_pre): x, y, dft_packed and pw_packed are refused unless 16-byte aligned; wav, hist,
 * nyq_sin, bias, pre_w and pre_b need only the 4 bytes of a float.
 * Size: any (64-bit offsets). */
int hilc_spec_block_supported(int n_fft, int hop, int C, int T);
int hilc_spec_block_packed_floats(int n_fft, int which);
int hilc_spec_block_pack(const float* w, float* packed, int K, int n_fft, int which, void* stream);
int hilc_spec_block(const float* wav, const float* hist, int hist_len, const float* dft_packed, const float* nyq_sin,
                    const float* pw_packed, const float* bias, const float* x, float* y, int B, int T, int n_fft, int hop,
                    float mean, float std, int normalize, float out_scale, void* stream);
/* First encoder stage: the same with x = the first conv of the same waveform, computed in the kernel instead of read:
 * x[b,m,t] = sum_j pre_w[m][j] * (pre_in_scale * wav[b, t-(ksize-1)+j]) + pre_b[m]   (hilc_conv_pre; `seanet.py:280-286`,
 * `:368-372`).  n_fft = 64, hop = 1, pre_ksize = 5 only (HILC_ERR_UNSUPPORTED otherwise); bit-identical to
 * hilc_conv_pre + hilc_spec_block. */
int hilc_spec_block_conv_pre(const float* wav, const float* hist, int hist_len, const float* dft_packed,
                             const float* nyq_sin, const float* pw_packed, const float* bias, const float* pre_w,
                             const float* pre_b, float pre_in_scale, float* y, int B, int T, int n_fft, int hop, int pre_ksize,
                             float mean, float std, int normalize, float out_scale, void* stream);

/* ---- streaming cache update: out[row][i] = last `pad` samples of [hist[row][0..hist_len) | x[row][0..T)] ----
 * Replaces: `cache = x[:, :, -causal_padding:]` after `torch.cat((cache, x), dim=2)`
 * (`causal_layers.py:160-162`, waveform cache `streaming.py:486-488`). hist may be NULL (zeros).
 * Alignment: every operand needs only the 4 bytes of a float. */
int hilc_tail(const float* x, const float* hist, float* out, long rows, int T, int pad, int hist_len,
              void* stream);

/* ---- L2 normalisation over channels: y = x / max(||x||_2, eps) * scale ---------------------------
 * x `[B][C][T]`; y `[B][C][T]` or, if channel_last_out, `[B][T][C]` (streaming encoder output).
 * Replaces: L2Norm (`seanet.py:151-162`, `streaming.py:279-286`).
 * Alignment: x and y need only the 4 bytes of a float. */
int hilc_l2norm(const float* x, float* y, int B, int C, int T, float eps, float scale,
                int channel_last_out, void* stream);

/* ---- residual VQ encode ------------------------------------------------------------------------
 * for i < n:  idx_i = argmin_k(norms[i][k] - 2 * <r, E_i[k]>) (first minimum), r -= E_i[idx_i], q += E_i[idx_i]
 * z: `[B][C][T]` (channel_last=0) or `[B][T][C]` (1).  codebooks `[Nq][K][C]`, codebooks_t `[Nq][C][K]`
 * (the same tables transposed, for coalesced scoring), norms `[Nq][K]` = |E|^2 (host: embed.pow(2).sum).
 * indices int64: `[B][n][T]` (stage_major=0, offline return_indices) or `[n][B][T]` (1, streaming).
 * q (optional) same layout as z.  frame_err (optional) `[B*T]` receives sum_c (z-q)^2 per frame.
 * Replaces: EuclideanCodebook.forward + ResidualVQ.forward eval branch
 * (`models/hilcodec/vector_quantize.py:132-176,199-243`, `modules/vector_quantize.py:141-195,490-516`,
 * `models/hilcodec/streaming.py:51-68,89-100`).  Returns HILC_ERR_RANGE unless 1 <= n <= Nq.
 * Every score is one fp32 fmaf chain over the channels in ascending order, whatever the batch size: small batches on the VALU
 * (4 or 16 frames per workgroup), 8 192 frames and more on the matrix pipe (v_mfma_f32_32x32x2_f32, 32 frames per workgroup,
 * the A operand read straight from codebooks_t) — same bits, same indices.  flags: 0, or HILC_RVQ_VALU_ONLY = keep large batches
 * on the VALU form too (16 frames per workgroup; the caller's switch should an fp32 MFMA ever stop being a sequential fmaf chain
 * over ascending k); any other bit: HILC_ERR_UNSUPPORTED.
 * Alignment: codebooks_t and norms must be 16-byte aligned for the matrix-pipe form (else large batches keep the VALU form: same indices);
 * everything else needs only the 4 bytes of a float.
 * Size: any, in both forms and in hilc_rvq_decode (64-bit offsets; the frame count B * T is a long). */
#define HILC_RVQ_VALU_ONLY 1
int hilc_rvq_encode(const float* z, const float* codebooks, const float* codebooks_t, const float* norms,
                    int64_t* indices, float* q, float* frame_err, int B, int C, int T, int K, int Nq, int n,
                    int channel_last, int stage_major, int flags, void* stream);

/* Mixed-bitrate batch (SURVEY §8f-3: `n` drawn per request from `dropout_index`, configs/hilcodec_*.yaml:38,
 * `infer_n` :117,130): clip b uses stages [0, n_per_clip[b]) (int32 `[B]`, device; values clamped to [1, n]);
 * rows >= n_per_clip[b] of `indices` are written as -1 and leave q / the residual untouched, so clip b's
 * results equal a uniform call with n = n_per_clip[b].  `n` = rows of `indices` (>= every entry).
 * n_per_clip == NULL is hilc_rvq_encode. */
int hilc_rvq_encode_mixed(const float* z, const float* codebooks, const float* codebooks_t, const float* norms,
                          const int* n_per_clip, int64_t* indices, float* q, float* frame_err, int B, int C,
                          int T, int K, int Nq, int n, int channel_last, int stage_major, int flags, void* stream);

/* mean over `count` of frame_err[0..frames) in a fixed order -> loss[0]  (F.mse_loss, `vector_quantize.py:233`) */
int hilc_mse_finalize(const float* frame_err, float* loss, int frames, double count, void* stream);

/* ---- residual VQ decode (Dequantizer): q = sum_{i<n} E_i[idx_i] ---------------------------------
 * Replaces: Dequantizer.forward (`streaming.py:148-157`) / F.embedding sums in ResidualVQ.
 * Alignment: codebooks and q need only the 4 bytes of a float. */
int hilc_rvq_decode(const int64_t* indices, const float* codebooks, float* q, int B, int C, int T,
                    int K, int Nq, int n, int channel_last, int stage_major, void* stream);

/* mixed-bitrate decode: clip b sums stages [0, n_per_clip[b]) only (rows beyond are ignored, e.g. the -1 rows
 * hilc_rvq_encode_mixed writes); n_per_clip == NULL is hilc_rvq_decode. */
int hilc_rvq_decode_mixed(const int64_t* indices, const float* codebooks, const int* n_per_clip, float* q, int B,
                          int C, int T, int K, int Nq, int n, int channel_last, int stage_major, void* stream);

/* ---- RVQ training side: EMA cluster statistics and codebook update (SURVEY §8f-4) -----------------
 * hilc_rvq_ema_stats: bucket `[n][K + K*C]`, per stage s: K counts (#frames with code k) then `[K][C]` sums of
 * the stage-s input residuals of those frames — `torch.cat([embed_onehot.sum(0), (embed_onehot.t() @ flatten).view(-1)])`
 * (`models/hilcodec/vector_quantize.py:155-162`) for all stages at once, so that the data-parallel reduction is ONE
 * all-reduce of n*(K + K*C) floats instead of n (`:163`).  `indices` as written by hilc_rvq_encode (rows =
 * index_rows >= n), `codebooks` = the tables the indices were computed with.  Deterministic (no atomics).
 * hilc_rvq_ema_update: ema_num = ema_num*decay + counts*(1-decay); ema_embed likewise; embed = ema_embed/ema_num
 * (`ema_inplace` `:16-17`, `:165-169`), in place on `[n][K]` / `[n][K][C]` tensors. */
int hilc_rvq_ema_stats(const float* z, const float* codebooks, const int64_t* indices, float* bucket, int B, int C,
                       int T, int K, int n, int index_rows, int channel_last, int stage_major, void* stream);
int hilc_rvq_ema_update(float* embed, float* ema_num, float* ema_embed, const float* bucket, double decay, int K,
                        int C, int n, void* stream);

/* ---- row layouts, codes and limits of the per-slot entry points below (ABI 16) -----------------------------------------------------
 * The one definition of every small int32 row, code and limit that the kernels (hilcodec_amd/csrc), the bindings and the bit-exact
 * host models share.  HILC_<MODULE>_<NAME> is hilcodec_amd.<module>.<NAME> in Python, value for value (tests/test_api_cpu.py proves
 * the mirror in both directions).  A "row" is one slot's int32 words; a [B][WORDS] tensor holds the rows of B slots back to back. */

/* control rows of a hop, int32 [B].  Action row (hilc_state_slots_apply and every kernel that takes `action`): KEEP, ZERO = start a
 * fresh stream, r >= LOAD = load record r - LOAD.  Hold row (hilc_state_slots_hold and every kernel that takes `hold`): ADVANCE, HELD,
 * and on the receiver SID = a SID arrived, SILENT = the stream is in DTX (both: comfort noise; every other kernel treats them as held). */
#define HILC_SESSIONS_ACTION_KEEP 0
#define HILC_SESSIONS_ACTION_ZERO (-1)
#define HILC_SESSIONS_ACTION_LOAD 1
#define HILC_SESSIONS_HOLD_ADVANCE 0
#define HILC_SESSIONS_HOLD_HELD 1
#define HILC_SESSIONS_HOLD_SID 2
#define HILC_SESSIONS_HOLD_SILENT 3

/* wire format (hilcodec_amd/wire.py).  A packet holds at most MAX_STAGES stages, primary + redundant.  Transport header: TRANSPORT_HEADER
 * bytes, bytes 0-1 the hop index mod 2^16 big-endian, byte 2 = SID_BIT | FEC_BIT | n in N_MASK, RSV_BIT zero.  A receiver report is
 * REPORT_BYTES bytes (seq, loss_q8, residual_q8), a NACK NACK_BYTES bytes (base and bitmap, big-endian).  Concealment row of a receiver slot, n_max + CONCEAL_CODES words: RUN = hops lost in a
 * row (0..F), HAS = has-codes (0/1), N = stored n, CODES + s for s < n_max = the code of stage s of the LAST frame of the last packet
 * received (0 for s >= stored n). */
#define HILC_WIRE_MAX_STAGES 32
#define HILC_WIRE_TRANSPORT_HEADER 3
#define HILC_WIRE_SID_BIT 0x80
#define HILC_WIRE_FEC_BIT 0x40
#define HILC_WIRE_RSV_BIT 0x20
#define HILC_WIRE_N_MASK 0x1F
#define HILC_WIRE_REPORT_BYTES 3
#define HILC_WIRE_NACK_BYTES 4
#define HILC_WIRE_CAP_BYTES 3
#define HILC_WIRE_SRTP_TAG_BYTES 10
#define HILC_WIRE_CONCEAL_RUN 0
#define HILC_WIRE_CONCEAL_HAS 1
#define HILC_WIRE_CONCEAL_N 2
#define HILC_WIRE_CONCEAL_CODES 3

/* samples per codec frame at 24 kHz (hilcodec_amd/resample.py): a hop of T frames is HOP T samples */
#define HILC_RESAMPLE_HOP 320

/* DTX and comfort noise (hilcodec_amd/dtx.py).  Kind of a sender's hop: HELD, SPEECH, SID, SILENT.  Order K <= MAX_ORDER, level L in
 * 0..LEVELS - 1, GOLDEN the multiplier of a slot's noise seed.  CN state row of a receiver slot, ST_Q + 2 K words: ST_HAS = has-SID,
 * ST_LEVEL = L, ST_COUNT = c (noise hops since the start, mod 2^32), ST_Q + i for i < K = q_{i+1}, then K fp32 words of filter memory
 * y[-K..-1]. */
#define HILC_DTX_HELD 0
#define HILC_DTX_SPEECH 1
#define HILC_DTX_SID 2
#define HILC_DTX_SILENT 3
#define HILC_DTX_MAX_ORDER 16
#define HILC_DTX_LEVELS 128
#define HILC_DTX_GOLDEN 0x9E3779B9u
#define HILC_DTX_ST_HAS 0
#define HILC_DTX_ST_LEVEL 1
#define HILC_DTX_ST_COUNT 2
#define HILC_DTX_ST_Q 3

/* jitter buffer (hilcodec_amd/jitter.py).  State row, ST_WORDS words: ST_ANCHORED, ST_WAIT, ST_NEXT (the playout clock), ST_IN_DTX,
 * ST_MASK (bit i: ring entry i occupied), then the counters STAT_*.  Meta word of a ring entry: h | META_SID | META_FEC |
 * n << META_N_SHIFT, 0 when free.  Adapt row, AD_WORDS words: a slot's debt, pending shift, stale windows, window minimum and count,
 * outlier run and its last h, the last full window's margin, then the counters AD_GROWN .. AD_RESYNC. */
#define HILC_JITTER_ST_ANCHORED 0
#define HILC_JITTER_ST_WAIT 1
#define HILC_JITTER_ST_NEXT 2
#define HILC_JITTER_ST_IN_DTX 3
#define HILC_JITTER_ST_MASK 4
#define HILC_JITTER_STAT_ACCEPTED 5
#define HILC_JITTER_STAT_DUPLICATE 6
#define HILC_JITTER_STAT_LATE 7
#define HILC_JITTER_STAT_EARLY 8
#define HILC_JITTER_STAT_MALFORMED 9
#define HILC_JITTER_STAT_DECODED 10
#define HILC_JITTER_STAT_FEC 11
#define HILC_JITTER_STAT_LOST 12
#define HILC_JITTER_STAT_NOISE 13
#define HILC_JITTER_ST_WORDS 14
#define HILC_JITTER_META_SID (1 << 16)
#define HILC_JITTER_META_FEC (1 << 17)
#define HILC_JITTER_META_N_SHIFT 18
#define HILC_JITTER_AD_DEBT 0
#define HILC_JITTER_AD_PENDING 1
#define HILC_JITTER_AD_STALE 2
#define HILC_JITTER_AD_MIN 3
#define HILC_JITTER_AD_COUNT 4
#define HILC_JITTER_AD_RUN 5
#define HILC_JITTER_AD_LAST 6
#define HILC_JITTER_AD_MARGIN 7
#define HILC_JITTER_AD_GROWN 8
#define HILC_JITTER_AD_SHRUNK 9
#define HILC_JITTER_AD_FORCED 10
#define HILC_JITTER_AD_RESYNC 11
#define HILC_JITTER_AD_WORDS 12

/* per-room mixing (hilcodec_amd/mixer.py): the most speakers of a room; the limiter's sub-frame (LimitConfig.sub) in samples, and the
 * longest hop it takes (at most HILC_MIXER_MAX_LIMIT_L / HILC_MIXER_MIN_SUB = 512 sub-frames) */
#define HILC_MIXER_MAX_TOP_K 8
#define HILC_MIXER_MIN_SUB 16
#define HILC_MIXER_MAX_SUB 512
#define HILC_MIXER_MAX_LIMIT_L 8192

/* receiver reports and loss-adaptive FEC (hilcodec_amd/report.py).  Report row, RP_WORDS words: RP_SEQ, RP_LOSS, RP_RESIDUAL (the
 * last report), RP_PHASE, RP_N, RP_F, RP_L, RP_HEAD (the interval phase, the window's counts and head), RP_DECODED .. RP_NOISE (the
 * remembered jitter counters), RP_REPORTS, then RP_RING_WORDS ring words from RP_RING, 2 bits per hop: CLASS_*.  FEC-adapt row,
 * FA_WORDS words: FA_ON, FA_CALM, FA_SEEN, FA_LAST (seq), FA_AGE, FA_LOSS, FA_RESIDUAL, then the counters FA_REPORTS .. FA_TIMEOUT.
 * A report travels to the sender's graph as one word: REPORT_PRESENT | seq << 16 | loss_q8 << 8 | residual_q8, 0 for none. */
#define HILC_REPORT_RP_SEQ 0
#define HILC_REPORT_RP_LOSS 1
#define HILC_REPORT_RP_RESIDUAL 2
#define HILC_REPORT_RP_PHASE 3
#define HILC_REPORT_RP_N 4
#define HILC_REPORT_RP_F 5
#define HILC_REPORT_RP_L 6
#define HILC_REPORT_RP_HEAD 7
#define HILC_REPORT_RP_DECODED 8
#define HILC_REPORT_RP_FEC 9
#define HILC_REPORT_RP_LOST 10
#define HILC_REPORT_RP_NOISE 11
#define HILC_REPORT_RP_REPORTS 12
#define HILC_REPORT_RP_RING 13
#define HILC_REPORT_RP_RING_WORDS 16
#define HILC_REPORT_RP_WORDS (HILC_REPORT_RP_RING + HILC_REPORT_RP_RING_WORDS)
#define HILC_REPORT_CLASS_NONE 0
#define HILC_REPORT_CLASS_D 1
#define HILC_REPORT_CLASS_F 2
#define HILC_REPORT_CLASS_L 3
#define HILC_REPORT_CLASS_NOISE 4
#define HILC_REPORT_FA_ON 0
#define HILC_REPORT_FA_CALM 1
#define HILC_REPORT_FA_SEEN 2
#define HILC_REPORT_FA_LAST 3
#define HILC_REPORT_FA_AGE 4
#define HILC_REPORT_FA_LOSS 5
#define HILC_REPORT_FA_RESIDUAL 6
#define HILC_REPORT_FA_REPORTS 7
#define HILC_REPORT_FA_STALE 8
#define HILC_REPORT_FA_TURNED_ON 9
#define HILC_REPORT_FA_TURNED_OFF 10
#define HILC_REPORT_FA_TIMEOUT 11
#define HILC_REPORT_FA_WORDS 12
#define HILC_REPORT_REPORT_PRESENT (1 << 24)

/* NACK and retransmission (hilcodec_amd/rtx.py).  NACK row of a receiver slot, NK_WORDS words: the counters NK_SENT, NK_ASKED,
 * NK_RECOVERED, NK_EXPIRED, then NK_RING_WORDS entry words from NK_RING, indexed like the jitter ring by h mod capacity: h | count << 16
 * | age << 24, 0 when free.  Counter row of a sender slot, RX_WORDS words: RX_STORED, RX_REQUESTS, RX_SENT, RX_MISS, RX_DROPPED; a tag
 * word of its history is h | nbytes << 16, 0 when empty; at most MAX_HISTORY entries and MAX_PER_HOP retransmissions per hop.  A NACK
 * travels to the sender's graph as two words: NACK_PRESENT | base and the bitmap, (0, 0) for none. */
#define HILC_RTX_NK_SENT 0
#define HILC_RTX_NK_ASKED 1
#define HILC_RTX_NK_RECOVERED 2
#define HILC_RTX_NK_EXPIRED 3
#define HILC_RTX_NK_RING 4
#define HILC_RTX_NK_RING_WORDS 32
#define HILC_RTX_NK_WORDS (HILC_RTX_NK_RING + HILC_RTX_NK_RING_WORDS)
#define HILC_RTX_RX_STORED 0
#define HILC_RTX_RX_REQUESTS 1
#define HILC_RTX_RX_SENT 2
#define HILC_RTX_RX_MISS 3
#define HILC_RTX_RX_DROPPED 4
#define HILC_RTX_RX_WORDS 5
#define HILC_RTX_NACK_PRESENT (1 << 16)
#define HILC_RTX_MAX_HISTORY 64
#define HILC_RTX_MAX_PER_HOP 4

/* report-driven rate control (hilcodec_amd/rate.py).  Rate row of a sender slot, RC_WORDS words: RC_RATE_Q8 (bits per hop x 256),
 * RC_CREDIT (the token bucket, in bits; it may be in debt), RC_SEEN, RC_LAST (seq), RC_AGE, RC_LOSS (the report memory), then the
 * counters RC_REPORTS .. RC_LIMITED.  A rate is at most MAX_RATE_BITS bits per hop. */
#define HILC_RATE_RC_RATE_Q8 0
#define HILC_RATE_RC_CREDIT 1
#define HILC_RATE_RC_SEEN 2
#define HILC_RATE_RC_LAST 3
#define HILC_RATE_RC_AGE 4
#define HILC_RATE_RC_LOSS 5
#define HILC_RATE_RC_REPORTS 6
#define HILC_RATE_RC_STALE 7
#define HILC_RATE_RC_DECREASED 8
#define HILC_RATE_RC_INCREASED 9
#define HILC_RATE_RC_TIMEOUT 10
#define HILC_RATE_RC_LIMITED 11
#define HILC_RATE_RC_WORDS 12
#define HILC_RATE_MAX_RATE_BITS (1 << 22)

/* delay-based bandwidth estimate (hilcodec_amd/bwe.py).  Estimate row of a receiver slot, BW_WORDS words: BW_RATE_Q8 (the estimate, bits
 * per hop x 256), BW_THR (the detector's adaptive threshold, Q16), BW_SEEN, BW_LAST_H, BW_LAST_T (the last sampled arrival: hop index and
 * tick), BW_ACC, BW_SM (the accumulated delay in ticks, smoothed in Q8), BW_COUNT, BW_PREV_M, BW_OVER_TICKS, BW_OVER_COUNT, BW_SIGNAL
 * (SIGNAL_*), BW_STATE (STATE_*), BW_PHASE, BW_SEQ (the cap's clock), BW_N, BW_HEAD, BW_RN, BW_RHEAD (the two rings' fill and next entry),
 * the counters BW_SAMPLES .. BW_CAPS, then the trend ring at BW_TREND (MAX_WINDOW pairs tick, smoothed delay) and the rate ring at BW_RING
 * (MAX_WINDOW pairs tick, bits).  Cap row of a sender slot, CP_WORDS words: CP_CAP_Q8, CP_SEEN, CP_LAST (seq), CP_AGE, then the counters
 * CP_CAPS .. CP_CLAMPED.  A cap travels to the sender's graph as one word: CAP_PRESENT | seq << 16 | cap_bits, 0 for none. */
#define HILC_BWE_BW_RATE_Q8 0
#define HILC_BWE_BW_THR 1
#define HILC_BWE_BW_SEEN 2
#define HILC_BWE_BW_LAST_H 3
#define HILC_BWE_BW_LAST_T 4
#define HILC_BWE_BW_ACC 5
#define HILC_BWE_BW_SM 6
#define HILC_BWE_BW_COUNT 7
#define HILC_BWE_BW_PREV_M 8
#define HILC_BWE_BW_OVER_TICKS 9
#define HILC_BWE_BW_OVER_COUNT 10
#define HILC_BWE_BW_SIGNAL 11
#define HILC_BWE_BW_STATE 12
#define HILC_BWE_BW_PHASE 13
#define HILC_BWE_BW_SEQ 14
#define HILC_BWE_BW_N 15
#define HILC_BWE_BW_HEAD 16
#define HILC_BWE_BW_RN 17
#define HILC_BWE_BW_RHEAD 18
#define HILC_BWE_BW_SAMPLES 19
#define HILC_BWE_BW_OLD 20
#define HILC_BWE_BW_RESET 21
#define HILC_BWE_BW_MALFORMED 22
#define HILC_BWE_BW_OVERUSE 23
#define HILC_BWE_BW_UNDERUSE 24
#define HILC_BWE_BW_DECREASED 25
#define HILC_BWE_BW_INCREASED 26
#define HILC_BWE_BW_CAPS 27
#define HILC_BWE_BW_TREND 28
#define HILC_BWE_MAX_WINDOW 32
#define HILC_BWE_BW_RING 92
#define HILC_BWE_BW_WORDS 156
#define HILC_BWE_HOP_TICKS 320
#define HILC_BWE_SIGNAL_NORMAL 0
#define HILC_BWE_SIGNAL_OVERUSE 1
#define HILC_BWE_SIGNAL_UNDERUSE 2
#define HILC_BWE_STATE_HOLD 0
#define HILC_BWE_STATE_INCREASE 1
#define HILC_BWE_THR_START (25 << 15)
#define HILC_BWE_THR_MIN (6 << 16)
#define HILC_BWE_THR_MAX (600 << 16)
#define HILC_BWE_THR_SKIP (15 << 16)
#define HILC_BWE_K_UP 6082
#define HILC_BWE_K_DOWN 27263
#define HILC_BWE_OVER_TICKS 240
#define HILC_BWE_ADAPT_TICKS 2400
#define HILC_BWE_COUNT_MAX 60
#define HILC_BWE_RATE_MIN 4
#define HILC_BWE_ACC_MAX (1 << 20)
#define HILC_BWE_SLOPE_MAX (1 << 22)
#define HILC_BWE_MAX_RESET_TICKS (1 << 17)
#define HILC_BWE_MAX_FRAMES 1024
#define HILC_BWE_MAX_ROW_BYTES (1 << 15)
#define HILC_BWE_MAX_CAP_BITS 65535
#define HILC_BWE_CP_CAP_Q8 0
#define HILC_BWE_CP_SEEN 1
#define HILC_BWE_CP_LAST 2
#define HILC_BWE_CP_AGE 3
#define HILC_BWE_CP_CAPS 4
#define HILC_BWE_CP_STALE 5
#define HILC_BWE_CP_TIMEOUT 6
#define HILC_BWE_CP_CLAMPED 7
#define HILC_BWE_CP_WORDS 8
#define HILC_BWE_CAP_PRESENT (1 << 24)

/* SRTP packet protection (hilcodec_amd/srtp.py), RFC 3711's AES_CM_128_HMAC_SHA1_80.  Key row of a slot, KEY_WORDS words, every word a
 * big-endian uint32 held in an int32: KEY_VALID (1: the slot has a key), KEY_SSRC, KEY_ROC (the rollover counter a start gives the slot's
 * row), the 44 AES round-key words of the session encryption key from KEY_RK, the 14-byte session salt and 2 zero bytes as 4 words from
 * KEY_SALT, and the HMAC-SHA1 midstates after the blocks k_a ^ ipad and k_a ^ opad, 5 words each, from KEY_INNER and KEY_OUTER.  Sender
 * row, TX_WORDS words: TX_ROC, TX_LAST (the last SEQ sent), TX_SENT, then the counters TX_PROTECTED, TX_NOKEY.  Receiver row, RX_WORDS
 * words: RX_ROC, RX_SL (the highest authenticated SEQ), RX_SEEN, RX_WIN_LO, RX_WIN_HI (the 64-packet replay window: bit k is the packet k
 * below the highest authenticated index), then the counters RX_OK, RX_AUTH_FAIL, RX_REPLAY, RX_SHORT, RX_NOKEY. */
#define HILC_SRTP_KEY_VALID 0
#define HILC_SRTP_KEY_SSRC 1
#define HILC_SRTP_KEY_ROC 2
#define HILC_SRTP_KEY_RK 3
#define HILC_SRTP_KEY_SALT 47
#define HILC_SRTP_KEY_INNER 51
#define HILC_SRTP_KEY_OUTER 56
#define HILC_SRTP_KEY_WORDS 61
#define HILC_SRTP_TX_ROC 0
#define HILC_SRTP_TX_LAST 1
#define HILC_SRTP_TX_SENT 2
#define HILC_SRTP_TX_PROTECTED 3
#define HILC_SRTP_TX_NOKEY 4
#define HILC_SRTP_TX_WORDS 5
#define HILC_SRTP_RX_ROC 0
#define HILC_SRTP_RX_SL 1
#define HILC_SRTP_RX_SEEN 2
#define HILC_SRTP_RX_WIN_LO 3
#define HILC_SRTP_RX_WIN_HI 4
#define HILC_SRTP_RX_OK 5
#define HILC_SRTP_RX_AUTH_FAIL 6
#define HILC_SRTP_RX_REPLAY 7
#define HILC_SRTP_RX_SHORT 8
#define HILC_SRTP_RX_NOKEY 9
#define HILC_SRTP_RX_WORDS 10
#define HILC_SRTP_WINDOW 64
#define HILC_SRTP_MAX_ROW_BYTES (1 << 15)

/* SRTP on the forwarding hop's routes (hilcodec_amd/forward_srtp.py).  Route row of a (listener, route), RT_WORDS words: RT_EPOCH (the
 * restarts of the route's stream: its SSRC is the key row's KEY_SSRC + HILC_FORWARD_MAX_FANOUT * RT_EPOCH + route), the index state
 * RT_ROC, RT_SL, RT_SEEN (0: nothing sent since the restart, 1: sent, SEEN_EXHAUSTED: restarted at MAX_EPOCH, sends nothing more),
 * RT_WIN_LO, RT_WIN_HI (the receiver row's meaning: bit k is the index k below the highest one sent), then the counters RT_PROTECTED,
 * RT_NOKEY, RT_STALE, RT_EXHAUSTED. */
#define HILC_FSRTP_RT_EPOCH 0
#define HILC_FSRTP_RT_ROC 1
#define HILC_FSRTP_RT_SL 2
#define HILC_FSRTP_RT_SEEN 3
#define HILC_FSRTP_RT_WIN_LO 4
#define HILC_FSRTP_RT_WIN_HI 5
#define HILC_FSRTP_RT_PROTECTED 6
#define HILC_FSRTP_RT_NOKEY 7
#define HILC_FSRTP_RT_STALE 8
#define HILC_FSRTP_RT_EXHAUSTED 9
#define HILC_FSRTP_RT_WORDS 10
#define HILC_FSRTP_SEEN_EXHAUSTED 2
#define HILC_FSRTP_MAX_EPOCH ((1 << 28) - 1)

/* selective forwarding (hilcodec_amd/forward.py).  Sender row of a slot, SD_WORDS words: SD_HANG (the hops it stays active, 0: not
 * active), SD_SINCE (the hops it has been active, at most 65535), then the counters SD_CODES, SD_SIDS, SD_MALFORMED, SD_OVERFLOW.
 * Listener row of a slot, LR_WORDS words: the counters LR_PACKETS, LR_BYTES, LR_TRIMMED, LR_SWITCHES.  A listener has at most
 * MAX_FANOUT routes, a sender at most MAX_BURST forwarded arrivals per hop, and stays active at most MAX_HANG_HOPS hops. */
#define HILC_FORWARD_SD_HANG 0
#define HILC_FORWARD_SD_SINCE 1
#define HILC_FORWARD_SD_CODES 2
#define HILC_FORWARD_SD_SIDS 3
#define HILC_FORWARD_SD_MALFORMED 4
#define HILC_FORWARD_SD_OVERFLOW 5
#define HILC_FORWARD_SD_WORDS 6
#define HILC_FORWARD_LR_PACKETS 0
#define HILC_FORWARD_LR_BYTES 1
#define HILC_FORWARD_LR_TRIMMED 2
#define HILC_FORWARD_LR_SWITCHES 3
#define HILC_FORWARD_LR_WORDS 4
#define HILC_FORWARD_MAX_FANOUT 8
#define HILC_FORWARD_MAX_BURST 4
#define HILC_FORWARD_MAX_HANG_HOPS 255
#define HILC_FORWARD_MAX_SINCE 65535

/* downlink control of the forwarding hop (hilcodec_amd/downlink.py).  Listener row of a slot, DL_WORDS words: DL_RATE_Q8 (bits per hop x
 * 256), DL_CREDIT (the bucket, bits), DL_AGE (hops since the last accepted report), DL_LOSS (the loss_q8 the rate last followed),
 * DL_LAYERS (the layers of the last hop's rows), then the counters.  One memory word per (listener, route): MEM_SEEN | last << 8 |
 * loss_q8, 0 when cleared.  Counter row of a sender's history, DS_WORDS words: DS_STORED, DS_REPLACED.  A history holds at most
 * MAX_HISTORY packets, a listener is sent at most MAX_PER_HOP retransmissions per hop. */
#define HILC_DOWNLINK_DL_RATE_Q8 0
#define HILC_DOWNLINK_DL_CREDIT 1
#define HILC_DOWNLINK_DL_AGE 2
#define HILC_DOWNLINK_DL_LOSS 3
#define HILC_DOWNLINK_DL_LAYERS 4
#define HILC_DOWNLINK_DL_REPORTS 5
#define HILC_DOWNLINK_DL_STALE 6
#define HILC_DOWNLINK_DL_DECREASED 7
#define HILC_DOWNLINK_DL_INCREASED 8
#define HILC_DOWNLINK_DL_TIMEOUT 9
#define HILC_DOWNLINK_DL_LIMITED 10
#define HILC_DOWNLINK_DL_PACKETS 11
#define HILC_DOWNLINK_DL_BYTES 12
#define HILC_DOWNLINK_DL_TRIMMED 13
#define HILC_DOWNLINK_DL_NACK_STALE 14
#define HILC_DOWNLINK_DL_REQUESTS 15
#define HILC_DOWNLINK_DL_RTX_SENT 16
#define HILC_DOWNLINK_DL_RTX_MISS 17
#define HILC_DOWNLINK_DL_RTX_DROPPED 18
#define HILC_DOWNLINK_DL_WORDS 19
#define HILC_DOWNLINK_DS_STORED 0
#define HILC_DOWNLINK_DS_REPLACED 1
#define HILC_DOWNLINK_DS_WORDS 2
#define HILC_DOWNLINK_MEM_SEEN (1 << 16)
#define HILC_DOWNLINK_MAX_HISTORY 64
#define HILC_DOWNLINK_MAX_PER_HOP 4

/* audio level and level-based speaker selection of the forwarding hop (hilcodec_amd/audio_level.py).  Speaker row of a slot, WORDS
 * words: SCORE (the smoothed loudness, 256 x (128 - level), in [0, 256 MAX_LOUD]), RANK (its place in its room on the previous hop's
 * keys, -1: none), STAGE (1: among the first `fanout`), then the counters LEVELLED (codes hops that came with a level) and STAGED.  A
 * loudness is 128 - level in [1, MAX_LOUD], 0: no level on this hop. */
#define HILC_SPEAKER_SCORE 0
#define HILC_SPEAKER_RANK 1
#define HILC_SPEAKER_STAGE 2
#define HILC_SPEAKER_LEVELLED 3
#define HILC_SPEAKER_STAGED 4
#define HILC_SPEAKER_WORDS 5
#define HILC_SPEAKER_MAX_LOUD 128
#define HILC_SPEAKER_MAX_ATTACK_SHIFT 4
#define HILC_SPEAKER_MAX_DECAY_Q8 32768
#define HILC_SPEAKER_MAX_MARGIN_DB 32

/* ---- per-stream session state of a streaming hop (ABI 16) ------------------------------------------------------------------
 * Layout: the caches of `streams` streams live in ONE fp32 block (hilcodec_amd/graph_step.py StateBlock): slice k (one
 * `[streams][C][L]` cache tensor, k < nslices, in the reference's order: 22 encoder then 30 decoder caches) starts at
 * block + slice_off[k], and stream b's part of it is the slice_len[k] = C*L floats at block + slice_off[k] + b * slice_len[k].
 * slice_off (int64) and slice_len (int32) are DEVICE arrays of nslices entries, built once per block.  A "record" is one
 * stream's nslices parts concatenated in order: sum(slice_len) floats (76 479 for both shipped models), records packed back to
 * back.  The reference's caches start at zero (`causal_layers.py:56-58,131-133,156-158`) and the codec keeps no other per-stream
 * state, so zeroing a stream's parts starts a fresh stream there and loading a record resumes one.
 * hilc_state_slots_apply: action[b] (int32, device, `streams` entries) = HILC_SESSIONS_ACTION_KEEP, _ZERO (zero stream b) or r >= _LOAD: copy record r - _LOAD of
 * `records` (nrecords records; may be NULL when nrecords == 0) into stream b; any other value: keep.  Meant to run at the head
 * of every hop (captured in its graph): a fixed grid that leaves after one barrier when no action is set.
 * hilc_state_slots_gather: record i of `records` = the current state of stream slots[i] (int32, device, i < nslots); a slot
 * outside [0, streams) leaves its record untouched.  Both: every slice must lie inside `block` (not checked: device tables);
 * nslices <= 128 (the table is staged in LDS), else HILC_ERR_UNSUPPORTED. */
int hilc_state_slots_apply(float* block, const int64_t* slice_off, const int* slice_len, int nslices, int streams,
                           const int* action, const float* records, int nrecords, void* stream);
int hilc_state_slots_gather(const float* block, const int64_t* slice_off, const int* slice_len, int nslices, int streams,
                            const int* slots, int nslots, float* records, void* stream);

/* ---- held streams of a streaming hop (additive under ABI 16) -------------------------------------------------------------------
 * One entry point added WITHOUT a version bump, as the packet entry points below: it changes no existing signature or struct.
 * hilc_state_slots_hold: for every stream b with hold[b] != 0 (int32, device, `streams` entries): its slices are copied from `src`
 * (the block the hop read) to `dst` (the block it wrote), in the layout of hilc_state_slots_apply, so the stream leaves the hop
 * exactly as it entered it; and its output rows are set: wav[b][0..wav_len) = 0 (fp32 [streams][wav_len]), indices[s][b][t] = -1
 * for s < n_max, t < frames (int64 [n_max][streams][frames]), packets[b][0..stride) = 0 (uint8 [streams][stride]), nbytes[b] = 0
 * (int32 [streams]).  Each output pointer may be NULL (that output is not touched); a non-NULL one with its length <= 0:
 * HILC_ERR_SHAPE.  Meant to run at the tail of every hop (captured in its graph, after the last write to `dst` and to the
 * outputs): a fixed grid that leaves after one barrier when no entry of `hold` is set.  nslices <= 128, else HILC_ERR_UNSUPPORTED. */
int hilc_state_slots_hold(const float* src, float* dst, const int64_t* slice_off, const int* slice_len, int nslices, int streams,
                          const int* hold, float* wav, int wav_len, int64_t* indices, int n_max, int frames, uint8_t* packets,
                          int stride, int* nbytes, void* stream);

/* ---- per-stream 10-bit packets of a streaming hop (additive under ABI 16) ------------------------------------------------------
 * Two entry points added WITHOUT a version bump: they change no existing signature or struct, so a binding of ABI 16 that does
 * not use them is unaffected; binders find them by symbol (dlsym), not by version.
 * Packet of stream b for one hop of T frames: its first n_b stages x T codes, stage-major (stage 0's T frames first), 10 bits per
 * code, MSB first, the last byte zero-padded — ceil(10 n_b T / 8) bytes, the body of hilcodec_amd/wire.py pack_indices_10bit(
 * indices[:n_b, b:b+1, :]) without its header.  A batch is `packets` uint8 [B][stride], stride = ceil(10 n_max T / 8), with row b's
 * bytes past its own length set to zero.  n_per_stream: optional int32 [B] (device; NULL = n_max for every stream), each entry
 * clamped to [1, n_max] as hilc_rvq_decode_mixed clamps n_per_clip.
 * hilc_pack_codes_10bit: indices int64 [n_max][B][T] (stage-major, as hilc_rvq_encode_mixed writes them; rows >= n_b are not read)
 * -> packets [B][stride] and nbytes int32 [B] (stream b's packet length).  A code outside [0, 1024) in a row < n_b is clamped into
 * it, as hilc_rvq_decode clamps its indices.  n_max < 1: HILC_ERR_RANGE.
 * hilc_rvq_decode_packed: the dequantiser read straight from packets -> q [B][T][C] (channel-last: what the streaming Dequantizer
 * hands the decoder), bit-identical to hilc_rvq_decode_mixed(channel_last = 1, stage_major = 1) on the unpacked indices (same
 * per-element sum in stage order).  codebooks [Nq][K][C]; n_max outside 1..Nq: HILC_ERR_RANGE; K != 1024 or n_max > HILC_WIRE_MAX_STAGES:
 * HILC_ERR_UNSUPPORTED. */
int hilc_pack_codes_10bit(const int64_t* indices, const int* n_per_stream, uint8_t* packets, int* nbytes, int B, int T, int n_max,
                          void* stream);
int hilc_rvq_decode_packed(const uint8_t* packets, const int* n_per_stream, const float* codebooks, float* q, int B, int C, int T,
                           int K, int Nq, int n_max, void* stream);

/* ---- loss concealment of the packet receiver (additive under ABI 16) ------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the packet entry points above.  A receiving hop of B streams, T frames and
 * packets of at most n_max stages (layout of hilc_rvq_decode_packed) keeps per stream b one int32 state row of n_max +
 * HILC_WIRE_CONCEAL_CODES words (HILC_WIRE_CONCEAL_*: run k, has-codes, stored n, the last frame's codes).  All zero = a fresh stream.  F = fade_hops >= 1.
 * hilc_conceal_prepare, at the head of the hop (after hilc_state_slots_apply, before hilc_rvq_decode_packed), per stream b, every
 * array int32 [B] on the device unless named otherwise:
 *   action[b] != 0 (a start or a resume on this hop, the action row of hilc_state_slots_apply): the state row is zeroed first;
 *   hold[b] != 0: nothing else (ramp[b] = 0);
 *   else lost[b] == 0 (received): the row stores the packet's last frame (stage s < n_b, n_b = n_per_stream[b] clamped to
 *     [1, n_max]) and n_b, has-codes 1, run 0; ramp[b] = -k if the run k was >= 1, else 0;
 *   else (lost) with has-codes and k < F: packets[b][0..stride) (uint8 [B][stride], stride = ceil(10 n_max T / 8)) is rewritten
 *     as the stored codes repeated over T frames in the 10-bit packet layout, n_per_stream[b] = stored n, run k + 1,
 *     ramp[b] = k + 1;
 *   else (lost, nothing received since the start, or k = F): hold[b] = 1 (hilc_state_slots_hold keeps the stream), ramp[b] = 0.
 * A stored run > F counts as F, a stored n is clamped to [1, n_max] and codes to 10 bits.  n_max or fade_hops < 1:
 * HILC_ERR_RANGE; n_max > HILC_WIRE_MAX_STAGES: HILC_ERR_UNSUPPORTED.
 * hilc_conceal_gain, after the decoder (before hilc_state_slots_hold): for each stream with ramp[b] in 1..F (a = ramp - 1,
 * c = ramp) or in -F..-1 (a = -ramp, c = 0), wav[b][s] (fp32 [B][samples]) *= gains[a] + (gains[c] - gains[a]) * weights[s], every
 * operation rounded on its own in fp32 (no contraction); gains fp32 [F + 1], weights fp32 [samples].  Any other ramp value: the row
 * is not touched.  Both: one wave per stream; fade_hops < 1: HILC_ERR_RANGE. */
int hilc_conceal_prepare(int* state, const int* action, int* hold, const int* lost, int* n_per_stream, uint8_t* packets, int* ramp,
                         int B, int T, int n_max, int fade_hops, void* stream);
int hilc_conceal_gain(float* wav, const int* ramp, const float* gains, const float* weights, int B, int samples, int fade_hops,
                      void* stream);

/* ---- sample-rate conversion at the codec's input and output (additive under ABI 16) --------------------------------------------
 * One entry point added WITHOUT a version bump, as the packet and concealment entry points above.  It replaces the reference's
 * `librosa.load(PATH, sr=sr)` (test_onnx.py:52, scripts/inference.ipynb), which resamples an input file to the model's rate, with the
 * project's own polyphase converter (hilcodec_amd/resample.py designs the filter and states the definition).
 * hilc_resample_poly: x fp32 [B][T_in] at the input rate -> y fp32 [B][T_out], T_out = ceil(T_in L / M), the rate ratio L / M in
 * lowest terms; taps fp32 [L][Q] phase-major (taps[p Q + j] = h[p + j L]).  For output m, ph = (m M) mod L, base = (m M - ph) / L:
 *   y[m] = sum_{j = 0 .. Q-1} taps[ph][j] * x[base - j], summed in order of j from 0.0f, each product and sum rounded on its own;
 * x[i < 0] = hist_in[b][Q - 1 + i] (fp32 [B][Q - 1]; NULL = zeros).  hist_out (fp32 [B][Q - 1]; NULL = not written) receives the
 * last Q - 1 samples of hist_in || x; it must not be hist_in (a hop reads one block and writes the other).  NULL x, y or taps:
 * HILC_ERR_NULL; B, T_in, L or M <= 0, Q < 2 or hist_out == hist_in: HILC_ERR_SHAPE; a filter too long for the kernel's LDS tiles
 * (more than 64 KiB for TILE = 64 outputs of 16 streams: every rate pair of resample.py fits with room to spare): HILC_ERR_UNSUPPORTED. */
int hilc_resample_poly(const float* x, const float* hist_in, float* hist_out, float* y, const float* taps, int B, int T_in, int L, int M,
                       int Q, void* stream);

/* ---- in-band forward error correction of the packet sender and receiver (additive under ABI 16) --------------------------------
 * Two entry points added WITHOUT a version bump, as the packet, concealment and resampling entry points above.  With m redundant
 * stages (1 <= m <= n_max, n_max + m <= HILC_WIRE_MAX_STAGES, else HILC_ERR_RANGE / HILC_ERR_UNSUPPORTED), the packet of stream b for hop k is the
 * 10-bit packet (layout of hilc_pack_codes_10bit) of the n_b + m stages cat(idx_k[:n_b, b], idx_{k-1}[:m, b]) — the primary codes
 * first, unchanged, then the first m stages of the stream's previous encoded hop — ceil(10 (n_b + m) T / 8) bytes; a stream without
 * a previous encoded hop sends the plain packet of its n_b stages.  A batch is uint8 [B][stride], stride = ceil(10 (n_max + m) T / 8),
 * row b zero past its length.
 * hilc_pack_codes_10bit_fec: indices int64 [n_max][B][T] as hilc_pack_codes_10bit (codes clamped into [0, 1024)); n_per_stream
 * optional int32 [B] (NULL = n_max), each entry clamped to [m, n_max]; prev_in and prev_out distinct int32 [B][1 + m T] rows of the
 * previous codes, [0] valid (0/1), [1 + s T + t] the code of stage s, frame t (the hop reads one, writes the other); action and hold
 * optional int32 [B] (NULL = 0): the action row of hilc_state_slots_apply and the hold row of hilc_state_slots_hold.  Per stream b:
 *   the input row counts as all zero if action[b] != 0 (a start or a resume: no previous hop);
 *   hold[b] != 0: prev_out[b] = that input row, packets[b] = 0, nbytes[b] = 0;
 *   else packets[b] = the packet above with the redundant section iff the input row is valid, nbytes[b] = its length, and
 *   prev_out[b] = {1, idx[s][b][t] clamped, s < m}.
 * hilc_fec_select: the receiver's compaction before hilc_conceal_prepare / hilc_rvq_decode_packed.  packets uint8 [B][stride] as
 * above, fec int32 [B], n_per_stream int32 [B] (in place) -> out uint8 [B][ceil(10 n_max T / 8)].  Per stream b: fec[b] == 0: out[b]
 * = the primary section of n_b = n_per_stream[b] clamped to [1, n_max] stages (the bits of its last byte past 10 n_b T zeroed);
 * fec[b] != 0 (the row holds the NEXT hop's packet, n_b its primary stage count, clamped to [m, n_max]): out[b] = the redundant
 * section re-packed at bit 0, an m-stage packet, and n_per_stream[b] = m.  Bytes of out[b] past the section are zero.  NULL
 * pointers: HILC_ERR_NULL; B or T <= 0, or prev_in == prev_out: HILC_ERR_SHAPE.  The sender: one thread per output byte; the
 * receiver: one wave per stream. */
int hilc_pack_codes_10bit_fec(const int64_t* indices, const int* n_per_stream, const int* prev_in, int* prev_out, const int* action,
                              const int* hold, uint8_t* packets, int* nbytes, int B, int T, int n_max, int m, void* stream);
int hilc_fec_select(const uint8_t* packets, const int* fec, int* n_per_stream, uint8_t* out, int B, int T, int n_max, int m,
                    void* stream);

/* ---- discontinuous transmission (DTX) and comfort noise (CN) of the packet sender and receiver (additive under ABI 16) ----------
 * Two entry points added WITHOUT a version bump, as the packet, concealment, resampling and FEC entry points above.  The definition,
 * bit for bit, is hilcodec_amd/dtx.py; K = order in 0..HILC_DTX_MAX_ORDER (else HILC_ERR_RANGE), S = HILC_RESAMPLE_HOP T samples per hop, and a SID (byte 0 the
 * level L in 0..HILC_DTX_LEVELS - 1, bytes 1..K the int8 reflection coefficients q_i) must fit a packet row: stride >= 1 + K (else HILC_ERR_SHAPE).
 * hilc_dtx_encode: the sender's last launch before hilc_state_slots_hold, after the packer.  x fp32 [B][S] (the encoder's 24 kHz
 * hop); action and hold optional int32 [B] (NULL = 0): the rows of hilc_state_slots_apply / hilc_state_slots_hold; run int32 [B]
 * (in place); kind int32 [B] (out: HILC_DTX_HELD / SPEECH / SID / SILENT); packets uint8 [B][stride] and nbytes int32 [B] as the packer
 * wrote them; indices int64 [n_max][B][T]; prev optional int32 [B][prev_words] (the FEC packer's output row, word 0 its valid flag);
 * level_thr float64 [HILC_DTX_LEVELS - 1] (dtx.level_table); thr_vad the activity threshold on R[0] / S; hangover H >= 0, sid_interval I >= 1.
 * Per stream b: action[b] != 0 resets run[b] to 0 first; hold[b] != 0: kind 0, nothing else.  Otherwise: R[k], k <= K, in float64
 * (lane l of 64 sums x[s] x[s - k] over s = l mod 64, s >= k, in increasing s, then the 64 partials in lane order); active iff
 * R[0] / S >= thr_vad; Levinson-Durbin on R'[0] = R[0] (1 + 2^-13) -> k_i, E_K; L = #{j : E_K / S < level_thr[j]};
 * q_i = clamp(rint(128 k_i), -127, 127); run = active ? 0 : run <= H ? run + 1 : H + 1 + (run - H) mod I; kind = speech if active or
 * run <= H, SID if run == H + 1, else silent.  SID: packets[b] = L, q_1..q_K, then zeros, nbytes[b] = 1 + K; silent: packets[b] = 0,
 * nbytes[b] = 0; both: indices of b = -1 and prev[b][0] = 0.  Speech rows are not touched.
 * hilc_cng_synth: the receiver's launch after the decoder.  packets uint8 [B][stride] (a SID slot's row: the SID); action optional;
 * hold int32 [B] (in place): HILC_SESSIONS_HOLD_SID = a SID arrived, _SILENT = the stream is in DTX, _ADVANCE = decoded, anything else =
 * held; state int32 [B][HILC_DTX_ST_Q + 2 K] (in place: HILC_DTX_ST_*); wav fp32 [B][S]; restore optional int32 [B] (out: 1 where the slot produced noise, else 0); gains fp32 [HILC_DTX_LEVELS]
 * (dtx.gain_table).  Per slot: action != 0 clears the state row first.  hold SID: L = min(byte 0, HILC_DTX_LEVELS - 1), q_i = clamp(int8 byte i,
 * -127, 127) are stored, has = 1, the filter memory starts from zero if has was 0; the slot produces noise.  hold SILENT: with has, noise
 * from the stored parameters; without, hold[b] = HELD.  hold ADVANCE: has = 0.  Noise: wav[b][s] = y[s] = g u[s] - a_K y[s - K] - ... -
 * a_1 y[s - 1] in fp32 (each product and difference rounded, left to right), g = gains[L], a = step-up of q_i / 128 in float64
 * rounded to fp32, u[s] = fp32(h >> 8) 2^-23 - 1, h = lowbias32(((c S + s) mod 2^32) ^ ((b + 1) HILC_DTX_GOLDEN mod 2^32)); if some |y[s]| >= 16
 * or is not finite the row and the memory become 0; then c += 1, the memory = the last K outputs, hold[b] = 0.  Rows of slots without noise are not touched.  NULL pointers: HILC_ERR_NULL; B or
 * T <= 0: HILC_ERR_SHAPE.  Both: one wave per stream. */
int hilc_dtx_encode(const float* x, const int* action, const int* hold, int* run, int* kind, uint8_t* packets, int* nbytes,
                    int64_t* indices, int* prev, const double* level_thr, double thr_vad, int B, int T, int order, int hangover,
                    int sid_interval, int n_max, int stride, int prev_words, void* stream);
int hilc_cng_synth(const uint8_t* packets, const int* action, int* hold, int* state, float* wav, int* restore, const float* gains,
                   int B, int T, int order, int stride, void* stream);

/* ---- transport header and jitter buffer of the packet sender and receiver (additive under ABI 16) -------------------------------
 * Two entry points added WITHOUT a version bump, as the packet, concealment, resampling, FEC and DTX entry points above.  Header
 * (hilcodec_amd/wire.py, pack_transport): byte 0-1 the hop index h mod 2^16 big-endian, byte 2 = HILC_WIRE_SID_BIT | HILC_WIRE_FEC_BIT | n (HILC_WIRE_RSV_BIT
 * zero, n 1..31 for codes, 0 for a SID), then the body; stride = ceil(10 (n_max + m) T / 8), a headed row is H + stride bytes, H =
 * HILC_WIRE_TRANSPORT_HEADER.  m in [0, n_max] (else HILC_ERR_RANGE), n_max <= 31 and n_max + m <= HILC_WIRE_MAX_STAGES (else
 * HILC_ERR_UNSUPPORTED).
 * hilc_packet_header: the sender's last launch.  packets uint8 [B][stride] and nbytes int32 [B] as the packer (and hilc_dtx_encode)
 * left them; n_per_stream, kind (hilc_dtx_encode's), action, hold optional int32 [B] (NULL = n_max, speech, 0, 0); counter_in and
 * counter_out distinct int32 [B] (the hop of parity p reads one, writes the other) -> out uint8 [B][H + stride], out_nbytes int32 [B].
 * Per stream b: c = action[b] != 0 ? 0 : counter_in[b] mod 2^16; hold[b] != 0: out[b] = 0, out_nbytes[b] = 0, counter_out[b] = c;
 * else counter_out[b] = (c + 1) mod 2^16 and, when nbytes[b] > 0, out[b] = header(c, SID iff kind[b] == HILC_DTX_SID, FEC iff m >= 1 and
 * nbytes[b] = ceil(10 (n_b + m) T / 8) with n_b = n_per_stream[b] clamped to [max(m, 1), n_max], n = 0 for a SID else n_b) then the
 * nbytes[b] packet bytes, out_nbytes[b] = H + nbytes[b]; nbytes[b] == 0: out[b] = 0, out_nbytes[b] = 0.  One thread per output byte.
 * hilc_jitter_step: the receiver's first launch; the rules, bit for bit, are hilcodec_amd/jitter.py (JitterModel).  arrivals int32
 * [max_arrivals][1 + ceil((H + stride) / 4)] (word 0 the byte count, then the headed packet), grouped by slot: slot b's arrivals are
 * records offsets[b] .. offsets[b + 1] - 1 (int32 [B + 1], clamped to [0, max_arrivals]) in push order; action optional int32 [B];
 * hold int32 [B] (in: the host's holds and stops; out: HILC_SESSIONS_HOLD_ADVANCE, _HELD, _SID or _SILENT); n_per_stream, lost (conceal != 0 only), fec
 * (m >= 1 only) int32 [B] and packets uint8 [B][stride] (out); state int32 [B][HILC_JITTER_ST_WORDS], meta int32 [B][capacity] and ring int32
 * [B][capacity][ceil(stride / 4)] (in place).  order = the receiver's comfort-noise order K, -1 for none (a SID needs 1 + K <=
 * stride, else HILC_ERR_SHAPE; K > HILC_DTX_MAX_ORDER: HILC_ERR_RANGE); capacity a power of two in [2, 32], 0 <= depth <= capacity - 2 (else
 * HILC_ERR_RANGE).  NULL pointers: HILC_ERR_NULL; B or T <= 0 or max_arrivals < 0: HILC_ERR_SHAPE.  One wave per slot. */
int hilc_packet_header(const uint8_t* packets, const int* nbytes, const int* n_per_stream, const int* kind, const int* action,
                       const int* hold, const int* counter_in, int* counter_out, uint8_t* out, int* out_nbytes, int B, int T, int n_max,
                       int m, void* stream);
int hilc_jitter_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold, int* n_per_stream,
                     int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B, int T, int n_max, int m, int order,
                     int conceal, int depth, int capacity, void* stream);

/* ---- adaptive playout of the jitter buffer (additive under ABI 16) ---------------------------------------------------------------
 * One entry point added WITHOUT a version bump.  hilc_jitter_adapt_step: hilc_jitter_step with an adaptive playout clock, the
 * receiver's first launch in its place; the rules, bit for bit, are hilcodec_amd/jitter.py (JitterModel with cfg.adapt).  The
 * arguments of hilc_jitter_step with their meaning and checks, then adapt int32 [B][HILC_JITTER_AD_WORDS] (in place: HILC_JITTER_AD_*, a slot's debt,
 * pending shift, window and outlier run, then the counters grown, shrunk, forced, resync; NULL: HILC_ERR_NULL) and the
 * jitter.AdaptConfig: 0 <= headroom <= capacity - 2, 1 <= max_late <= capacity - 2, window >= 1, resync >= 2, force_windows >= 0
 * (else HILC_ERR_RANGE; capacity 2 leaves no max_late).  action[b] != 0 clears slot b's adapt row with its state row.  One wave
 * per slot. */
int hilc_jitter_adapt_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold, int* n_per_stream,
                           int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B, int T, int n_max, int m,
                           int order, int conceal, int depth, int capacity, int* adapt, int headroom, int max_late, int window,
                           int resync, int force_windows, void* stream);

/* ---- per-room mixing of the receiver's output (additive under ABI 16) -----------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/mixer.py;
 * wav fp32 [B][L] (the receiver's final output rows, assumed finite), any L >= 1.
 * hilc_mix_levels: score float64 [B], in place; action optional int32 [B].  Per slot b: p[l] = the sum over i = l (mod 64), i
 * ascending, of (double)wav[b][i]^2 (every product and sum rounded on its own in float64), E = p[0] + p[1] + ... + p[63] in that
 * order, score[b] = max(E, 0.5 prev) with prev = score[b], or 0 when action[b] != 0.  One wave per slot.
 * hilc_mix_rooms: room int32 [B] (-1: in no room, else a room id in [0, B)); score as hilc_mix_levels left it; top_k in [1, HILC_MIXER_MAX_TOP_K] (else
 * HILC_ERR_UNSUPPORTED) -> mixed fp32 [B][L], speakers int32 [B], every element written.  The candidates of room r are the slots with
 * room == r and score > 0, ordered by (score descending, slot ascending); the first min(top_k, count) are its speakers (speakers[b] =
 * 1, else 0).  mixed[b] for room[b] = r >= 0: the rows of r's speakers other than b, added per sample in ascending slot order
 * (acc = wav[t0][i], then acc = acc + wav[t1][i], ...: every sum rounded in fp32), clamped to [-1, 1]; no such speaker, or
 * room[b] < 0: zeros.  One workgroup per listener slot, no atomics; mixed must not overlap wav.
 * Both: NULL pointers (action excepted): HILC_ERR_NULL; B or L < 1: HILC_ERR_SHAPE. */
int hilc_mix_levels(const float* wav, double* score, const int* action, int B, int L, void* stream);
int hilc_mix_rooms(const float* wav, const int* room, const double* score, int top_k, float* mixed, int* speakers, int B, int L,
                   void* stream);

/* ---- per-speaker levelling and a limiter for the room mixer (additive under ABI 16) ------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above; hilc_mix_levels and hilc_mix_rooms are unchanged.  The
 * definition, bit for bit, is hilcodec_amd/mixer.py (LevelConfig, LimitConfig); every float64 operation below is one operation rounded
 * on its own.  A slot with action[b] != 0 (action optional int32 [B]) first takes its rows as cleared: gains (1, 1), power 0, limiter
 * (0, 1).
 * hilc_mix_gains: gains float64 [B][2] (the hop-start and hop-end gain), power float64 [B], in place, every slot on every hop.  E as
 * in hilc_mix_levels, m = E / L, g0 = the previous gains[b][1], pw = the previous power[b].  If m >= gate2: pw = m when pw == 0, else
 * pw + smooth (m - pw); v = (g0 g0) pw; v < lo: g1 = min(g0 up, max_gain); v > hi: g1 = max(g0 down, min_gain); else g1 = g0.
 * Otherwise pw and g1 = g0 stay.  gains[b] = (g0, g1), power[b] = pw.  One wave per slot.  Constants outside gate2 > 0, 0 < lo < hi,
 * up > 1, 0 < down < 1, 0 < min_gain <= 1 <= max_gain, 0 < smooth <= 1: HILC_ERR_UNSUPPORTED.
 * hilc_mix_rooms_dyn: hilc_mix_rooms (the same selection, on the raw score) with two optional rows.  gains (NULL: none), as
 * hilc_mix_gains left it: speaker j's sample i enters the sum as fp32((double)wav[j][i] (g0 + (g1 - g0) ((double)(i + 1) / (double)L)))
 * with j's (g0, g1).  limiter float64 [B][2] (NULL: none, the clamp of hilc_mix_rooms), the envelope and the gain, in place: on the
 * listener's sum acc (a row of zeros without terms or for room[b] < 0), sub-frame s = samples [s sub, min((s + 1) sub, L)), n_s of
 * them: p_s = max |acc[i]| (fp32), e_s = max(p_s, release e_(s-1)), G_s = ceiling / e_s when e_s > ceiling, else 1; the sample at offset
 * k of sub-frame s takes g = G_s when G_s <= G_(s-1), else G_(s-1) + (G_s - G_(s-1)) ((double)(k + 1) / (double)n_s); mixed =
 * min(max(fp32((double)acc g), -1), 1); limiter[b] = (e_last, G_last).  So |mixed| <= fp32(ceiling) up to one fp32 ulp.  With a limiter:
 * sub outside [HILC_MIXER_MIN_SUB, HILC_MIXER_MAX_SUB], L > HILC_MIXER_MAX_LIMIT_L, ceiling outside (0, 1] or release outside (0, 1):
 * HILC_ERR_UNSUPPORTED; without one, ceiling, release and sub are not read.  Both rows NULL: hilc_mix_rooms bit for bit.  One workgroup
 * per listener slot, no atomics; every element of mixed, speakers and the limiter row is written on every hop.
 * Both: NULL pointers (action and the optional rows excepted): HILC_ERR_NULL; B or L < 1: HILC_ERR_SHAPE; top_k as hilc_mix_rooms. */
int hilc_mix_gains(const float* wav, double* gains, double* power, const int* action, double gate2, double lo, double hi, double up,
                   double down, double min_gain, double max_gain, double smooth, int B, int L, void* stream);
int hilc_mix_rooms_dyn(const float* wav, const int* room, const double* score, int top_k, const double* gains, double* limiter,
                       double ceiling, double release, int sub, const int* action, float* mixed, int* speakers, int B, int L,
                       void* stream);

/* ---- quality-targeted variable bitrate of the packet sender (additive under ABI 16) ----------------------------------------------
 * One entry point added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/vbr.py.
 * hilc_vbr_select: the sender's launch between the quantiser and the packer.  z fp32 [B][T][C] (the quantiser's input, channel-last);
 * indices int64 [n][B][T] (stage-major, in place); codebooks fp32 [Nq][K][C]; n_per_stream, action, hold optional int32 [B] (NULL = n,
 * 0, 0): the slot's ceiling n_b (clamped to [1, n]) and the rows of hilc_state_slots_apply / hilc_state_slots_hold; credit optional
 * int32 [B] (in place; NULL = no cap, then rate_bits must be 0) -> n_eff int32 [B], distortion float64 [B][n + 1].  Per slot b:
 *   per frame t ascending, r = z[b][t][:]; for s = 0 .. n_b: e(t, s) = |r|^2, then (s < n_b) r[c] = r[c] - codebooks[s][k][c] with k =
 *   indices[s][b][t] clamped to [0, K), one fp32 subtraction per channel (rvq_encode_kernel's chain).  |r|^2 in float64: lane l of 64
 *   sums (double)r[c] (double)r[c] over c = l, l + 64, ... ascending, each product and each sum rounded on its own, then the 64
 *   partials are added in lane order.  D[s] = sum over t ascending of e(t, s); D[s > n_b] = D[n_b].
 *   n_q = the smallest s in [lo, n_b] with D[s] <= rho D[0] (one rounded float64 product), else n_b; lo = min(n_b, n_lo).
 *   With credit: c = burst_bits if action[b] != 0, else credit[b]; then c = min(c + rate_bits, burst_bits), n_eff = min(n_q,
 *   clamp(c / stage_bits, lo, n_b)), credit[b] = c - n_eff stage_bits.  Without: n_eff = n_q.
 *   hold[b] != 0: n_eff[b] = n_b, distortion[b] = 0, credit[b] = c before the refill (so an action on the same hop still fills it).
 *   Finally indices[s][b][:] = -1 for s >= n_eff[b].
 * C a multiple of 64 and <= 512, n <= HILC_WIRE_MAX_STAGES (else HILC_ERR_UNSUPPORTED); 1 <= n <= Nq, 1 <= n_lo <= n, 0 < rho <= 1, and with credit
 * stage_bits >= 1, rate_bits >= stage_bits n_lo, rate_bits <= burst_bits <= 2^30 (else HILC_ERR_RANGE); NULL pointers (the optional
 * rows excepted; credit NULL with rate_bits != 0): HILC_ERR_NULL; B, T, C, K or Nq <= 0: HILC_ERR_SHAPE.  One wave per slot, no
 * atomics; every element of n_eff and distortion is written. */
int hilc_vbr_select(const float* z, int64_t* indices, const float* codebooks, const int* n_per_stream, const int* action,
                    const int* hold, int* credit, int* n_eff, double* distortion, int B, int T, int C, int K, int Nq, int n, int n_lo,
                    double rho, int stage_bits, int rate_bits, int burst_bits, void* stream);

/* ---- receiver reports and loss-adaptive in-band FEC (additive under ABI 16) -------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/report.py.
 * hilc_rx_report: the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step.  jitter_state int32 [B][HILC_JITTER_ST_WORDS] (read only: the
 * rows that launch left); action optional int32 [B]; rows int32 [B][HILC_REPORT_RP_WORDS] (in place: HILC_REPORT_RP_*, the last report, the interval phase, the
 * window's counts and head, the remembered counters, the reports emitted, then the ring words); reports uint8 [B][HILC_WIRE_REPORT_BYTES] (seq, loss_q8,
 * residual_q8 of the slot's latest report: written when one is emitted, zeroed by action[b] != 0, else untouched); due int32 [B] (every
 * element written: 1 where a report was emitted on this hop).  Per slot: the hop's class is the first of the counters DECODED, FEC,
 * LOST, NOISE that differs from the remembered one (none: nothing but due changes); D, F and L hops enter a window of the last
 * `window` such hops, 2 bits each; every class advances the phase, and at phase >= interval the phase restarts and, with N >= 1
 * entries, seq = (seq + 1) mod 256, loss_q8 = min(255, (256 (F + L) + N / 2) / N), residual_q8 = min(255, (256 L + N / 2) / N).
 * 8 <= window <= 256 and 1 <= interval <= 1024, B >= 1 (else HILC_ERR_SHAPE).
 * hilc_fec_adapt: the sender's launch ahead of hilc_vbr_select / hilc_pack_codes_10bit_fec.  report optional int32 [B] (per slot 0, or
 * HILC_REPORT_REPORT_PRESENT | seq << 16 | loss_q8 << 8 | residual_q8); action, hold optional int32 [B] (the rows of hilc_state_slots_apply /
 * hilc_state_slots_hold); rows int32 [B][HILC_REPORT_FA_WORDS] (in place: HILC_REPORT_FA_*, on, calm, seen, last seq, age, loss, residual, then the counters
 * reports, stale, turned_on, turned_off, timeout); prev int32 [B][1 + m T] (the previous-codes rows the packer reads on this hop: only
 * word 0 of a slot that is not held and off is written, with 0); fec_on int32 [B] (every element written).  Per slot: action[b] != 0
 * clears the row to on = initial_on; a report is accepted when none was seen since the clear or (seq - last) mod 256 is in [1, 127]
 * (else stale), and then loss >= on_q8 switches on, loss <= off_q8 counts calm and switches off at calm_reports in a row, anything
 * between restarts the count; a slot that is not held ages by one hop, and at timeout_hops > 0 hops without an accepted report falls
 * back to initial_on and forgets the sequence number.  0 <= off_q8 < on_q8 <= 255, calm_reports >= 1, timeout_hops >= 0, B, T, m >= 1
 * (else HILC_ERR_SHAPE).
 * Both: NULL pointers (the optional rows excepted): HILC_ERR_NULL.  One wave per slot, no LDS, no atomics. */
int hilc_rx_report(const int* jitter_state, const int* action, int* rows, uint8_t* reports, int* due, int B, int window, int interval,
                   void* stream);
int hilc_fec_adapt(const int* report, const int* action, const int* hold, int* rows, int* prev, int* fec_on, int B, int T, int m,
                   int on_q8, int off_q8, int calm_reports, int timeout_hops, int initial_on, void* stream);

/* ---- NACK and retransmission (additive under ABI 16) ----------------------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/rtx.py.
 * hilc_nack_build: the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step, beside hilc_rx_report.  jitter_state int32
 * [B][HILC_JITTER_ST_WORDS] and meta int32 [B][capacity] (read only: the rows that launch left); action optional int32 [B]; rows int32
 * [B][HILC_RTX_NK_WORDS] (in place: HILC_RTX_NK_*, the counters sent, asked, recovered, expired, then one entry word per ring entry);
 * nacks uint8 [B][HILC_WIRE_NACK_BYTES] (base and bitmap of the slot's latest NACK, big-endian: written when one is emitted, zeroed by
 * action[b] != 0, else untouched); due int32 [B] (every element written: 1 where a NACK was emitted on this hop).  Per anchored slot,
 * with next = its playout clock: entry words whose hop is in the window and now in the ring count recovered, those outside the window
 * expired, and are freed; the holes below the highest occupied entry are asked for — not those with d + 1 < rtt_hops, in a silent
 * stretch (behind a SID, or behind nothing with ST_IN_DTX set) or, with skip_fecable and m >= 1, in front of a packet with the FEC flag
 * — when their word is free or age >= retry_hops and count < max_requests: the first is base, those at most 16 above it the bitmap;
 * a hole asked for restarts its age and counts, every other hole with count > 0 ages by one (at most 255).  capacity a power of two in
 * [2, 32], rtt_hops in [1, 30], retry_hops and max_requests in [1, 255], m >= 0 (else HILC_ERR_RANGE); B >= 1 (else HILC_ERR_SHAPE).
 * hilc_rtx_step: the sender's last launch, after hilc_packet_header.  packets uint8 [B][row_bytes] and nbytes int32 [B] as that launch
 * left them (row_bytes = HILC_WIRE_TRANSPORT_HEADER + stride); nack_base, nack_bitmap optional int32 [B] (both or neither: per slot
 * HILC_RTX_NACK_PRESENT | base and the bitmap, 0 and 0 for none); action optional int32 [B]; tags int32 [B][history], ring int32
 * [B][history][ceil(row_bytes / 4)] and rows int32 [B][HILC_RTX_RX_WORDS] (in place) -> out uint8 [B][per_hop][row_bytes], out_nbytes
 * int32 [B][per_hop], every element written.  Per slot: action[b] != 0 empties the tags; nbytes[b] > 0 stores the packet at entry h mod
 * history, h its bytes 0-1 (the row zero past min(nbytes[b], row_bytes) bytes, tag h | nbytes << 16); a NACK's hops, base first, then
 * base + 1 + j for every set bit j ascending, are looked up by tag: a match goes to the next free output row with its byte count, a match
 * behind per_hop rows counts dropped, anything else a miss.  history a power of two in [2, HILC_RTX_MAX_HISTORY], per_hop in [1,
 * HILC_RTX_MAX_PER_HOP] (else HILC_ERR_RANGE); B >= 1, HILC_WIRE_TRANSPORT_HEADER < row_bytes < 2^15 (else HILC_ERR_SHAPE); one of the
 * two NACK rows without the other: HILC_ERR_NULL.
 * Both: NULL pointers (the optional rows excepted): HILC_ERR_NULL.  One wave per slot, integer only, no LDS, no atomics. */
int hilc_nack_build(const int* jitter_state, const int* meta, const int* action, int* rows, uint8_t* nacks, int* due, int B,
                    int capacity, int m, int rtt_hops, int retry_hops, int max_requests, int skip_fecable, void* stream);
int hilc_rtx_step(const uint8_t* packets, const int* nbytes, const int* nack_base, const int* nack_bitmap, const int* action, int* tags,
                  int* ring, int* rows, uint8_t* out, int* out_nbytes, int B, int row_bytes, int history, int per_hop, void* stream);

/* ---- report-driven rate control of the sender (additive under ABI 16) -------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/rate.py.
 * hilc_rate_ceiling: the sender's launch in front of hilc_rvq_encode, behind hilc_fec_adapt.  report optional int32 [B] (per slot 0, or
 * HILC_REPORT_REPORT_PRESENT | seq << 16 | loss_q8 << 8 | residual_q8); action, hold optional int32 [B]; n_per_stream optional int32 [B]
 * (the slots' own ceilings, clamped to [1, n_max]; NULL: n_max); prev optional int32 [B][1 + m T] (the previous-codes rows the packer
 * reads on this hop, read only: word 0; NULL: no redundant section is live); rows int32 [B][HILC_RATE_RC_WORDS] (in place: HILC_RATE_RC_*);
 * n_ceil int32 [B] (every element written).  Per slot: action[b] != 0 resets the row to rate = 256 start_bits, credit = burst_hops
 * start_bits; a report is accepted as by hilc_fec_adapt (else stale), and then loss_q8 >= high_q8: rate = max(256 min_bits, (rate (512 -
 * loss_q8)) >> 9), loss_q8 <= low_q8: rate = min(256 max_bits, rate + max(256, (rate increase_q8) >> 8)); a slot that is not held ages by
 * one hop, at timeout_hops > 0 hops without an accepted report falls back to the start rate and forgets the sequence number, and fills
 * its bucket: credit = min(credit + (rate >> 8), burst_hops (rate >> 8)); overhead = 8 HILC_WIRE_TRANSPORT_HEADER (header != 0) + 10 m T
 * (m >= 1, no action, prev word 0 non-zero); n_ceil = clamp(max(0, credit - overhead) / (10 T), min(n_b, max(m, 1)), n_b), counted
 * limited when below n_b; a held slot reports n_b.  B, T >= 1, 1 <= n_max <= HILC_WIRE_MAX_STAGES, 0 <= m <= n_max, 0 <= low_q8 < high_q8
 * <= 255, 0 <= increase_q8 <= 65535, burst_hops >= 1, timeout_hops >= 0, 8 HILC_WIRE_TRANSPORT_HEADER (header != 0) + 10 T (max(m, 1) + m)
 * <= min_bits <= start_bits <= max_bits <= HILC_RATE_MAX_RATE_BITS and max_bits burst_hops <= 2^30 (else HILC_ERR_SHAPE).
 * hilc_rate_charge: the sender's last launch, after hilc_rtx_step.  nbytes int32 [B] (the hop's packets as sent); rtx_nbytes int32
 * [B][per_hop] (its retransmissions; NULL with per_hop = 0); rows as above, in place: credit = max(credit - 8 (nbytes[b] + the sum of
 * rtx_nbytes[b][.]), -burst_hops (rate >> 8)), for every slot, held or not.  B >= 1, 0 <= per_hop <= HILC_RTX_MAX_PER_HOP, burst_hops >=
 * 1 (else HILC_ERR_SHAPE).
 * Both: NULL pointers (the optional rows excepted): HILC_ERR_NULL.  One wave per slot, integer only, no LDS, no atomics. */
int hilc_rate_ceiling(const int* report, const int* action, const int* hold, const int* n_per_stream, const int* prev, int* rows,
                      int* n_ceil, int B, int T, int n_max, int m, int header, int min_bits, int max_bits, int start_bits, int high_q8,
                      int low_q8, int increase_q8, int burst_hops, int timeout_hops, void* stream);
int hilc_rate_charge(const int* nbytes, const int* rtx_nbytes, int* rows, int B, int per_hop, int burst_hops, void* stream);

/* ---- selective forwarding hop (additive under ABI 16) -------------------------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/forward.py.
 * Both read one hop's arrivals in the form of hilc_jitter_step: arrivals int32 [max_arrivals][1 + ceil(tb / 4)] (word 0 the byte count,
 * then the headed packet, tb = HILC_WIRE_TRANSPORT_HEADER + packet_bytes(n_max + m, T)), grouped by slot; offsets int32 [B + 1] (slot b's
 * records are [offsets[b], offsets[b + 1]), clamped to [0, max_arrivals]); action optional int32 [B] (non-zero: the slot was joined on
 * this hop).  order: the comfort-noise order of the SIDs accepted, -1 for none.
 * hilc_forward_classify: the hop's first launch.  rows int32 [B][HILC_FORWARD_SD_WORDS] (in place: HILC_FORWARD_SD_*); pick int32
 * [B][burst] and pick_count int32 [B] (every element written).  Per slot: action[b] != 0 clears the row; each arrival for which
 * wire.parse_transport raises counts SD_MALFORMED; each other one SD_CODES or SD_SIDS, the first `burst` of them go to pick[b][k] (their
 * record index, -1 behind pick_count[b]), each further one counts SD_OVERFLOW; SD_HANG = hang_hops + 1 when a valid codes arrival was
 * seen, else max(SD_HANG - 1, 0); SD_SINCE = min(SD_SINCE + 1, HILC_FORWARD_MAX_SINCE) while SD_HANG > 0, else 0.
 * hilc_forward_route: the hop's second launch, after hilc_forward_classify has finished for every slot.  room int32 [B] (-1: none);
 * layers int32 [B] (clamped to [1, n_max]); sender_rows, pick, pick_count as the first launch left them (read only); routes int32
 * [B][fanout] (in place: each route's owner, -1 when free), new_routes int32 [B][fanout], rows int32 [B][HILC_FORWARD_LR_WORDS] (in
 * place: HILC_FORWARD_LR_*), out uint8 [B][fanout][burst][tb] and out_nbytes int32 [B][fanout][burst]: every element written.  Per
 * listener b: action[b] != 0 frees its routes and clears its row; the slots t != b with room[t] == room[b] >= 0 and SD_HANG > 0, in
 * (SD_HANG descending, SD_SINCE descending, slot ascending) order, the first `fanout` of them are selected; a route whose owner is not
 * selected or has action != 0 is freed, the selected slots without a route take the free routes (ascending slot, lowest free route
 * first); new_routes[b][j] = 1 where route j has an owner other than before this hop (LR_SWITCHES counts them); row (b, j, k), k <
 * pick_count[owner], is arrival pick[owner][k] cut to min(n, layers[b]) stages — a SID byte for byte; else header byte 2 rewritten,
 * the primary's first stages, then the redundant section when it has one, keep_fec != 0 and min(n, layers[b]) >= m, the pad bits zero —
 * zero past its length, its byte count beside it; every other row zero with count 0.  LR_PACKETS, LR_BYTES count the rows written,
 * LR_TRIMMED those whose n was cut.
 * Both: NULL pointers (action excepted): HILC_ERR_NULL; B, T >= 1, max_arrivals >= 0, tb < 2^15 (else HILC_ERR_SHAPE); 1 <= n_max <= 31,
 * 0 <= m <= n_max, n_max + m <= HILC_WIRE_MAX_STAGES, -1 <= order <= HILC_DTX_MAX_ORDER, 1 <= burst <= HILC_FORWARD_MAX_BURST, 0 <=
 * hang_hops <= HILC_FORWARD_MAX_HANG_HOPS, 1 <= fanout <= HILC_FORWARD_MAX_FANOUT (else HILC_ERR_RANGE).  One wave per slot, integer only,
 * no LDS, no atomics. */
int hilc_forward_classify(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* rows, int* pick,
                          int* pick_count, int B, int T, int n_max, int m, int order, int burst, int hang_hops, void* stream);
int hilc_forward_route(const int* arrivals, int max_arrivals, const int* action, const int* room, const int* layers,
                       const int* sender_rows, const int* pick, const int* pick_count, int* routes, int* new_routes, int* rows,
                       uint8_t* out, int* out_nbytes, int B, int T, int n_max, int m, int order, int fanout, int burst, int keep_fec,
                       void* stream);

/* ---- downlink control of the forwarding hop (additive under ABI 16) -----------------------------------------------------------------
 * Two entry points added WITHOUT a version bump: the third and fourth launch of a forwarding hop.  The definition, bit for bit, is
 * hilcodec_amd/downlink.py.  tb, aw = ceil(tb / 4) and the arrival records are those of hilc_forward_classify.
 * hilc_downlink_store: after hilc_forward_classify.  pick int32 [B][burst] and pick_count int32 [B] as that launch left them (read only);
 * tags int32 [B][history], ring int32 [B][history][1 + aw] and rows int32 [B][HILC_DOWNLINK_DS_WORDS] (in place).  Per sender slot t:
 * action[t] != 0 empties its tags (the counters stay); each picked arrival, in pick order, goes to entry h mod history, h its own bytes
 * 0-1: the row becomes its arrival record, zero past the packet's length, the tag h | nbytes << 16; DS_STORED counts them, DS_REPLACED
 * those whose entry's tag was not 0.  A pick outside [0, max_arrivals) or with a byte count outside [HILC_WIRE_TRANSPORT_HEADER, tb] is
 * skipped (never for what hilc_forward_classify picked).
 * hilc_downlink_step: after hilc_forward_route and hilc_downlink_store have finished for every slot.  routes, new_routes int32
 * [B][fanout], in uint8 [B][fanout][burst][tb] and in_nbytes int32 [B][fanout][burst] as the route launch left them, layers int32 [B],
 * tags and ring as the store launch left them (all read only; tags and ring are not read with history == 0 and may be NULL); report
 * (report words, read with rate_on != 0), nack_base and nack_bitmap (NACK words as hilc_rtx_step's, read with history > 0; both or
 * neither) optional int32 [B][fanout], NULL: no feedback; rows int32 [B][HILC_DOWNLINK_DL_WORDS] and memory int32 [B][fanout] (in place);
 * eff_layers int32 [B], out uint8 [B][fanout][burst][tb], out_nbytes int32 [B][fanout][burst] and, with history > 0, rtx_out uint8
 * [B][per_hop][tb], rtx_nbytes and rtx_routes int32 [B][per_hop]: every element written.  Per listener b: action[b] != 0 resets the row
 * (DL_RATE_Q8 = 256 start_bits, DL_CREDIT = burst_hops start_bits, the rest 0) and clears its routes' memory; a route that is free or new
 * on this hop has its memory cleared and its feedback dropped (DL_STALE for a report, DL_NACK_STALE for a NACK); with rate_on != 0 the
 * other reports are accepted by hilc_rate_ceiling's rule into the route's memory word (else DL_STALE), and on a hop with an accepted
 * report DL_LOSS = the least stored loss_q8 over the routes that have one, DL_AGE = 0 and the rate moves once by hilc_rate_ceiling's
 * arithmetic; then DL_AGE += 1 with the timeout of hilc_rate_ceiling (it clears every route's seen flag) and the bucket fills;
 * Lmax = layers[b] clamped to [1, n_max]; L_eff = the largest L in [1, Lmax] for which 8 x the bytes of the non-empty rows cut to L stages
 * is at most DL_CREDIT, 1 if none is, Lmax with rate_on == 0 or without rows; DL_LAYERS = eff_layers[b] = L_eff, DL_LIMITED += 1 when a
 * row's n is cut; out row (b, j, k) is in row (b, j, k) cut to L_eff stages by the rule of hilc_forward_route, zero past its length, its
 * byte count beside it (DL_PACKETS, DL_BYTES, DL_TRIMMED count); with history > 0 the NACKs of the other routes, ascending
 * (DL_REQUESTS), are answered from the owner's history as hilc_rtx_step answers them — DL_RTX_SENT, DL_RTX_MISS, DL_RTX_DROPPED — each row
 * cut to L_eff stages, rtx_routes its route, the rows not used zero with count 0 and route -1; with rate_on != 0 DL_CREDIT = max(DL_CREDIT
 * - 8 (the bytes of out and of rtx_out), -burst_hops (rate >> 8)).
 * Both: NULL pointers (action, the feedback rows and what history == 0 leaves unread excepted): HILC_ERR_NULL; B, T >= 1, max_arrivals >=
 * 0, tb < 2^15, and with rate_on != 0: 1 <= min_bits <= start_bits <= max_bits <= HILC_RATE_MAX_RATE_BITS, burst_hops >= 1, max_bits
 * burst_hops <= 2^30, timeout_hops >= 0 (else HILC_ERR_SHAPE); n_max, m, fanout, burst as hilc_forward_route; history a power of two in
 * [2, HILC_DOWNLINK_MAX_HISTORY] (hilc_downlink_step: or 0), 1 <= per_hop <= HILC_DOWNLINK_MAX_PER_HOP, history > 0 or rate_on != 0, and
 * with rate_on != 0: 0 <= low_q8 < high_q8 <= 255, 0 <= increase_q8 <= 65535 (else HILC_ERR_RANGE).  One wave per slot, integer only, no
 * LDS, no atomics. */
int hilc_downlink_store(const int* arrivals, int max_arrivals, const int* action, const int* pick, const int* pick_count, int* tags,
                        int* ring, int* rows, int B, int T, int n_max, int m, int burst, int history, void* stream);
int hilc_downlink_step(const int* routes, const int* new_routes, const uint8_t* in, const int* in_nbytes, const int* layers,
                       const int* action, const int* report, const int* nack_base, const int* nack_bitmap, const int* tags,
                       const int* ring, int* rows, int* memory, int* eff_layers, uint8_t* out, int* out_nbytes, uint8_t* rtx_out,
                       int* rtx_nbytes, int* rtx_routes, int B, int T, int n_max, int m, int fanout, int burst, int keep_fec, int history,
                       int per_hop, int rate_on, int min_bits, int max_bits, int start_bits, int high_q8, int low_q8, int increase_q8,
                       int burst_hops, int timeout_hops, void* stream);

/* ---- audio level and level-based speaker selection (additive under ABI 16) ----------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/audio_level.py.
 * hilc_audio_level: the sender's level launch.  x fp32 [B][L] (the 24 kHz hop the encoder reads); thr float64 [HILC_DTX_LEVELS - 1]
 * (dtx.level_table); hold optional int32 [B]; level int32 [B] (every element written).  Per slot: hold[b] != 0 gives HILC_DTX_LEVELS - 1
 * and the row is not read; else E is the energy of hilc_mix_levels (lane l sums the squares of the samples i = l mod 64 in ascending i
 * in float64, the 64 partials are added in lane order, every product and sum rounded on its own), m = E / (double)L, and level[b] = #{j
 * < HILC_DTX_LEVELS - 1 : m < thr[j]}: -dBov in 1 dB steps, 127 for silence, 0 for a full-scale square.  B, L >= 1 (else
 * HILC_ERR_SHAPE).
 * hilc_forward_rank: the forwarding hop's launch between hilc_forward_classify and hilc_forward_route.  sd int32
 * [B][HILC_FORWARD_SD_WORDS] as the first launch left it (read only); loud int32 [B] (0: no level on this hop, else 128 - level; clamped
 * to [0, HILC_SPEAKER_MAX_LOUD]); room int32 [B]; action optional int32 [B]; shadow_prev int32 [B][HILC_FORWARD_SD_WORDS], the rows this
 * launch wrote on the previous hop (read only; another buffer than shadow); shadow int32 [B][HILC_FORWARD_SD_WORDS] (every element
 * written); rows int32 [B][HILC_SPEAKER_WORDS] (in place).  Per slot b: action[b] != 0 clears its row and counts its previous shadow row
 * as zero; talk = SD_HANG == hang_hops + 1; target = 256 loud[b] when talk, else 0 (LEVELLED += 1 when talk and loud[b] > 0); SCORE (read
 * clamped to [0, 256 HILC_SPEAKER_MAX_LOUD]) += (target - SCORE + 2^attack_shift - 1) >> attack_shift when target > SCORE, else SCORE =
 * max(target, SCORE - decay_q8); RANK = -1 unless room[b] >= 0, action[b] == 0 and b's previous shadow SD_HANG > 0, else the number of
 * slots s != b with room[s] == room[b], action[s] == 0 and a previous shadow SD_HANG > 0 that are ahead of b in hilc_forward_route's order
 * of the previous shadow rows (SD_HANG descending, SD_SINCE descending, slot ascending, with that launch's clamps); STAGE = 0 <= RANK <
 * fanout (STAGED += STAGE); candidate = SD_HANG > 0 and SCORE >= 256 (HILC_SPEAKER_MAX_LOUD - floor_level); key = ((SCORE + (STAGE ? 256
 * margin_db : 0)) << 8) | min(max(SD_SINCE, 0), 255) < 2^24; shadow[b] = sd[b] but SD_HANG = candidate ? 1 + (key >> 16) : 0 and SD_SINCE
 * = candidate ? key & 0xFFFF : 0.  hilc_forward_route handed `shadow` as its sender_rows then selects by key.  B >= 1 (else
 * HILC_ERR_SHAPE); shadow must be neither shadow_prev nor sd (else HILC_ERR_UNSUPPORTED); 1 <= fanout <= HILC_FORWARD_MAX_FANOUT, 0 <=
 * hang_hops <= HILC_FORWARD_MAX_HANG_HOPS, 0 <= floor_level < HILC_SPEAKER_MAX_LOUD, 0 <= attack_shift <= HILC_SPEAKER_MAX_ATTACK_SHIFT, 1
 * <= decay_q8 <= HILC_SPEAKER_MAX_DECAY_Q8, 0 <= margin_db <= HILC_SPEAKER_MAX_MARGIN_DB (else HILC_ERR_RANGE).
 * Both: NULL pointers (hold, action excepted): HILC_ERR_NULL.  One wave per slot, no LDS, no atomics. */
int hilc_audio_level(const float* x, const double* thr, const int* hold, int* level, int B, int L, void* stream);
int hilc_forward_rank(const int* sd, const int* loud, const int* room, const int* action, const int* shadow_prev, int* shadow, int* rows,
                      int B, int fanout, int hang_hops, int floor_level, int attack_shift, int decay_q8, int margin_db, void* stream);

/* ---- delay-based bandwidth estimate (additive under ABI 16) ------------------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/bwe.py.
 * hilc_rx_bwe: the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step, beside hilc_rx_report and hilc_nack_build and
 * independent of both.  arrivals, offsets, max_arrivals: one hop's arrivals in the form of hilc_jitter_step (read only); times int32
 * [max_arrivals]: the arrival tick (1/24000 s, mod 2^32) of each arrival record; action optional int32 [B]; rows int32
 * [B][HILC_BWE_BW_WORDS] (in place: HILC_BWE_BW_*); caps uint8 [B][HILC_WIRE_CAP_BYTES] (seq, then the cap in bits per hop as a big-endian
 * uint16: written when one is emitted, zeroed by an action); due int32 [B] (every element written: 1 where a cap was emitted).  Per slot:
 * action[b] != 0 clears the row (the estimate 256 max_bits, the threshold HILC_BWE_THR_START); each arrival that hilc_jitter_step's header
 * check accepts and whose hop index is ahead of the last sampled one gives one delay sample d = int32(t - last t) - 320 T int16(h - last
 * h), which goes through the accumulated and smoothed delay, the least-squares trend over the last `window` samples, the adaptive
 * threshold and the over-use detector; the AIMD controller then lowers the estimate to beta_q8 / 256 of the measured incoming rate on an
 * over-use, holds it on an under-use and raises it by increase_q16 / 65536 per hop index otherwise; every `interval` hops, and at once
 * after a decrease, the slot's cap is emitted.  B >= 1, max_arrivals >= 0, 1 <= T <= HILC_BWE_MAX_FRAMES, 1 <= n_max <= 31, 0 <= m <= n_max,
 * n_max + m <= HILC_WIRE_MAX_STAGES, -1 <= order <= HILC_DTX_MAX_ORDER, tb <= HILC_BWE_MAX_ROW_BYTES, 1 <= min_bits <= max_bits <=
 * HILC_BWE_MAX_CAP_BITS, 2 <= window <= HILC_BWE_MAX_WINDOW, HILC_BWE_RATE_MIN <= rate_window <= HILC_BWE_MAX_WINDOW, 1 <= alpha_q8 <= 256,
 * 1 <= beta_q8 <= 255, 0 <= increase_q16 <= 65535, 1 <= interval <= 1024, 1 <= reset_ticks <= HILC_BWE_MAX_RESET_TICKS (else
 * HILC_ERR_SHAPE).  One thread per slot: a slot's arrivals are a sequence.
 * hilc_rate_cap: the sender's launch directly in front of hilc_rate_ceiling.  cap optional int32 [B] (per slot 0, or HILC_BWE_CAP_PRESENT |
 * seq << 16 | cap_bits); action, hold optional int32 [B]; rows int32 [B][HILC_BWE_CP_WORDS] (in place: HILC_BWE_CP_*); rate_rows int32
 * [B][HILC_RATE_RC_WORDS] (in place: HILC_RATE_RC_RATE_Q8 only).  Per slot: action[b] != 0 clears the cap row; a cap is accepted by
 * hilc_rate_ceiling's sequence rule (else stale) and stored as 256 clamp(cap_bits, min_bits, max_bits); a slot that is not held ages by
 * one hop and at timeout_hops > 0 hops without an accepted cap forgets it; while it has one, the rate row's rate is at most the cap
 * (counted clamped when that lowered it).  B >= 1, 1 <= min_bits <= max_bits <= HILC_RATE_MAX_RATE_BITS, timeout_hops >= 0 (else
 * HILC_ERR_SHAPE).  One wave per slot.
 * Both: NULL pointers (the optional rows excepted): HILC_ERR_NULL.  Integer only, no LDS, no atomics. */
int hilc_rx_bwe(const int* arrivals, const int* offsets, const int* times, int max_arrivals, const int* action, int* rows, uint8_t* caps,
                int* due, int B, int T, int n_max, int m, int order, int min_bits, int max_bits, int window, int rate_window, int alpha_q8,
                int beta_q8, int increase_q16, int interval, int reset_ticks, void* stream);
int hilc_rate_cap(const int* cap, const int* action, const int* hold, int* rows, int* rate_rows, int B, int min_bits, int max_bits,
                  int timeout_hops, void* stream);

/* ---- SRTP packet protection (additive under ABI 16) ---------------------------------------------------------------------------------
 * Two entry points added WITHOUT a version bump, as the entry points above.  The definition, bit for bit, is hilcodec_amd/srtp.py; the
 * transform is AES_CM_128_HMAC_SHA1_80 of RFC 3711.  A protected packet is a headed packet (hilc_packet_header) whose first
 * HILC_WIRE_TRANSPORT_HEADER bytes stay clear, whose other bytes are XORed with the AES-128 counter-mode keystream from keystream byte 0
 * (RFC 3711 4.1.1: counter block j = ((k_s 2^16) ^ (SSRC 2^64) ^ (i 2^16)) + j, i = ROC 2^16 + SEQ, SEQ the header's hop index, 3.3.1)
 * and that carries HILC_WIRE_SRTP_TAG_BYTES tag bytes behind it: the first 10 bytes of HMAC-SHA1 over header, ciphertext and the ROC
 * as 4 bytes big-endian (4.2).  keys int32 [B][HILC_SRTP_KEY_WORDS] (read only, built on the host: key derivation 4.3.1 with kdr = 0, the
 * AES key expansion and the two HMAC pad blocks are done there); action optional int32 [B]: action[b] != 0 clears the slot's row and sets
 * its ROC to the key row's KEY_ROC (0 without a valid key).
 * hilc_srtp_protect: the sender's launch behind hilc_packet_header, in front of hilc_rtx_step and hilc_rate_charge.  packets uint8
 * [B][row_bytes] and nbytes int32 [B] (read only); rows int32 [B][HILC_SRTP_TX_WORDS] (in place); out uint8 [B][row_bytes +
 * HILC_WIRE_SRTP_TAG_BYTES] and out_nbytes int32 [B] (every element written).  Per slot, nb = min(nbytes, row_bytes): nb <
 * HILC_WIRE_TRANSPORT_HEADER (nothing sent) leaves the row alone, out zero, out_nbytes 0; a slot without a valid key sends nothing (out
 * zero, out_nbytes 0, TX_NOKEY += 1); else TX_ROC += 1 if the slot has sent before and SEQ < TX_LAST as unsigned 16 bit (3.3.1: the
 * sender's rollover), TX_LAST = SEQ, and out is the packet protected under TX_ROC, zero past nb + 10 bytes, out_nbytes = nb + 10.
 * hilc_srtp_unprotect: the receiver's first launch.  arrivals int32 [max_arrivals][1 + ceil((row_bytes + 10) / 4)] and offsets int32
 * [B + 1]: one hop's arrivals in the form of hilc_jitter_step, each record a protected packet (read only); rows int32
 * [B][HILC_SRTP_RX_WORDS] (in place); plain int32 [max_arrivals][1 + ceil(row_bytes / 4)]: the records of every slot's range are written,
 * in the form hilc_jitter_step takes.  Per slot and arrival, in order: no valid key: RX_NOKEY; a byte count below
 * HILC_WIRE_TRANSPORT_HEADER + 10 or above row_bytes + 10: RX_SHORT; the ROC estimate v from (RX_SL, RX_ROC, SEQ) by 3.3.1 (the slot's
 * first packet: v = RX_ROC), v = -1: RX_REPLAY; the index v 2^16 + SEQ more than 63 below the highest authenticated one or its window
 * bit set (3.3.2): RX_REPLAY; a tag that differs in any of its 10 bytes, all compared (4.2): RX_AUTH_FAIL; each of these writes a
 * record of 0 bytes, all words zero, and changes nothing but its counter.  Otherwise the record is the decrypted packet with its byte
 * count less 10, RX_OK += 1, the window bit is set and, for a new highest index, the window moves up, RX_SL = SEQ and RX_ROC = v (3.3.1).
 * Both: B >= 1, max_arrivals >= 0, HILC_WIRE_TRANSPORT_HEADER < row_bytes <= HILC_SRTP_MAX_ROW_BYTES (else HILC_ERR_SHAPE); NULL pointers
 * (action excepted): HILC_ERR_NULL.  One thread per slot, workgroups of 64, one 256-word AES table in LDS; the byte rows of
 * hilc_srtp_protect are read and written as words where base and row width are multiples of 4 and byte by byte otherwise, so any view
 * is accepted.  Integer only, no atomics. */
int hilc_srtp_protect(const uint8_t* packets, const int* nbytes, const int* keys, int* rows, const int* action, uint8_t* out,
                      int* out_nbytes, int B, int row_bytes, void* stream);
int hilc_srtp_unprotect(const int* arrivals, const int* offsets, int max_arrivals, const int* keys, int* rows, const int* action,
                        int* plain, int B, int row_bytes, void* stream);

/* ---- SRTP on the forwarding hop's routes (additive under ABI 16) --------------------------------------------------------------------
 * One entry point added WITHOUT a version bump.  The definition, bit for bit, is hilcodec_amd/forward_srtp.py (RouteModel).  The
 * forwarder relays arrivals — reordered, retransmitted, from a route whose owner changes — so hilc_srtp_protect's sender rule does not
 * hold for it; each (listener, route) keeps the receiver's index state instead and refuses what that state would call a replay.
 * hilc_srtp_protect_routes: the forwarding hop's last launch.  rows uint8 [B][fanout][burst][row_bytes] and nbytes int32
 * [B][fanout][burst]: the hop's final rows (hilc_forward_route's or hilc_downlink_step's), read only; routes, new_routes int32
 * [B][fanout] as hilc_forward_route left them; action, rekey_up, rekey_down optional int32 [B] (a slot joined / given an uplink / a
 * downlink key on this hop); keys int32 [B][HILC_SRTP_KEY_WORDS]: each listener's downlink key row; route_rows int32
 * [B][fanout][HILC_FSRTP_RT_WORDS] (in place); out uint8 [B][fanout][burst][row_bytes + HILC_WIRE_SRTP_TAG_BYTES] and out_nbytes int32
 * [B][fanout][burst]: every element written.  Per (b, j), t = routes[b][j]: new_routes[b][j], action[b], rekey_down[b], or (0 <= t < B
 * and (action[t] or rekey_up[t])) non-zero restarts the route: RT_EPOCH += 1 and RT_ROC, RT_SL, RT_SEEN and the window are cleared; at
 * HILC_FSRTP_MAX_EPOCH the epoch stays and RT_SEEN becomes HILC_FSRTP_SEEN_EXHAUSTED.  Then its rows in k order, nb = min(nbytes,
 * row_bytes): nb < HILC_WIRE_TRANSPORT_HEADER: out zero, out_nbytes 0; no valid key: the same, RT_NOKEY += 1; an exhausted route: the
 * same, RT_EXHAUSTED += 1; the ROC estimate v from (RT_SL, RT_ROC, SEQ) by RFC 3711 3.3.1 (the first packet: v = RT_ROC): v = -1, an
 * index more than 63 below the highest sent, or its window bit set: the same, RT_STALE += 1; otherwise the window takes the index as
 * hilc_srtp_unprotect's does, out is the packet protected under index v 2^16 + SEQ, the key row and SSRC = KEY_SSRC +
 * HILC_FORWARD_MAX_FANOUT * RT_EPOCH + j (mod 2^32), zero past nb + 10 bytes, out_nbytes = nb + 10, RT_PROTECTED += 1.
 * B >= 1, 1 <= fanout <= HILC_FORWARD_MAX_FANOUT, 1 <= burst <= HILC_FORWARD_MAX_BURST, HILC_WIRE_TRANSPORT_HEADER < row_bytes <=
 * HILC_SRTP_MAX_ROW_BYTES (else HILC_ERR_SHAPE); NULL pointers (the three optional rows excepted): HILC_ERR_NULL.  One thread per
 * output row, the rows of a route in one workgroup of 64 (64 / burst whole routes): each thread replays the integer rule for the rows in
 * front of its own and runs its own packet's AES / SHA-1 chain; the thread of a route's last row writes the route row.  Byte rows are
 * read and written as words where base and row width are multiples of 4 and byte by byte otherwise.  Integer only, no atomics. */
int hilc_srtp_protect_routes(const uint8_t* rows, const int* nbytes, const int* routes, const int* new_routes, const int* action,
                             const int* rekey_up, const int* rekey_down, const int* keys, int* route_rows, uint8_t* out, int* out_nbytes,
                             int B, int fanout, int burst, int row_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HILCODEC_AMD_H */
