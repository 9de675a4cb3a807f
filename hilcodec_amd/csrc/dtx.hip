// Discontinuous transmission (DTX) and comfort noise (CN) of the graphed sender / receiver pair (graph_step.GraphedEncodeHop(dtx=),
// GraphedDecodeHop(cng_order=)): a sender stops sending during silence except for a small silence descriptor (SID) every few hops,
// and the receiver synthesises background noise of the SID's level and spectral envelope.  The definition, bit for bit, is
// hilcodec_amd/dtx.py.  Two launches, one per side:
//
//   hilc_dtx_encode  the sender's last launch before hilc_state_slots_hold, after the packer: per stream, the float64 autocorrelation
//                    of the 24 kHz hop, the activity decision, Levinson-Durbin, the level and the quantised reflection coefficients;
//                    the run counter (in place) and the hop's kind; SID / SILENT hops get their rows rewritten.
//   hilc_cng_synth   the receiver's launch after the decoder: per slot that produces noise, the SID's (or the stored) parameters
//                    through the all-pole synthesis filter into the slot's wav row; the CN state row is updated in place.
//
// Both kernels: one wave per stream (slot.h), wave-uniform branches only, the order K a template parameter (the filter memory and
// the coefficients stay in registers).
#include "slot.h"

namespace {

using namespace slot;

constexpr float NOISE_BOUND = 16.f; // dtx.NOISE_BOUND: a noise hop with a sample outside (-16, 16) is replaced by silence

// the wave's LDS writes are visible to its other lanes (a wave runs its LDS operations in order; this keeps the compiler from moving
// the reads above the writes)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int readlane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ uint32_t lowbias32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

template <int K>
__global__ __launch_bounds__(THREADS) void dtx_encode_kernel(const float* __restrict__ x, const int* __restrict__ action,
                                                             const int* __restrict__ hold, int* __restrict__ run, int* __restrict__ kind,
                                                             uint8_t* __restrict__ packets, int* __restrict__ nbytes,
                                                             int64_t* __restrict__ indices, int* __restrict__ prev,
                                                             const double* __restrict__ level_thr, double thr_vad, int B, int T,
                                                             int H, int I, int n_max, int stride, int prev_words) {
  __shared__ double part[WAVES][K + 1][LANES + 1];        // +1: lane k's column read is free of bank conflicts
  __shared__ float xs[WAVES][HILC_DTX_MAX_ORDER + HILC_RESAMPLE_HOP];
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int w = me.w, b = me.b, lane = me.lane();
  const int S = HILC_RESAMPLE_HOP * T;
  const bool reset = is_reset(action, b);
  const int run0 = reset ? 0 : run[b];
  const double thr0 = level_thr[lane];
  const double thr1 = lane + LANES < HILC_DTX_LEVELS - 1 ? level_thr[lane + LANES] : 0.0;
  if (is_held(hold, b)) {                                 // held: run kept (a start on this hop clears it), nothing else
    if (lane == 0) {
      run[b] = run0;
      kind[b] = HILC_DTX_HELD;
    }
    return;
  }
  // autocorrelation: lane l's partial of lag k over s = l (mod 64), s >= k, in increasing s (exact products in float64).  The hop
  // goes through LDS one frame (with the HILC_DTX_MAX_ORDER samples before it) at a time: one round of independent loads per frame.
  const float* xb = x + (long)b * S;
  double p[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) p[k] = 0.0;
  for (int base = 0; base < S; base += HILC_RESAMPLE_HOP) {
    float v[HILC_RESAMPLE_HOP / LANES];
#pragma unroll
    for (int i = 0; i < HILC_RESAMPLE_HOP / LANES; ++i) v[i] = xb[base + i * LANES + lane];
    const float hv = (lane < HILC_DTX_MAX_ORDER && base > 0) ? xb[base - HILC_DTX_MAX_ORDER + lane] : 0.f;
    wave_sync();                                           // the previous frame's reads are done
#pragma unroll
    for (int i = 0; i < HILC_RESAMPLE_HOP / LANES; ++i) xs[w][HILC_DTX_MAX_ORDER + i * LANES + lane] = v[i];
    if (lane < HILC_DTX_MAX_ORDER) xs[w][lane] = hv;
    wave_sync();
#pragma unroll
    for (int i = 0; i < HILC_RESAMPLE_HOP / LANES; ++i) {
      const int s = base + i * LANES + lane;
      const double xd = (double)v[i];
#pragma unroll
      for (int k = 0; k <= K; ++k)
        if (s >= k) p[k] = __dadd_rn(p[k], __dmul_rn(xd, (double)xs[w][HILC_DTX_MAX_ORDER + i * LANES + lane - k]));
    }
  }
#pragma unroll
  for (int k = 0; k <= K; ++k) part[w][k][lane] = p[k];
  wave_sync();
  // lane k <= K: R[k] = the 64 partials in lane order
  double rk = 0.0;
  if (lane <= K)
    for (int l = 0; l < LANES; ++l) rk = __dadd_rn(rk, part[w][lane][l]);
  double R[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) R[k] = readlane_d(rk, k);
  const bool active = __ddiv_rn(R[0], (double)S) >= thr_vad;
  // Levinson-Durbin on R'[0] = R[0] (1 + 2^-13), every lane the same (wave-uniform values)
  double a[K + 1], kr[K + 1];
#pragma unroll
  for (int i = 0; i <= K; ++i) a[i] = kr[i] = 0.0;
  double E = __dmul_rn(R[0], 1.0 + 0x1p-13);
  bool alive = true;
#pragma unroll
  for (int i = 1; i <= K; ++i) {
    double acc = R[i];
#pragma unroll
    for (int j = 1; j < i; ++j) acc = __dadd_rn(acc, __dmul_rn(a[j], R[i - j]));
    bool ok = alive && E > 0.0;
    double ki = ok ? __ddiv_rn(-acc, E) : 0.0;
    ok = ok && fabs(ki) < 1.0;
    if (ok) {
      double na[K + 1];
#pragma unroll
      for (int j = 1; j < i; ++j) na[j] = __dadd_rn(a[j], __dmul_rn(ki, a[i - j]));
#pragma unroll
      for (int j = 1; j < i; ++j) a[j] = na[j];
      a[i] = ki;
      E = __dmul_rn(E, __dsub_rn(1.0, __dmul_rn(ki, ki)));
      kr[i] = ki;
    }
    alive = ok;
  }
  // level: #{j < 127 : E_K / S < thr[j]}, lanes j and j + 64
  const double ev = __ddiv_rn(E, (double)S);
  const bool c0 = ev < thr0;
  const bool c1 = lane + LANES < HILC_DTX_LEVELS - 1 && ev < thr1;
  const int L = __popcll(__ballot(c0)) + __popcll(__ballot(c1));
  // the state machine
  int r;
  if (active) r = 0;
  else if (run0 <= H) r = run0 + 1;
  else r = H + 1 + (run0 - H) % I;
  const int kd = (active || r <= H) ? HILC_DTX_SPEECH : (r == H + 1 ? HILC_DTX_SID : HILC_DTX_SILENT);
  if (lane == 0) {
    run[b] = r;
    kind[b] = kd;
  }
  if (kd == HILC_DTX_SPEECH) return;
  // SID / SILENT: the packet row, its byte count, the indices and the FEC row's valid flag
  int byte = 0;
  if (kd == HILC_DTX_SID) {
    if (lane == 0) byte = L;
#pragma unroll
    for (int i = 1; i <= K; ++i) {
      const int q = (int)fmax(-127.0, fmin(127.0, rint(__dmul_rn(kr[i], 128.0))));
      if (lane == i) byte = q & 0xFF;
    }
  }
  uint8_t* row = packets + (long)b * stride;
  for (int j = lane; j < stride; j += LANES) row[j] = (uint8_t)(j == lane ? byte : 0);
  if (lane == 0) nbytes[b] = kd == HILC_DTX_SID ? 1 + K : 0;
  clear_rows(indices, 0, n_max, B, b, T, lane);
  if (prev != nullptr && lane == 0) prev[(long)b * prev_words] = 0;
}

template <int K>
__global__ __launch_bounds__(THREADS) void cng_synth_kernel(const uint8_t* __restrict__ packets, const int* __restrict__ action,
                                                            int* __restrict__ hold, int* __restrict__ state, float* __restrict__ wav,
                                                            int* __restrict__ restore, const float* __restrict__ gains, int B, int S,
                                                            int stride) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  constexpr int W = HILC_DTX_ST_Q + 2 * K;
  int* st = state + (long)b * W;
  const bool reset = is_reset(action, b);                 // the state row starts from zero
  const int h = hold[b];
  int word = (lane < W && !reset) ? st[lane] : 0;
  const int byte = (h == HILC_SESSIONS_HOLD_SID && lane <= K) ? (int)packets[(long)b * stride + lane] : 0;
  const int has = readlane_i(word, HILC_DTX_ST_HAS);
  const bool noise = h == HILC_SESSIONS_HOLD_SID || (h == HILC_SESSIONS_HOLD_SILENT && has != 0);
  if (!noise) {
    if (h == HILC_SESSIONS_HOLD_ADVANCE && lane == HILC_DTX_ST_HAS) word = 0;   // decoded: the next SID starts from zero filter memory
    if (lane < W) st[lane] = word;
    if (lane == 0) {
      if (h == HILC_SESSIONS_HOLD_SILENT) hold[b] = HILC_SESSIONS_HOLD_HELD;     // silent without a SID: held by the graph
      if (restore != nullptr) restore[b] = 0;
    }
    return;
  }
  int L;
  int q[K + 1];
  float mem[K + 1];
  if (h == HILC_SESSIONS_HOLD_SID) {
    L = min(readlane_i(byte, 0), HILC_DTX_LEVELS - 1);
#pragma unroll
    for (int i = 1; i <= K; ++i) q[i] = max(-127, min(127, (int)(int8_t)readlane_i(byte, i)));
#pragma unroll
    for (int i = 0; i < K; ++i) mem[i] = has != 0 ? __int_as_float(readlane_i(word, HILC_DTX_ST_Q + K + i)) : 0.f;
  } else {
    L = readlane_i(word, HILC_DTX_ST_LEVEL);
#pragma unroll
    for (int i = 1; i <= K; ++i) q[i] = readlane_i(word, HILC_DTX_ST_Q + i - 1);
#pragma unroll
    for (int i = 0; i < K; ++i) mem[i] = __int_as_float(readlane_i(word, HILC_DTX_ST_Q + K + i));
  }
  const uint32_t c = (uint32_t)readlane_i(word, HILC_DTX_ST_COUNT);
  // step-up recursion in float64, rounded once to fp32
  double ad[K + 1];
#pragma unroll
  for (int i = 0; i <= K; ++i) ad[i] = 0.0;
#pragma unroll
  for (int i = 1; i <= K; ++i) {
    const double kh = (double)q[i] * 0.0078125;
    double na[K + 1];
#pragma unroll
    for (int j = 1; j < i; ++j) na[j] = __dadd_rn(ad[j], __dmul_rn(kh, ad[i - j]));
#pragma unroll
    for (int j = 1; j < i; ++j) ad[j] = na[j];
    ad[i] = kh;
  }
  float a[K + 1];
#pragma unroll
  for (int i = 1; i <= K; ++i) a[i] = (float)ad[i];
  const float g = gains[L];
  const uint32_t seed = (uint32_t)(b + 1) * HILC_DTX_GOLDEN;
  float* out = wav + (long)b * S;
  bool wild = false;                                      // some |y[s]| >= NOISE_BOUND or not finite
  for (int c0 = 0; c0 < S; c0 += LANES) {
    const uint32_t key = c * (uint32_t)S + (uint32_t)(c0 + lane);
    const uint32_t hh = lowbias32(key ^ seed);
    const float u = __fsub_rn(__fmul_rn((float)(hh >> 8), 0x1p-23f), 1.0f);
    const float e = __fmul_rn(g, u);
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < LANES; ++i) {
      float acc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), i));
#pragma unroll
      for (int j = K; j >= 1; --j) acc = __fsub_rn(acc, __fmul_rn(a[j], mem[K - j]));   // mem[K - j] = y[s - j]
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) mem[j] = mem[j + 1];
      if (K > 0) mem[K - 1] = acc;
      mine = lane == i ? acc : mine;
    }
    out[c0 + lane] = mine;
    wild = wild || !(fabsf(mine) < NOISE_BOUND);
  }
  if (__any(wild)) {                                      // a SID the fp32 filter cannot follow: a silent hop, the memory cleared
    for (int s = lane; s < S; s += LANES) out[s] = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) mem[i] = 0.f;
  }
  // the new state row: has 1, L, c + 1, q, the filter memory
  int nw = 0;
  if (lane == HILC_DTX_ST_HAS) nw = 1;
  if (lane == HILC_DTX_ST_LEVEL) nw = L;
  if (lane == HILC_DTX_ST_COUNT) nw = (int)(c + 1u);
#pragma unroll
  for (int i = 1; i <= K; ++i)
    if (lane == HILC_DTX_ST_Q + i - 1) nw = q[i];
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (lane == HILC_DTX_ST_Q + K + i) nw = __float_as_int(mem[i]);
  if (lane < W) st[lane] = nw;
  if (lane == 0) {
    hold[b] = HILC_SESSIONS_HOLD_ADVANCE;
    if (restore != nullptr) restore[b] = 1;
  }
}

#define HILC_DTX_ORDERS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

}  // namespace

extern "C" int hilc_dtx_encode(const float* x, const int* action, const int* hold, int* run, int* kind, uint8_t* packets, int* nbytes,
                               int64_t* indices, int* prev, const double* level_thr, double thr_vad, int B, int T, int order,
                               int hangover, int sid_interval, int n_max, int stride, int prev_words, void* stream) {
  if (!x || !run || !kind || !packets || !nbytes || !indices || !level_thr) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || n_max <= 0 || stride <= 0 || (prev && prev_words <= 0)) return HILC_ERR_SHAPE;
  if (T > (1 << 20) / HILC_RESAMPLE_HOP) return HILC_ERR_SHAPE;
  if (order < 0 || order > HILC_DTX_MAX_ORDER || hangover < 0 || sid_interval < 1 || hangover > (1 << 30) || sid_interval > (1 << 30))
    return HILC_ERR_RANGE;
  if (stride < 1 + order) return HILC_ERR_SHAPE;          // a SID must fit the row
  switch (order) {
#define X(K)                                                                                                                  \
  case K:                                                                                                                     \
    return launch(dtx_encode_kernel<K>, waves_grid(B), stream, x, action, hold, run, kind, packets, nbytes, indices, prev,    \
                  level_thr, thr_vad, B, T, hangover, sid_interval, n_max, stride, prev_words);
    HILC_DTX_ORDERS(X)
#undef X
  }
  return HILC_ERR_RANGE;                                  // not reached: the order was checked above
}

extern "C" int hilc_cng_synth(const uint8_t* packets, const int* action, int* hold, int* state, float* wav, int* restore,
                              const float* gains, int B, int T, int order, int stride, void* stream) {
  if (!packets || !hold || !state || !wav || !gains) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || T > (1 << 20) / HILC_RESAMPLE_HOP) return HILC_ERR_SHAPE;
  if (order < 0 || order > HILC_DTX_MAX_ORDER) return HILC_ERR_RANGE;
  if (stride < 1 + order) return HILC_ERR_SHAPE;
  switch (order) {
#define X(K) \
  case K:    \
    return launch(cng_synth_kernel<K>, waves_grid(B), stream, packets, action, hold, state, wav, restore, gains, B, HILC_RESAMPLE_HOP * T, stride);
    HILC_DTX_ORDERS(X)
#undef X
  }
  return HILC_ERR_RANGE;                                  // not reached: the order was checked above
}
