// Polyphase sample-rate conversion at the codec's input and output (hilcodec_amd/resample.py; graph_step.GraphedEncodeHop(input_rate=)
// and GraphedDecodeHop(output_rate=)).  The reference loads every input with `librosa.load(PATH, sr=sr)` (test_onnx.py:52), which
// resamples a file of any rate to the model's 24 kHz; this is the project's own converter for that step, defined exactly:
//
//   ph = (m M) mod L,  base = (m M - ph) / L,  y[m] = sum_{j = 0 .. Q-1} taps[ph][j] * x[base - j]
//
// summed in order of j from 0.0f, every product and every sum rounded on its own (no contraction), so a torch CPU loop over j
// (resample.reference) reproduces it bit for bit.  x[i < 0] is read from the history (the last Q - 1 input samples of the stream),
// zero without one.
//
// One launch: a workgroup computes a tile of TILE consecutive outputs for SB streams.  The output phases depend on m only, so the tile's
// tap rows are staged in LDS once and shared by its streams: the whole [L][Q] table when L <= TILE (then a row is a phase), else the
// TILE rows of the tile's own outputs (consecutive outputs have distinct phases when TILE <= L).  Rows are padded to an odd stride so
// that lanes reading different rows at the same j hit different banks.  Each stream's input window (Q - 1 samples before the tile's
// first base up to its last base) is staged beside them.  Lane i of wave w computes output m0 + i of SPT streams, so each tap read
// from LDS serves SPT products.  The workgroups of the first tile also write the new history.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = 64;                 // outputs per workgroup: one per lane
constexpr int SPT = 4;                   // streams per thread
constexpr int SB = WAVES * SPT;          // streams per workgroup
constexpr int STAGE = 8;                 // tap loads in flight per thread while staging
constexpr long MAX_LDS = 64 * 1024;

__host__ __device__ inline int tap_rows(int L) { return L <= TILE ? L : TILE; }
__host__ __device__ inline int tap_stride(int Q) { return Q | 1; }
// longest input window of a tile: the bases of TILE consecutive outputs span at most ceil((TILE - 1) M / L) samples
__host__ __device__ inline int window_len(int L, int M, int Q) { return (int)(((long)(TILE - 1) * M + L - 1) / L) + Q; }

// input sample g of stream s (g < 0: the history; 0 past the batch or where `ok` is false)
__device__ __forceinline__ float in_at(const float* __restrict__ x, const float* __restrict__ hist_in, int s, long g, bool ok, int B,
                                       int T_in, int Q) {
  if (!ok || s >= B) return 0.f;
  if (g >= 0) return x[(long)s * T_in + g];
  return hist_in ? hist_in[(long)s * (Q - 1) + (Q - 1) + g] : 0.f;
}

__global__ __launch_bounds__(THREADS) void resample_poly_kernel(const float* __restrict__ x, const float* __restrict__ hist_in,
                                                                float* __restrict__ hist_out, float* __restrict__ y,
                                                                const float* __restrict__ taps, int B, int T_in, int T_out, int L,
                                                                int M, int Q) {
  extern __shared__ float smem[];
  const int QP = tap_stride(Q);
  const int rows = tap_rows(L);
  const int W = window_len(L, M, Q);
  float* tap_s = smem;                                  // [rows][QP]
  float* win_s = smem + rows * QP;                      // [SB][W]
  const int tid = threadIdx.x;
  const long m0 = (long)blockIdx.x * TILE;
  const int s0 = blockIdx.y * SB;
  const long m_last = min(m0 + TILE, (long)T_out) - 1;
  const long lo = (m0 * M) / L - (Q - 1);               // input index of window sample 0 (negative: history)
  const int span = (int)((m_last * M) / L - lo) + 1;   // window samples the tile reads (<= W)

  // staging: every global load of a thread's batch is issued before the first is waited for (a loop of single loads would pay
  // one memory latency per iteration, which dominated the launch at 1 024 streams)
  for (int k0 = 0; k0 < rows * Q; k0 += THREADS * STAGE) {
    float v[STAGE];
#pragma unroll
    for (int u = 0; u < STAGE; ++u) {
      const int k = min(k0 + u * THREADS + tid, rows * Q - 1);     // past the table: a repeated in-bounds read, not stored
      const int r = k / Q, j = k - r * Q;
      const int ph = L <= TILE ? r : (int)(((m0 + r) * M) % L);
      v[u] = taps[(long)ph * Q + j];
    }
#pragma unroll
    for (int u = 0; u < STAGE; ++u) {
      const int k = k0 + u * THREADS + tid;
      const int r = k / Q;
      if (k < rows * Q) tap_s[r * QP + (k - r * Q)] = v[u];
    }
  }
  for (int i0 = 0; i0 < span; i0 += THREADS) {
    const int i = i0 + tid;
    const long g = lo + i;
    float v[SB];
#pragma unroll
    for (int sl = 0; sl < SB; ++sl) v[sl] = in_at(x, hist_in, s0 + sl, g, i < span, B, T_in, Q);
#pragma unroll
    for (int sl = 0; sl < SB; ++sl)
      if (i < span) win_s[sl * W + i] = v[sl];
  }
  if (hist_out && blockIdx.x == 0) {
    // the new history: the last Q - 1 samples of history || x
    for (int i = tid; i < Q - 1; i += THREADS) {
      const long g = (long)T_in - (Q - 1) + i;
      float v[SB];
#pragma unroll
      for (int sl = 0; sl < SB; ++sl) v[sl] = in_at(x, hist_in, s0 + sl, g, true, B, T_in, Q);
#pragma unroll
      for (int sl = 0; sl < SB; ++sl)
        if (s0 + sl < B) hist_out[(long)(s0 + sl) * (Q - 1) + i] = v[sl];
    }
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const long m = m0 + lane;
  if (m >= T_out) return;
  const long mM = m * M;
  const int ph = (int)(mM % L);
  const int off = (int)(mM / L - lo);                   // window index of x[base]
  const float* tr = tap_s + (L <= TILE ? ph : lane) * QP;
  const int sl0 = wave * SPT;
  const float* w0 = win_s + sl0 * W + off;
  float acc[SPT];
#pragma unroll
  for (int k = 0; k < SPT; ++k) acc[k] = 0.f;
#pragma unroll 4
  for (int j = 0; j < Q; ++j) {
    const float t = tr[j];
#pragma unroll
    for (int k = 0; k < SPT; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(t, w0[k * W - j]));
  }
#pragma unroll
  for (int k = 0; k < SPT; ++k) {
    const int s = s0 + sl0 + k;
    if (s < B) y[(long)s * T_out + m] = acc[k];
  }
}

}  // namespace

extern "C" int hilc_resample_poly(const float* x, const float* hist_in, float* hist_out, float* y, const float* taps, int B, int T_in,
                                  int L, int M, int Q, void* stream) {
  if (!x || !y || !taps) return HILC_ERR_NULL;
  if (B <= 0 || T_in <= 0 || L <= 0 || M <= 0 || Q <= 1) return HILC_ERR_SHAPE;
  if (hist_in && hist_in == hist_out) return HILC_ERR_SHAPE;   // the history blocks of a hop ping-pong
  const long T_out = ((long)T_in * L + M - 1) / M;
  const long lds = 4L * ((long)tap_rows(L) * tap_stride(Q) + (long)SB * window_len(L, M, Q));
  if (lds > MAX_LDS || T_out > (1L << 30) || (long)T_in * M > (1L << 40) || (long)L * Q > (1L << 24) ||
      (B + SB - 1) / SB > 65535) return HILC_ERR_UNSUPPORTED;
  HILC_CLEAR_ERROR();
  const dim3 grid((unsigned)((T_out + TILE - 1) / TILE), (unsigned)((B + SB - 1) / SB));
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(THREADS), (size_t)lds, (hipStream_t)stream, x, hist_in, hist_out, y, taps, B,
                     T_in, (int)T_out, L, M, Q);
  HILC_CHECK_LAUNCH();
  return HILC_OK;
}
