// Per-stream 10-bit packets of a streaming hop: the sender's last launch (codes -> packets) and the receiver's first
// (packets -> the dequantised latent the decoder reads).  The packet layout and its helpers: slot.h.
#include "slot.h"

namespace {

using namespace slot;

constexpr int DEQ_MAX_FRAMES = 16;  // frames per workgroup of the packed dequantiser

// one thread per output byte
__global__ __launch_bounds__(THREADS) void pack_codes_kernel(const int64_t* __restrict__ indices, const int* __restrict__ n_per_stream,
                                                             uint8_t* __restrict__ packets, int* __restrict__ nbytes, int B, int T,
                                                             int n_max, int stride) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= (long)B * stride) return;
  const int b = (int)(e / stride);
  const int j = (int)(e - (long)b * stride);
  const int nb = clamp_n(n_per_stream, b, 1, n_max);
  const int count = nb * T;
  const int len = packet_bytes(nb, T);
  if (j == 0) nbytes[b] = len;
  uint32_t out = 0;
  if (j < len) {
    const PackedByte at = packed_byte(j);              // at.i0 < count because 8 j < 10 count
    uint32_t w = 0;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int i = at.i0 + d;
      uint32_t c = 0;
      if (i < count) {
        const int s = i / T, t = i - (i / T) * T;
        c = (uint32_t)clamp_code(indices[index_at(s, B, b, T, t)]);
      }
      w = (w << 10) | c;
    }
    out = at.of(w);
  }
  packets[e] = (uint8_t)out;
}

// workgroup = F consecutive frames g = b * T + t (F = 256 / C, at most 16).  Phase 1: every (frame, stage) code of the tile is
// taken out of its packet once, into LDS.  Phase 2: element (frame, c) sums the codebook rows in stage order, the chain of
// rvq_decode_kernel (acc = 0; acc = acc + cb[s][k][c]; no contraction), so the result is that kernel's to the bit.
__global__ __launch_bounds__(THREADS) void rvq_decode_packed_kernel(const uint8_t* __restrict__ packets, const int* __restrict__ n_per_stream,
                                                                    const float* __restrict__ cb, float* __restrict__ q, int B, int C,
                                                                    int T, int K, int n_max, int stride, int F) {
  __shared__ int codes[DEQ_MAX_FRAMES][MAX_N];
  __shared__ int nbs[DEQ_MAX_FRAMES];
  const long frames = (long)B * T;
  const long g0 = (long)blockIdx.x * F;
  for (int w = threadIdx.x; w < F * n_max; w += THREADS) {
    const int f = w / n_max, s = w - (w / n_max) * n_max;
    const long g = g0 + f;
    if (g >= frames) continue;
    const int b = (int)(g / T), t = (int)(g - (long)(g / T) * T);
    const int nb = clamp_n(n_per_stream, b, 1, n_max);
    if (s == 0) nbs[f] = nb;
    if (s < nb) {
      const int bit = 10 * (s * T + t);
      codes[f][s] = code_at(packets + (long)b * stride, bit);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < F * C; e += THREADS) {
    const int f = e / C, c = e - (e / C) * C;
    const long g = g0 + f;
    if (g >= frames) break;                            // e only grows: later elements lie in later frames
    const int nb = nbs[f];
    float acc = 0.f;
    for (int s = 0; s < nb; ++s) acc = acc + cb[((long)s * K + codes[f][s]) * C + c];
    q[g * C + c] = acc;
  }
}

}  // namespace

extern "C" int hilc_pack_codes_10bit(const int64_t* indices, const int* n_per_stream, uint8_t* packets, int* nbytes, int B, int T,
                                     int n_max, void* stream) {
  if (!indices || !packets || !nbytes) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0) return HILC_ERR_SHAPE;
  if (n_max < 1) return HILC_ERR_RANGE;
  const long stride = packet_bytes<long>(n_max, T);
  if (stride > (1L << 30)) return HILC_ERR_SHAPE;
  return launch(pack_codes_kernel, threads_grid(B * stride), stream, indices, n_per_stream, packets, nbytes, B, T, n_max, (int)stride);
}

extern "C" int hilc_rvq_decode_packed(const uint8_t* packets, const int* n_per_stream, const float* codebooks, float* q, int B, int C,
                                      int T, int K, int Nq, int n_max, void* stream) {
  if (!packets || !codebooks || !q) return HILC_ERR_NULL;
  if (B <= 0 || C <= 0 || T <= 0 || K <= 0 || Nq <= 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || n_max > Nq) return HILC_ERR_RANGE;
  if (K != 1024 || n_max > MAX_N) return HILC_ERR_UNSUPPORTED;
  const int stride = packet_bytes(n_max, T);
  const int F = C >= THREADS ? 1 : (THREADS / C > DEQ_MAX_FRAMES ? DEQ_MAX_FRAMES : THREADS / C);
  const long frames = (long)B * T;
  return launch(rvq_decode_packed_kernel, dim3((unsigned)((frames + F - 1) / F)), stream, packets, n_per_stream, codebooks, q, B, C, T,
                K, n_max, stride, F);
}
