// The vocabulary of the per-slot kernels around the codec (packets, fec, conceal, dtx, jitter, jitter_adapt, mix, vbr, state): one
// wave per slot, the launchers' tail, the lane-ordered float64 sum, the 10-bit packet format, the control rows and the stage-major
// index address.  Every helper is a __forceinline__ restatement of what those kernels spelled out one by one; the bit-exact CPU
// models (wire.py, mixer.py, vbr.py) define the packed byte and the lane-ordered sum, so each exists once, here.
//
// Packet of stream b for one hop of T frames: its first n_b stages x T codes in stage-major order (stage 0's T frames first), 10 bits
// per code, MSB first, the last byte zero-padded: packet_bytes(n_b, T) = ceil(10 n_b T / 8) bytes — the body of
// wire.pack_indices_10bit(indices[:n_b, b:b+1, :]) without its header.  A batch of packets is `[B][stride]` bytes, stride =
// packet_bytes(n_max, T), row b's bytes past its own length zero.  Code i occupies bits [10 i, 10 i + 10); 10 i is even, so its bit
// offset inside its first byte is 0, 2, 4 or 6 and every code lies inside two consecutive bytes, both inside the packet.  Byte j
// holds bits [8 j, 8 j + 8), i.e. parts of codes i0 = 8 j / 10 and i0 + 1: a 20-bit window, the byte at bit offset 8 j - 10 i0 in
// {0, 2, 4, 6, 8} of it (packed_byte).
#pragma once
#include "common.h"

namespace slot {

constexpr int THREADS = 256;
constexpr int LANES = 64;
constexpr int WAVES = THREADS / LANES;
constexpr int MAX_N = HILC_WIRE_MAX_STAGES;   // stages of one packet (primary + redundant): hilc_rvq_decode_packed stages that many per frame in LDS

// ---- one wave per slot (WAVES slots per workgroup); a ragged last workgroup's spare waves are out of range and leave at once
struct Wave {
  int w, b;                          // wave of the workgroup, slot (wave-uniform)
  bool ok;                           // b < B
  __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
};

__device__ __forceinline__ Wave this_wave(int B) {
  Wave me;
  me.w = (int)threadIdx.x >> 6;
  me.b = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WAVES + me.w);
  me.ok = me.b < B;
  return me;
}

static inline dim3 waves_grid(int B) { return dim3((unsigned)((B + WAVES - 1) / WAVES)); }

// one thread per element of a flat range
static inline dim3 threads_grid(long total) { return dim3((unsigned)((total + THREADS - 1) / THREADS)); }

// a launcher's tail: THREADS threads per workgroup, no dynamic LDS; HILC_OK or HILC_ERR_LAUNCH
template <typename... P, typename... A>
static inline int launch(void (*kernel)(P...), dim3 grid, void* stream, A... args) {
  HILC_CLEAR_ERROR();
  hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, static_cast<P>(args)...);
  HILC_CHECK_LAUNCH();
  return HILC_OK;
}

// ---- small arithmetic
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(u & 0xFFFFFFFFll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// the wave's 64 partials in lane order: lane 0's, then lanes 1..63 added one by one, each sum rounded (mixer.py, vbr.py)
__device__ __forceinline__ double lane_ordered_sum(double partial) {
  double e = readlane_d(partial, 0);
#pragma unroll
  for (int l = 1; l < LANES; ++l) e = __dadd_rn(e, readlane_d(partial, l));
  return e;
}

// ---- the 10-bit packet (layout: the head of this file)
template <typename I>
__host__ __device__ __forceinline__ I code_bytes(I count) { return (10 * count + 7) >> 3; }     // bytes of `count` codes

template <typename I>
__host__ __device__ __forceinline__ I packet_bytes(I n, I T) { return code_bytes(n * T); }      // wire.packet_bytes

__device__ __forceinline__ int clamp_code(int64_t k) { return (int)(k < 0 ? 0 : (k > 1023 ? 1023 : k)); }

// stages of stream b's packet: n_max without a per-stream row, else its entry clamped to [lo, n_max].  I: int or long, the same
// value either way (the thread-per-byte packers hand in the width of their other row addresses, which the compiler then shares)
template <typename I>
__device__ __forceinline__ int clamp_n(const int* n_per_stream, I b, int lo, int n_max) {
  return n_per_stream == nullptr ? n_max : clampi(n_per_stream[b], lo, n_max);
}

// the code at bit offset `bit` (a multiple of 10) of a packet row
__device__ __forceinline__ int code_at(const uint8_t* row, int bit) {
  const uint8_t* q = row + (bit >> 3);
  const uint32_t v = ((uint32_t)q[0] << 8) | (uint32_t)q[1];
  return (int)((v >> (6 - (bit & 7))) & 1023u);
}

// byte j of a packet: cut from the 20-bit window (c0 << 10) | c1 of code i0 and the code after it (0 past the packet's last)
struct PackedByte {
  int i0, off;                       // 8 j / 10; the byte's bit offset in the window: 0, 2, 4, 6 or 8
  __device__ __forceinline__ uint32_t of(uint32_t window) const { return (window >> (12 - off)) & 0xFFu; }
};

__device__ __forceinline__ PackedByte packed_byte(int j) {
  PackedByte p;
  p.i0 = (8 * j) / 10;
  p.off = 8 * j - 10 * p.i0;
  return p;
}

// ---- control rows of a hop (a null row: no slot starts / is held).  conceal_prepare_kernel loads its rows, never null, in one round with
// the rest of the slot, and vbr_select_kernel reads them through readfirstlane: those two keep their own form.
__device__ __forceinline__ bool is_reset(const int* action, long b) { return action != nullptr && action[b] != 0; }   // a start or a resume

__device__ __forceinline__ bool is_held(const int* hold, long b) { return hold != nullptr && hold[b] != 0; }

// ---- stage-major indices [n][B][T]
__device__ __forceinline__ long index_at(long s, long B, long b, long T, long t) { return (s * B + b) * T + t; }

// rows [s0, n) of slot b to -1 ("no code"), by the slot's wave
__device__ __forceinline__ void clear_rows(int64_t* indices, int s0, int n, int B, int b, int T, int lane) {
  const int cut = (n - s0) * T;
  for (int i = lane; i < cut; i += LANES) {
    const int s = s0 + i / T, t = i - (i / T) * T;
    indices[index_at(s, B, b, T, t)] = -1;
  }
}

}  // namespace slot
