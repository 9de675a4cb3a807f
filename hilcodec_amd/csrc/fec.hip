// In-band forward error correction of the graphed sender / receiver pair (graph_step.GraphedEncodeHop(fec_stages=m),
// GraphedDecodeHop(fec_stages=m)): the packet of hop k also carries the first m stages of the stream's hop k - 1, so a receiver
// that lost packet k but holds packet k + 1 decodes hop k from real codes.  Format (hilcodec_amd/wire.py, fec_packet_bytes):
// the 10-bit packet of the [n_b + m, T] codes cat(idx_k[:n_b], idx_{k-1}[:m]); a stream without a previous encoded hop sends
// the plain n_b-stage packet.  Two launches, one per side:
//
//   hilc_pack_codes_10bit_fec  the sender's last launch before hilc_state_slots_hold, in place of hilc_pack_codes_10bit: packets and
//                              byte counts from the indices and each stream's previous-codes row (read one parity, write the other).
//   hilc_fec_select            the receiver's launch after hilc_state_slots_apply: compacts the wide upload rows into the
//                              [B][packet_bytes(n_max, T)] rows hilc_conceal_prepare and hilc_rvq_decode_packed read — the primary
//                              section of a received packet, the redundant section (at n = m) of a slot recovered by FEC.
//
// Previous-codes row of stream b (int32, 1 + m T words): [0] valid (0/1), [1 + s T + t] code of stage s < m, frame t of the last
// encoded hop.  The packet layout and its helpers: slot.h.
#include "slot.h"

namespace {

using namespace slot;

// one thread per output byte, the shape of pack_codes_kernel; thread j < 1 + m T also writes word j of the stream's next
// previous-codes row (stride = ceil(10 (n_max + m) T / 8) >= 2.5 m T >= 1 + m T, so every word has a thread)
__global__ __launch_bounds__(THREADS) void pack_codes_fec_kernel(const int64_t* __restrict__ indices, const int* __restrict__ n_per_stream,
                                                                 const int* __restrict__ prev_in, int* __restrict__ prev_out,
                                                                 const int* __restrict__ action, const int* __restrict__ hold,
                                                                 uint8_t* __restrict__ packets, int* __restrict__ nbytes, int B, int T,
                                                                 int n_max, int m, int stride) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= (long)B * stride) return;
  const int b = (int)(e / stride);
  const int j = (int)(e - (long)b * stride);
  const int W = 1 + m * T;
  const int* pin = prev_in + (long)b * W;
  const bool reset = is_reset(action, b);                   // no previous hop
  const bool held = is_held(hold, b);
  const int nb = clamp_n(n_per_stream, (long)b, m, n_max);
  if (j < W) {
    int w;
    if (held) {
      w = reset ? 0 : pin[j];                              // a held slot keeps its row (a start on the same hop clears it)
    } else if (j == 0) {
      w = 1;
    } else {
      const int s = (j - 1) / T, t = (j - 1) - ((j - 1) / T) * T;
      w = clamp_code(indices[index_at(s, B, b, T, t)]);
    }
    prev_out[(long)b * W + j] = w;
  }
  uint32_t out = 0;
  if (held) {
    if (j == 0) nbytes[b] = 0;
  } else {
    const bool valid = !reset && pin[0] != 0;
    const int count_p = nb * T;
    const int count = count_p + (valid ? m * T : 0);
    const int len = code_bytes(count);
    if (j == 0) nbytes[b] = len;
    if (j < len) {
      const PackedByte at = packed_byte(j);
      uint32_t w = 0;
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int i = at.i0 + d;
        uint32_t c = 0;
        if (i < count_p) {
          const int s = i / T, t = i - (i / T) * T;
          c = (uint32_t)clamp_code(indices[index_at(s, B, b, T, t)]);
        } else if (i < count) {
          c = (uint32_t)pin[1 + i - count_p] & 1023u;
        }
        w = (w << 10) | c;
      }
      out = at.of(w);
    }
  }
  packets[e] = (uint8_t)out;
}

// one wave per stream (4 per workgroup): n_per_stream[b] is read by every lane before lane 0 rewrites it, inside one wave, so no
// other thread can see the rewritten value.  Output byte j = bits [start + 8 j, start + 8 j + 8) of the wide row, the bits past
// the section's 10 cnt zeroed.
__global__ __launch_bounds__(THREADS) void fec_select_kernel(const uint8_t* __restrict__ wide, const int* __restrict__ fec,
                                                             int* __restrict__ n_per_stream, uint8_t* __restrict__ out, int B, int T,
                                                             int n_max, int m, int wstride, int ostride) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const bool red = fec[b] != 0;
  const int n_in = n_per_stream[b];
  const int nb = red ? clampi(n_in, m, n_max) : clampi(n_in, 1, n_max);
  const int start = red ? 10 * nb * T : 0;               // even: a code boundary
  const int bits = 10 * (red ? m : nb) * T;
  const uint8_t* src = wide + (long)b * wstride;
  uint8_t* dst = out + (long)b * ostride;
  for (int j = lane; j < ostride; j += 64) {
    const int rem = bits - 8 * j;                         // bits of the section from this byte on
    uint32_t v = 0;
    if (rem > 0) {
      const int p = start + 8 * j;
      const int q = p >> 3, sh = p & 7;
      const uint32_t hi = src[q];
      const uint32_t lo = (sh != 0 && q + 1 < wstride) ? (uint32_t)src[q + 1] : 0u;
      v = (((hi << 8) | lo) >> (8 - sh)) & 0xFFu;
      if (rem < 8) v &= (0xFFu << (8 - rem)) & 0xFFu;
    }
    dst[j] = (uint8_t)v;
  }
  if (red && lane == 0) n_per_stream[b] = m;
}

}  // namespace

extern "C" int hilc_pack_codes_10bit_fec(const int64_t* indices, const int* n_per_stream, const int* prev_in, int* prev_out,
                                         const int* action, const int* hold, uint8_t* packets, int* nbytes, int B, int T, int n_max,
                                         int m, void* stream) {
  if (!indices || !prev_in || !prev_out || !packets || !nbytes) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || prev_in == prev_out) return HILC_ERR_SHAPE;
  if (n_max < 1 || m < 1 || m > n_max) return HILC_ERR_RANGE;
  if (n_max + m > MAX_N) return HILC_ERR_UNSUPPORTED;
  const long stride = packet_bytes<long>(n_max + m, T);
  if (stride > (1L << 30)) return HILC_ERR_SHAPE;
  return launch(pack_codes_fec_kernel, threads_grid(B * stride), stream, indices, n_per_stream, prev_in, prev_out, action, hold, packets,
                nbytes, B, T, n_max, m, (int)stride);
}

extern "C" int hilc_fec_select(const uint8_t* packets, const int* fec, int* n_per_stream, uint8_t* out, int B, int T, int n_max, int m,
                               void* stream) {
  if (!packets || !fec || !n_per_stream || !out) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || m < 1 || m > n_max) return HILC_ERR_RANGE;
  if (n_max + m > MAX_N) return HILC_ERR_UNSUPPORTED;
  const long wstride = packet_bytes<long>(n_max + m, T);
  if (wstride > (1L << 30)) return HILC_ERR_SHAPE;
  return launch(fec_select_kernel, waves_grid(B), stream, packets, fec, n_per_stream, out, B, T, n_max, m, (int)wstride,
                packet_bytes(n_max, T));
}
