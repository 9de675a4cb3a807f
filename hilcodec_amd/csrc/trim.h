// The cut of forward.trim_packet, shared by the forwarding hop's launches that write packet rows (forward.hip: hilc_forward_route;
// downlink.hip: hilc_downlink_step): what a valid headed packet becomes at L stages, and byte q of that row.  Packets are stage-major,
// so the first L stages are a bit prefix of the body (slot.h); the redundant section, when it survives, moves up behind them.
// The rule, bit for bit: hilcodec_amd/forward.py (trim_packet, trim_bits).
#pragma once
#include "jitter_ring.h"

namespace trim {

using namespace jring;

// What an output row is cut from: the headed packet's bytes (null: an empty row), and the cut of forward.trim_packet
struct Cut {
  const uint8_t* src;                // the headed packet's bytes; null: the row is empty
  int len;                           // bytes of the output row
  int flags;                         // its header byte 2
  int body;                          // the source's body bytes
  int prim, end, shift;              // body bits [0, prim) come from the same source bit, [prim, end) from source bit + shift
  bool sid, trimmed;
};

__device__ __forceinline__ Cut no_cut() {
  Cut c;
  c.src = nullptr;
  c.len = c.flags = c.body = c.prim = c.end = c.shift = 0;
  c.sid = c.trimmed = false;
  return c;
}

// the cut to L stages of a valid headed packet at `src`: a SID or not, with the FEC flag or not, n stages, `body` bytes behind the header
__device__ __forceinline__ Cut cut_packet(const uint8_t* src, bool sid, bool fb, int n, int body, int L, int T, int m, int keep_fec) {
  Cut c = no_cut();
  c.src = src;
  c.sid = sid;
  c.body = body;
  if (sid) {
    c.len = HILC_WIRE_TRANSPORT_HEADER + body;
    return c;
  }
  const int keep = min(n, L);
  const bool red = fb && keep_fec != 0 && keep >= m;
  c.prim = 10 * keep * T;
  c.end = c.prim + (red ? 10 * m * T : 0);
  c.shift = 10 * (n - keep) * T;
  c.flags = keep | (red ? HILC_WIRE_FEC_BIT : 0);
  c.len = HILC_WIRE_TRANSPORT_HEADER + code_bytes(c.end / 10);
  c.trimmed = keep < n;
  return c;
}

// the 8 bits from bit `bit` on of a body of `body` bytes (behind the header), zero past its last byte
__device__ __forceinline__ uint32_t window8(const uint8_t* __restrict__ src, int bit, int body) {
  const int q = bit >> 3;
  const uint32_t hi = q < body ? src[HILC_WIRE_TRANSPORT_HEADER + q] : 0u;
  const uint32_t lo = q + 1 < body ? src[HILC_WIRE_TRANSPORT_HEADER + q + 1] : 0u;
  return (((hi << 8) | lo) >> (8 - (bit & 7))) & 0xFFu;
}

// the `count` leading bits of a byte, count clamped to [0, 8]
__device__ __forceinline__ uint32_t lead_bits(int count) { return (0xFF00u >> clampi(count, 0, 8)) & 0xFFu; }

// byte q of the cut's output row, 0 from its length on
__device__ __forceinline__ uint32_t cut_byte(const Cut& c, int q) {
  uint32_t v = 0;
  if (q < c.len) {
    if (c.sid || q < 2) {
      v = c.src[q];
    } else if (q == 2) {
      v = (uint32_t)c.flags;
    } else {
      const int bit = 8 * (q - HILC_WIRE_TRANSPORT_HEADER);
      const uint32_t ma = lead_bits(c.prim - bit), mb = lead_bits(c.end - bit) & ~ma;
      if (ma) v = window8(c.src, bit, c.body) & ma;
      if (mb) v |= window8(c.src, bit + c.shift, c.body) & mb;
    }
  }
  return v;
}

}  // namespace trim
