// What the two jitter kernels share (jitter.hip: hilc_jitter_step; jitter_adapt.hip: hilc_jitter_adapt_step): the layout of a slot's
// state row (HILC_JITTER_ST_* / STAT_* / META_*: include/hilcodec_amd.h), ring and arrival records, the header check of
// wire.parse_transport, the body copies and the play rule of one ring entry.
// The rules, bit for bit: hilcodec_amd/jitter.py.
//
// Arrival record a (int32, 1 + aw words, aw = ceil((H + stride) / 4), H = HILC_WIRE_TRANSPORT_HEADER): [0] byte count, then the headed
// packet's bytes (little-endian words).  Ring of slot b: meta int32 [C] (jitter.meta_word, 0 when free) and body int32 [C][rw], rw = ceil(stride / 4), the packet
// body zero past its length.  Lane j of the slot's wave owns body word j (and j + 64, ...) in every pass, so a body stored by an
// arrival and read back when played is read by the lane that wrote it; the meta words live in lanes 0..C-1 and move by shuffles.
// The wave-per-slot shape and the packet length: slot.h.
#pragma once
#include "slot.h"

namespace jring {

using namespace slot;

__device__ __forceinline__ int int16_of(int v) { return ((v + 0x8000) & 0xFFFF) - 0x8000; }

struct Arrival {
  bool ok, sid, fb;
  uint32_t hop;
  int n, body;                       // body: the bytes behind the header
  __device__ __forceinline__ uint32_t meta() const {
    return hop | (sid ? HILC_JITTER_META_SID : 0u) | (fb ? HILC_JITTER_META_FEC : 0u) | ((uint32_t)n << HILC_JITTER_META_N_SHIFT);
  }
};

// wire.parse_transport on one arrival record: ok = false where it raises (tb = header + stride)
__device__ __forceinline__ Arrival parse_arrival(const int* __restrict__ rec, int tb, int T, int n_max, int m, int order) {
  Arrival p;
  const int nb = rec[0];
  p.body = nb - HILC_WIRE_TRANSPORT_HEADER;
  p.ok = nb >= HILC_WIRE_TRANSPORT_HEADER && nb <= tb;
  p.hop = 0;
  uint32_t flags = 0;
  if (p.ok) {
    const uint32_t w = (uint32_t)rec[1];                    // packet bytes 0..3
    p.hop = ((w & 0xFFu) << 8) | ((w >> 8) & 0xFFu);
    flags = (w >> 16) & 0xFFu;
  }
  p.sid = (flags & HILC_WIRE_SID_BIT) != 0;
  p.fb = (flags & HILC_WIRE_FEC_BIT) != 0;
  p.n = (int)(flags & HILC_WIRE_N_MASK);
  if (p.ok) {
    if (flags & HILC_WIRE_RSV_BIT)
      p.ok = false;
    else if (p.fb && (m < 1 || p.n < m))
      p.ok = false;
    else if (p.sid)
      p.ok = order >= 0 && p.n == 0 && p.body == 1 + order;
    else
      p.ok = p.n >= 1 && p.n <= n_max && p.body == (p.fb ? packet_bytes(p.n + m, T) : packet_bytes(p.n, T));
  }
  return p;
}

// the body of an arrival into one ring row (rw words, zero past the body's length)
__device__ __forceinline__ void store_body(const int* __restrict__ rec, int* row, int body, int aw, int rw, int lane) {
  for (int j = lane; j < rw; j += 64) {
    const uint32_t lo = (uint32_t)rec[1 + j];               // body byte 4 j = packet byte 4 j + 3
    const uint32_t hi = (2 + j <= aw) ? (uint32_t)rec[2 + j] : 0u;
    uint32_t w = (lo >> 24) | (hi << 8);
    const int keep = body - 4 * j;                          // body bytes in this word
    if (keep < 4) w = keep <= 0 ? 0u : (w & ((1u << (8 * keep)) - 1u));
    row[j] = (int)w;
  }
}

// the slot's packet row: ring row `src` of `rrow`, or zeros (src < 0)
__device__ __forceinline__ void write_packet_row(uint8_t* __restrict__ prow, const int* rrow, int src, int stride, int rw, int lane) {
  for (int j = lane; j < rw; j += 64) {
    const uint32_t w = src >= 0 ? (uint32_t)rrow[(long)src * rw + j] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * j + k < stride) prow[4 * j + k] = (uint8_t)(w >> (8 * k));
  }
}

// jitter.py, play: the entry the clock s[HILC_JITTER_ST_NEXT] points at, for a slot that is anchored, primed and not held.
// Wave-uniform; every lane calls it (the meta words move by shuffles).
__device__ __forceinline__ void play_entry(int* s, uint32_t& my_meta, int lane, int C, int m, int conceal, int& ho, int& no, int& lo,
                                           int& fo, int& src) {
  const int h = s[HILC_JITTER_ST_NEXT];
  const int i = h & (C - 1), j = (h + 1) & (C - 1);
  uint32_t mask = (uint32_t)s[HILC_JITTER_ST_MASK];
  const uint32_t mi = (uint32_t)__shfl((int)my_meta, i);
  const uint32_t mj = (uint32_t)__shfl((int)my_meta, j);
  if ((mask >> i) & 1u) {
    src = i;
    if (mi & HILC_JITTER_META_SID) {
      ho = HILC_SESSIONS_HOLD_SID;
      s[HILC_JITTER_ST_IN_DTX] = 1;
      ++s[HILC_JITTER_STAT_NOISE];
    } else {
      no = (int)(mi >> HILC_JITTER_META_N_SHIFT);
      s[HILC_JITTER_ST_IN_DTX] = 0;
      ++s[HILC_JITTER_STAT_DECODED];
    }
    mask &= ~(1u << i);
    if (lane == i) my_meta = 0u;
  } else if (s[HILC_JITTER_ST_IN_DTX]) {
    ho = HILC_SESSIONS_HOLD_SILENT;
    ++s[HILC_JITTER_STAT_NOISE];
  } else if (m >= 1 && ((mask >> j) & 1u) && !(mj & HILC_JITTER_META_SID) && (mj & HILC_JITTER_META_FEC)) {
    src = j;
    fo = 1;
    no = (int)(mj >> HILC_JITTER_META_N_SHIFT);
    ++s[HILC_JITTER_STAT_FEC];
  } else {
    if (conceal)
      lo = 1;
    else
      ho = HILC_SESSIONS_HOLD_HELD;
    ++s[HILC_JITTER_STAT_LOST];
  }
  s[HILC_JITTER_ST_MASK] = (int)mask;
  s[HILC_JITTER_ST_NEXT] = (h + 1) & 0xFFFF;
}

// the argument checks both entry points share; on HILC_OK *stride is the packet row's bytes
static inline int check_args(const void* arrivals, const void* offsets, int max_arrivals, const void* hold, const void* n_per_stream,
                             const void* lost, const void* fec, const void* packets, const void* state, const void* meta,
                             const void* ring, int B, int T, int n_max, int m, int order, int conceal, int depth, int capacity,
                             long* stride) {
  if (!arrivals || !offsets || !hold || !n_per_stream || !packets || !state || !meta || !ring) return HILC_ERR_NULL;
  if ((conceal != 0 && !lost) || (m >= 1 && !fec)) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || max_arrivals < 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || m < 0 || m > n_max || order < -1 || order > HILC_DTX_MAX_ORDER) return HILC_ERR_RANGE;
  if (capacity < 2 || capacity > 32 || (capacity & (capacity - 1)) || depth < 0 || depth > capacity - 2) return HILC_ERR_RANGE;
  if (n_max > 31 || n_max + m > MAX_N) return HILC_ERR_UNSUPPORTED;
  *stride = packet_bytes<long>(n_max + m, T);
  if (*stride > (1L << 29) || (order >= 0 && 1 + order > *stride)) return HILC_ERR_SHAPE;
  return HILC_OK;
}

}  // namespace jring
