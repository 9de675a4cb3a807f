// NACK and retransmission of the graphed hops (graph_step.GraphedDecodeHop(nack=NackConfig(...)), GraphedEncodeHop(rtx=RtxConfig(...))).
// Two launches, one per side, each one wave per slot, integer work only:
//
//   hilc_nack_build  the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step, beside hilc_rx_report: reads the slot's
//                    jitter state and the ring's meta words, keeps one entry word per ring entry (hop, requests, age) and emits a
//                    4-byte NACK (wire.pack_nack: base, bitmap) for the holes that are worth asking for.
//   hilc_rtx_step    the sender's last launch, after hilc_packet_header: stores the hop's headed packet in the slot's history ring
//                    and copies the packets a NACK asks for into the slot's retransmission rows.
//
// The rules, bit for bit: hilcodec_amd/rtx.py (NackModel, RtxModel); the rows: include/hilcodec_amd.h (HILC_RTX_*).
#include "jitter_ring.h"

namespace {

using namespace slot;

__device__ __forceinline__ uint32_t low_bits(int count) { return count >= 32 ? 0xFFFFFFFFu : ((1u << count) - 1u); }

// Lane d < C is window position d, ring entry i = (next + d) mod C: d -> i is one to one, so lane d also owns entry word i of the
// NACK row.  Occupancy, SID and FEC flags of the window are ballots (bit d: position d), i.e. ST_MASK rotated by next; the counters
// are popcounts of ballots, wave-uniform, stored by lane 0.
__global__ __launch_bounds__(THREADS) void nack_build_kernel(const int* __restrict__ jstate, const int* __restrict__ meta,
                                                             const int* __restrict__ action, int* __restrict__ rows,
                                                             uint8_t* __restrict__ nacks, int* __restrict__ due, int B, int C, int m,
                                                             int rtt_hops, int retry_hops, int max_requests, int skip_fecable) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const int* js = jstate + (long)b * HILC_JITTER_ST_WORDS;
  int* row = rows + (long)b * HILC_RTX_NK_WORDS;
  const bool start = is_reset(action, b);
  int cnt[HILC_RTX_NK_RING];
#pragma unroll
  for (int k = 0; k < HILC_RTX_NK_RING; ++k) cnt[k] = start ? 0 : row[k];
  const bool anchored = js[HILC_JITTER_ST_ANCHORED] != 0;
  const int next = js[HILC_JITTER_ST_NEXT] & 0xFFFF;
  const uint32_t mask = (uint32_t)js[HILC_JITTER_ST_MASK];
  const bool in_dtx = js[HILC_JITTER_ST_IN_DTX] != 0;
  const bool mine = lane < C;                                 // this lane is a window position
  const int d = lane;
  const int i = (next + d) & (C - 1);
  const int h = (next + d) & 0xFFFF;
  const bool occ = mine && anchored && ((mask >> i) & 1u);
  const uint32_t mt = occ ? (uint32_t)meta[(long)b * C + i] : 0u;
  uint32_t w = (mine && !start) ? (uint32_t)row[HILC_RTX_NK_RING + i] : 0u;
  // housekeeping: a word whose hop is in the window sits at that hop's position, i.e. int16(hop - next) == d
  {
    const bool pending = mine && anchored && ((w >> 16) & 255u) != 0u;
    const bool inside = jring::int16_of((int)(w & 0xFFFFu) - next) == d;
    const bool recovered = pending && inside && occ, expired = pending && !inside;
    cnt[HILC_RTX_NK_RECOVERED] += __popcll(__ballot(recovered));
    cnt[HILC_RTX_NK_EXPIRED] += __popcll(__ballot(expired));
    if (recovered || expired) w = 0u;
  }
  const uint32_t occ_b = (uint32_t)__ballot(occ);
  const uint32_t sid_b = (uint32_t)__ballot(occ && (mt & HILC_JITTER_META_SID));
  const uint32_t fec_b = (uint32_t)__ballot(occ && !(mt & HILC_JITTER_META_SID) && (mt & HILC_JITTER_META_FEC));
  const int top = occ_b ? 31 - __builtin_clz(occ_b) : 0;      // no occupied entry: no hole, the rule ends
  const bool hole = mine && anchored && !occ && d < top;
  const uint32_t below = occ_b & low_bits(d);                 // d < 32 for a hole
  const bool silent = below ? ((sid_b >> (31 - __builtin_clz(below))) & 1u) : in_dtx;
  const bool fecable = skip_fecable && m >= 1 && ((fec_b >> ((d + 1) & 31)) & 1u);       // a hole has d + 1 <= top < C
  const int count = (int)((w >> 16) & 255u), age = (int)(w >> 24);
  const bool eligible = hole && d + 1 >= rtt_hops && !silent && !fecable && (count == 0 || (age >= retry_hops && count < max_requests));
  const uint32_t elig_b = (uint32_t)__ballot(eligible);
  const int d0 = elig_b ? __builtin_ctz(elig_b) : 0;
  const bool taken = eligible && d - d0 <= 16;
  const uint32_t taken_b = (uint32_t)__ballot(taken);
  const bool emit = taken_b != 0u;
  if (taken)
    w = (uint32_t)h | ((uint32_t)(count + 1) << 16);
  else if (hole && count > 0)
    w = (w & 0xFFFFFFu) | ((uint32_t)min(age + 1, 255) << 24);
  cnt[HILC_RTX_NK_ASKED] += __popc(taken_b);
  cnt[HILC_RTX_NK_SENT] += emit ? 1 : 0;
  // entry words: lane d stores word i; on a start the words past the ring are cleared by the lanes past the window
  if (mine)
    row[HILC_RTX_NK_RING + i] = (int)w;
  else if (start && lane < HILC_RTX_NK_RING_WORDS)
    row[HILC_RTX_NK_RING + lane] = 0;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_RTX_NK_RING; ++k) row[k] = cnt[k];
    due[b] = emit ? 1 : 0;
  }
  if (lane < HILC_WIRE_NACK_BYTES && (start || emit)) {
    const uint32_t base = (uint32_t)(next + d0) & 0xFFFFu;
    const uint32_t bitmap = d0 >= 31 ? 0u : ((taken_b >> (d0 + 1)) & 0xFFFFu);
    const uint32_t both = (base << 16) | bitmap;              // big-endian: byte k is bits [24 - 8 k, 32 - 8 k)
    nacks[(long)b * HILC_WIRE_NACK_BYTES + lane] = emit ? (uint8_t)(both >> (24 - 8 * lane)) : (uint8_t)0;
  }
}

// word j of a byte row that need not be 4-byte aligned: bytes 4 j .. 4 j + 3, little-endian, zero from byte `len` on
__device__ __forceinline__ uint32_t row_word(const uint8_t* __restrict__ src, int j, int len) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * j + k < len) v |= (uint32_t)src[4 * j + k] << (8 * k);
  return v;
}

__device__ __forceinline__ void put_row(uint8_t* __restrict__ dst, int j, uint32_t v, int tb) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * j + k < tb) dst[4 * j + k] = (uint8_t)(v >> (8 * k));
}

// Lane e < R holds tag e; lane j owns word j (and j + 64, ...) of every ring row in every pass, so a packet stored on this hop and
// asked for on the same hop is read back by the lane that wrote it.  The requested hops are resolved one by one with wave-uniform
// control flow (the NACK words go through readfirstlane); only the row copies are per lane.
__global__ __launch_bounds__(THREADS) void rtx_step_kernel(const uint8_t* __restrict__ packets, const int* __restrict__ nbytes,
                                                           const int* __restrict__ nack_base, const int* __restrict__ nack_bitmap,
                                                           const int* __restrict__ action, int* __restrict__ tags,
                                                           int* __restrict__ ring, int* __restrict__ rows, uint8_t* __restrict__ out,
                                                           int* __restrict__ out_nbytes, int B, int tb, int rw, int R, int per_hop) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* trow = tags + (long)b * R;
  int* rrow = ring + (long)b * R * rw;
  int* row = rows + (long)b * HILC_RTX_RX_WORDS;
  const uint8_t* prow = packets + (long)b * tb;
  uint8_t* orow = out + (long)b * per_hop * tb;
  const bool start = is_reset(action, b);
  int cnt[HILC_RTX_RX_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_RTX_RX_WORDS; ++k) cnt[k] = row[k];
  int tag = (lane < R && !start) ? trow[lane] : 0;
  const int nb = __builtin_amdgcn_readfirstlane(min(nbytes[b], tb));
  if (nb > 0) {
    const int h = __builtin_amdgcn_readfirstlane(((int)prow[0] << 8) | (int)prow[1]);
    const int e = h & (R - 1);
    for (int j = lane; j < rw; j += LANES) rrow[(long)e * rw + j] = (int)row_word(prow, j, nb);
    if (lane == e) tag = h | (nb << 16);
    ++cnt[HILC_RTX_RX_STORED];
  }
  const int word = nack_base != nullptr ? __builtin_amdgcn_readfirstlane(nack_base[b]) : 0;
  const int bitmap = nack_base != nullptr ? __builtin_amdgcn_readfirstlane(nack_bitmap[b]) & 0xFFFF : 0;
  int q = 0;
  if (word & HILC_RTX_NACK_PRESENT) {
    ++cnt[HILC_RTX_RX_REQUESTS];
    for (int k = 0; k <= 16; ++k) {                           // wire.nack_hops: base, then base + 1 + j for every set bit j
      if (k > 0 && !((bitmap >> (k - 1)) & 1)) continue;
      const int h = ((word & 0xFFFF) + k) & 0xFFFF;
      const int e = h & (R - 1);
      const int t = __shfl(tag, e);
      if (t == 0 || (t & 0xFFFF) != h) {
        ++cnt[HILC_RTX_RX_MISS];
      } else if (q >= per_hop) {
        ++cnt[HILC_RTX_RX_DROPPED];
      } else {
        for (int j = lane; j < rw; j += LANES) put_row(orow + (long)q * tb, j, (uint32_t)rrow[(long)e * rw + j], tb);
        if (lane == 0) out_nbytes[(long)b * per_hop + q] = (int)((uint32_t)t >> 16);
        ++cnt[HILC_RTX_RX_SENT];
        ++q;
      }
    }
  }
  for (; q < per_hop; ++q) {                                  // the rows not used
    for (int j = lane; j < rw; j += LANES) put_row(orow + (long)q * tb, j, 0u, tb);
    if (lane == 0) out_nbytes[(long)b * per_hop + q] = 0;
  }
  if (lane < R) trow[lane] = tag;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_RTX_RX_WORDS; ++k) row[k] = cnt[k];
  }
}

static inline bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int hilc_nack_build(const int* jitter_state, const int* meta, const int* action, int* rows, uint8_t* nacks, int* due, int B,
                               int capacity, int m, int rtt_hops, int retry_hops, int max_requests, int skip_fecable, void* stream) {
  if (!jitter_state || !meta || !rows || !nacks || !due) return HILC_ERR_NULL;
  if (B <= 0) return HILC_ERR_SHAPE;
  if (!pow2_in(capacity, 2, HILC_RTX_NK_RING_WORDS) || m < 0 || rtt_hops < 1 || rtt_hops > 30 || retry_hops < 1 || retry_hops > 255 ||
      max_requests < 1 || max_requests > 255)
    return HILC_ERR_RANGE;
  return launch(nack_build_kernel, waves_grid(B), stream, jitter_state, meta, action, rows, nacks, due, B, capacity, m, rtt_hops,
                retry_hops, max_requests, skip_fecable != 0 ? 1 : 0);
}

extern "C" int hilc_rtx_step(const uint8_t* packets, const int* nbytes, const int* nack_base, const int* nack_bitmap, const int* action,
                             int* tags, int* ring, int* rows, uint8_t* out, int* out_nbytes, int B, int row_bytes, int history,
                             int per_hop, void* stream) {
  if (!packets || !nbytes || !tags || !ring || !rows || !out || !out_nbytes) return HILC_ERR_NULL;
  if ((nack_base == nullptr) != (nack_bitmap == nullptr)) return HILC_ERR_NULL;
  if (B <= 0 || row_bytes <= HILC_WIRE_TRANSPORT_HEADER || row_bytes >= (1 << 15)) return HILC_ERR_SHAPE;
  if (!pow2_in(history, 2, HILC_RTX_MAX_HISTORY) || per_hop < 1 || per_hop > HILC_RTX_MAX_PER_HOP) return HILC_ERR_RANGE;
  return launch(rtx_step_kernel, waves_grid(B), stream, packets, nbytes, nack_base, nack_bitmap, action, tags, ring, rows, out,
                out_nbytes, B, row_bytes, (row_bytes + 3) / 4, history, per_hop);
}
