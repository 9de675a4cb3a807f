// Transport header and jitter buffer of the graphed sender / receiver pair (graph_step.GraphedEncodeHop(header=True),
// GraphedDecodeHop(jitter=JitterConfig(...))).  Format: hilcodec_amd/wire.py (pack_transport); the receiver's rules, bit for bit:
// hilcodec_amd/jitter.py (JitterModel).  Two launches, one per side, integer work only:
//
//   hilc_packet_header  the sender's last launch (after hilc_state_slots_hold, and after hilc_dtx_encode with DTX): prefixes each
//                       packet with its slot's hop counter, SID / FEC flags and n, and advances the counter (read one parity, write
//                       the other, as the FEC previous-codes rows).
//   hilc_jitter_step    the receiver's first launch: takes this hop's arrivals of each slot into its ring, plays the entry the slot's
//                       clock points at and writes the hold, n, lost and fec rows and the packet matrix the explicit step() uploads.
//
// The layout of the arrival records and the ring, and what the adaptive kernel (jitter_adapt.hip) shares: jitter_ring.h.
#include "jitter_ring.h"

namespace {

using namespace jring;

// one thread per output byte, the shape of pack_codes_kernel; thread 0 of a row writes its byte count and next counter
__global__ __launch_bounds__(THREADS) void packet_header_kernel(const uint8_t* __restrict__ packets, const int* __restrict__ nbytes,
                                                                const int* __restrict__ n_per_stream, const int* __restrict__ kind,
                                                                const int* __restrict__ action, const int* __restrict__ hold,
                                                                const int* __restrict__ ctr_in, int* __restrict__ ctr_out,
                                                                uint8_t* __restrict__ out, int* __restrict__ out_nbytes, int B, int T,
                                                                int n_max, int m, int istride, int ostride) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= (long)B * ostride) return;
  const int b = (int)(e / ostride);
  const int j = (int)(e - (long)b * ostride);
  const bool reset = is_reset(action, b);                   // the counter restarts at 0
  const bool held = is_held(hold, b);
  const int cur = reset ? 0 : (ctr_in[b] & 0xFFFF);
  const int len = held ? 0 : clampi(nbytes[b], 0, istride);
  if (j == 0) {
    ctr_out[b] = held ? cur : ((cur + 1) & 0xFFFF);         // a DTX SILENT hop (len 0, not held) advances it too
    out_nbytes[b] = len > 0 ? HILC_WIRE_TRANSPORT_HEADER + len : 0;
  }
  uint32_t v = 0;
  if (len > 0) {
    if (j == 0) {
      v = (uint32_t)cur >> 8;
    } else if (j == 1) {
      v = (uint32_t)cur & 0xFFu;
    } else if (j == 2) {
      if (kind != nullptr && kind[b] == HILC_DTX_SID) {
        v = HILC_WIRE_SID_BIT;
      } else {
        const int nb = clamp_n(n_per_stream, (long)b, m > 1 ? m : 1, n_max);
        v = (uint32_t)nb | ((m >= 1 && len == packet_bytes(nb + m, T)) ? HILC_WIRE_FEC_BIT : 0u);
      }
    } else if (j - HILC_WIRE_TRANSPORT_HEADER < len) {
      v = packets[(long)b * istride + (j - HILC_WIRE_TRANSPORT_HEADER)];
    }
  }
  out[e] = (uint8_t)v;
}

// one wave per slot; every branch but the body copies is wave-uniform
__global__ __launch_bounds__(THREADS) void jitter_step_kernel(const int* __restrict__ arr, const int* __restrict__ off, int max_a, int aw,
                                                              const int* __restrict__ action, int* __restrict__ hold,
                                                              int* __restrict__ n_per_stream, int* __restrict__ lost, int* __restrict__ fec,
                                                              uint8_t* __restrict__ packets, int* __restrict__ state, int* __restrict__ meta,
                                                              int* __restrict__ ring, int B, int T, int n_max, int m, int order,
                                                              int conceal, int depth, int C, int stride, int rw) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* st = state + (long)b * HILC_JITTER_ST_WORDS;
  int* mrow = meta + (long)b * C;
  int* rrow = ring + (long)b * C * rw;
  const bool start = is_reset(action, b);
  int s[HILC_JITTER_ST_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_JITTER_ST_WORDS; ++k) s[k] = start ? 0 : st[k];
  uint32_t my_meta = (lane < C && !start) ? (uint32_t)mrow[lane] : 0u;
  const int tb = HILC_WIRE_TRANSPORT_HEADER + stride;
  const int a0 = clampi(off[b], 0, max_a);
  const int a1 = clampi(off[b + 1], a0, max_a);
  for (int a = a0; a < a1; ++a) {
    const int* rec = arr + (long)a * (1 + aw);
    const Arrival p = parse_arrival(rec, tb, T, n_max, m, order);
    if (!p.ok) {
      ++s[HILC_JITTER_STAT_MALFORMED];
      continue;
    }
    const int i = (int)p.hop & (C - 1);
    if (!s[HILC_JITTER_ST_ANCHORED]) {
      s[HILC_JITTER_ST_ANCHORED] = 1;
      s[HILC_JITTER_ST_NEXT] = (int)p.hop;
      s[HILC_JITTER_ST_WAIT] = depth;
    } else {
      const int d = int16_of((int)p.hop - s[HILC_JITTER_ST_NEXT]);
      if (d < 0) {
        ++s[HILC_JITTER_STAT_LATE];
        continue;
      }
      if (d >= C) {
        ++s[HILC_JITTER_STAT_EARLY];
        continue;
      }
      if (((uint32_t)s[HILC_JITTER_ST_MASK] >> i) & 1u) {
        ++s[HILC_JITTER_STAT_DUPLICATE];
        continue;
      }
    }
    if (lane == i) my_meta = p.meta();
    store_body(rec, rrow + (long)i * rw, p.body, aw, rw, lane);
    s[HILC_JITTER_ST_MASK] = (int)((uint32_t)s[HILC_JITTER_ST_MASK] | (1u << i));
    ++s[HILC_JITTER_STAT_ACCEPTED];
  }

  // play
  const int hin = hold[b];
  int ho = hin, no = n_max, lo = 0, fo = 0, src = -1;
  if (hin == 0) {
    if (!s[HILC_JITTER_ST_ANCHORED]) {
      ho = HILC_SESSIONS_HOLD_HELD;
    } else if (s[HILC_JITTER_ST_WAIT] > 0) {
      --s[HILC_JITTER_ST_WAIT];
      ho = HILC_SESSIONS_HOLD_HELD;
    } else {
      play_entry(s, my_meta, lane, C, m, conceal, ho, no, lo, fo, src);
    }
  }
  write_packet_row(packets + (long)b * stride, rrow, src, stride, rw, lane);
  if (lane < C) mrow[lane] = (int)my_meta;
  if (lane == 0) {
    hold[b] = ho;
    n_per_stream[b] = no;
    if (lost != nullptr) lost[b] = lo;
    if (fec != nullptr) fec[b] = fo;
#pragma unroll
    for (int k = 0; k < HILC_JITTER_ST_WORDS; ++k) st[k] = s[k];
  }
}

}  // namespace

extern "C" int hilc_packet_header(const uint8_t* packets, const int* nbytes, const int* n_per_stream, const int* kind, const int* action,
                                  const int* hold, const int* counter_in, int* counter_out, uint8_t* out, int* out_nbytes, int B, int T,
                                  int n_max, int m, void* stream) {
  if (!packets || !nbytes || !counter_in || !counter_out || !out || !out_nbytes) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || counter_in == counter_out) return HILC_ERR_SHAPE;
  if (n_max < 1 || m < 0 || m > n_max) return HILC_ERR_RANGE;
  if (n_max > 31 || n_max + m > MAX_N) return HILC_ERR_UNSUPPORTED;
  const long istride = packet_bytes<long>(n_max + m, T);
  if (istride > (1L << 29)) return HILC_ERR_SHAPE;
  const long ostride = HILC_WIRE_TRANSPORT_HEADER + istride;
  return launch(packet_header_kernel, threads_grid(B * ostride), stream, packets, nbytes, n_per_stream, kind, action, hold, counter_in,
                counter_out, out, out_nbytes, B, T, n_max, m, (int)istride, (int)ostride);
}

extern "C" int hilc_jitter_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold,
                                int* n_per_stream, int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B, int T,
                                int n_max, int m, int order, int conceal, int depth, int capacity, void* stream) {
  long stride = 0;
  const int rc = check_args(arrivals, offsets, max_arrivals, hold, n_per_stream, lost, fec, packets, state, meta, ring, B, T, n_max, m,
                            order, conceal, depth, capacity, &stride);
  if (rc != HILC_OK) return rc;
  const int rw = (int)((stride + 3) / 4);
  const int aw = (int)((HILC_WIRE_TRANSPORT_HEADER + stride + 3) / 4);
  return launch(jitter_step_kernel, waves_grid(B), stream, arrivals, offsets, max_arrivals, aw, action, hold, n_per_stream, lost, fec,
                packets, state, meta, ring, B, T, n_max, m, order, conceal != 0 ? 1 : 0, depth, capacity, (int)stride, rw);
}
