// Adaptive playout of the receiver's jitter buffer (graph_step.GraphedDecodeHop(jitter=JitterConfig(..., adapt=AdaptConfig(...)))):
// hilc_jitter_adapt_step takes the place of hilc_jitter_step as the receiver graph's first launch.  Same arrivals, ring, state row and
// output rows (jitter_ring.h); beside them one adapt row per slot (HILC_JITTER_AD_*), with which the slot moves its playout clock
// against the sender's: an inserted hop (grow), a skipped entry (shrink) or a new anchor (resync).  The rules, bit for bit:
// hilcodec_amd/jitter.py (JitterModel with cfg.adapt).  Integer work only.
#include "jitter_ring.h"

namespace {

using namespace jring;

__device__ __forceinline__ void clear_control(int* ad, int C, int depth) {
#pragma unroll
  for (int k = 0; k < HILC_JITTER_AD_GROWN; ++k) ad[k] = 0;
  ad[HILC_JITTER_AD_MIN] = C;
  ad[HILC_JITTER_AD_MARGIN] = depth;
}

__device__ __forceinline__ int sign_of(int v) { return (v > 0) - (v < 0); }

// one wave per slot, the shape of jitter_step_kernel; every branch but the body copies is wave-uniform
__global__ __launch_bounds__(THREADS) void jitter_adapt_step_kernel(
    const int* __restrict__ arr, const int* __restrict__ off, int max_a, int aw, const int* __restrict__ action, int* __restrict__ hold,
    int* __restrict__ n_per_stream, int* __restrict__ lost, int* __restrict__ fec, uint8_t* __restrict__ packets, int* __restrict__ state,
    int* __restrict__ meta, int* __restrict__ ring, int* __restrict__ adapt, int B, int T, int n_max, int m, int order, int conceal,
    int depth, int C, int stride, int rw, int headroom, int max_late, int window, int resync, int force_windows) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* st = state + (long)b * HILC_JITTER_ST_WORDS;
  int* arow = adapt + (long)b * HILC_JITTER_AD_WORDS;
  int* mrow = meta + (long)b * C;
  int* rrow = ring + (long)b * C * rw;
  const bool start = is_reset(action, b);
  int s[HILC_JITTER_ST_WORDS], ad[HILC_JITTER_AD_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_JITTER_ST_WORDS; ++k) s[k] = start ? 0 : st[k];
#pragma unroll
  for (int k = 0; k < HILC_JITTER_AD_WORDS; ++k) ad[k] = start ? 0 : arow[k];
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
    const int hop = (int)p.hop;
    const int i = hop & (C - 1);
    if (!s[HILC_JITTER_ST_ANCHORED]) {
      s[HILC_JITTER_ST_ANCHORED] = 1;
      s[HILC_JITTER_ST_NEXT] = hop;
      s[HILC_JITTER_ST_WAIT] = depth;
      clear_control(ad, C, depth);
    } else {
      const int d = int16_of(hop - s[HILC_JITTER_ST_NEXT]);
      if (d < 0 || d >= C) {
        if (d < 0)
          ++s[HILC_JITTER_STAT_LATE];
        else
          ++s[HILC_JITTER_STAT_EARLY];
        const int gap = int16_of(hop - ad[HILC_JITTER_AD_LAST]);
        ad[HILC_JITTER_AD_RUN] = (ad[HILC_JITTER_AD_RUN] > 0 && (gap < 0 ? -gap : gap) < C) ? ad[HILC_JITTER_AD_RUN] + 1 : 1;
        ad[HILC_JITTER_AD_LAST] = hop;
        if (ad[HILC_JITTER_AD_RUN] < resync) {
          if (s[HILC_JITTER_ST_WAIT] == 0) {                            // dropped, but close enough to move the clock at once
            if (d < 0) {
              if (-d <= max_late) ad[HILC_JITTER_AD_DEBT] = max(ad[HILC_JITTER_AD_DEBT], -d);
            } else if (d - (C - 1) <= max_late) {
              ad[HILC_JITTER_AD_DEBT] = min(ad[HILC_JITTER_AD_DEBT], (C - 1) - d);
            }
          }
          continue;
        }
        // resync: the run of outliers is the stream; the slot anchors on this one and the ring starts empty
        s[HILC_JITTER_ST_NEXT] = hop;
        s[HILC_JITTER_ST_WAIT] = depth;
        s[HILC_JITTER_ST_IN_DTX] = 0;
        s[HILC_JITTER_ST_MASK] = 0;
        my_meta = 0u;
        clear_control(ad, C, depth);
        ++ad[HILC_JITTER_AD_RESYNC];
      } else if (((uint32_t)s[HILC_JITTER_ST_MASK] >> i) & 1u) {
        ++s[HILC_JITTER_STAT_DUPLICATE];
        ad[HILC_JITTER_AD_RUN] = 0;
        continue;
      } else {
        ad[HILC_JITTER_AD_RUN] = 0;
        if (s[HILC_JITTER_ST_WAIT] == 0) ad[HILC_JITTER_AD_MIN] = min(ad[HILC_JITTER_AD_MIN], d);
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
      const int h = s[HILC_JITTER_ST_NEXT];
      const int i = h & (C - 1), j = (h + 1) & (C - 1);
      const uint32_t mask = (uint32_t)s[HILC_JITTER_ST_MASK];
      const uint32_t mj = (uint32_t)__shfl((int)my_meta, j);
      const bool present = ((mask >> i) & 1u) != 0;
      const bool fecable = m >= 1 && ((mask >> j) & 1u) && !(mj & HILC_JITTER_META_SID) && (mj & HILC_JITTER_META_FEC);
      const bool free_hop = !present && (s[HILC_JITTER_ST_IN_DTX] || !fecable);     // noise or a loss whatever the clock does
      const bool forced = force_windows > 0 && ad[HILC_JITTER_AD_STALE] >= force_windows;
      int step = 0;
      if (ad[HILC_JITTER_AD_DEBT] != 0) {
        step = sign_of(ad[HILC_JITTER_AD_DEBT]);
        ad[HILC_JITTER_AD_DEBT] -= step;
        if (sign_of(ad[HILC_JITTER_AD_PENDING]) == step) ad[HILC_JITTER_AD_PENDING] -= step;
      } else if (ad[HILC_JITTER_AD_PENDING] != 0 && (free_hop || forced)) {
        step = sign_of(ad[HILC_JITTER_AD_PENDING]);
        ad[HILC_JITTER_AD_PENDING] -= step;
        if (!free_hop) ++ad[HILC_JITTER_AD_FORCED];
      }
      if (step != 0) {
        ad[HILC_JITTER_AD_MIN] = C;
        ad[HILC_JITTER_AD_COUNT] = 0;
        if (ad[HILC_JITTER_AD_PENDING] == 0) ad[HILC_JITTER_AD_STALE] = 0;
      }
      if (step > 0) {                                       // grow: an inserted hop, the clock stands
        ++ad[HILC_JITTER_AD_GROWN];
        if (s[HILC_JITTER_ST_IN_DTX])
          ho = HILC_SESSIONS_HOLD_SILENT;
        else if (conceal)
          lo = 1;
        else
          ho = HILC_SESSIONS_HOLD_HELD;
      } else {
        if (step < 0) {                                     // shrink: entry h is skipped, the hop plays h + 1
          if (present) {
            s[HILC_JITTER_ST_MASK] = (int)(mask & ~(1u << i));
            if (lane == i) my_meta = 0u;
          }
          s[HILC_JITTER_ST_NEXT] = (h + 1) & 0xFFFF;
          ++ad[HILC_JITTER_AD_SHRUNK];
        }
        play_entry(s, my_meta, lane, C, m, conceal, ho, no, lo, fo, src);   // its shuffles and src come after the skip
        if (++ad[HILC_JITTER_AD_COUNT] >= window) {
          if (ad[HILC_JITTER_AD_MIN] < C) {
            const int want = headroom - ad[HILC_JITTER_AD_MIN];
            ad[HILC_JITTER_AD_MARGIN] = ad[HILC_JITTER_AD_MIN];
            ad[HILC_JITTER_AD_STALE] = (want != 0 && sign_of(want) == sign_of(ad[HILC_JITTER_AD_PENDING])) ? ad[HILC_JITTER_AD_STALE] + 1 : 0;
            ad[HILC_JITTER_AD_PENDING] = want;
          }
          ad[HILC_JITTER_AD_MIN] = C;
          ad[HILC_JITTER_AD_COUNT] = 0;
        }
      }
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
#pragma unroll
    for (int k = 0; k < HILC_JITTER_AD_WORDS; ++k) arow[k] = ad[k];
  }
}

}  // namespace

extern "C" int hilc_jitter_adapt_step(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* hold,
                                      int* n_per_stream, int* lost, int* fec, uint8_t* packets, int* state, int* meta, int* ring, int B,
                                      int T, int n_max, int m, int order, int conceal, int depth, int capacity, int* adapt, int headroom,
                                      int max_late, int window, int resync, int force_windows, void* stream) {
  if (!adapt) return HILC_ERR_NULL;
  long stride = 0;
  const int rc = check_args(arrivals, offsets, max_arrivals, hold, n_per_stream, lost, fec, packets, state, meta, ring, B, T, n_max, m,
                            order, conceal, depth, capacity, &stride);
  if (rc != HILC_OK) return rc;
  if (headroom < 0 || headroom > capacity - 2 || max_late < 1 || max_late > capacity - 2) return HILC_ERR_RANGE;
  if (window < 1 || resync < 2 || force_windows < 0) return HILC_ERR_RANGE;
  const int rw = (int)((stride + 3) / 4);
  const int aw = (int)((HILC_WIRE_TRANSPORT_HEADER + stride + 3) / 4);
  return launch(jitter_adapt_step_kernel, waves_grid(B), stream, arrivals, offsets, max_arrivals, aw, action, hold, n_per_stream, lost,
                fec, packets, state, meta, ring, adapt, B, T, n_max, m, order, conceal != 0 ? 1 : 0, depth, capacity, (int)stride, rw,
                headroom, max_late, window, resync, force_windows);
}
