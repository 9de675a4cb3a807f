// Delay-based bandwidth estimation of the graphed hops (graph_step.GraphedDecodeHop(bwe=BweConfig(...)),
// GraphedEncodeHop(cap=CapConfig(...))).  Two launches, one per side, integer work only:
//
//   hilc_rx_bwe    the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step, beside hilc_rx_report and hilc_nack_build:
//                  reads the hop's arrival records and their arrival ticks, takes one delay sample per in-order arrival (accumulated and
//                  smoothed delay, least-squares trend over a window, adaptive threshold, over-use detector), runs the AIMD controller
//                  on the incoming rate it measures and emits a 3-byte cap (wire.pack_cap) every `interval` hops or at once after a
//                  decrease.  One THREAD per slot: a slot's arrivals are a sequence, each step a few words of its own row.
//   hilc_rate_cap  the sender's launch directly in front of hilc_rate_ceiling: takes the slot's cap of this hop by that kernel's
//                  sequence rule and keeps the rate row's rate at or below it.  One wave per slot, like hilc_rate_ceiling.
//
// The rules, bit for bit: hilcodec_amd/bwe.py (BweModel, CapModel); the rows: include/hilcodec_amd.h (HILC_BWE_*).  The header check of
// an arrival is jitter_ring.h's.  A slot's two rings stay in its row in global memory: the thread that writes them is the one that reads
// them back.  Every 64-bit product is bounded in bwe.py's docstring.
#include "jitter_ring.h"

namespace {

using namespace slot;

struct BweParams {
  int T, n_max, m, order, tb, aw;
  int min_q8, max_q8, window, rate_window, alpha_q8, beta_q8, increase_q16, interval, reset_ticks;
};

__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one pair into a ring of `size` pairs (n entries, head the next to be written)
__device__ __forceinline__ void ring_push(int* ring, int& n, int& head, int size, int a, int b) {
  ring[2 * head] = a;
  ring[2 * head + 1] = b;
  head = head + 1 >= size ? 0 : head + 1;
  n = min(n + 1, size);
}

// the trendline's slope in Q16 over a full window (oldest entry: head)
__device__ __forceinline__ int trend_slope(const int* trend, int head, int W) {
  const uint32_t t0 = (uint32_t)trend[2 * head];
  const long long y0 = trend[2 * head + 1];
  long long sx = 0, sy = 0, sxy = 0, sxx = 0;
  int idx = head;
  for (int i = 0; i < W; ++i) {
    const long long x = (long long)(((uint32_t)trend[2 * idx] - t0) >> 4);
    const long long y = (long long)trend[2 * idx + 1] - y0;
    sx += x;
    sy += y;
    sxy += x * y;
    sxx += x * x;
    idx = idx + 1 >= W ? 0 : idx + 1;
  }
  const long long num = W * sxy - sx * sy, den = W * sxx - sx * sx;
  if (den <= 0) return 0;
  return (int)clampll(floor_div(16 * num, den), -HILC_BWE_SLOPE_MAX, HILC_BWE_SLOPE_MAX);
}

// R_q8 of the rate ring, -1 when it is not valid
__device__ __forceinline__ long long incoming_q8(const int* ring, int n, int head, int size, int T) {
  if (n < HILC_BWE_RATE_MIN) return -1;
  int idx = head - n;
  if (idx < 0) idx += size;
  const uint32_t t0 = (uint32_t)ring[2 * idx];
  uint32_t t1 = t0;
  long long bits = 0;
  for (int i = 1; i < n; ++i) {
    idx = idx + 1 >= size ? 0 : idx + 1;
    bits += ring[2 * idx + 1];
    t1 = (uint32_t)ring[2 * idx];
  }
  const long long span = (long long)(t1 - t0);
  if (span <= 0) return -1;
  return (bits * 256 * HILC_BWE_HOP_TICKS * T) / span;        // both non-negative
}

__global__ __launch_bounds__(THREADS) void rx_bwe_kernel(const int* __restrict__ arr, const int* __restrict__ off,
                                                         const int* __restrict__ times, int max_a, const int* __restrict__ action,
                                                         int* rows, uint8_t* __restrict__ caps, int* __restrict__ due, int B,
                                                         BweParams p) {
  const int b = (int)blockIdx.x * THREADS + (int)threadIdx.x;
  if (b >= B) return;
  int* row = rows + (long)b * HILC_BWE_BW_WORDS;
  int* trend = row + HILC_BWE_BW_TREND;
  int* ring = row + HILC_BWE_BW_RING;
  const bool start = is_reset(action, b);
  int r[HILC_BWE_BW_TREND];
#pragma unroll
  for (int k = 0; k < HILC_BWE_BW_TREND; ++k) r[k] = start ? 0 : row[k];
  if (start) {
    r[HILC_BWE_BW_RATE_Q8] = p.max_q8;
    r[HILC_BWE_BW_THR] = HILC_BWE_THR_START;
    for (int k = HILC_BWE_BW_TREND; k < HILC_BWE_BW_WORDS; ++k) row[k] = 0;
  }
  // a row this kernel wrote is in range already
  r[HILC_BWE_BW_N] = clampi(r[HILC_BWE_BW_N], 0, p.window);
  r[HILC_BWE_BW_HEAD] = clampi(r[HILC_BWE_BW_HEAD], 0, p.window - 1);
  r[HILC_BWE_BW_RN] = clampi(r[HILC_BWE_BW_RN], 0, p.rate_window);
  r[HILC_BWE_BW_RHEAD] = clampi(r[HILC_BWE_BW_RHEAD], 0, p.rate_window - 1);
  bool decreased = false;
  const int a0 = clampi(off[b], 0, max_a);
  const int a1 = clampi(off[b + 1], a0, max_a);
  for (int a = a0; a < a1; ++a) {
    const int* rec = arr + (long)a * (1 + p.aw);
    const jring::Arrival q = jring::parse_arrival(rec, p.tb, p.T, p.n_max, p.m, p.order);
    if (!q.ok) {
      ++r[HILC_BWE_BW_MALFORMED];
      continue;
    }
    const int h = (int)q.hop, t = times[a], nbits = 8 * rec[0];
    const bool first = r[HILC_BWE_BW_SEEN] == 0;
    int dh = 0, da = 0;
    if (!first) {
      dh = jring::int16_of(h - r[HILC_BWE_BW_LAST_H]);
      if (dh <= 0) {
        ++r[HILC_BWE_BW_OLD];
        continue;
      }
      da = (int)((uint32_t)t - (uint32_t)r[HILC_BWE_BW_LAST_T]);
    }
    r[HILC_BWE_BW_LAST_H] = h;
    r[HILC_BWE_BW_LAST_T] = t;
    if (first || da < 0 || da > p.reset_ticks) {
      if (first) {
        r[HILC_BWE_BW_SEEN] = 1;
      } else {
        ++r[HILC_BWE_BW_RESET];
        r[HILC_BWE_BW_THR] = HILC_BWE_THR_START;
        r[HILC_BWE_BW_ACC] = r[HILC_BWE_BW_SM] = r[HILC_BWE_BW_COUNT] = r[HILC_BWE_BW_PREV_M] = 0;
        r[HILC_BWE_BW_OVER_TICKS] = r[HILC_BWE_BW_OVER_COUNT] = r[HILC_BWE_BW_SIGNAL] = 0;
        r[HILC_BWE_BW_N] = r[HILC_BWE_BW_HEAD] = 0;
      }
      r[HILC_BWE_BW_RN] = r[HILC_BWE_BW_RHEAD] = 0;
      if (!q.sid) ring_push(ring, r[HILC_BWE_BW_RN], r[HILC_BWE_BW_RHEAD], p.rate_window, t, nbits);
      continue;
    }
    if (q.sid)
      r[HILC_BWE_BW_RN] = r[HILC_BWE_BW_RHEAD] = 0;
    else
      ring_push(ring, r[HILC_BWE_BW_RN], r[HILC_BWE_BW_RHEAD], p.rate_window, t, nbits);
    ++r[HILC_BWE_BW_SAMPLES];
    const long long d = clampll((long long)da - (long long)HILC_BWE_HOP_TICKS * p.T * dh, -HILC_BWE_ACC_MAX, HILC_BWE_ACC_MAX);
    const int acc = (int)clampll((long long)r[HILC_BWE_BW_ACC] + d, -HILC_BWE_ACC_MAX, HILC_BWE_ACC_MAX);
    int sm = r[HILC_BWE_BW_SM];
    sm += (int)(((256LL * acc - sm) * p.alpha_q8) >> 8);
    r[HILC_BWE_BW_ACC] = acc;
    r[HILC_BWE_BW_SM] = sm;
    ring_push(trend, r[HILC_BWE_BW_N], r[HILC_BWE_BW_HEAD], p.window, t, sm);
    const int count = min(r[HILC_BWE_BW_COUNT] + 1, HILC_BWE_COUNT_MAX);
    r[HILC_BWE_BW_COUNT] = count;
    const int slope = r[HILC_BWE_BW_N] >= p.window ? trend_slope(trend, r[HILC_BWE_BW_HEAD], p.window) : 0;
    const int m = slope * count * 4;
    const int thr = r[HILC_BWE_BW_THR];
    if (m > thr) {
      r[HILC_BWE_BW_OVER_TICKS] = min(r[HILC_BWE_BW_OVER_TICKS] + da, 1 << 30);
      r[HILC_BWE_BW_OVER_COUNT] = min(r[HILC_BWE_BW_OVER_COUNT] + 1, 1 << 30);
      if (r[HILC_BWE_BW_OVER_TICKS] > HILC_BWE_OVER_TICKS && r[HILC_BWE_BW_OVER_COUNT] > 1 && m >= r[HILC_BWE_BW_PREV_M]) {
        r[HILC_BWE_BW_SIGNAL] = HILC_BWE_SIGNAL_OVERUSE;
        ++r[HILC_BWE_BW_OVERUSE];
        r[HILC_BWE_BW_OVER_TICKS] = r[HILC_BWE_BW_OVER_COUNT] = 0;
      }
    } else {
      if (m < -thr) {
        r[HILC_BWE_BW_UNDERUSE] += r[HILC_BWE_BW_SIGNAL] != HILC_BWE_SIGNAL_UNDERUSE;
        r[HILC_BWE_BW_SIGNAL] = HILC_BWE_SIGNAL_UNDERUSE;
      } else {
        r[HILC_BWE_BW_SIGNAL] = HILC_BWE_SIGNAL_NORMAL;
      }
      r[HILC_BWE_BW_OVER_TICKS] = r[HILC_BWE_BW_OVER_COUNT] = 0;
    }
    r[HILC_BWE_BW_PREV_M] = m;
    const int am = m < 0 ? -m : m;
    if (am - thr <= HILC_BWE_THR_SKIP) {
      const long long prod = (long long)(am - thr) * min(da, HILC_BWE_ADAPT_TICKS) * (am < thr ? HILC_BWE_K_DOWN : HILC_BWE_K_UP);
      r[HILC_BWE_BW_THR] = (int)clampll(thr + (prod >> 24), HILC_BWE_THR_MIN, HILC_BWE_THR_MAX);
    }
    int rate = r[HILC_BWE_BW_RATE_Q8];
    if (r[HILC_BWE_BW_SIGNAL] == HILC_BWE_SIGNAL_OVERUSE) {
      const long long R = incoming_q8(ring, r[HILC_BWE_BW_RN], r[HILC_BWE_BW_RHEAD], p.rate_window, p.T);
      if (R >= 0) {
        long long cut = (R * p.beta_q8) >> 8;
        if (cut < p.min_q8) cut = p.min_q8;
        if (cut < rate) {
          rate = (int)cut;
          decreased = true;
          ++r[HILC_BWE_BW_DECREASED];
        }
      }
      r[HILC_BWE_BW_STATE] = HILC_BWE_STATE_HOLD;
    } else if (r[HILC_BWE_BW_SIGNAL] == HILC_BWE_SIGNAL_UNDERUSE) {
      r[HILC_BWE_BW_STATE] = HILC_BWE_STATE_HOLD;
    } else {
      r[HILC_BWE_BW_STATE] = HILC_BWE_STATE_INCREASE;
      long long up = ((long long)rate * p.increase_q16 * dh) >> 16;
      up = (up < 1 ? 1 : up) + rate;
      rate = up > p.max_q8 ? p.max_q8 : (int)up;
      ++r[HILC_BWE_BW_INCREASED];
    }
    r[HILC_BWE_BW_RATE_Q8] = rate;
  }
  ++r[HILC_BWE_BW_PHASE];
  const bool emit = decreased || (r[HILC_BWE_BW_PHASE] >= p.interval && r[HILC_BWE_BW_SEEN] != 0);
  if (emit) {
    r[HILC_BWE_BW_PHASE] = 0;
    r[HILC_BWE_BW_SEQ] = (r[HILC_BWE_BW_SEQ] + 1) & 255;
    ++r[HILC_BWE_BW_CAPS];
  }
#pragma unroll
  for (int k = 0; k < HILC_BWE_BW_TREND; ++k) row[k] = r[k];
  due[b] = emit ? 1 : 0;
  if (start || emit) {
    const int cap = min(HILC_BWE_MAX_CAP_BITS, r[HILC_BWE_BW_RATE_Q8] >> 8);
    uint8_t* out = caps + (long)b * HILC_WIRE_CAP_BYTES;
    out[0] = emit ? (uint8_t)r[HILC_BWE_BW_SEQ] : (uint8_t)0;
    out[1] = emit ? (uint8_t)(cap >> 8) : (uint8_t)0;
    out[2] = emit ? (uint8_t)(cap & 255) : (uint8_t)0;
  }
}

__global__ __launch_bounds__(THREADS) void rate_cap_kernel(const int* __restrict__ cap, const int* __restrict__ action,
                                                           const int* __restrict__ hold, int* __restrict__ rows,
                                                           int* __restrict__ rate_rows, int B, int min_bits, int max_bits,
                                                           int timeout_hops) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_BWE_CP_WORDS;
  int* rate = rate_rows + (long)b * HILC_RATE_RC_WORDS + HILC_RATE_RC_RATE_Q8;
  const bool start = is_reset(action, b);
  const bool held = is_held(hold, b);
  int r[HILC_BWE_CP_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_BWE_CP_WORDS; ++k) r[k] = start ? 0 : row[k];
  const int word = cap != nullptr ? cap[b] : 0;
  if (word & HILC_BWE_CAP_PRESENT) {
    const int seq = (word >> 16) & 255, bits = word & 0xFFFF;
    const int d = (seq - r[HILC_BWE_CP_LAST]) & 255;
    if (r[HILC_BWE_CP_SEEN] != 0 && (d < 1 || d > 127)) {
      ++r[HILC_BWE_CP_STALE];
    } else {
      r[HILC_BWE_CP_SEEN] = 1;
      r[HILC_BWE_CP_LAST] = seq;
      r[HILC_BWE_CP_AGE] = 0;
      r[HILC_BWE_CP_CAP_Q8] = clampi(bits, min_bits, max_bits) << 8;
      ++r[HILC_BWE_CP_CAPS];
    }
  }
  if (!held) {
    ++r[HILC_BWE_CP_AGE];
    if (timeout_hops > 0 && r[HILC_BWE_CP_AGE] >= timeout_hops) {
      r[HILC_BWE_CP_SEEN] = 0;
      r[HILC_BWE_CP_AGE] = 0;
      ++r[HILC_BWE_CP_TIMEOUT];
    }
  }
  const bool clamp = r[HILC_BWE_CP_SEEN] != 0 && *rate > r[HILC_BWE_CP_CAP_Q8];
  r[HILC_BWE_CP_CLAMPED] += clamp;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_BWE_CP_WORDS; ++k) row[k] = r[k];
    if (clamp) *rate = r[HILC_BWE_CP_CAP_Q8];
  }
}

}  // namespace

extern "C" int hilc_rx_bwe(const int* arrivals, const int* offsets, const int* times, int max_arrivals, const int* action, int* rows,
                           uint8_t* caps, int* due, int B, int T, int n_max, int m, int order, int min_bits, int max_bits, int window,
                           int rate_window, int alpha_q8, int beta_q8, int increase_q16, int interval, int reset_ticks, void* stream) {
  if (!arrivals || !offsets || !times || !rows || !caps || !due) return HILC_ERR_NULL;
  if (B <= 0 || max_arrivals < 0 || T < 1 || T > HILC_BWE_MAX_FRAMES) return HILC_ERR_SHAPE;
  if (n_max < 1 || n_max > 31 || m < 0 || m > n_max || n_max + m > MAX_N || order < -1 || order > HILC_DTX_MAX_ORDER) return HILC_ERR_SHAPE;
  const long tb = HILC_WIRE_TRANSPORT_HEADER + packet_bytes<long>(n_max + m, T);
  if (tb > HILC_BWE_MAX_ROW_BYTES) return HILC_ERR_SHAPE;
  if (min_bits < 1 || min_bits > max_bits || max_bits > HILC_BWE_MAX_CAP_BITS) return HILC_ERR_SHAPE;
  if (window < 2 || window > HILC_BWE_MAX_WINDOW || rate_window < HILC_BWE_RATE_MIN || rate_window > HILC_BWE_MAX_WINDOW) return HILC_ERR_SHAPE;
  if (alpha_q8 < 1 || alpha_q8 > 256 || beta_q8 < 1 || beta_q8 > 255 || increase_q16 < 0 || increase_q16 > 65535 || interval < 1 ||
      interval > 1024 || reset_ticks < 1 || reset_ticks > HILC_BWE_MAX_RESET_TICKS)
    return HILC_ERR_SHAPE;
  const BweParams p = {T, n_max, m, order, (int)tb, (int)((tb + 3) / 4), min_bits << 8, max_bits << 8, window, rate_window, alpha_q8,
                       beta_q8, increase_q16, interval, reset_ticks};
  return launch(rx_bwe_kernel, threads_grid(B), stream, arrivals, offsets, times, max_arrivals, action, rows, caps, due, B, p);
}

extern "C" int hilc_rate_cap(const int* cap, const int* action, const int* hold, int* rows, int* rate_rows, int B, int min_bits,
                             int max_bits, int timeout_hops, void* stream) {
  if (!rows || !rate_rows) return HILC_ERR_NULL;
  if (B <= 0 || min_bits < 1 || min_bits > max_bits || max_bits > HILC_RATE_MAX_RATE_BITS || timeout_hops < 0) return HILC_ERR_SHAPE;
  return launch(rate_cap_kernel, waves_grid(B), stream, cap, action, hold, rows, rate_rows, B, min_bits, max_bits, timeout_hops);
}
