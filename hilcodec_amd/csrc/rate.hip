// Report-driven rate control of the graphed sender (graph_step.GraphedEncodeHop(rate=RateConfig(...))).  Two launches, each one wave
// per slot, integer work only:
//
//   hilc_rate_ceiling  in front of the quantiser (behind hilc_fec_adapt when the sender has one): takes the slot's report of this hop,
//                      moves its rate (down by loss / 2 at a high reported loss, up by a fraction at a low one), fills its token
//                      bucket at that rate and writes n_ceil, the most stages the bucket pays for behind the hop's overhead (the
//                      transport header, a live redundant section).
//   hilc_rate_charge   the graph's last launch, behind hilc_rtx_step: charges the bucket with the bytes the slot really sent, the
//                      hop's packet and its retransmissions, down to a bounded debt.
//
// The rules, bit for bit: hilcodec_amd/rate.py (RateModel); the row: include/hilcodec_amd.h (HILC_RATE_*).  The report is accepted by
// fec_adapt_kernel's rule (report.hip), restated here.  Every value is wave-uniform; lane 0 stores the row (plain vector stores).
#include "slot.h"

namespace {

using namespace slot;

struct RateParams {
  int n_max, m, stage_bits, header_bits;
  int min_q8, max_q8, start_q8;
  int high_q8, low_q8, increase_q8, burst_hops, timeout_hops;
};

__global__ __launch_bounds__(THREADS) void rate_ceiling_kernel(const int* __restrict__ report, const int* __restrict__ action,
                                                               const int* __restrict__ hold, const int* __restrict__ n_slot,
                                                               const int* __restrict__ prev, int* __restrict__ rows,
                                                               int* __restrict__ n_ceil, int B, int prev_words, RateParams p) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_RATE_RC_WORDS;
  const bool start = is_reset(action, b);
  const bool held = is_held(hold, b);
  int r[HILC_RATE_RC_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_RATE_RC_WORDS; ++k) r[k] = start ? 0 : row[k];
  if (start) {
    r[HILC_RATE_RC_RATE_Q8] = p.start_q8;
    r[HILC_RATE_RC_CREDIT] = p.burst_hops * (p.start_q8 >> 8);
  }
  int rate = r[HILC_RATE_RC_RATE_Q8];
  const int word = report != nullptr ? report[b] : 0;
  if (word & HILC_REPORT_REPORT_PRESENT) {
    const int seq = (word >> 16) & 255, loss = (word >> 8) & 255;
    const int d = (seq - r[HILC_RATE_RC_LAST]) & 255;
    if (r[HILC_RATE_RC_SEEN] != 0 && (d < 1 || d > 127)) {
      ++r[HILC_RATE_RC_STALE];
    } else {
      r[HILC_RATE_RC_SEEN] = 1;
      r[HILC_RATE_RC_LAST] = seq;
      r[HILC_RATE_RC_AGE] = 0;
      r[HILC_RATE_RC_LOSS] = loss;
      ++r[HILC_RATE_RC_REPORTS];
      if (loss >= p.high_q8) {
        const long long cut = ((long long)rate * (512 - loss)) >> 9;
        rate = cut < p.min_q8 ? p.min_q8 : (int)cut;
        ++r[HILC_RATE_RC_DECREASED];
      } else if (loss <= p.low_q8) {
        long long up = ((long long)rate * p.increase_q8) >> 8;
        up = (up < 256 ? 256 : up) + rate;
        rate = up > p.max_q8 ? p.max_q8 : (int)up;
        ++r[HILC_RATE_RC_INCREASED];
      }
    }
  }
  if (!held) {
    ++r[HILC_RATE_RC_AGE];
    if (p.timeout_hops > 0 && r[HILC_RATE_RC_AGE] >= p.timeout_hops) {
      rate = p.start_q8;
      r[HILC_RATE_RC_SEEN] = 0;
      r[HILC_RATE_RC_AGE] = 0;
      ++r[HILC_RATE_RC_TIMEOUT];
    }
    const int bits = rate >> 8;
    r[HILC_RATE_RC_CREDIT] = min(r[HILC_RATE_RC_CREDIT] + bits, p.burst_hops * bits);
  }
  r[HILC_RATE_RC_RATE_Q8] = rate;
  const bool redundant = p.m >= 1 && !start && prev != nullptr && prev[(long)b * prev_words] != 0;
  const int overhead = p.header_bits + (redundant ? p.stage_bits * p.m : 0);
  const int ns = clamp_n(n_slot, b, 1, p.n_max);
  int nc = clampi(max(0, r[HILC_RATE_RC_CREDIT] - overhead) / p.stage_bits, min(ns, max(p.m, 1)), ns);
  if (held)
    nc = ns;
  else
    r[HILC_RATE_RC_LIMITED] += nc < ns;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_RATE_RC_WORDS; ++k) row[k] = r[k];
    n_ceil[b] = nc;
  }
}

__global__ __launch_bounds__(THREADS) void rate_charge_kernel(const int* __restrict__ nbytes, const int* __restrict__ rtx_nbytes,
                                                              int* __restrict__ rows, int B, int per_hop, int burst_hops) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_RATE_RC_WORDS;
  long long sent = nbytes[b];
  for (int q = 0; q < per_hop; ++q) sent += rtx_nbytes[(long)b * per_hop + q];
  const long long debt = -(long long)burst_hops * (row[HILC_RATE_RC_RATE_Q8] >> 8);
  const long long credit = (long long)row[HILC_RATE_RC_CREDIT] - 8 * sent;
  if (lane == 0) row[HILC_RATE_RC_CREDIT] = (int)(credit < debt ? debt : credit);
}

}  // namespace

extern "C" int hilc_rate_ceiling(const int* report, const int* action, const int* hold, const int* n_per_stream, const int* prev,
                                 int* rows, int* n_ceil, int B, int T, int n_max, int m, int header, int min_bits, int max_bits,
                                 int start_bits, int high_q8, int low_q8, int increase_q8, int burst_hops, int timeout_hops,
                                 void* stream) {
  if (!rows || !n_ceil) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || n_max < 1 || n_max > MAX_N || m < 0 || m > n_max || (long)n_max * T > (1L << 24)) return HILC_ERR_SHAPE;
  if (low_q8 < 0 || low_q8 >= high_q8 || high_q8 > 255 || increase_q8 < 0 || increase_q8 > 65535 || burst_hops < 1 || timeout_hops < 0)
    return HILC_ERR_SHAPE;
  const int hdr = header != 0 ? 8 * HILC_WIRE_TRANSPORT_HEADER : 0;
  const long need = hdr + 10L * T * ((m > 1 ? m : 1) + m);
  if (min_bits > start_bits || start_bits > max_bits || min_bits < need || max_bits > HILC_RATE_MAX_RATE_BITS ||
      (long)max_bits * burst_hops > (1L << 30))
    return HILC_ERR_SHAPE;
  const RateParams p = {n_max, m, 10 * T, hdr, min_bits << 8, max_bits << 8, start_bits << 8, high_q8, low_q8, increase_q8, burst_hops,
                        timeout_hops};
  return launch(rate_ceiling_kernel, waves_grid(B), stream, report, action, hold, n_per_stream, prev, rows, n_ceil, B, 1 + m * T, p);
}

extern "C" int hilc_rate_charge(const int* nbytes, const int* rtx_nbytes, int* rows, int B, int per_hop, int burst_hops, void* stream) {
  if (!nbytes || !rows || (per_hop > 0 && !rtx_nbytes)) return HILC_ERR_NULL;
  if (B <= 0 || per_hop < 0 || per_hop > HILC_RTX_MAX_PER_HOP || burst_hops < 1) return HILC_ERR_SHAPE;
  return launch(rate_charge_kernel, waves_grid(B), stream, nbytes, rtx_nbytes, rows, B, per_hop, burst_hops);
}
