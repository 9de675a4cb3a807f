// Receiver reports and loss-adaptive in-band FEC of the graphed hops (graph_step.GraphedDecodeHop(report=ReportConfig(...)),
// GraphedEncodeHop(fec_adapt=FecAdaptConfig(...))).  Two launches, one per side, each one wave per slot, integer work only:
//
//   hilc_rx_report  the receiver's launch after hilc_jitter_step / hilc_jitter_adapt_step: classes the hop from the slot's jitter
//                   counters, keeps a sliding window of its last W decoded / repaired / lost hops and emits a 3-byte report (seq,
//                   loss_q8, residual_q8: wire.pack_report) every R classed hops.
//   hilc_fec_adapt  the sender's launch ahead of hilc_vbr_select / hilc_pack_codes_10bit_fec: takes the slot's report of this hop,
//                   moves its on / off switch and, for a slot that is off, clears word 0 ("valid") of its previous-codes row, so the
//                   packer appends no redundant section.
//
// The rules, bit for bit: hilcodec_amd/report.py (ReportModel, FecAdaptModel); the rows: include/hilcodec_amd.h (HILC_REPORT_*).
// Every value is wave-uniform; lane 0 stores the rows (plain vector stores), the ring words of a report row are stored one per lane.
#include "slot.h"

namespace {

using namespace slot;

__global__ __launch_bounds__(THREADS) void rx_report_kernel(const int* __restrict__ jstate, const int* __restrict__ action,
                                                            int* __restrict__ rows, uint8_t* __restrict__ reports,
                                                            int* __restrict__ due, int B, int window, int interval) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const int* js = jstate + (long)b * HILC_JITTER_ST_WORDS;
  int* row = rows + (long)b * HILC_REPORT_RP_WORDS;
  const bool start = is_reset(action, b);
  int r[HILC_REPORT_RP_RING];
#pragma unroll
  for (int k = 0; k < HILC_REPORT_RP_RING; ++k) r[k] = start ? 0 : row[k];
  int cls = HILC_REPORT_CLASS_NONE;
#pragma unroll
  for (int c = 0; c < 4; ++c) {                             // D, F, L, NOISE: jitter.py's and report.py's order
    const int now = js[HILC_JITTER_STAT_DECODED + c];
    if (cls == HILC_REPORT_CLASS_NONE && now != r[HILC_REPORT_RP_DECODED + c]) cls = HILC_REPORT_CLASS_D + c;
    r[HILC_REPORT_RP_DECODED + c] = now;
  }
  bool touched = false, emit = false;
  int w = 0, word = 0;
  if (cls != HILC_REPORT_CLASS_NONE) {
    if (cls != HILC_REPORT_CLASS_NOISE) {
      const int head = clampi(r[HILC_REPORT_RP_HEAD], 0, window - 1);   // a row this kernel wrote is in range already
      const int sh = 2 * (head & 15);
      w = head >> 4;
      uint32_t u = start ? 0u : (uint32_t)row[HILC_REPORT_RP_RING + w];
      if (r[HILC_REPORT_RP_N] >= window) {                              // the oldest entry leaves the counts
        const int old = (int)((u >> sh) & 3u);
        r[HILC_REPORT_RP_F] -= old == HILC_REPORT_CLASS_F;
        r[HILC_REPORT_RP_L] -= old == HILC_REPORT_CLASS_L;
      } else {
        ++r[HILC_REPORT_RP_N];
      }
      u = (u & ~(3u << sh)) | ((uint32_t)cls << sh);
      word = (int)u;
      touched = true;
      r[HILC_REPORT_RP_F] += cls == HILC_REPORT_CLASS_F;
      r[HILC_REPORT_RP_L] += cls == HILC_REPORT_CLASS_L;
      r[HILC_REPORT_RP_HEAD] = head + 1 >= window ? 0 : head + 1;
    }
    if (++r[HILC_REPORT_RP_PHASE] >= interval) {
      r[HILC_REPORT_RP_PHASE] = 0;
      const int N = r[HILC_REPORT_RP_N];
      if (N >= 1) {
        r[HILC_REPORT_RP_SEQ] = (r[HILC_REPORT_RP_SEQ] + 1) & 255;
        r[HILC_REPORT_RP_LOSS] = min(255, (256 * (r[HILC_REPORT_RP_F] + r[HILC_REPORT_RP_L]) + N / 2) / N);
        r[HILC_REPORT_RP_RESIDUAL] = min(255, (256 * r[HILC_REPORT_RP_L] + N / 2) / N);
        ++r[HILC_REPORT_RP_REPORTS];
        emit = true;
      }
    }
  }
  // ring words: lane k owns word k, one store per lane (a start clears them all; else only the word entered changes)
  if (lane < HILC_REPORT_RP_RING_WORDS && (start || (touched && lane == w))) row[HILC_REPORT_RP_RING + lane] = (touched && lane == w) ? word : 0;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_REPORT_RP_RING; ++k) row[k] = r[k];
    due[b] = emit ? 1 : 0;
  }
  if (lane < HILC_WIRE_REPORT_BYTES && (start || emit)) {
    const int field = lane == 0 ? r[HILC_REPORT_RP_SEQ] : (lane == 1 ? r[HILC_REPORT_RP_LOSS] : r[HILC_REPORT_RP_RESIDUAL]);
    reports[(long)b * HILC_WIRE_REPORT_BYTES + lane] = emit ? (uint8_t)field : (uint8_t)0;
  }
}

__global__ __launch_bounds__(THREADS) void fec_adapt_kernel(const int* __restrict__ report, const int* __restrict__ action,
                                                            const int* __restrict__ hold, int* __restrict__ rows,
                                                            int* __restrict__ prev, int* __restrict__ fec_on, int B, int prev_words,
                                                            int on_q8, int off_q8, int calm_reports, int timeout_hops,
                                                            int initial_on) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_REPORT_FA_WORDS;
  const bool start = is_reset(action, b);
  const bool held = is_held(hold, b);
  int r[HILC_REPORT_FA_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_REPORT_FA_WORDS; ++k) r[k] = start ? 0 : row[k];
  if (start) r[HILC_REPORT_FA_ON] = initial_on;
  const int word = report != nullptr ? report[b] : 0;
  if (word & HILC_REPORT_REPORT_PRESENT) {
    const int seq = (word >> 16) & 255, loss = (word >> 8) & 255, residual = word & 255;
    const int d = (seq - r[HILC_REPORT_FA_LAST]) & 255;
    if (r[HILC_REPORT_FA_SEEN] != 0 && (d < 1 || d > 127)) {
      ++r[HILC_REPORT_FA_STALE];
    } else {
      r[HILC_REPORT_FA_SEEN] = 1;
      r[HILC_REPORT_FA_LAST] = seq;
      r[HILC_REPORT_FA_AGE] = 0;
      r[HILC_REPORT_FA_LOSS] = loss;
      r[HILC_REPORT_FA_RESIDUAL] = residual;
      ++r[HILC_REPORT_FA_REPORTS];
      if (loss >= on_q8) {
        r[HILC_REPORT_FA_CALM] = 0;
        r[HILC_REPORT_FA_TURNED_ON] += r[HILC_REPORT_FA_ON] == 0;
        r[HILC_REPORT_FA_ON] = 1;
      } else if (loss <= off_q8) {
        if (++r[HILC_REPORT_FA_CALM] >= calm_reports) {
          r[HILC_REPORT_FA_TURNED_OFF] += r[HILC_REPORT_FA_ON] == 1;
          r[HILC_REPORT_FA_ON] = 0;
        }
      } else {
        r[HILC_REPORT_FA_CALM] = 0;
      }
    }
  }
  if (!held) {
    ++r[HILC_REPORT_FA_AGE];
    if (timeout_hops > 0 && r[HILC_REPORT_FA_AGE] >= timeout_hops) {
      r[HILC_REPORT_FA_ON] = initial_on;
      r[HILC_REPORT_FA_CALM] = 0;
      r[HILC_REPORT_FA_SEEN] = 0;
      r[HILC_REPORT_FA_AGE] = 0;
      ++r[HILC_REPORT_FA_TIMEOUT];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_REPORT_FA_WORDS; ++k) row[k] = r[k];
    if (!held && r[HILC_REPORT_FA_ON] == 0) prev[(long)b * prev_words] = 0;      // the valid word: the packer appends no redundant section
    fec_on[b] = r[HILC_REPORT_FA_ON];
  }
}

}  // namespace

extern "C" int hilc_rx_report(const int* jitter_state, const int* action, int* rows, uint8_t* reports, int* due, int B, int window,
                              int interval, void* stream) {
  if (!jitter_state || !rows || !reports || !due) return HILC_ERR_NULL;
  if (B <= 0 || window < 8 || window > 16 * HILC_REPORT_RP_RING_WORDS || interval < 1 || interval > 1024) return HILC_ERR_SHAPE;
  return launch(rx_report_kernel, waves_grid(B), stream, jitter_state, action, rows, reports, due, B, window, interval);
}

extern "C" int hilc_fec_adapt(const int* report, const int* action, const int* hold, int* rows, int* prev, int* fec_on, int B, int T,
                              int m, int on_q8, int off_q8, int calm_reports, int timeout_hops, int initial_on, void* stream) {
  if (!rows || !prev || !fec_on) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || m < 1 || (long)m * T > (1L << 24)) return HILC_ERR_SHAPE;
  if (off_q8 < 0 || off_q8 >= on_q8 || on_q8 > 255 || calm_reports < 1 || timeout_hops < 0) return HILC_ERR_SHAPE;
  return launch(fec_adapt_kernel, waves_grid(B), stream, report, action, hold, rows, prev, fec_on, B, 1 + m * T, on_q8, off_q8,
                calm_reports, timeout_hops, initial_on != 0 ? 1 : 0);
}
