// Downlink control of the selective forwarding hop (graph_step.GraphedForwardHop(downlink=)): what closes the feedback loops of a
// forwarded conference per listener.  Two launches behind hilc_forward_classify and hilc_forward_route, each one wave per slot, integer
// work only:
//
//   hilc_downlink_store  per sender slot: the arrivals the first launch picked enter the slot's history (rtx.py's sender rule, stated
//                        for what the forwarder received); a row keeps the arrival-record form, the byte count word then the packet.
//   hilc_downlink_step   per listener slot: takes the hop's receiver reports (one per route; the rate follows the least loss among
//                        them), fills the listener's bucket, finds the most layers the bucket pays for — lane L - 1 sums the cost of
//                        the hop's rows at L layers, one ballot picks —, cuts the route launch's rows to it, answers the hop's NACKs
//                        from the owners' histories and charges what it wrote.
//
// The rules, bit for bit: hilcodec_amd/downlink.py (DownlinkModel); the rows: include/hilcodec_amd.h (HILC_DOWNLINK_*).
#include "trim.h"

namespace {

using namespace trim;

// Lane e < R holds tag e; lane j owns word j (and j + 64, ...) of every history row in every pass.  The picks are taken one by one with
// wave-uniform control flow.
__global__ __launch_bounds__(THREADS) void downlink_store_kernel(const int* __restrict__ arr, int max_a, int aw,
                                                                 const int* __restrict__ action, const int* __restrict__ pick,
                                                                 const int* __restrict__ pick_count, int* __restrict__ tags,
                                                                 int* __restrict__ ring, int* __restrict__ rows, int B, int tb, int burst,
                                                                 int R) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int t = me.b, lane = me.lane();
  int* trow = tags + (long)t * R;
  int* row = rows + (long)t * HILC_DOWNLINK_DS_WORDS;
  int cnt[HILC_DOWNLINK_DS_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_DOWNLINK_DS_WORDS; ++k) cnt[k] = row[k];
  int tag = (lane < R && !is_reset(action, t)) ? trow[lane] : 0;
  const int npick = __builtin_amdgcn_readfirstlane(clampi(pick_count[t], 0, burst));
  for (int k = 0; k < npick; ++k) {
    const int a = __builtin_amdgcn_readfirstlane(pick[(long)t * burst + k]);
    if (a < 0 || a >= max_a) continue;                        // never for what the first launch picked
    const int* rec = arr + (long)a * (1 + aw);
    const int nb = __builtin_amdgcn_readfirstlane(rec[0]);
    if (nb < HILC_WIRE_TRANSPORT_HEADER || nb > tb) continue; // likewise
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(rec[1]);
    const int h = (int)(((w & 0xFFu) << 8) | ((w >> 8) & 0xFFu));
    const int e = h & (R - 1);
    int* dst = ring + ((long)t * R + e) * (1 + aw);
    for (int j = lane; j < aw; j += LANES) {
      uint32_t v = (uint32_t)rec[1 + j];
      const int keep = nb - 4 * j;                            // packet bytes in this word
      if (keep < 4) v = keep <= 0 ? 0u : (v & ((1u << (8 * keep)) - 1u));
      dst[1 + j] = (int)v;
    }
    if (lane == 0) dst[0] = nb;
    if (__shfl(tag, e) != 0) ++cnt[HILC_DOWNLINK_DS_REPLACED];
    if (lane == e) tag = h | (nb << 16);
    ++cnt[HILC_DOWNLINK_DS_STORED];
  }
  if (lane < R) trow[lane] = tag;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_DOWNLINK_DS_WORDS; ++k) row[k] = cnt[k];
  }
}

// a route row or a history row as the cut reads it: its byte count (0: empty) and its header byte 2
struct Row {
  int nb, flags;
  __device__ __forceinline__ bool sid() const { return (flags & HILC_WIRE_SID_BIT) != 0; }
  __device__ __forceinline__ bool fb() const { return (flags & HILC_WIRE_FEC_BIT) != 0; }
  __device__ __forceinline__ int n() const { return flags & HILC_WIRE_N_MASK; }
};

__device__ __forceinline__ Cut cut_row(const uint8_t* src, Row r, int L, int T, int m, int keep_fec) {
  if (r.nb <= 0) return no_cut();
  return cut_packet(src, r.sid(), r.fb(), r.n(), r.nb - HILC_WIRE_TRANSPORT_HEADER, L, T, m, keep_fec);
}

// the bytes of forward.trim_packet(row, L): the cut's length, which does not read the packet
__device__ __forceinline__ int len_at(Row r, int L, int T, int m, int keep_fec) { return cut_row(nullptr, r, L, T, m, keep_fec).len; }

struct RateArgs {
  int on, min_bits, max_bits, start_bits, high_q8, low_q8, increase_q8, burst_hops, timeout_hops;
};

// Lane j < fanout holds route j (owner, memory word, feedback words), lane c < fanout * burst cell c = (route, pick) of the hop's rows,
// lane L - 1 the cost of the hop at L layers; they meet by shuffles and ballots.  The row's words live in registers, the same in every
// lane, and lane 0 stores them.
__global__ __launch_bounds__(THREADS) void downlink_step_kernel(const int* __restrict__ routes, const int* __restrict__ new_routes,
                                                                const uint8_t* __restrict__ in, const int* __restrict__ in_nbytes,
                                                                const int* __restrict__ layers, const int* __restrict__ action,
                                                                const int* __restrict__ report, const int* __restrict__ nack_base,
                                                                const int* __restrict__ nack_bitmap, const int* __restrict__ tags,
                                                                const int* __restrict__ ring, int* __restrict__ rows,
                                                                int* __restrict__ memory, int* __restrict__ eff_layers,
                                                                uint8_t* __restrict__ out, int* __restrict__ out_nbytes,
                                                                uint8_t* __restrict__ rtx_out, int* __restrict__ rtx_nbytes,
                                                                int* __restrict__ rtx_routes, int B, int T, int n_max, int m, int tb,
                                                                int fanout, int burst, int keep_fec, int R, int per_hop, RateArgs ra) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_DOWNLINK_DL_WORDS;
  const bool start = is_reset(action, b);
  int s[HILC_DOWNLINK_DL_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_DOWNLINK_DL_WORDS; ++k) s[k] = start ? 0 : row[k];
  if (start && ra.on) {
    s[HILC_DOWNLINK_DL_RATE_Q8] = 256 * ra.start_bits;
    s[HILC_DOWNLINK_DL_CREDIT] = ra.burst_hops * ra.start_bits;
  }

  // rules 1 and 2: the routes, their memory and the feedback that is dropped
  const bool is_route = lane < fanout;
  const int owner = is_route ? routes[(long)b * fanout + lane] : -1;
  const bool live = is_route && owner >= 0 && owner < B && new_routes[(long)b * fanout + lane] != 1;
  int mem = (live && !start) ? memory[(long)b * fanout + lane] : 0;
  const int rword = (ra.on && report != nullptr && is_route) ? report[(long)b * fanout + lane] : 0;
  const int nword = (R > 0 && nack_base != nullptr && is_route) ? nack_base[(long)b * fanout + lane] : 0;
  const int nbits = (R > 0 && nack_base != nullptr && is_route) ? (nack_bitmap[(long)b * fanout + lane] & 0xFFFF) : 0;
  const bool has_report = (rword & HILC_REPORT_REPORT_PRESENT) != 0, has_nack = (nword & HILC_RTX_NACK_PRESENT) != 0;
  s[HILC_DOWNLINK_DL_STALE] += __popcll(__ballot(has_report && !live));
  s[HILC_DOWNLINK_DL_NACK_STALE] += __popcll(__ballot(has_nack && !live));

  // rules 3 to 5: the reports, the age and the bucket
  long long rate = s[HILC_DOWNLINK_DL_RATE_Q8];
  if (ra.on) {
    bool accepted = false, stale = false;
    if (has_report && live) {
      const int seq = (rword >> 16) & 255, loss = (rword >> 8) & 255;
      const int d = (seq - ((mem >> 8) & 255)) & 255;
      if ((mem & HILC_DOWNLINK_MEM_SEEN) && !(d >= 1 && d <= 127)) {
        stale = true;
      } else {
        mem = HILC_DOWNLINK_MEM_SEEN | (seq << 8) | loss;
        accepted = true;
      }
    }
    s[HILC_DOWNLINK_DL_STALE] += __popcll(__ballot(stale));
    const int naccepted = __popcll(__ballot(accepted));
    s[HILC_DOWNLINK_DL_REPORTS] += naccepted;
    if (naccepted > 0) {
      int loss = (mem & HILC_DOWNLINK_MEM_SEEN) ? (mem & 255) : 256;
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) loss = min(loss, __shfl_xor(loss, x, 64));
      s[HILC_DOWNLINK_DL_LOSS] = loss;
      s[HILC_DOWNLINK_DL_AGE] = 0;
      if (loss >= ra.high_q8) {
        rate = max(256LL * ra.min_bits, (rate * (512 - loss)) >> 9);
        ++s[HILC_DOWNLINK_DL_DECREASED];
      } else if (loss <= ra.low_q8) {
        rate = min(256LL * ra.max_bits, rate + max(256LL, (rate * ra.increase_q8) >> 8));
        ++s[HILC_DOWNLINK_DL_INCREASED];
      }
    }
    ++s[HILC_DOWNLINK_DL_AGE];
    if (ra.timeout_hops > 0 && s[HILC_DOWNLINK_DL_AGE] >= ra.timeout_hops) {
      rate = 256LL * ra.start_bits;
      mem &= ~HILC_DOWNLINK_MEM_SEEN;
      s[HILC_DOWNLINK_DL_AGE] = 0;
      ++s[HILC_DOWNLINK_DL_TIMEOUT];
    }
    const long long bits = rate >> 8;
    s[HILC_DOWNLINK_DL_CREDIT] = (int)min((long long)s[HILC_DOWNLINK_DL_CREDIT] + bits, ra.burst_hops * bits);
    s[HILC_DOWNLINK_DL_RATE_Q8] = (int)rate;
  }
  if (is_route) memory[(long)b * fanout + lane] = mem;

  // rule 6: lane c < cells reads cell c's byte count and header byte 2; lane L - 1 sums the hop's cost at L layers
  const int cells = fanout * burst;                           // at most 32
  const uint8_t* irow = in + (long)b * cells * tb;
  Row mine;
  mine.nb = mine.flags = 0;
  if (lane < cells) {
    const int nb = in_nbytes[(long)b * cells + lane];
    if (nb >= HILC_WIRE_TRANSPORT_HEADER && nb <= tb) {       // always, for what the route launch wrote; 0: an empty row
      mine.nb = nb;
      mine.flags = irow[(long)lane * tb + 2];
    }
  }
  const int Lmax = clampi(layers[b], 1, n_max);
  int cost = 0;
  for (int c = 0; c < cells; ++c) {
    Row r;
    r.nb = __shfl(mine.nb, c);
    r.flags = __shfl(mine.flags, c);
    cost += 8 * len_at(r, lane + 1, T, m, keep_fec);
  }
  int L_eff = Lmax;
  if (ra.on && __ballot(mine.nb > 0) != 0ull) {
    const unsigned long long fits = __ballot(lane < Lmax && cost <= s[HILC_DOWNLINK_DL_CREDIT]);
    L_eff = fits != 0ull ? 64 - __builtin_clzll(fits) : 1;
  }
  L_eff = __builtin_amdgcn_readfirstlane(L_eff);
  s[HILC_DOWNLINK_DL_LAYERS] = L_eff;

  // rule 7, the byte counts and the counters
  int sent;
  {
    const int len = len_at(mine, L_eff, T, m, keep_fec);
    const bool trimmed = mine.nb > 0 && !mine.sid() && mine.n() > L_eff;
    if (lane < cells) out_nbytes[(long)b * cells + lane] = len;
    const int ntrimmed = __popcll(__ballot(trimmed));
    s[HILC_DOWNLINK_DL_PACKETS] += __popcll(__ballot(len > 0));
    s[HILC_DOWNLINK_DL_TRIMMED] += ntrimmed;
    s[HILC_DOWNLINK_DL_LIMITED] += ntrimmed > 0 ? 1 : 0;
    sent = len;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) sent += __shfl_xor(sent, x, 64);
    s[HILC_DOWNLINK_DL_BYTES] += sent;
  }
  // the rows: one lane per output byte; every lane runs every pass (the cells move by shuffles)
  {
    const int total = cells * tb;
    uint8_t* orow = out + (long)b * total;
    for (int base = 0; base < total; base += LANES) {
      const int e = base + lane;
      const int c = min(e / tb, cells - 1);
      Row r;
      r.nb = __shfl(mine.nb, c);
      r.flags = __shfl(mine.flags, c);
      if (e >= total) continue;
      orow[e] = (uint8_t)cut_byte(cut_row(irow + (long)c * tb, r, L_eff, T, m, keep_fec), e - c * tb);
    }
  }

  // rule 8: the NACKs, one by one with wave-uniform control flow; lane e < R holds tag e of the route's owner
  if (R > 0) {
    int q = 0;
    for (int j = 0; j < fanout; ++j) {
      const int word = __builtin_amdgcn_readfirstlane(__shfl(nword, j));
      const int bitmap = __builtin_amdgcn_readfirstlane(__shfl(nbits, j));
      const int t = __builtin_amdgcn_readfirstlane(__shfl(live ? owner : -1, j));
      if (!(word & HILC_RTX_NACK_PRESENT) || t < 0) continue;
      ++s[HILC_DOWNLINK_DL_REQUESTS];
      const int tag = lane < R ? tags[(long)t * R + lane] : 0;
      for (int k = 0; k <= 16; ++k) {                         // wire.nack_hops: base, then base + 1 + i for every set bit i
        if (k > 0 && !((bitmap >> (k - 1)) & 1)) continue;
        const int h = ((word & 0xFFFF) + k) & 0xFFFF;
        const int e = h & (R - 1);
        const int tg = __builtin_amdgcn_readfirstlane(__shfl(tag, e));
        if (tg == 0 || (tg & 0xFFFF) != h) {
          ++s[HILC_DOWNLINK_DL_RTX_MISS];
        } else if (q >= per_hop) {
          ++s[HILC_DOWNLINK_DL_RTX_DROPPED];
        } else {
          const int* rec = ring + ((long)t * R + e) * (1 + (tb + 3) / 4);
          Row r;
          r.nb = (int)((uint32_t)tg >> 16);
          r.flags = (int)(((uint32_t)__builtin_amdgcn_readfirstlane(rec[1]) >> 16) & 0xFFu);
          if (r.nb < HILC_WIRE_TRANSPORT_HEADER || r.nb > tb) r.nb = 0;      // never for a tag the store launch wrote
          const Cut c = cut_row((const uint8_t*)(rec + 1), r, L_eff, T, m, keep_fec);
          uint8_t* dst = rtx_out + ((long)b * per_hop + q) * tb;
          for (int i = lane; i < tb; i += LANES) dst[i] = (uint8_t)cut_byte(c, i);
          if (lane == 0) {
            rtx_nbytes[(long)b * per_hop + q] = c.len;
            rtx_routes[(long)b * per_hop + q] = j;
          }
          sent += c.len;
          ++s[HILC_DOWNLINK_DL_RTX_SENT];
          ++q;
        }
      }
    }
    for (; q < per_hop; ++q) {                                // the rows not used
      uint8_t* dst = rtx_out + ((long)b * per_hop + q) * tb;
      for (int i = lane; i < tb; i += LANES) dst[i] = (uint8_t)0;
      if (lane == 0) {
        rtx_nbytes[(long)b * per_hop + q] = 0;
        rtx_routes[(long)b * per_hop + q] = -1;
      }
    }
  }

  // rule 9
  if (ra.on) s[HILC_DOWNLINK_DL_CREDIT] = (int)max((long long)s[HILC_DOWNLINK_DL_CREDIT] - 8LL * sent, -(ra.burst_hops * (rate >> 8)));
  if (lane == 0) {
    eff_layers[b] = L_eff;
#pragma unroll
    for (int k = 0; k < HILC_DOWNLINK_DL_WORDS; ++k) row[k] = s[k];
  }
}

static inline bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// the shape of the senders' packets; on HILC_OK *tb is the headed row's bytes
static inline int check_packets(int B, int T, int n_max, int m, int burst, long* tb) {
  if (B <= 0 || T <= 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || n_max > 31 || m < 0 || m > n_max || n_max + m > MAX_N) return HILC_ERR_RANGE;
  if (burst < 1 || burst > HILC_FORWARD_MAX_BURST) return HILC_ERR_RANGE;
  *tb = HILC_WIRE_TRANSPORT_HEADER + packet_bytes<long>(n_max + m, T);
  if (*tb >= (1L << 15)) return HILC_ERR_SHAPE;
  return HILC_OK;
}

}  // namespace

extern "C" int hilc_downlink_store(const int* arrivals, int max_arrivals, const int* action, const int* pick, const int* pick_count,
                                   int* tags, int* ring, int* rows, int B, int T, int n_max, int m, int burst, int history, void* stream) {
  if (!arrivals || !pick || !pick_count || !tags || !ring || !rows) return HILC_ERR_NULL;
  if (max_arrivals < 0) return HILC_ERR_SHAPE;
  long tb = 0;
  const int rc = check_packets(B, T, n_max, m, burst, &tb);
  if (rc != HILC_OK) return rc;
  if (!pow2_in(history, 2, HILC_DOWNLINK_MAX_HISTORY)) return HILC_ERR_RANGE;
  return launch(downlink_store_kernel, waves_grid(B), stream, arrivals, max_arrivals, (int)((tb + 3) / 4), action, pick, pick_count, tags,
                ring, rows, B, (int)tb, burst, history);
}

extern "C" int hilc_downlink_step(const int* routes, const int* new_routes, const uint8_t* in, const int* in_nbytes, const int* layers,
                                  const int* action, const int* report, const int* nack_base, const int* nack_bitmap, const int* tags,
                                  const int* ring, int* rows, int* memory, int* eff_layers, uint8_t* out, int* out_nbytes,
                                  uint8_t* rtx_out, int* rtx_nbytes, int* rtx_routes, int B, int T, int n_max, int m, int fanout,
                                  int burst, int keep_fec, int history, int per_hop, int rate_on, int min_bits, int max_bits,
                                  int start_bits, int high_q8, int low_q8, int increase_q8, int burst_hops, int timeout_hops,
                                  void* stream) {
  if (!routes || !new_routes || !in || !in_nbytes || !layers || !rows || !memory || !eff_layers || !out || !out_nbytes)
    return HILC_ERR_NULL;
  if (history != 0 && (!tags || !ring || !rtx_out || !rtx_nbytes || !rtx_routes)) return HILC_ERR_NULL;
  if ((nack_base == nullptr) != (nack_bitmap == nullptr)) return HILC_ERR_NULL;
  long tb = 0;
  const int rc = check_packets(B, T, n_max, m, burst, &tb);
  if (rc != HILC_OK) return rc;
  if (fanout < 1 || fanout > HILC_FORWARD_MAX_FANOUT) return HILC_ERR_RANGE;
  if ((history != 0 && !pow2_in(history, 2, HILC_DOWNLINK_MAX_HISTORY)) || per_hop < 1 || per_hop > HILC_DOWNLINK_MAX_PER_HOP ||
      (history == 0 && rate_on == 0))
    return HILC_ERR_RANGE;
  RateArgs ra = {0, 0, 0, 0, 0, 0, 0, 1, 0};
  if (rate_on != 0) {
    if (min_bits < 1 || start_bits < min_bits || max_bits < start_bits || max_bits > HILC_RATE_MAX_RATE_BITS || burst_hops < 1 ||
        (long)max_bits * burst_hops > (1L << 30) || timeout_hops < 0)
      return HILC_ERR_SHAPE;
    if (low_q8 < 0 || high_q8 > 255 || low_q8 >= high_q8 || increase_q8 < 0 || increase_q8 > 65535) return HILC_ERR_RANGE;
    ra = {1, min_bits, max_bits, start_bits, high_q8, low_q8, increase_q8, burst_hops, timeout_hops};
  }
  return launch(downlink_step_kernel, waves_grid(B), stream, routes, new_routes, in, in_nbytes, layers, action, report, nack_base,
                nack_bitmap, tags, ring, rows, memory, eff_layers, out, out_nbytes, rtx_out, rtx_nbytes, rtx_routes, B, T, n_max, m,
                (int)tb, fanout, burst, keep_fec != 0 ? 1 : 0, history, per_hop, ra);
}
