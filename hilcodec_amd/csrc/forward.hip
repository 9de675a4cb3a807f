// Selective forwarding hop (graph_step.GraphedForwardHop): a conference server that routes packets and cuts them to a listener's
// number of stages without decoding.  Packets are stage-major, so the first L stages of an n-stage packet are a bit prefix of its body
// (slot.h).  Two launches, each one wave per slot, integer work only:
//
//   hilc_forward_classify  per sender slot: checks the hop's arrivals (wire.parse_transport), picks the first `burst` valid ones and
//                          keeps the activity row (hang-over, hops active) the selection reads.
//   hilc_forward_route     per listener slot: selects the room's most active other members by `fanout` rounds of a wave-wide
//                          lexicographic arg-max over the B sender rows, keeps each owner on its route, hands the free routes to the
//                          newcomers and writes every output row, one lane per byte, cut to the listener's layers.
//
// The rules, bit for bit: hilcodec_amd/forward.py (SenderModel, ListenerModel); the rows: include/hilcodec_amd.h (HILC_FORWARD_*).
#include "trim.h"

namespace {

using namespace trim;

// Wave-uniform control flow over the slot's arrivals; the counters live in registers and lane 0 stores them.  Lane k < burst keeps
// the k-th picked record index.
__global__ __launch_bounds__(THREADS) void forward_classify_kernel(const int* __restrict__ arr, const int* __restrict__ off, int max_a,
                                                                   int aw, const int* __restrict__ action, int* __restrict__ rows,
                                                                   int* __restrict__ pick, int* __restrict__ pick_count, int B, int T,
                                                                   int n_max, int m, int order, int tb, int burst, int hang_hops) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_FORWARD_SD_WORDS;
  const bool start = is_reset(action, b);
  int s[HILC_FORWARD_SD_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_FORWARD_SD_WORDS; ++k) s[k] = start ? 0 : row[k];
  const int a0 = clampi(off[b], 0, max_a);
  const int a1 = clampi(off[b + 1], a0, max_a);
  int npick = 0, mine = -1;
  bool talk = false;
  for (int a = a0; a < a1; ++a) {
    const Arrival p = parse_arrival(arr + (long)a * (1 + aw), tb, T, n_max, m, order);
    if (!p.ok) {
      ++s[HILC_FORWARD_SD_MALFORMED];
      continue;
    }
    if (p.sid) {
      ++s[HILC_FORWARD_SD_SIDS];
    } else {
      ++s[HILC_FORWARD_SD_CODES];
      talk = true;
    }
    if (npick < burst) {
      if (lane == npick) mine = a;
      ++npick;
    } else {
      ++s[HILC_FORWARD_SD_OVERFLOW];
    }
  }
  s[HILC_FORWARD_SD_HANG] = talk ? hang_hops + 1 : max(s[HILC_FORWARD_SD_HANG] - 1, 0);
  s[HILC_FORWARD_SD_SINCE] = s[HILC_FORWARD_SD_HANG] > 0 ? min(s[HILC_FORWARD_SD_SINCE] + 1, HILC_FORWARD_MAX_SINCE) : 0;
  if (lane < burst) pick[(long)b * burst + lane] = mine;
  if (lane == 0) {
    pick_count[b] = npick;
#pragma unroll
    for (int k = 0; k < HILC_FORWARD_SD_WORDS; ++k) row[k] = s[k];
  }
}

// a candidate's rank as two ints, compared lexicographically, larger first: hi = SD_HANG << 16 | SD_SINCE, lo = -slot; hi < 0: none
__device__ __forceinline__ bool ahead(int ha, int la, int hb, int lb) { return ha > hb || (ha == hb && la > lb); }

// What row (b, j, k) is cut from: the arrival record (an empty Cut: an empty row), and the cut of forward.trim_packet (trim.h)
__device__ __forceinline__ Cut cut_of(const int* __restrict__ arr, int max_a, int aw, const int* __restrict__ pick,
                                      const int* __restrict__ pick_count, int t, int k, int burst, int L, int tb, int T, int n_max, int m,
                                      int order, int keep_fec) {
  if (t < 0 || k >= min(pick_count[t], burst)) return no_cut();
  const int a = pick[(long)t * burst + k];
  if (a < 0 || a >= max_a) return no_cut();
  const int* rec = arr + (long)a * (1 + aw);
  const Arrival p = parse_arrival(rec, tb, T, n_max, m, order);
  if (!p.ok) return no_cut();                               // never for a record the first launch picked
  return cut_packet((const uint8_t*)(rec + 1), p.sid, p.fb, p.n, p.body, L, T, m, keep_fec);
}

// Lane j < fanout holds route j's owner, lane k < fanout round k's pick; both move by shuffles under wave-uniform control flow.
__global__ __launch_bounds__(THREADS) void forward_route_kernel(const int* __restrict__ arr, int max_a, int aw,
                                                                const int* __restrict__ action, const int* __restrict__ room,
                                                                const int* __restrict__ layers, const int* __restrict__ srows,
                                                                const int* __restrict__ pick, const int* __restrict__ pick_count,
                                                                int* __restrict__ routes, int* __restrict__ new_routes,
                                                                int* __restrict__ rows, uint8_t* __restrict__ out,
                                                                int* __restrict__ out_nbytes, int B, int T, int n_max, int m, int order,
                                                                int tb, int fanout, int burst, int keep_fec) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_FORWARD_LR_WORDS;
  const bool start = is_reset(action, b);
  int cnt[HILC_FORWARD_LR_WORDS];
#pragma unroll
  for (int k = 0; k < HILC_FORWARD_LR_WORDS; ++k) cnt[k] = start ? 0 : row[k];
  const bool is_route = lane < fanout;
  const int before = (is_route && !start) ? routes[(long)b * fanout + lane] : -1;
  const int r = room[b];
  const int L = clampi(layers[b], 1, n_max);

  // the selection: round k picks the first candidate behind round k - 1's pick; lane k keeps it
  int sel = -1, nsel = 0;
  bool kept = false;                                        // this route's owner is selected
  int last_h = -1, last_l = 0;
  for (int k = 0; k < fanout; ++k) {
    int bh = -1, bl = 0;
    if (r >= 0) {
      for (int t = lane; t < B; t += LANES) {
        if (t == b || room[t] != r) continue;
        const int hang = srows[(long)t * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_HANG];
        if (hang <= 0) continue;
        const int h = (min(hang, HILC_FORWARD_MAX_HANG_HOPS + 1) << 16) |
                      clampi(srows[(long)t * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_SINCE], 0, HILC_FORWARD_MAX_SINCE);
        if (last_h >= 0 && !ahead(last_h, last_l, h, -t)) continue;      // picked in an earlier round
        if (ahead(h, -t, bh, bl)) { bh = h; bl = -t; }
      }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const int oh = __shfl_xor(bh, x, 64);
      const int ol = __shfl_xor(bl, x, 64);
      if (ahead(oh, ol, bh, bl)) { bh = oh; bl = ol; }
    }
    if (bh < 0) break;                                      // no more candidates (the same in every lane)
    if (lane == k) sel = -bl;
    if (is_route && before == -bl) kept = true;
    last_h = bh;
    last_l = bl;
    ++nsel;
  }
  // a route is freed when its owner is not selected or was joined on this hop
  const bool rejoined = kept && is_reset(action, before);   // kept: `before` is a selected slot
  int owner = (kept && !rejoined) ? before : -1;
  // the selected slots without a route, ranked by slot, take the free routes in route order
  bool has = false;
  for (int j = 0; j < fanout; ++j) {
    const int o = __shfl(owner, j);
    if (lane < nsel && o == sel) has = true;
  }
  const bool fresh = lane < nsel && !has;
  const uint32_t fresh_b = (uint32_t)__ballot(fresh);
  int rank = 0;
  for (int k = 0; k < nsel; ++k) {
    const int s = __shfl(sel, k);
    if (((fresh_b >> k) & 1u) && s < sel) ++rank;
  }
  const bool free_route = is_route && owner < 0;
  const uint32_t free_b = (uint32_t)__ballot(free_route);
  const int free_rank = __popc(free_b & ((1u << (lane & 31)) - 1u));       // lane < 32 for a route
  for (int k = 0; k < nsel; ++k) {
    const int s = __shfl(sel, k);
    const int rk = __shfl(rank, k);
    if (free_route && ((fresh_b >> k) & 1u) && rk == free_rank) owner = s;
  }
  const bool is_new = is_route && owner >= 0 && owner != before;
  cnt[HILC_FORWARD_LR_SWITCHES] += __popcll(__ballot(is_new));
  if (is_route) {
    routes[(long)b * fanout + lane] = owner;
    new_routes[(long)b * fanout + lane] = is_new ? 1 : 0;
  }

  // byte counts and counters: lane c < fanout * burst is row (c / burst, c % burst)
  {
    const int cells = fanout * burst;                       // at most 32
    const int j = min(lane / burst, fanout - 1);
    const int t = __shfl(owner, j);
    int len = 0;
    bool trimmed = false;
    if (lane < cells) {
      const Cut c = cut_of(arr, max_a, aw, pick, pick_count, t, lane % burst, burst, L, tb, T, n_max, m, order, keep_fec);
      len = c.len;
      trimmed = c.trimmed;
      out_nbytes[(long)b * cells + lane] = len;
    }
    cnt[HILC_FORWARD_LR_PACKETS] += __popcll(__ballot(len > 0));
    cnt[HILC_FORWARD_LR_TRIMMED] += __popcll(__ballot(trimmed));
    int sum = len;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) sum += __shfl_xor(sum, x, 64);
    cnt[HILC_FORWARD_LR_BYTES] += sum;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HILC_FORWARD_LR_WORDS; ++k) row[k] = cnt[k];
  }

  // the rows: one lane per output byte; every lane runs every pass (the owners move by shuffles)
  const int per_route = burst * tb, total = fanout * per_route;
  uint8_t* orow = out + (long)b * total;
  for (int base = 0; base < total; base += LANES) {
    const int e = base + lane;
    const int j = min(e / per_route, fanout - 1);
    const int t = __shfl(owner, j);
    if (e >= total) continue;
    const int k = (e - j * per_route) / tb;
    const int q = e - j * per_route - k * tb;               // the byte of the row
    const Cut c = cut_of(arr, max_a, aw, pick, pick_count, t, k, burst, L, tb, T, n_max, m, order, keep_fec);
    orow[e] = (uint8_t)cut_byte(c, q);
  }
}

static inline int check_common(int B, int T, int max_arrivals, int n_max, int m, int order, int burst, long* tb) {
  if (B <= 0 || T <= 0 || max_arrivals < 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || n_max > 31 || m < 0 || m > n_max || n_max + m > MAX_N || order < -1 || order > HILC_DTX_MAX_ORDER) return HILC_ERR_RANGE;
  if (burst < 1 || burst > HILC_FORWARD_MAX_BURST) return HILC_ERR_RANGE;
  *tb = HILC_WIRE_TRANSPORT_HEADER + packet_bytes<long>(n_max + m, T);
  if (*tb >= (1L << 15) || (order >= 0 && HILC_WIRE_TRANSPORT_HEADER + 1 + order > *tb)) return HILC_ERR_SHAPE;
  return HILC_OK;
}

}  // namespace

extern "C" int hilc_forward_classify(const int* arrivals, const int* offsets, int max_arrivals, const int* action, int* rows, int* pick,
                                     int* pick_count, int B, int T, int n_max, int m, int order, int burst, int hang_hops, void* stream) {
  if (!arrivals || !offsets || !rows || !pick || !pick_count) return HILC_ERR_NULL;
  long tb = 0;
  const int rc = check_common(B, T, max_arrivals, n_max, m, order, burst, &tb);
  if (rc != HILC_OK) return rc;
  if (hang_hops < 0 || hang_hops > HILC_FORWARD_MAX_HANG_HOPS) return HILC_ERR_RANGE;
  return launch(forward_classify_kernel, waves_grid(B), stream, arrivals, offsets, max_arrivals, (int)((tb + 3) / 4), action, rows, pick,
                pick_count, B, T, n_max, m, order, (int)tb, burst, hang_hops);
}

extern "C" int hilc_forward_route(const int* arrivals, int max_arrivals, const int* action, const int* room, const int* layers,
                                  const int* sender_rows, const int* pick, const int* pick_count, int* routes, int* new_routes,
                                  int* rows, uint8_t* out, int* out_nbytes, int B, int T, int n_max, int m, int order, int fanout,
                                  int burst, int keep_fec, void* stream) {
  if (!arrivals || !room || !layers || !sender_rows || !pick || !pick_count || !routes || !new_routes || !rows || !out || !out_nbytes)
    return HILC_ERR_NULL;
  long tb = 0;
  const int rc = check_common(B, T, max_arrivals, n_max, m, order, burst, &tb);
  if (rc != HILC_OK) return rc;
  if (fanout < 1 || fanout > HILC_FORWARD_MAX_FANOUT) return HILC_ERR_RANGE;
  return launch(forward_route_kernel, waves_grid(B), stream, arrivals, max_arrivals, (int)((tb + 3) / 4), action, room, layers,
                sender_rows, pick, pick_count, routes, new_routes, rows, out, out_nbytes, B, T, n_max, m, order, (int)tb, fanout, burst,
                keep_fec != 0 ? 1 : 0);
}
