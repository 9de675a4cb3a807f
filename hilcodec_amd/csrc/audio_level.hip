// Audio level and level-based speaker selection (hilcodec_amd/audio_level.py: the rules, bit for bit).  A forwarding hop never decodes,
// so it cannot measure who speaks: the sender measures its own hop and says it (an RFC 6464 style level, -dBov in 1 dB steps), and the
// forwarder ranks its senders by what they said.  Two launches, each one wave per slot:
//
//   hilc_audio_level   (sender, graph_step.GraphedEncodeHop(audio_level=True)) per slot, the float64 energy of its 24 kHz hop — 64 lane
//                      partials added in lane order, mixer.py's "Level" — over the hop's length, counted against the 127 thresholds of
//                      dtx.level_table with two wave-wide ballots.
//   hilc_forward_rank  (forwarder, graph_step.GraphedForwardHop(speakers=)) per slot, between hilc_forward_classify and
//                      hilc_forward_route: the slot's smoothed loudness, its rank in its room on the previous hop's keys (a lane-strided
//                      scan over the B slots, the count reduced by shuffles) and the shadow sender row that makes the unchanged
//                      hilc_forward_route order its candidates by loudness.  Integer only.
//
// No LDS, no atomics; every branch around a cross-lane operation is wave-uniform.  The rows: include/hilcodec_amd.h (HILC_SPEAKER_*).
#include "slot.h"

namespace {

using namespace slot;

__global__ __launch_bounds__(THREADS) void audio_level_kernel(const float* __restrict__ x, const double* __restrict__ thr,
                                                              const int* __restrict__ hold, int* __restrict__ level, int B, int L) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  if (is_held(hold, b)) {                                   // wave-uniform: the row is not read
    if (lane == 0) level[b] = HILC_DTX_LEVELS - 1;
    return;
  }
  // lane l: the squares of the samples i = l (mod 64) in increasing i (each product is exact in float64, each sum rounded); then the
  // 64 partials in lane order (mixer.levels)
  const float* row = x + (long)b * L;
  double p = 0.0;
  for (int i = lane; i < L; i += LANES) {
    const double xd = (double)row[i];
    p = __dadd_rn(p, __dmul_rn(xd, xd));
  }
  const double m = __ddiv_rn(lane_ordered_sum(p), (double)L);
  // #{j < 127 : m < thr[j]}, lanes j and j + 64 (a NaN is below no threshold)
  const bool c0 = m < thr[lane];
  const bool c1 = lane + LANES < HILC_DTX_LEVELS - 1 && m < thr[min(lane + LANES, HILC_DTX_LEVELS - 2)];
  const int count = __popcll(__ballot(c0)) + __popcll(__ballot(c1));
  if (lane == 0) level[b] = count;
}

// a slot's place in the order hilc_forward_route sorts by, as that kernel reads a sender row: hi = SD_HANG << 16 | SD_SINCE with its
// clamps, then the lower slot; a is ahead of b
__device__ __forceinline__ int order_word(int hang, int since) {
  return (min(hang, HILC_FORWARD_MAX_HANG_HOPS + 1) << 16) | clampi(since, 0, HILC_FORWARD_MAX_SINCE);
}

__device__ __forceinline__ bool ahead(int ha, int sa, int hb, int sb) { return ha > hb || (ha == hb && sa < sb); }

struct SpeakerRule {
  int fanout, hang_hops, floor_level, attack_shift, decay_q8, margin_db;
};

__global__ __launch_bounds__(THREADS) void forward_rank_kernel(const int* __restrict__ sd, const int* __restrict__ loud,
                                                               const int* __restrict__ room, const int* __restrict__ action,
                                                               const int* __restrict__ shadow_prev, int* __restrict__ shadow,
                                                               int* __restrict__ rows, int B, SpeakerRule rule) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  int* row = rows + (long)b * HILC_SPEAKER_WORDS;
  const int* mine = sd + (long)b * HILC_FORWARD_SD_WORDS;
  const bool start = is_reset(action, b);
  const int hang = mine[HILC_FORWARD_SD_HANG], since = mine[HILC_FORWARD_SD_SINCE];

  // the smoothed loudness: a fast attack towards this hop's level, a linear decay
  int score = start ? 0 : clampi(row[HILC_SPEAKER_SCORE], 0, 256 * HILC_SPEAKER_MAX_LOUD);
  const bool talk = hang == rule.hang_hops + 1;
  const int said = clampi(loud[b], 0, HILC_SPEAKER_MAX_LOUD);
  const int target = talk ? 256 * said : 0;
  if (target > score) score += (target - score + (1 << rule.attack_shift) - 1) >> rule.attack_shift;
  else score = max(target, score - rule.decay_q8);

  // the rank in the room on the previous hop's shadow rows: the slots ahead of this one, counted lane-strided
  const int r = room[b];
  const int my_hang = start ? 0 : shadow_prev[(long)b * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_HANG];
  const bool ranked = r >= 0 && my_hang > 0;                // wave-uniform
  int aheads = 0;
  if (ranked) {
    const int my_h = order_word(my_hang, shadow_prev[(long)b * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_SINCE]);
    for (int t = lane; t < B; t += LANES) {
      if (t == b || room[t] != r || is_reset(action, t)) continue;
      const int h = shadow_prev[(long)t * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_HANG];
      if (h <= 0) continue;
      if (ahead(order_word(h, shadow_prev[(long)t * HILC_FORWARD_SD_WORDS + HILC_FORWARD_SD_SINCE]), t, my_h, b)) ++aheads;
    }
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) aheads += __shfl_xor(aheads, x, 64);
  const int rank = ranked ? aheads : -1;
  const bool stage = rank >= 0 && rank < rule.fanout;

  // the key and the shadow row: hilc_forward_route orders by (SD_HANG, SD_SINCE), which is the key's order
  const bool candidate = hang > 0 && score >= 256 * (HILC_SPEAKER_MAX_LOUD - rule.floor_level);
  const int key = ((score + (stage ? 256 * rule.margin_db : 0)) << 8) | clampi(since, 0, 255);
  if (lane < HILC_FORWARD_SD_WORDS) {
    int v = mine[lane];
    if (lane == HILC_FORWARD_SD_HANG) v = candidate ? 1 + (key >> 16) : 0;
    if (lane == HILC_FORWARD_SD_SINCE) v = candidate ? key & 0xFFFF : 0;
    shadow[(long)b * HILC_FORWARD_SD_WORDS + lane] = v;
  }
  if (lane == 0) {
    const int levelled = start ? 0 : row[HILC_SPEAKER_LEVELLED], staged = start ? 0 : row[HILC_SPEAKER_STAGED];
    row[HILC_SPEAKER_SCORE] = score;
    row[HILC_SPEAKER_RANK] = rank;
    row[HILC_SPEAKER_STAGE] = stage ? 1 : 0;
    row[HILC_SPEAKER_LEVELLED] = levelled + ((talk && said > 0) ? 1 : 0);
    row[HILC_SPEAKER_STAGED] = staged + (stage ? 1 : 0);
  }
}

}  // namespace

extern "C" int hilc_audio_level(const float* x, const double* thr, const int* hold, int* level, int B, int L, void* stream) {
  if (!x || !thr || !level) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  return launch(audio_level_kernel, waves_grid(B), stream, x, thr, hold, level, B, L);
}

extern "C" int hilc_forward_rank(const int* sd, const int* loud, const int* room, const int* action, const int* shadow_prev, int* shadow,
                                 int* rows, int B, int fanout, int hang_hops, int floor_level, int attack_shift, int decay_q8,
                                 int margin_db, void* stream) {
  if (!sd || !loud || !room || !shadow_prev || !shadow || !rows) return HILC_ERR_NULL;
  if (B < 1) return HILC_ERR_SHAPE;
  if (shadow == shadow_prev || shadow == sd) return HILC_ERR_UNSUPPORTED;      // a slot reads every slot's previous row
  if (fanout < 1 || fanout > HILC_FORWARD_MAX_FANOUT || hang_hops < 0 || hang_hops > HILC_FORWARD_MAX_HANG_HOPS) return HILC_ERR_RANGE;
  if (floor_level < 0 || floor_level >= HILC_SPEAKER_MAX_LOUD || attack_shift < 0 || attack_shift > HILC_SPEAKER_MAX_ATTACK_SHIFT ||
      decay_q8 < 1 || decay_q8 > HILC_SPEAKER_MAX_DECAY_Q8 || margin_db < 0 || margin_db > HILC_SPEAKER_MAX_MARGIN_DB)
    return HILC_ERR_RANGE;
  const SpeakerRule rule = {fanout, hang_hops, floor_level, attack_shift, decay_q8, margin_db};
  return launch(forward_rank_kernel, waves_grid(B), stream, sd, loud, room, action, shadow_prev, shadow, rows, B, rule);
}
