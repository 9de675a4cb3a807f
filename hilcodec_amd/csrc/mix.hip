// Room mixing at the tail of the graphed receiver (graph_step.GraphedDecodeHop(mix=MixConfig(...))): every slot in a room hears the
// sum of the room's loudest other members (an "N - 1" mix over the room's top-k speakers).  The definition, bit for bit, is
// hilcodec_amd/mixer.py.  Two launches, because the selection needs every slot's score, and a third with per-speaker levelling:
//
//   hilc_mix_levels     per slot, the float64 energy of its output row (64 lane partials, added in lane order) and the peak-hold score
//                       max(E, prev / 2), updated in place (prev = 0 on a hop with an action).  One wave per slot (slot.h).
//   hilc_mix_gains      (MixConfig.level) per slot, the same energy and from it the slot's smoothed power and its gain at the hop's
//                       start and end, updated in place.  One wave per slot; lane 0 does the update.
//   hilc_mix_rooms      per listener slot, its room's speakers by top_k rounds of a lexicographic (score, lowest slot) arg-max over the
//                       B slots, then the fp32 sum of the speakers other than itself in ascending slot order, clamped to [-1, 1].
//                       One workgroup per listener; every element of `mixed` and `speakers` is written on every hop.
//   hilc_mix_rooms_dyn  (MixConfig.level or .limit) hilc_mix_rooms with levelled terms (each speaker's row times its gain, which moves
//                       linearly over the hop) and / or the per-listener limiter in place of the clamp: the sums go to LDS, the
//                       waves take the sub-frames' peaks, one thread scans the envelope over the at most 512 sub-frames, a thread
//                       per sub-frame turns it into the sub-frame's gain, and a second pass applies the gains.
//                       Hops of at most 1 024 samples take an instantiation with a short LDS row (one round of workgroups at 1 024 listeners).
//
// No atomics; wave-uniform or workgroup-uniform branches around every barrier.  Every float64 operation of the gain and limiter
// rules is a single rounded operation (__dadd_rn, __dmul_rn, __ddiv_rn): mixer.py states the same ones in numpy.
#include "slot.h"

namespace {

using namespace slot;

// the limiter keeps a listener's sums in LDS: a row of SHORT_L samples for the hops the product plays (at most 3 200 samples at 48 kHz,
// 320 at 24 kHz) leaves room for every workgroup of 1 024 listeners at once; the longest row takes a quarter of a CU's LDS
constexpr int SHORT_L = 1024;

// the lane-ordered float64 energy of slot me.b's row (mixer.levels)
__device__ __forceinline__ double row_energy(const float* __restrict__ x, int L, int lane) {
  // lane l: the squares of the samples i = l (mod 64) in increasing i (each product is exact in float64, each sum rounded)
  double p = 0.0;
  for (int i = lane; i < L; i += LANES) {
    const double xd = (double)x[i];
    p = __dadd_rn(p, __dmul_rn(xd, xd));
  }
  return lane_ordered_sum(p);
}

__global__ __launch_bounds__(THREADS) void mix_levels_kernel(const float* __restrict__ wav, double* __restrict__ score,
                                                             const int* __restrict__ action, int B, int L) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const double E = row_energy(wav + (long)b * L, L, lane);
  if (lane == 0) {
    // slot::is_reset, spelled out: inlined from the helper, the compiler lays this branch's blocks out in another order
    const double prev = (action != nullptr && action[b] != 0) ? 0.0 : score[b];
    const double half = __dmul_rn(0.5, prev);
    score[b] = E > half ? E : half;
  }
}

// the levelling rule of mixer.update_gains
struct LevelRule {
  double gate2, lo, hi, up, down, min_gain, max_gain, smooth;
};

__global__ __launch_bounds__(THREADS) void mix_gains_kernel(const float* __restrict__ wav, double* __restrict__ gains,
                                                            double* __restrict__ power, const int* __restrict__ action,
                                                            LevelRule rule, int B, int L) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const double E = row_energy(wav + (long)b * L, L, lane);
  if (lane == 0) {
    const bool reset = is_reset(action, b);
    const double g0 = reset ? 1.0 : gains[2 * (long)b + 1];
    double pw = reset ? 0.0 : power[b];
    double g1 = g0;
    const double m = __ddiv_rn(E, (double)L);
    if (m >= rule.gate2) {
      if (pw == 0.0) pw = m;
      else pw = __dadd_rn(pw, __dmul_rn(rule.smooth, __dsub_rn(m, pw)));
      const double v = __dmul_rn(__dmul_rn(g0, g0), pw);
      if (v < rule.lo) {
        const double g = __dmul_rn(g0, rule.up);
        g1 = g < rule.max_gain ? g : rule.max_gain;
      } else if (v > rule.hi) {
        const double g = __dmul_rn(g0, rule.down);
        g1 = g > rule.min_gain ? g : rule.min_gain;
      }
    }
    gains[2 * (long)b] = g0;
    gains[2 * (long)b + 1] = g1;
    power[b] = pw;
  }
}

// a is ahead of b in (score descending, slot ascending); a slot of -1 is "none" and loses to every candidate
__device__ __forceinline__ bool ahead(double sa, int ja, double sb, int jb) {
  if (ja < 0) return false;
  if (jb < 0) return true;
  return sa > sb || (sa == sb && ja < jb);
}

// The speakers of listener b's room r >= 0 into sel[0 .. count) in ascending slot order, and speakers[b]; returns the count.  Called
// by every thread of the workgroup (it holds barriers); sel is complete for every thread on return.
__device__ __forceinline__ int select_speakers(const int* __restrict__ room, const double* __restrict__ score, int top_k, int r, int b,
                                               int B, double* wbest, int* wslot, int* sel, int* __restrict__ speakers) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the room's speakers: round k picks the first candidate behind round k - 1's pick in (score descending, slot ascending)
  double last_s = 0.0;
  int last_j = -1;                                        // -1: no pick yet
  int nsel = 0;
  for (int k = 0; k < top_k; ++k) {
    double bs = 0.0;
    int bj = -1;
    for (int j = tid; j < B; j += THREADS) {
      if (room[j] != r) continue;
      const double s = score[j];
      if (!(s > 0.0)) continue;
      if (last_j >= 0 && !ahead(last_s, last_j, s, j)) continue;   // picked in an earlier round
      if (ahead(s, j, bs, bj)) { bs = s; bj = j; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(bs, m, 64);
      const int oj = __shfl_xor(bj, m, 64);
      if (ahead(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (lane == 0) { wbest[wave] = bs; wslot[wave] = bj; }
    __syncthreads();
    bs = wbest[0];
    bj = wslot[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (ahead(wbest[w], wslot[w], bs, bj)) { bs = wbest[w]; bj = wslot[w]; }
    __syncthreads();                                      // every thread has read this round's partials
    if (bj < 0) break;                                    // the room has no more candidates (the same in every thread)
    if (tid == 0) sel[nsel] = bj;
    last_s = bs;
    last_j = bj;
    ++nsel;
  }
  // into ascending slot order (at most 8 entries: one thread)
  if (tid == 0) {
    for (int i = 1; i < nsel; ++i) {
      const int v = sel[i];
      int j = i - 1;
      for (; j >= 0 && sel[j] > v; --j) sel[j + 1] = sel[j];
      sel[j + 1] = v;
    }
    int mine = 0;
    for (int i = 0; i < nsel; ++i) mine |= sel[i] == b;
    speakers[b] = mine;
  }
  __syncthreads();
  return nsel;
}

__global__ __launch_bounds__(THREADS) void mix_rooms_kernel(const float* __restrict__ wav, const int* __restrict__ room,
                                                            const double* __restrict__ score, int top_k, float* __restrict__ mixed,
                                                            int* __restrict__ speakers, int B, int L) {
  __shared__ double wbest[WAVES];
  __shared__ int wslot[WAVES];
  __shared__ int sel[HILC_MIXER_MAX_TOP_K];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int r = room[b];
  float* out = mixed + (long)b * L;
  if (r < 0) {                                            // in no room: a zero row, not a speaker (workgroup-uniform)
    for (int i = tid; i < L; i += THREADS) out[i] = 0.f;
    if (tid == 0) speakers[b] = 0;
    return;
  }
  const int nsel = select_speakers(room, score, top_k, r, b, B, wbest, wslot, sel, speakers);
  for (int i = tid; i < L; i += THREADS) {
    float acc = 0.f;
    bool first = true;
    for (int t = 0; t < nsel; ++t) {
      const int j = sel[t];
      if (j == b) continue;
      const float v = wav[(long)j * L + i];
      acc = first ? v : __fadd_rn(acc, v);
      first = false;
    }
    out[i] = fminf(fmaxf(acc, -1.f), 1.f);
  }
}

struct LimitRule {
  double ceiling, release;
  int sub;
};

// LEVEL: gains != null, the terms are levelled; LIMIT: limiter != null (then L <= MAX_L <= HILC_MIXER_MAX_LIMIT_L and sub in
// [HILC_MIXER_MIN_SUB, HILC_MIXER_MAX_SUB], so at most MAX_L / HILC_MIXER_MIN_SUB sub-frames: checked by the entry point), the limiter
// in place of the clamp.  Neither: mix_rooms_kernel's result by the same operations.
template <bool LEVEL, bool LIMIT, int MAX_L>
__global__ __launch_bounds__(THREADS) void mix_rooms_dyn_kernel(const float* __restrict__ wav, const int* __restrict__ room,
                                                                const double* __restrict__ score, int top_k,
                                                                const double* __restrict__ gains, double* __restrict__ limiter,
                                                                LimitRule rule, const int* __restrict__ action,
                                                                float* __restrict__ mixed, int* __restrict__ speakers, int B, int L) {
  __shared__ double wbest[WAVES];
  __shared__ int wslot[WAVES];
  __shared__ int sel[HILC_MIXER_MAX_TOP_K];
  __shared__ double g_start[HILC_MIXER_MAX_TOP_K], g_step[HILC_MIXER_MAX_TOP_K];   // a speaker's g0 and g1 - g0
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = room[b];
  float* out = mixed + (long)b * L;
  int nsel = 0;                                           // in no room: no terms, not a speaker (r is workgroup-uniform)
  if (r >= 0) nsel = select_speakers(room, score, top_k, r, b, B, wbest, wslot, sel, speakers);
  else if (tid == 0) speakers[b] = 0;
  if constexpr (LEVEL) {
    if (tid < nsel) {
      const long j = sel[tid];
      const double g0 = gains[2 * j];
      g_start[tid] = g0;
      g_step[tid] = __dsub_rn(gains[2 * j + 1], g0);
    }
    __syncthreads();
  }
  // listener b's sum at sample i: its speakers other than itself in ascending slot order, every sum rounded in fp32
  auto sum_at = [&](int i) {
    float acc = 0.f;
    bool first = true;
    double ramp = 0.0;
    if constexpr (LEVEL) ramp = __ddiv_rn((double)(i + 1), (double)L);
    for (int t = 0; t < nsel; ++t) {
      const int j = sel[t];
      if (j == b) continue;
      float v = wav[(long)j * L + i];
      if constexpr (LEVEL) {
        const double g = __dadd_rn(g_start[t], __dmul_rn(g_step[t], ramp));
        v = __double2float_rn(__dmul_rn((double)v, g));
      }
      acc = first ? v : __fadd_rn(acc, v);
      first = false;
    }
    return acc;
  };
  if constexpr (!LIMIT) {
    for (int i = tid; i < L; i += THREADS) out[i] = fminf(fmaxf(sum_at(i), -1.f), 1.f);
  } else {
    constexpr int MAX_SUBFRAMES = MAX_L / HILC_MIXER_MIN_SUB;
    __shared__ float acc_row[MAX_L];
    __shared__ float peak[MAX_SUBFRAMES];
    __shared__ double env[MAX_SUBFRAMES];                 // e_s
    __shared__ double gain[MAX_SUBFRAMES + 1];            // gain[s + 1] = G_s, gain[0] = G_(-1)
    const int sub = rule.sub;
    const int nsub = (L + sub - 1) / sub;                 // <= MAX_SUBFRAMES
    // pass 1: the sums, then each sub-frame's peak by one wave (max is exact and order-free)
    for (int i = tid; i < L; i += THREADS) acc_row[i] = sum_at(i);
    __syncthreads();
    for (int s = wave; s < nsub; s += WAVES) {
      const int lo = s * sub, n = min(sub, L - lo);
      float p = 0.f;
      for (int k = lane; k < n; k += LANES) p = fmaxf(p, fabsf(acc_row[lo + k]));
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) p = fmaxf(p, __shfl_xor(p, m, 64));
      if (lane == 0) peak[s] = p;
    }
    __syncthreads();
    // the envelope: one thread reads the state and scans the sub-frames; then a thread per sub-frame turns e_s into G_s, and the last
    // sub-frame's thread writes the state (behind the barrier that follows thread 0's reads of it)
    if (tid == 0) {
      const bool reset = is_reset(action, b);
      double e = reset ? 0.0 : limiter[2 * (long)b];
      gain[0] = reset ? 1.0 : limiter[2 * (long)b + 1];
      for (int s = 0; s < nsub; ++s) {
        const double p = (double)peak[s], rel = __dmul_rn(rule.release, e);
        e = p > rel ? p : rel;
        env[s] = e;
      }
    }
    __syncthreads();
    for (int s = tid; s < nsub; s += THREADS) {
      const double e = env[s];
      const double G = e > rule.ceiling ? __ddiv_rn(rule.ceiling, e) : 1.0;
      gain[s + 1] = G;
      if (s == nsub - 1) {
        limiter[2 * (long)b] = e;
        limiter[2 * (long)b + 1] = G;
      }
    }
    __syncthreads();
    // pass 2: an immediate attack, a linear release over the sub-frame
    for (int i = tid; i < L; i += THREADS) {
      const int s = i / sub, k = i - s * sub, n = min(sub, L - s * sub);
      const double Gp = gain[s], Gs = gain[s + 1];
      double g = Gs;
      if (!(Gs <= Gp)) g = __dadd_rn(Gp, __dmul_rn(__dsub_rn(Gs, Gp), __ddiv_rn((double)(k + 1), (double)n)));
      const float v = __double2float_rn(__dmul_rn((double)acc_row[i], g));
      out[i] = fminf(fmaxf(v, -1.f), 1.f);
    }
  }
}

}  // namespace

extern "C" int hilc_mix_levels(const float* wav, double* score, const int* action, int B, int L, void* stream) {
  if (!wav || !score) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  return launch(mix_levels_kernel, waves_grid(B), stream, wav, score, action, B, L);
}

extern "C" int hilc_mix_gains(const float* wav, double* gains, double* power, const int* action, double gate2, double lo, double hi,
                              double up, double down, double min_gain, double max_gain, double smooth, int B, int L, void* stream) {
  if (!wav || !gains || !power) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  // mixer.LevelConfig's conditions, on the derived constants (a NaN fails every comparison)
  if (!(gate2 > 0.0 && lo > 0.0 && hi > lo && up > 1.0 && down > 0.0 && down < 1.0 && min_gain > 0.0 && min_gain <= 1.0 &&
        max_gain >= 1.0 && smooth > 0.0 && smooth <= 1.0))
    return HILC_ERR_UNSUPPORTED;
  const LevelRule rule = {gate2, lo, hi, up, down, min_gain, max_gain, smooth};
  return launch(mix_gains_kernel, waves_grid(B), stream, wav, gains, power, action, rule, B, L);
}

extern "C" int hilc_mix_rooms(const float* wav, const int* room, const double* score, int top_k, float* mixed, int* speakers, int B,
                              int L, void* stream) {
  if (!wav || !room || !score || !mixed || !speakers) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  if (top_k < 1 || top_k > HILC_MIXER_MAX_TOP_K) return HILC_ERR_UNSUPPORTED;
  return launch(mix_rooms_kernel, dim3((unsigned)B), stream, wav, room, score, top_k, mixed, speakers, B, L);
}

extern "C" int hilc_mix_rooms_dyn(const float* wav, const int* room, const double* score, int top_k, const double* gains,
                                  double* limiter, double ceiling, double release, int sub, const int* action, float* mixed,
                                  int* speakers, int B, int L, void* stream) {
  if (!wav || !room || !score || !mixed || !speakers) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  if (top_k < 1 || top_k > HILC_MIXER_MAX_TOP_K) return HILC_ERR_UNSUPPORTED;
  LimitRule rule = {1.0, 0.5, HILC_MIXER_MIN_SUB};
  if (limiter) {
    if (sub < HILC_MIXER_MIN_SUB || sub > HILC_MIXER_MAX_SUB || L > HILC_MIXER_MAX_LIMIT_L) return HILC_ERR_UNSUPPORTED;
    if (!(ceiling > 0.0 && ceiling <= 1.0 && release > 0.0 && release < 1.0)) return HILC_ERR_UNSUPPORTED;
    rule = {ceiling, release, sub};
  }
  const dim3 grid((unsigned)B);
  auto go = [&](auto kernel) {
    return launch(kernel, grid, stream, wav, room, score, top_k, gains, limiter, rule, action, mixed, speakers, B, L);
  };
  if (gains && limiter) return L <= SHORT_L ? go(mix_rooms_dyn_kernel<true, true, SHORT_L>) : go(mix_rooms_dyn_kernel<true, true, HILC_MIXER_MAX_LIMIT_L>);
  if (limiter) return L <= SHORT_L ? go(mix_rooms_dyn_kernel<false, true, SHORT_L>) : go(mix_rooms_dyn_kernel<false, true, HILC_MIXER_MAX_LIMIT_L>);
  if (gains) return go(mix_rooms_dyn_kernel<true, false, 0>);
  return go(mix_rooms_dyn_kernel<false, false, 0>);
}
