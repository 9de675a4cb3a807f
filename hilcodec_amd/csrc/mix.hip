// Room mixing at the tail of the graphed receiver (graph_step.GraphedDecodeHop(mix=MixConfig(...))): every slot in a room hears the
// sum of the room's loudest other members (an "N - 1" mix over the room's top-k speakers).  The definition, bit for bit, is
// hilcodec_amd/mixer.py.  Two launches, because the selection needs every slot's score:
//
//   hilc_mix_levels  per slot, the float64 energy of its output row (64 lane partials, added in lane order) and the peak-hold score
//                    max(E, prev / 2), updated in place (prev = 0 on a hop with an action).  One wave per slot (slot.h).
//   hilc_mix_rooms   per listener slot, its room's speakers by top_k rounds of a lexicographic (score, lowest slot) arg-max over the
//                    B slots, then the fp32 sum of the speakers other than itself in ascending slot order, clamped to [-1, 1].
//                    One workgroup per listener; every element of `mixed` and `speakers` is written on every hop.
//
// No atomics; wave-uniform or workgroup-uniform branches around every barrier.
#include "slot.h"

namespace {

using namespace slot;


__global__ __launch_bounds__(THREADS) void mix_levels_kernel(const float* __restrict__ wav, double* __restrict__ score,
                                                             const int* __restrict__ action, int B, int L) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const float* x = wav + (long)b * L;
  // lane l: the squares of the samples i = l (mod 64) in increasing i (each product is exact in float64, each sum rounded)
  double p = 0.0;
  for (int i = lane; i < L; i += LANES) {
    const double xd = (double)x[i];
    p = __dadd_rn(p, __dmul_rn(xd, xd));
  }
  const double E = lane_ordered_sum(p);
  if (lane == 0) {
    // slot::is_reset, spelled out: inlined from the helper, the compiler lays this branch's blocks out in another order
    const double prev = (action != nullptr && action[b] != 0) ? 0.0 : score[b];
    const double half = __dmul_rn(0.5, prev);
    score[b] = E > half ? E : half;
  }
}

// a is ahead of b in (score descending, slot ascending); a slot of -1 is "none" and loses to every candidate
__device__ __forceinline__ bool ahead(double sa, int ja, double sb, int jb) {
  if (ja < 0) return false;
  if (jb < 0) return true;
  return sa > sb || (sa == sb && ja < jb);
}

__global__ __launch_bounds__(THREADS) void mix_rooms_kernel(const float* __restrict__ wav, const int* __restrict__ room,
                                                            const double* __restrict__ score, int top_k, float* __restrict__ mixed,
                                                            int* __restrict__ speakers, int B, int L) {
  __shared__ double wbest[WAVES];
  __shared__ int wslot[WAVES];
  __shared__ int sel[HILC_MIXER_MAX_TOP_K];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = room[b];
  float* out = mixed + (long)b * L;
  if (r < 0) {                                            // in no room: a zero row, not a speaker (workgroup-uniform)
    for (int i = tid; i < L; i += THREADS) out[i] = 0.f;
    if (tid == 0) speakers[b] = 0;
    return;
  }
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

}  // namespace

extern "C" int hilc_mix_levels(const float* wav, double* score, const int* action, int B, int L, void* stream) {
  if (!wav || !score) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  return launch(mix_levels_kernel, waves_grid(B), stream, wav, score, action, B, L);
}

extern "C" int hilc_mix_rooms(const float* wav, const int* room, const double* score, int top_k, float* mixed, int* speakers, int B,
                              int L, void* stream) {
  if (!wav || !room || !score || !mixed || !speakers) return HILC_ERR_NULL;
  if (B < 1 || L < 1) return HILC_ERR_SHAPE;
  if (top_k < 1 || top_k > HILC_MIXER_MAX_TOP_K) return HILC_ERR_UNSUPPORTED;
  return launch(mix_rooms_kernel, dim3((unsigned)B), stream, wav, room, score, top_k, mixed, speakers, B, L);
}
