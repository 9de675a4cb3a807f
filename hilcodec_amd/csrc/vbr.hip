// Quality-targeted variable bitrate of the graphed sender (graph_step.GraphedEncodeHop(vbr=VbrConfig(...))): per slot and hop, how many
// of the quantiser's stages the packet carries.  The quantiser is trained with quantiser dropout, so the first s stages of an n-stage code
// are a valid s-stage code, and the encoder's caches do not depend on the quantiser: truncating a code after the fact is exact.  The
// definition, bit for bit, is hilcodec_amd/vbr.py.  One launch between the quantiser and the packer:
//
//   hilc_vbr_select  per slot, the float64 distortion D[s] of the hop after s stages (the residual chain of rvq_encode_kernel replayed
//                    from the indices; 64 lane partials per frame, added in lane order), the smallest s in [n_lo, n_b] with
//                    D[s] <= rho D[0], an optional integer token bucket (bits of credit per slot, updated in place) that caps it, and
//                    the rows >= n_eff of the slot's indices set to -1.  One wave per slot (slot.h).
//
// No atomics, no barriers; every output element is written on every hop.
#include "slot.h"

namespace {

using namespace slot;

constexpr int MAX_J = 8;           // channels per lane: C <= 512 (and n <= MAX_N: D[0..n] sits in lanes 0..n)

__global__ __launch_bounds__(THREADS) void vbr_select_kernel(const float* __restrict__ z, int64_t* indices,
                                                             const float* __restrict__ codebooks, const int* __restrict__ n_per_stream,
                                                             const int* __restrict__ action, const int* __restrict__ hold,
                                                             int* __restrict__ credit, int* __restrict__ n_eff,
                                                             double* __restrict__ distortion, int B, int T, int C, int K, int n, int n_lo,
                                                             double rho, int stage_bits, int rate_bits, int burst_bits) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const int J = C >> 6;
  const int nb = n_per_stream == nullptr ? n : clampi(__builtin_amdgcn_readfirstlane(n_per_stream[b]), 1, n);
  const int lo = n_lo < nb ? n_lo : nb;
  const bool fresh = action != nullptr && __builtin_amdgcn_readfirstlane(action[b]) != 0;   // a start, a resume or a bitrate change
  const bool held = hold != nullptr && __builtin_amdgcn_readfirstlane(hold[b]) != 0;
  long cr = 0;
  if (credit != nullptr) cr = fresh ? burst_bits : __builtin_amdgcn_readfirstlane(credit[b]);

  double acc = 0.0;                                       // lane s <= nb: D[s]
  int ne = nb;
  if (!held) {                                            // wave-uniform
    for (int t = 0; t < T; ++t) {
      const float* zr = z + ((long)b * T + t) * C + lane;
      float r[MAX_J];
#pragma unroll
      for (int j = 0; j < MAX_J; ++j) r[j] = j < J ? zr[64 * j] : 0.f;
      for (int s = 0; s <= nb; ++s) {
        // lane l: the squares of its channels l + 64 j in increasing j (each product and each sum rounded in float64)
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < MAX_J; ++j)
          if (j < J) {
            const double rd = (double)r[j];
            p = __dadd_rn(p, __dmul_rn(rd, rd));
          }
        const double sum = __dadd_rn(acc, lane_ordered_sum(p));
        acc = lane == s ? sum : acc;
        if (s < nb) {
          const long long code = indices[index_at(s, B, b, T, t)];        // wave-uniform
          const int k = __builtin_amdgcn_readfirstlane((int)(code < 0 ? 0 : (code > K - 1 ? K - 1 : code)));
          const float* cb = codebooks + ((long)s * K + k) * C + lane;
#pragma unroll
          for (int j = 0; j < MAX_J; ++j)
            if (j < J) r[j] = __fsub_rn(r[j], cb[64 * j]);
        }
      }
    }
    // the smallest s in [lo, nb] with D[s] <= rho D[0]
    const double bar = __dmul_rn(rho, readlane_d(acc, 0));
    const unsigned long long ok = __ballot(lane >= lo && lane <= nb && acc <= bar);
    ne = ok != 0ull ? (int)__builtin_ctzll(ok) : nb;
    if (credit != nullptr) {
      cr = cr + rate_bits < burst_bits ? cr + rate_bits : burst_bits;
      const long most = cr / stage_bits;
      const int n_cap = most < lo ? lo : (most > nb ? nb : (int)most);
      ne = ne < n_cap ? ne : n_cap;
      cr -= (long)ne * stage_bits;
    }
  }
  // D[s > nb] repeats D[nb]; a held slot's row is zero
  const double d_last = readlane_d(acc, __builtin_amdgcn_readfirstlane(nb));
  if (lane <= n) distortion[(long)b * (n + 1) + lane] = held ? 0.0 : (lane <= nb ? acc : d_last);
  if (lane == 0) {
    n_eff[b] = ne;
    if (credit != nullptr) credit[b] = (int)cr;
  }
  clear_rows(indices, ne, n, B, b, T, lane);              // the rows >= n_eff of this slot
}

}  // namespace

extern "C" int hilc_vbr_select(const float* z, int64_t* indices, const float* codebooks, const int* n_per_stream, const int* action,
                               const int* hold, int* credit, int* n_eff, double* distortion, int B, int T, int C, int K, int Nq, int n,
                               int n_lo, double rho, int stage_bits, int rate_bits, int burst_bits, void* stream) {
  if (!z || !indices || !codebooks || !n_eff || !distortion) return HILC_ERR_NULL;
  if (!credit && rate_bits != 0) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0 || C <= 0 || K <= 0 || Nq <= 0) return HILC_ERR_SHAPE;
  if (n < 1 || n > Nq || n_lo < 1 || n_lo > n || !(rho > 0.0 && rho <= 1.0)) return HILC_ERR_RANGE;
  if (credit) {
    // the bucket never runs dry below the floor, and 2 burst_bits fits an int
    if (stage_bits < 1 || (long)rate_bits < (long)stage_bits * n_lo || burst_bits < rate_bits || burst_bits > (1 << 30))
      return HILC_ERR_RANGE;
  }
  if (n > MAX_N || (C & 63) != 0 || C > 64 * MAX_J) return HILC_ERR_UNSUPPORTED;
  return launch(vbr_select_kernel, waves_grid(B), stream, z, indices, codebooks, n_per_stream, action, hold, credit, n_eff, distortion,
                B, T, C, K, n, n_lo, rho, stage_bits, rate_bits, burst_bits);
}
