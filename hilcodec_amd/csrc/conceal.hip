// Loss concealment of the graphed receiver (graph_step.GraphedDecodeHop(conceal=True)): a slot whose packet did not arrive
// is decoded from the codes of the last frame it received, repeated over the hop, and its wav row is faded towards silence over
// F hops; a received packet after a loss fades back in.  Two launches per hop, both captured in the receiver's graph:
//
//   hilc_conceal_prepare  after hilc_state_slots_apply, before hilc_rvq_decode_packed.  Works on the receiver's per-hop control
//                         buffer (re-uploaded in full by the host every hop, so the graph may write into it for this hop): per slot
//                         it updates the concealment state, writes a substitute packet and n for a concealed slot, marks a
//                         device-decided hold, and records the slot's gain ramp.
//   hilc_conceal_gain     after the decoder, before hilc_state_slots_hold: multiplies the wav rows that have a ramp.
//
// State row of slot b (int32, n_max + HILC_WIRE_CONCEAL_CODES words): HILC_WIRE_CONCEAL_RUN k (hops lost in a row, 0..F), _HAS, _N
// (stored n), _CODES + s the code of stage s of the last frame of the last packet received (0 for s >= stored n).  Ramp word of slot
// b: 0 none; r in 1..F: a lost hop, gains G[r - 1] -> G[r]; r in -F..-1: a received hop after -r lost ones, gains G[-r] -> G[0].
//
// Both kernels: one wave per slot (slot.h), wave-uniform branches only.  The common case (every packet received) costs one round of
// loads and one of stores per slot in prepare, and one load per slot in gain.
#include "slot.h"

namespace {

using namespace slot;

__global__ __launch_bounds__(THREADS) void conceal_prepare_kernel(int* __restrict__ state, const int* __restrict__ action,
                                                                  int* __restrict__ hold, const int* __restrict__ lost,
                                                                  int* __restrict__ n_slot, uint8_t* __restrict__ packets,
                                                                  int* __restrict__ ramp, int B, int T, int n_max, int stride, int F) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b, lane = me.lane();
  const int words = n_max + HILC_WIRE_CONCEAL_CODES;
  int* st = state + (long)b * words;
  uint8_t* pk = packets + (long)b * stride;
  // every load of the slot in one round: the last frame's code of stage `lane` is read whether or not the packet arrived
  const int act = action[b], held = hold[b], gone = lost[b], n_in = n_slot[b];
  const int old = lane < words ? st[lane] : 0;
  const int fresh = lane < n_max ? code_at(pk, 10 * (lane * T + T - 1)) : 0;
  const int run0 = __builtin_amdgcn_readfirstlane(__shfl(old, HILC_WIRE_CONCEAL_RUN));
  const int has0 = __builtin_amdgcn_readfirstlane(__shfl(old, HILC_WIRE_CONCEAL_HAS));
  const int n0 = __builtin_amdgcn_readfirstlane(__shfl(old, HILC_WIRE_CONCEAL_N));
  const bool reset = act != 0;                         // a start or a resume on this hop: no stored codes, run 0
  const int k = reset ? 0 : clampi(run0, 0, F);
  const bool has = !reset && has0 != 0;
  int word = reset ? 0 : old;                          // this lane's word of the state row after the hop
  int r = 0;
  if (held != 0) {
    // host-held or stopped: the state is left as it is (a start on the same hop is applied first)
  } else if (gone == 0) {
    const int nb = clampi(n_in, 1, n_max);
    const int s = lane - HILC_WIRE_CONCEAL_CODES;
    const int c = __shfl(fresh, s < 0 ? 0 : s);        // lane s read stage s's code of the packet's last frame
    word = lane == HILC_WIRE_CONCEAL_RUN ? 0 : (lane == HILC_WIRE_CONCEAL_HAS ? 1 : (lane == HILC_WIRE_CONCEAL_N ? nb : (s < nb ? c : 0)));
    r = k > 0 ? -k : 0;
  } else if (has && k < F) {
    const int nb = clampi(n0, 1, n_max);
    const int count = nb * T;
    const int len = code_bytes(count);
    // the substitute packet: stage s of every frame = stored code s, in the layout of hilc_pack_codes_10bit
    for (int j0 = 0; j0 < stride; j0 += 64) {
      const int j = j0 + lane;
      const PackedByte at = packed_byte(j);
      const int i0 = at.i0;
      const int s0 = min(i0 / T, MAX_N - 1), s1 = min((i0 + 1) / T, MAX_N - 1);
      const uint32_t c0 = (uint32_t)__shfl(old, HILC_WIRE_CONCEAL_CODES + s0) & 1023u;
      const uint32_t c1 = (uint32_t)__shfl(old, HILC_WIRE_CONCEAL_CODES + s1) & 1023u;
      if (j < stride) {
        uint32_t out = 0;
        if (j < len) out = at.of((c0 << 10) | (i0 + 1 < count ? c1 : 0u));
        pk[j] = (uint8_t)out;
      }
    }
    if (lane == 0) n_slot[b] = nb;
    if (lane == HILC_WIRE_CONCEAL_RUN) word = k + 1;
    r = k + 1;
  } else {
    // nothing received since the start, or faded out: a device-decided hold
    if (lane == 0) hold[b] = HILC_SESSIONS_HOLD_HELD;
  }
  if (lane < words) st[lane] = word;
  if (lane == 0) ramp[b] = r;
}

__global__ __launch_bounds__(THREADS) void conceal_gain_kernel(float* __restrict__ wav, const int* __restrict__ ramp,
                                                               const float* __restrict__ gains, const float* __restrict__ weights,
                                                               int B, int S, int F) {
  const Wave me = this_wave(B);
  if (!me.ok) return;
  const int b = me.b;
  const int r = ramp[b];
  if (r == 0 || r > F || r < -F) return;               // no ramp: the row is not touched
  const int a = r > 0 ? r - 1 : -r;
  const int c = r > 0 ? r : 0;
  const float ga = gains[a];
  const float d = __fsub_rn(gains[c], ga);
  float* row = wav + (long)b * S;
  for (int s = me.lane(); s < S; s += LANES) row[s] = __fmul_rn(row[s], __fadd_rn(ga, __fmul_rn(d, weights[s])));
}

}  // namespace

extern "C" int hilc_conceal_prepare(int* state, const int* action, int* hold, const int* lost, int* n_per_stream, uint8_t* packets,
                                    int* ramp, int B, int T, int n_max, int fade_hops, void* stream) {
  if (!state || !action || !hold || !lost || !n_per_stream || !packets || !ramp) return HILC_ERR_NULL;
  if (B <= 0 || T <= 0) return HILC_ERR_SHAPE;
  if (n_max < 1 || fade_hops < 1) return HILC_ERR_RANGE;
  if (n_max > MAX_N) return HILC_ERR_UNSUPPORTED;
  const long stride = packet_bytes<long>(n_max, T);
  if (stride > (1L << 30)) return HILC_ERR_SHAPE;
  return launch(conceal_prepare_kernel, waves_grid(B), stream, state, action, hold, lost, n_per_stream, packets, ramp, B, T, n_max,
                (int)stride, fade_hops);
}

extern "C" int hilc_conceal_gain(float* wav, const int* ramp, const float* gains, const float* weights, int B, int samples,
                                 int fade_hops, void* stream) {
  if (!wav || !ramp || !gains || !weights) return HILC_ERR_NULL;
  if (B <= 0 || samples <= 0) return HILC_ERR_SHAPE;
  if (fade_hops < 1) return HILC_ERR_RANGE;
  return launch(conceal_gain_kernel, waves_grid(B), stream, wav, ramp, gains, weights, B, samples, fade_hops);
}
