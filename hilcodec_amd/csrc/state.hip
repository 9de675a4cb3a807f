// Per-stream sessions of a graphed streaming hop: zero one stream's caches, load them from a staged record, or gather
// them into a record, inside the state block (hilcodec_amd/graph_step.py StateBlock: slice k of stream b at
// block + slice_off[k] + b * slice_len[k]).  A record is one stream's slices concatenated in slice order.
//
// hilc_state_slots_apply runs at the head of every hop and almost always has nothing to do, so the idle case decides
// its form: a fixed grid of APPLY_WGS workgroups, each of which reads the whole `action` array (1024 streams = 4 loads
// per thread, L2-resident) and leaves after one barrier when no entry is active.  When some are, every workgroup
// builds the same list of active streams in LDS (ballot order, deterministic) and the (stream, piece) work items of
// that list are spread over the whole grid: one stream's 306 KB are copied by up to 19 workgroups side by side
// instead of one workgroup's latency-bound loop; each item finds its slices in an LDS copy of the slice table.  (One workgroup per stream that exits on action[b] == 0 would issue
// 1024 workgroups per idle hop and still copy a resumed stream through a single workgroup.)
//
// hilc_state_slots_hold runs at the tail of every hop, after the last write to the block the hop wrote and to its outputs, and
// has the same idle form.  A held stream's slices are copied back from the block the hop read (so it leaves the hop as it
// entered it) and its output rows are set to "nothing this hop"; one more work item per held stream does the outputs.
#include "slot.h"

namespace {

using slot::THREADS;
constexpr int PASS = 4 * THREADS;   // streams scanned per pass: the LDS list holds the active streams of one pass
constexpr int PIECE = 4096;         // floats of a record per work item: 16 per thread, one round of loads (19 items per stream)
constexpr int APPLY_WGS = 256;      // one per CU
constexpr int GATHER_WGS = 256;
// 4 per CU: an item of a held stream is ~3 dependent load -> store rounds (a piece spans ~3 slices), so the copy is latency-bound
// and wants more workgroups in flight than one per CU (1 024 streams, 128 held: 61.6 us with 256, 32.8 with 1 024, 31.0 with
// 2 048; idle: 3.0 / 3.2 / 3.9 us)
constexpr int HOLD_WGS = 1024;

constexpr int MAX_SLICES = 128;     // the slice table lives in LDS (52 slices for the shipped models)

struct Layout {
  const int64_t* off;
  const int* len;
  int nslices;
};

// the slice table in LDS, with the record offset of every slice (pre[k] = sum of len[0..k)): a work item finds its slices with
// a binary search over LDS instead of a walk of dependent scalar loads (one L2 round trip per slice: 26 us for a resumed stream)
struct Table {
  int64_t off[MAX_SLICES];
  int64_t pre[MAX_SLICES + 1];
  int len[MAX_SLICES];
};

__device__ __forceinline__ void load_table(Table& tb, const Layout& L) {
  const int t = threadIdx.x;
  for (int k = t; k < L.nslices; k += THREADS) {
    tb.off[k] = L.off[k];
    tb.len[k] = L.len[k];
  }
  if (t < 64) {                            // wave 0: pre[] by an inclusive wave scan, 64 slices per step
    const int lane = t;
    long carry = 0;
    for (int base = 0; base < L.nslices; base += 64) {
      const int k = base + lane;
      long v = k < L.nslices ? (long)L.len[k] : 0;
      for (int d = 1; d < 64; d <<= 1) {
        const long u = __shfl_up(v, d);
        if (lane >= d) v += u;
      }
      if (k < L.nslices) tb.pre[k + 1] = carry + v;
      carry += __shfl(v, 63);
    }
    if (lane == 0) tb.pre[0] = 0;
  }
  __syncthreads();
}

// dst[0..n) = src[0..n), or zeros when src == nullptr; n <= PIECE; every thread of the workgroup takes part.
// 16-byte vectors only where both addresses are 16-B aligned and n is a multiple of 4 (the per-stream slices of the
// [1, 1023] waveform history, and every slice of a record behind it, are not): dwords otherwise.
__device__ __forceinline__ void move(float* __restrict__ dst, const float* __restrict__ src, int n) {
  const int t = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0 && (n & 3) == 0) {
    const int n4 = n >> 2;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[PIECE / 4 / THREADS];
#pragma unroll
    for (int i = 0; i < PIECE / 4 / THREADS; ++i) {
      const int j = t + i * THREADS;
      v[i] = src != nullptr && j < n4 ? reinterpret_cast<const f32x4*>(src)[j] : z;
    }
#pragma unroll
    for (int i = 0; i < PIECE / 4 / THREADS; ++i) {
      const int j = t + i * THREADS;
      if (j < n4) reinterpret_cast<f32x4*>(dst)[j] = v[i];
    }
  } else {
    float v[PIECE / THREADS];
#pragma unroll
    for (int i = 0; i < PIECE / THREADS; ++i) {
      const int j = t + i * THREADS;
      v[i] = src != nullptr && j < n ? src[j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PIECE / THREADS; ++i) {
      const int j = t + i * THREADS;
      if (j < n) dst[j] = v[i];
    }
  }
}

// the parts of record floats [p0, p1) of stream b: f(block offset of the part, its record offset, its length <= PIECE)
template <typename F>
__device__ __forceinline__ void for_piece(const Table& tb, int nslices, long b, long p0, long p1, F f) {
  int lo = 0, hi = nslices - 1;            // the last slice with pre[k] <= p0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tb.pre[mid] <= p0) lo = mid; else hi = mid - 1;
  }
  for (int k = lo; k < nslices && tb.pre[k] < p1; ++k) {
    const long pre = tb.pre[k], len = tb.len[k];
    const long a = p0 > pre ? p0 : pre;
    const long e = p1 < pre + len ? p1 : pre + len;
    if (e > a) f(tb.off[k] + b * len + (a - pre), a, (int)(e - a));
  }
}

// record floats [p0, p1) of stream b: TO_BLOCK = record -> block (rec == nullptr: zeros), else block -> record
template <bool TO_BLOCK>
__device__ void move_piece(float* block, const Table& tb, int nslices, long b, float* rec, long p0, long p1) {
  for_piece(tb, nslices, b, p0, p1, [&](long at, long r, int n) {
    if (TO_BLOCK)
      move(block + at, rec != nullptr ? rec + r : nullptr, n);
    else
      move(rec + r, block + at, n);
  });
}

// one pass of the stream scan: the streams base + i * THREADS + t with ok[i] set, in ballot order (the same list in every
// workgroup), go to list_b and their val[i] to list_v; returns how many.  Every thread of the workgroup takes part.
__device__ __forceinline__ int compact(const bool (&ok)[4], const int (&val)[4], int base, int* list_b, int* list_v,
                                       int (&cnt)[4][THREADS / 64]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint64_t m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = __ballot(ok[i]);
    if (lane == 0) cnt[i][wave] = __popcll(m[i]);
  }
  __syncthreads();
  int run = 0, pos[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    for (int w = 0; w < THREADS / 64; ++w) {
      if (w == wave) pos[i] = run;
      run += cnt[i][w];
    }
  const uint64_t lt = __lanemask_lt();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (ok[i]) {
      const int p = pos[i] + __popcll(m[i] & lt);
      list_b[p] = base + i * THREADS + t;
      list_v[p] = val[i];
    }
  __syncthreads();
  return run;
}

__global__ __launch_bounds__(THREADS) void state_apply_kernel(float* block, Layout L, int streams, const int* action,
                                                              const float* records, int nrecords) {
  __shared__ int list_b[PASS], list_a[PASS];
  __shared__ int cnt[4][THREADS / 64];
  __shared__ Table tb;
  const int t = threadIdx.x;
  long reclen = -1, npieces = 0;
  for (int base = 0; base < streams; base += PASS) {
    int act[4];
    bool ok[4], any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = base + i * THREADS + t;
      act[i] = b < streams ? action[b] : 0;
      ok[i] = act[i] == -1 || (act[i] >= 1 && act[i] <= nrecords);    // anything else: keep
      any |= ok[i];
    }
    if (!__syncthreads_or(any)) continue;                              // the idle hop ends here
    const int run = compact(ok, act, base, list_b, list_a, cnt);
    if (reclen < 0) {
      load_table(tb, L);
      reclen = tb.pre[L.nslices];
      npieces = (reclen + PIECE - 1) / PIECE;
    }
    const long items = (long)run * npieces;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
      const int j = (int)(it / npieces);
      const long p0 = (it % npieces) * PIECE;
      const long p1 = p0 + PIECE < reclen ? p0 + PIECE : reclen;
      const int b = __builtin_amdgcn_readfirstlane(list_b[j]);
      const int a = __builtin_amdgcn_readfirstlane(list_a[j]);
      float* rec = a > 0 ? const_cast<float*>(records) + (long)(a - 1) * reclen : nullptr;
      move_piece<true>(block, tb, L.nslices, b, rec, p0, p1);
    }
    __syncthreads();                                                   // the next pass rewrites the list
  }
}

__global__ __launch_bounds__(THREADS) void state_gather_kernel(const float* block, Layout L, int streams, const int* slots,
                                                               int nslots, float* records) {
  __shared__ Table tb;
  load_table(tb, L);
  const long reclen = tb.pre[L.nslices];
  const long npieces = (reclen + PIECE - 1) / PIECE;
  const long items = (long)nslots * npieces;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int j = (int)(it / npieces);
    const long p0 = (it % npieces) * PIECE;
    const long p1 = p0 + PIECE < reclen ? p0 + PIECE : reclen;
    const int b = __builtin_amdgcn_readfirstlane(slots[j]);
    if (b < 0 || b >= streams) continue;                               // record i left as it was
    move_piece<false>(const_cast<float*>(block), tb, L.nslices, b, records + (long)j * reclen, p0, p1);
  }
}

// the output rows of a hop that a held stream leaves behind (any pointer may be null: that output is not touched)
struct HoldOutputs {
  float* wav;          // [streams][wav_len]
  long wav_len;
  int64_t* indices;    // [n_max][streams][frames]
  int n_max, frames;
  uint8_t* packets;    // [streams][stride]
  long stride;
  int* nbytes;         // [streams]
};

// stream b's output rows: wav 0, indices -1, packet bytes 0, nbytes 0; every thread of the workgroup takes part
__device__ void clear_outputs(const HoldOutputs& o, int streams, long b) {
  const int t = threadIdx.x;
  if (o.wav != nullptr)
    for (long i = t; i < o.wav_len; i += THREADS) o.wav[b * o.wav_len + i] = 0.f;
  if (o.indices != nullptr)
    for (long i = t; i < (long)o.n_max * o.frames; i += THREADS)
      o.indices[slot::index_at(i / o.frames, streams, b, o.frames, i % o.frames)] = -1;
  if (o.packets != nullptr)
    for (long i = t; i < o.stride; i += THREADS) o.packets[b * o.stride + i] = 0;
  if (o.nbytes != nullptr && t == 0) o.nbytes[b] = 0;
}

__global__ __launch_bounds__(THREADS) void state_hold_kernel(const float* src, float* dst, Layout L, int streams, const int* hold,
                                                             HoldOutputs o) {
  __shared__ int list_b[PASS], list_h[PASS];
  __shared__ int cnt[4][THREADS / 64];
  __shared__ Table tb;
  const int t = threadIdx.x;
  long reclen = -1, per = 0;
  for (int base = 0; base < streams; base += PASS) {
    int h[4];
    bool ok[4], any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = base + i * THREADS + t;
      h[i] = b < streams ? hold[b] : 0;
      ok[i] = h[i] != 0;
      any |= ok[i];
    }
    if (!__syncthreads_or(any)) continue;                              // the idle hop ends here
    const int run = compact(ok, h, base, list_b, list_h, cnt);
    if (reclen < 0) {
      load_table(tb, L);
      reclen = tb.pre[L.nslices];
      per = (reclen + PIECE - 1) / PIECE + 1;                           // the record's pieces, then the output rows
    }
    const long items = (long)run * per;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
      const int j = (int)(it / per);
      const long piece = it % per;
      const int b = __builtin_amdgcn_readfirstlane(list_b[j]);
      if (piece == per - 1) {
        clear_outputs(o, streams, b);
        continue;
      }
      const long p0 = piece * PIECE;
      const long p1 = p0 + PIECE < reclen ? p0 + PIECE : reclen;
      for_piece(tb, L.nslices, b, p0, p1, [&](long at, long, int n) { move(dst + at, src + at, n); });
    }
    __syncthreads();                                                   // the next pass rewrites the list
  }
}

}  // namespace

extern "C" int hilc_state_slots_apply(float* block, const int64_t* slice_off, const int* slice_len, int nslices,
                                      int streams, const int* action, const float* records, int nrecords, void* stream) {
  if (!block || !slice_off || !slice_len || !action || (!records && nrecords > 0)) return HILC_ERR_NULL;
  if (nslices <= 0 || streams <= 0 || nrecords < 0) return HILC_ERR_SHAPE;
  if (nslices > MAX_SLICES) return HILC_ERR_UNSUPPORTED;
  const Layout L = {slice_off, slice_len, nslices};
  return slot::launch(state_apply_kernel, dim3(APPLY_WGS), stream, block, L, streams, action, records, nrecords);
}

extern "C" int hilc_state_slots_gather(const float* block, const int64_t* slice_off, const int* slice_len, int nslices,
                                       int streams, const int* slots, int nslots, float* records, void* stream) {
  if (!block || !slice_off || !slice_len || !slots || !records) return HILC_ERR_NULL;
  if (nslices <= 0 || streams <= 0 || nslots <= 0) return HILC_ERR_SHAPE;
  if (nslices > MAX_SLICES) return HILC_ERR_UNSUPPORTED;
  const Layout L = {slice_off, slice_len, nslices};
  return slot::launch(state_gather_kernel, dim3(GATHER_WGS), stream, block, L, streams, slots, nslots, records);
}

extern "C" int hilc_state_slots_hold(const float* src, float* dst, const int64_t* slice_off, const int* slice_len, int nslices,
                                     int streams, const int* hold, float* wav, int wav_len, int64_t* indices, int n_max, int frames,
                                     uint8_t* packets, int stride, int* nbytes, void* stream) {
  if (!src || !dst || !slice_off || !slice_len || !hold) return HILC_ERR_NULL;
  if (nslices <= 0 || streams <= 0) return HILC_ERR_SHAPE;
  if ((wav && wav_len <= 0) || (indices && (n_max <= 0 || frames <= 0)) || (packets && stride <= 0)) return HILC_ERR_SHAPE;
  if (nslices > MAX_SLICES) return HILC_ERR_UNSUPPORTED;
  const Layout L = {slice_off, slice_len, nslices};
  const HoldOutputs o = {wav, wav_len, indices, n_max, frames, packets, stride, nbytes};
  return slot::launch(state_hold_kernel, dim3(HOLD_WGS), stream, src, dst, L, streams, hold, o);
}
