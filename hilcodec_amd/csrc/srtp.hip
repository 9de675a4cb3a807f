// SRTP packet protection of the graphed hops (graph_step.GraphedEncodeHop(srtp=SrtpConfig()), GraphedDecodeHop(srtp=SrtpConfig())): the
// default transform of RFC 3711, AES_CM_128_HMAC_SHA1_80.  One launch per side, and one for the forwarder's routes; integer work only:
//
//   hilc_srtp_protect    the sender's launch behind hilc_packet_header and in front of hilc_rtx_step / hilc_rate_charge: encrypts bytes
//                        [3, nbytes) of each slot's headed packet in AES-128 counter mode and appends the 10-byte HMAC-SHA1 tag.
//   hilc_srtp_unprotect  the receiver's first launch: takes the hop's protected arrival records slot by slot in push order (index
//                        estimate, replay window, tag, decryption) and writes plain records for the jitter step.
//   hilc_srtp_protect_routes  the forwarder's last launch (GraphedForwardHop(srtp=); rules: hilcodec_amd/forward_srtp.py): protects
//                        every row a listener is sent under that listener's key and the route's own SSRC and index state.  One
//                        thread per ROW, not per route: see the kernel.
//
// The rules, bit for bit: hilcodec_amd/srtp.py (SenderModel, ReceiverModel); the rows: include/hilcodec_amd.h (HILC_SRTP_*).  One THREAD
// per slot: the rollover counter and the replay window make a slot's packets a sequence, and a packet is five SHA-1 compressions and at
// most six AES blocks at the hops' sizes.  Workgroups of 64 with the one AES table Te0 in LDS; the other three tables are its rotations
// and the last round's S-box is its byte 1.  Round keys and HMAC midstates come from the key row: no kernel expands a key or hashes a
// pad.  A packet is handled as big-endian words: word t is its bytes [4 t, 4 t + 4), read with one load where the row is word-aligned
// and byte by byte where it is not (a view, or a row width that is no multiple of 4).
#include "slot.h"

namespace {

using namespace slot;

constexpr int WG = 64;
constexpr int TAG = HILC_WIRE_SRTP_TAG_BYTES;
constexpr int HEAD = HILC_WIRE_TRANSPORT_HEADER;

// ---- Te0[x] = (2 S[x], S[x], S[x], 3 S[x]), built at compile time from the definition of the S-box (FIPS 197 §5.1.1)
struct Te0Table {
  uint32_t v[256];
};

constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 8; ++i) {
    if (b & 1) r ^= a;
    a = (a << 1) ^ ((a & 0x80) ? 0x11Bu : 0u);
    b >>= 1;
  }
  return r & 0xFF;
}

constexpr Te0Table make_te0() {
  Te0Table t = {};
  for (uint32_t x = 0; x < 256; ++x) {
    uint32_t inv = 1, sq = x;                // x^254 = x^2 x^4 ... x^128: the inverse, 0 for 0
    for (int i = 1; i < 8; ++i) {
      sq = gf_mul(sq, sq);
      inv = gf_mul(inv, sq);
    }
    uint32_t s = inv;
    for (int k = 1; k < 5; ++k) s ^= ((inv << k) | (inv >> (8 - k))) & 0xFF;
    s ^= 0x63;
    const uint32_t s2 = gf_mul(s, 2);
    t.v[x] = (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
  }
  return t;
}

__device__ constexpr Te0Table TE0 = make_te0();

__device__ __forceinline__ uint32_t ror(uint32_t v, int r) { return __builtin_rotateright32(v, r); }
__device__ __forceinline__ uint32_t rol(uint32_t v, int r) { return __builtin_rotateleft32(v, r); }

// ---- AES-128, one block (big-endian words)
__device__ __forceinline__ void aes_block(const uint32_t* te, const uint32_t (&rk)[44], uint32_t s0, uint32_t s1, uint32_t s2,
                                          uint32_t s3, uint32_t (&out)[4]) {
  s0 ^= rk[0];
  s1 ^= rk[1];
  s2 ^= rk[2];
  s3 ^= rk[3];
#pragma unroll
  for (int r = 1; r < 10; ++r) {
    const uint32_t t0 = te[s0 >> 24] ^ ror(te[(s1 >> 16) & 255], 8) ^ ror(te[(s2 >> 8) & 255], 16) ^ ror(te[s3 & 255], 24) ^ rk[4 * r];
    const uint32_t t1 = te[s1 >> 24] ^ ror(te[(s2 >> 16) & 255], 8) ^ ror(te[(s3 >> 8) & 255], 16) ^ ror(te[s0 & 255], 24) ^ rk[4 * r + 1];
    const uint32_t t2 = te[s2 >> 24] ^ ror(te[(s3 >> 16) & 255], 8) ^ ror(te[(s0 >> 8) & 255], 16) ^ ror(te[s1 & 255], 24) ^ rk[4 * r + 2];
    const uint32_t t3 = te[s3 >> 24] ^ ror(te[(s0 >> 16) & 255], 8) ^ ror(te[(s1 >> 8) & 255], 16) ^ ror(te[s2 & 255], 24) ^ rk[4 * r + 3];
    s0 = t0;
    s1 = t1;
    s2 = t2;
    s3 = t3;
  }
#define HILC_SRTP_SB(v) ((te[(v) & 255] >> 8) & 255u)
  out[0] = ((HILC_SRTP_SB(s0 >> 24) << 24) | (HILC_SRTP_SB(s1 >> 16) << 16) | (HILC_SRTP_SB(s2 >> 8) << 8) | HILC_SRTP_SB(s3)) ^ rk[40];
  out[1] = ((HILC_SRTP_SB(s1 >> 24) << 24) | (HILC_SRTP_SB(s2 >> 16) << 16) | (HILC_SRTP_SB(s3 >> 8) << 8) | HILC_SRTP_SB(s0)) ^ rk[41];
  out[2] = ((HILC_SRTP_SB(s2 >> 24) << 24) | (HILC_SRTP_SB(s3 >> 16) << 16) | (HILC_SRTP_SB(s0 >> 8) << 8) | HILC_SRTP_SB(s1)) ^ rk[42];
  out[3] = ((HILC_SRTP_SB(s3 >> 24) << 24) | (HILC_SRTP_SB(s0 >> 16) << 16) | (HILC_SRTP_SB(s1 >> 8) << 8) | HILC_SRTP_SB(s2)) ^ rk[43];
#undef HILC_SRTP_SB
}

// ---- SHA-1, one block (FIPS 180): the schedule rolls through the 16 words
__device__ __forceinline__ void sha1_compress(uint32_t (&h)[5], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    if (t >= 16) w[t & 15] = rol(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
    uint32_t f, k;
    if (t < 20) {
      f = (b & c) | (~b & d);
      k = 0x5A827999u;
    } else if (t < 40) {
      f = b ^ c ^ d;
      k = 0x6ED9EBA1u;
    } else if (t < 60) {
      f = (b & c) | (b & d) | (c & d);
      k = 0x8F1BBCDCu;
    } else {
      f = b ^ c ^ d;
      k = 0xCA62C1D6u;
    }
    const uint32_t tmp = rol(a, 5) + f + e + k + w[t & 15];
    e = d;
    d = c;
    c = rol(b, 30);
    b = a;
    a = tmp;
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
}

// ---- a byte row as big-endian words.  cap: the bytes that may be touched; aligned: base and cap are multiples of 4
struct Row {
  uint8_t* p;
  int cap;
  bool aligned;
  __device__ __forceinline__ uint32_t be(int t) const {
    const int o = 4 * t;
    if (o >= cap) return 0u;
    if (aligned) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p + o));
    uint32_t v = (uint32_t)p[o] << 24;
    if (o + 1 < cap) v |= (uint32_t)p[o + 1] << 16;
    if (o + 2 < cap) v |= (uint32_t)p[o + 2] << 8;
    if (o + 3 < cap) v |= (uint32_t)p[o + 3];
    return v;
  }
  __device__ __forceinline__ void put(int t, uint32_t v) const {
    const int o = 4 * t;
    if (o >= cap) return;
    if (aligned) {
      *reinterpret_cast<uint32_t*>(p + o) = __builtin_bswap32(v);
      return;
    }
    p[o] = (uint8_t)(v >> 24);
    if (o + 1 < cap) p[o + 1] = (uint8_t)(v >> 16);
    if (o + 2 < cap) p[o + 2] = (uint8_t)(v >> 8);
    if (o + 3 < cap) p[o + 3] = (uint8_t)v;
  }
  // the 4 bytes at byte offset `off` (any alignment), zero past cap
  __device__ __forceinline__ uint32_t be_at(int off) const {
    const int t = off >> 2, s = 8 * (off & 3);
    const uint32_t a = be(t);
    return s == 0 ? a : (a << s) | (be(t + 1) >> (32 - s));
  }
  __device__ __forceinline__ int words() const { return (cap + 3) >> 2; }
  __device__ __forceinline__ void zero(int t0) const {
    for (int t = t0; t < words(); ++t) put(t, 0u);
  }
};

// the bytes of word t that lie below byte nb
__device__ __forceinline__ uint32_t keep(int nb, int t) {
  const int v = nb - 4 * t;
  return v <= 0 ? 0u : (v >= 4 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (8 * (4 - v)));
}

// what a big-endian word at byte offset `off` relative to a word's first byte contributes to that word
__device__ __forceinline__ uint32_t place(uint32_t v, int off) {
  if (off <= -4 || off >= 4) return 0u;
  return off >= 0 ? v >> (8 * off) : v << (-8 * off);
}

struct Key {
  uint32_t rk[44];
  uint32_t iv[4];                      // salt 2^16 XOR SSRC 2^64; the index goes in per packet
};

__device__ __forceinline__ void load_key(const int* key, Key& k) {
#pragma unroll
  for (int i = 0; i < 44; ++i) k.rk[i] = (uint32_t)key[HILC_SRTP_KEY_RK + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) k.iv[i] = (uint32_t)key[HILC_SRTP_KEY_SALT + i];
  k.iv[1] ^= (uint32_t)key[HILC_SRTP_KEY_SSRC];
}

// RFC 3711 §4.1.1: words [0, ceil(nb / 4)) of `out` = the nb bytes of `in` with bytes [3, nb) XORed with the keystream of index
// roc 2^16 + seq (the last word zero past nb).  Packet byte 3 + k takes keystream byte k, so packet word t takes the last 3 bytes of
// keystream word t - 1 and the first of keystream word t.
__device__ __forceinline__ void crypt(const uint32_t* te, const Key& k, uint32_t roc, uint32_t seq, const Row& in, int nb, const Row& out) {
  const int nw = (nb + 3) >> 2;
  const uint32_t iv2 = k.iv[2] ^ roc, iv3 = k.iv[3] ^ (seq << 16);
  uint32_t prev = 0u;
  for (int q = 0; 4 * q < nw; ++q) {
    uint32_t ks[4];
    aes_block(te, k.rk, k.iv[0], k.iv[1], iv2, iv3 | (uint32_t)q, ks);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = 4 * q + j;
      const uint32_t x = (prev << 8) | (ks[j] >> 24);
      prev = ks[j];
      if (t < nw) out.put(t, (in.be(t) ^ x) & keep(nb, t));
    }
  }
}

// RFC 3711 §4.2: the first 10 bytes of HMAC-SHA1 over the nb bytes of `in` and roc as 4 bytes, from the key row's midstates:
// tag[0], tag[1] and the upper half of tag[2]
__device__ __forceinline__ void hmac_tag(const int* key, const Row& in, int nb, uint32_t roc, uint32_t (&tag)[3]) {
  uint32_t h[5], digest[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    h[i] = (uint32_t)key[HILC_SRTP_KEY_INNER + i];
    digest[i] = 0u;
  }
  const int nblk = (nb + 4 + 9 + 63) >> 6;             // the message, 0x80 and the 8-byte length
  for (int c = 0; c <= nblk; ++c) {
    uint32_t w[16];
    if (c < nblk) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = 16 * c + i;
        uint32_t v = 4 * t < nb ? in.be(t) & keep(nb, t) : 0u;
        v |= place(roc, nb - 4 * t) | place(0x80000000u, nb + 4 - 4 * t);
        w[i] = v;
      }
      if (c == nblk - 1) w[15] = (uint32_t)(64 + nb + 4) * 8u;
    } else {
#pragma unroll
      for (int i = 0; i < 5; ++i) w[i] = digest[i];
      w[5] = 0x80000000u;
#pragma unroll
      for (int i = 6; i < 15; ++i) w[i] = 0u;
      w[15] = (64 + 20) * 8;
    }
    sha1_compress(h, w);
    if (c == nblk - 1) {
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        digest[i] = h[i];
        h[i] = (uint32_t)key[HILC_SRTP_KEY_OUTER + i];
      }
    }
  }
  tag[0] = h[0];
  tag[1] = h[1];
  tag[2] = h[2] & 0xFFFF0000u;
}

__device__ __forceinline__ void load_te0(uint32_t* te) {
#pragma unroll
  for (int i = 0; i < 256 / WG; ++i) te[threadIdx.x + WG * i] = TE0.v[threadIdx.x + WG * i];
  __syncthreads();
}

__global__ __launch_bounds__(WG) void srtp_protect_kernel(const uint8_t* __restrict__ packets, const int* __restrict__ nbytes,
                                                          const int* __restrict__ keys, int* rows, const int* __restrict__ action,
                                                          uint8_t* __restrict__ out, int* __restrict__ out_nbytes, int B, int tb,
                                                          int in_aligned, int out_aligned) {
  __shared__ uint32_t te[256];
  load_te0(te);
  const int b = (int)blockIdx.x * WG + (int)threadIdx.x;
  if (b >= B) return;
  const int* key = keys + (long)b * HILC_SRTP_KEY_WORDS;
  int* row = rows + (long)b * HILC_SRTP_TX_WORDS;
  const bool valid = key[HILC_SRTP_KEY_VALID] != 0;
  int r[HILC_SRTP_TX_WORDS];
  const bool start = is_reset(action, b);
#pragma unroll
  for (int k = 0; k < HILC_SRTP_TX_WORDS; ++k) r[k] = start ? 0 : row[k];
  if (start) r[HILC_SRTP_TX_ROC] = valid ? key[HILC_SRTP_KEY_ROC] : 0;
  const Row in = {const_cast<uint8_t*>(packets) + (long)b * tb, tb, in_aligned != 0};
  const Row o = {out + (long)b * (tb + TAG), tb + TAG, out_aligned != 0};
  const int nb = min(nbytes[b], tb);
  int sent = 0;
  if (nb < HEAD) {
    o.zero(0);
  } else if (!valid) {
    ++r[HILC_SRTP_TX_NOKEY];
    o.zero(0);
  } else {
    const uint32_t seq = in.be(0) >> 16;
    if (r[HILC_SRTP_TX_SENT] != 0 && seq < ((uint32_t)r[HILC_SRTP_TX_LAST] & 0xFFFFu))
      r[HILC_SRTP_TX_ROC] = (int)((uint32_t)r[HILC_SRTP_TX_ROC] + 1u);
    r[HILC_SRTP_TX_LAST] = (int)seq;
    r[HILC_SRTP_TX_SENT] = 1;
    const uint32_t roc = (uint32_t)r[HILC_SRTP_TX_ROC];
    Key k;
    load_key(key, k);
    crypt(te, k, roc, seq, in, nb, o);
    uint32_t tag[3];
    hmac_tag(key, o, nb, roc, tag);        // reads back the ciphertext this thread wrote
    for (int t = nb >> 2; t < o.words(); ++t) {
      const uint32_t ct = 4 * t < nb ? o.be(t) & keep(nb, t) : 0u;
      o.put(t, ct | place(tag[0], nb - 4 * t) | place(tag[1], nb + 4 - 4 * t) | place(tag[2], nb + 8 - 4 * t));
    }
    sent = nb + TAG;
    ++r[HILC_SRTP_TX_PROTECTED];
  }
  out_nbytes[b] = sent;
#pragma unroll
  for (int k = 0; k < HILC_SRTP_TX_WORDS; ++k) row[k] = r[k];
}

__global__ __launch_bounds__(WG) void srtp_unprotect_kernel(const int* __restrict__ arr, const int* __restrict__ off, int max_a,
                                                            const int* __restrict__ keys, int* rows, const int* __restrict__ action,
                                                            int* __restrict__ plain, int B, int tb) {
  __shared__ uint32_t te[256];
  load_te0(te);
  const int b = (int)blockIdx.x * WG + (int)threadIdx.x;
  if (b >= B) return;
  const int* key = keys + (long)b * HILC_SRTP_KEY_WORDS;
  int* row = rows + (long)b * HILC_SRTP_RX_WORDS;
  const bool valid = key[HILC_SRTP_KEY_VALID] != 0;
  int r[HILC_SRTP_RX_WORDS];
  const bool start = is_reset(action, b);
#pragma unroll
  for (int k = 0; k < HILC_SRTP_RX_WORDS; ++k) r[k] = start ? 0 : row[k];
  if (start) r[HILC_SRTP_RX_ROC] = valid ? key[HILC_SRTP_KEY_ROC] : 0;
  const int pw = (tb + TAG + 3) >> 2, aw = (tb + 3) >> 2;
  const int a0 = clampi(off[b], 0, max_a);
  const int a1 = clampi(off[b + 1], a0, max_a);
  Key k;
  if (valid && a1 > a0) load_key(key, k);
  for (int a = a0; a < a1; ++a) {
    int* rec_in = const_cast<int*>(arr) + (long)a * (1 + pw);
    int* rec_out = plain + (long)a * (1 + aw);
    const Row in = {reinterpret_cast<uint8_t*>(rec_in + 1), 4 * pw, true};
    const Row o = {reinterpret_cast<uint8_t*>(rec_out + 1), 4 * aw, true};
    const int nbytes = rec_in[0];
    bool ok = false;
    uint32_t v = 0u, seq = 0u;
    long long delta = 1;
    uint64_t window = (uint32_t)r[HILC_SRTP_RX_WIN_LO] | ((uint64_t)(uint32_t)r[HILC_SRTP_RX_WIN_HI] << 32);
    const int nb = nbytes - TAG;
    if (!valid) {
      ++r[HILC_SRTP_RX_NOKEY];
    } else if (nbytes < HEAD + TAG || nbytes > tb + TAG) {
      ++r[HILC_SRTP_RX_SHORT];
    } else {
      seq = in.be(0) >> 16;
      const uint32_t roc = (uint32_t)r[HILC_SRTP_RX_ROC], s_l = (uint32_t)r[HILC_SRTP_RX_SL] & 0xFFFFu;
      const bool seen = r[HILC_SRTP_RX_SEEN] != 0;
      bool before = false;                  // v = -1
      v = roc;
      if (seen) {
        if (s_l < 32768u) {
          if ((int)seq - (int)s_l > 32768) {
            before = roc == 0u;
            v = roc - 1u;
          }
        } else if ((int)s_l - 32768 > (int)seq) {
          v = roc + 1u;
        }
        delta = (long long)(((uint64_t)v << 16) | seq) - (long long)(((uint64_t)roc << 16) | s_l);
      }
      if (before || (delta <= 0 && (-delta >= 64 || ((window >> (int)(-delta)) & 1ull)))) {
        ++r[HILC_SRTP_RX_REPLAY];
      } else {
        uint32_t tag[3];
        hmac_tag(key, in, nb, v, tag);
        const uint32_t diff = (tag[0] ^ in.be_at(nb)) | (tag[1] ^ in.be_at(nb + 4)) | ((tag[2] ^ in.be_at(nb + 8)) & 0xFFFF0000u);
        if (diff != 0u)
          ++r[HILC_SRTP_RX_AUTH_FAIL];
        else
          ok = true;
      }
    }
    if (!ok) {
      rec_out[0] = 0;
      o.zero(0);
      continue;
    }
    crypt(te, k, v, seq, in, nb, o);
    o.zero((nb + 3) >> 2);
    rec_out[0] = nb;
    if (delta > 0) {
      window = (r[HILC_SRTP_RX_SEEN] == 0 || delta >= 64) ? 1ull : ((window << (int)delta) | 1ull);
      r[HILC_SRTP_RX_SL] = (int)seq;
      r[HILC_SRTP_RX_ROC] = (int)v;
      r[HILC_SRTP_RX_SEEN] = 1;
    } else {
      window |= 1ull << (int)(-delta);
    }
    r[HILC_SRTP_RX_WIN_LO] = (int)(uint32_t)window;
    r[HILC_SRTP_RX_WIN_HI] = (int)(uint32_t)(window >> 32);
    ++r[HILC_SRTP_RX_OK];
  }
#pragma unroll
  for (int k2 = 0; k2 < HILC_SRTP_RX_WORDS; ++k2) row[k2] = r[k2];
}

// ---- the forwarder's egress (graph_step.GraphedForwardHop(srtp=); the rules, bit for bit: hilcodec_amd/forward_srtp.py, RouteModel)
// A route's index state: the receiver rule's steps 2, 3 and 5 (srtp.py) on the route row's (RT_ROC, RT_SL, RT_SEEN, window), so the
// egress refuses exactly what the client's replay window would, and no index leaves twice.
struct RouteIndex {
  uint32_t roc, sl;
  bool seen;
  uint64_t window;
  // SEQ -> accepted (v: the rollover counter it is sent under; the state moves) or refused (the state stays)
  __device__ __forceinline__ bool admit(uint32_t seq, uint32_t& v) {
    bool before = false;                    // v = -1
    long long delta = 1;
    v = roc;
    if (seen) {
      if (sl < 32768u) {
        if ((int)seq - (int)sl > 32768) {
          before = roc == 0u;
          v = roc - 1u;
        }
      } else if ((int)sl - 32768 > (int)seq) {
        v = roc + 1u;
      }
      delta = (long long)(((uint64_t)v << 16) | seq) - (long long)(((uint64_t)roc << 16) | sl);
    }
    if (before || (delta <= 0 && (-delta >= HILC_SRTP_WINDOW || ((window >> (int)(-delta)) & 1ull)))) return false;
    if (delta > 0) {
      window = (!seen || delta >= HILC_SRTP_WINDOW) ? 1ull : ((window << (int)delta) | 1ull);
      sl = seq;
      roc = v;
      seen = true;
    } else {
      window |= 1ull << (int)(-delta);
    }
    return true;
  }
};

// One THREAD per output row (b, j, k).  The P rows of a route sit side by side in one workgroup (64 / P whole routes, the other lanes
// idle); a route's sequential part is a few integer steps per row, so thread k replays the rule for the rows in front of its own and
// then runs its own packet's AES / SHA-1 chain: the launch costs one packet's chain whatever the burst.  Every thread reads the
// route row, a barrier follows, and the thread of the route's last row, which has replayed all of them, writes the row back.
__global__ __launch_bounds__(WG) void srtp_protect_routes_kernel(const uint8_t* __restrict__ in_rows, const int* __restrict__ nbytes,
                                                                 const int* __restrict__ routes, const int* __restrict__ new_routes,
                                                                 const int* __restrict__ action, const int* __restrict__ rekey_up,
                                                                 const int* __restrict__ rekey_down, const int* __restrict__ keys,
                                                                 int* rt_rows, uint8_t* __restrict__ out, int* __restrict__ out_nbytes,
                                                                 int B, int F, int P, int tb, int in_aligned, int out_aligned) {
  __shared__ uint32_t te[256];
  load_te0(te);
  const int per_wg = WG / P;                             // whole routes of a workgroup
  const int lane_route = (int)threadIdx.x / P, k = (int)threadIdx.x - lane_route * P;
  const long route = (long)blockIdx.x * per_wg + lane_route;
  const bool mine = lane_route < per_wg && route < (long)B * F;
  int r[HILC_FSRTP_RT_WORDS];
  int* rt = rt_rows + (mine ? route : 0) * HILC_FSRTP_RT_WORDS;
#pragma unroll
  for (int i = 0; i < HILC_FSRTP_RT_WORDS; ++i) r[i] = mine ? rt[i] : 0;
  __syncthreads();                                       // every reader of a route row is in front of its one writer
  if (!mine) return;
  const int b = (int)(route / F), j = (int)(route - (long)b * F);
  const int* key = keys + (long)b * HILC_SRTP_KEY_WORDS;
  const bool valid = key[HILC_SRTP_KEY_VALID] != 0;
  const int t = routes[route];
  bool restart = new_routes[route] != 0 || is_reset(action, b) || is_reset(rekey_down, b);
  if (t >= 0 && t < B) restart = restart || is_reset(action, t) || is_reset(rekey_up, t);
  if (restart) {
    if (r[HILC_FSRTP_RT_EPOCH] < HILC_FSRTP_MAX_EPOCH) {
      ++r[HILC_FSRTP_RT_EPOCH];
      r[HILC_FSRTP_RT_SEEN] = 0;
    } else {
      r[HILC_FSRTP_RT_SEEN] = HILC_FSRTP_SEEN_EXHAUSTED;  // no SSRC is left for another stream
    }
    r[HILC_FSRTP_RT_ROC] = r[HILC_FSRTP_RT_SL] = r[HILC_FSRTP_RT_WIN_LO] = r[HILC_FSRTP_RT_WIN_HI] = 0;
  }
  const bool exhausted = r[HILC_FSRTP_RT_SEEN] == HILC_FSRTP_SEEN_EXHAUSTED;
  RouteIndex ix = {(uint32_t)r[HILC_FSRTP_RT_ROC], (uint32_t)r[HILC_FSRTP_RT_SL] & 0xFFFFu, r[HILC_FSRTP_RT_SEEN] == 1,
                   (uint32_t)r[HILC_FSRTP_RT_WIN_LO] | ((uint64_t)(uint32_t)r[HILC_FSRTP_RT_WIN_HI] << 32)};
  const long row0 = route * P;
  bool send = false;
  uint32_t v = 0u, seq = 0u;
  int nb = 0;
  for (int q = 0; q <= k; ++q) {                         // the rows in front of this thread's, then its own
    const Row rq = {const_cast<uint8_t*>(in_rows) + (row0 + q) * tb, tb, in_aligned != 0};
    nb = min(nbytes[row0 + q], tb);
    send = false;
    if (nb < HEAD) continue;
    if (!valid) {
      ++r[HILC_FSRTP_RT_NOKEY];
    } else if (exhausted) {
      ++r[HILC_FSRTP_RT_EXHAUSTED];
    } else {
      seq = rq.be(0) >> 16;
      send = ix.admit(seq, v);
      if (send)
        ++r[HILC_FSRTP_RT_PROTECTED];
      else
        ++r[HILC_FSRTP_RT_STALE];
    }
  }
  if (k == P - 1) {
    if (!exhausted) {
      r[HILC_FSRTP_RT_ROC] = (int)ix.roc;
      r[HILC_FSRTP_RT_SL] = (int)ix.sl;
      r[HILC_FSRTP_RT_SEEN] = ix.seen ? 1 : 0;
      r[HILC_FSRTP_RT_WIN_LO] = (int)(uint32_t)ix.window;
      r[HILC_FSRTP_RT_WIN_HI] = (int)(uint32_t)(ix.window >> 32);
    }
#pragma unroll
    for (int i = 0; i < HILC_FSRTP_RT_WORDS; ++i) rt[i] = r[i];
  }
  const Row in = {const_cast<uint8_t*>(in_rows) + (row0 + k) * tb, tb, in_aligned != 0};
  const Row o = {out + (row0 + k) * (tb + TAG), tb + TAG, out_aligned != 0};
  if (!send) {
    o.zero(0);
    out_nbytes[row0 + k] = 0;
    return;
  }
  Key ky;
#pragma unroll
  for (int i = 0; i < 44; ++i) ky.rk[i] = (uint32_t)key[HILC_SRTP_KEY_RK + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) ky.iv[i] = (uint32_t)key[HILC_SRTP_KEY_SALT + i];
  // the route's own SSRC: base + MAX_FANOUT epoch + route (mod 2^32)
  ky.iv[1] ^= (uint32_t)key[HILC_SRTP_KEY_SSRC] + (uint32_t)HILC_FORWARD_MAX_FANOUT * (uint32_t)r[HILC_FSRTP_RT_EPOCH] + (uint32_t)j;
  crypt(te, ky, v, seq, in, nb, o);
  uint32_t tag[3];
  hmac_tag(key, o, nb, v, tag);            // reads back the ciphertext this thread wrote
  for (int w = nb >> 2; w < o.words(); ++w) {
    const uint32_t ct = 4 * w < nb ? o.be(w) & keep(nb, w) : 0u;
    o.put(w, ct | place(tag[0], nb - 4 * w) | place(tag[1], nb + 4 - 4 * w) | place(tag[2], nb + 8 - 4 * w));
  }
  out_nbytes[row0 + k] = nb + TAG;
}

static inline dim3 slots_grid(int B) { return dim3((unsigned)((B + WG - 1) / WG)); }

static inline bool word_aligned(const void* p, long stride) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)stride) & 3) == 0; }

}  // namespace

extern "C" int hilc_srtp_protect(const uint8_t* packets, const int* nbytes, const int* keys, int* rows, const int* action, uint8_t* out,
                                 int* out_nbytes, int B, int row_bytes, void* stream) {
  if (!packets || !nbytes || !keys || !rows || !out || !out_nbytes) return HILC_ERR_NULL;
  if (B <= 0 || row_bytes <= HEAD || row_bytes > HILC_SRTP_MAX_ROW_BYTES) return HILC_ERR_SHAPE;
  // a byte row is read as words only where its base and its stride are multiples of 4: a view 1..3 bytes off, or an odd width, takes
  // the byte path of the same kernel
  const int in_aligned = word_aligned(packets, row_bytes), out_aligned = word_aligned(out, row_bytes + TAG);
  HILC_CLEAR_ERROR();
  hipLaunchKernelGGL(srtp_protect_kernel, slots_grid(B), dim3(WG), 0, (hipStream_t)stream, packets, nbytes, keys, rows, action, out,
                     out_nbytes, B, row_bytes, in_aligned, out_aligned);
  HILC_CHECK_LAUNCH();
  return HILC_OK;
}

extern "C" int hilc_srtp_unprotect(const int* arrivals, const int* offsets, int max_arrivals, const int* keys, int* rows,
                                   const int* action, int* plain, int B, int row_bytes, void* stream) {
  if (!arrivals || !offsets || !keys || !rows || !plain) return HILC_ERR_NULL;
  if (B <= 0 || max_arrivals < 0 || row_bytes <= HEAD || row_bytes > HILC_SRTP_MAX_ROW_BYTES) return HILC_ERR_SHAPE;
  HILC_CLEAR_ERROR();
  hipLaunchKernelGGL(srtp_unprotect_kernel, slots_grid(B), dim3(WG), 0, (hipStream_t)stream, arrivals, offsets, max_arrivals, keys, rows,
                     action, plain, B, row_bytes);
  HILC_CHECK_LAUNCH();
  return HILC_OK;
}

extern "C" int hilc_srtp_protect_routes(const uint8_t* rows, const int* nbytes, const int* routes, const int* new_routes,
                                        const int* action, const int* rekey_up, const int* rekey_down, const int* keys, int* route_rows,
                                        uint8_t* out, int* out_nbytes, int B, int fanout, int burst, int row_bytes, void* stream) {
  if (!rows || !nbytes || !routes || !new_routes || !keys || !route_rows || !out || !out_nbytes) return HILC_ERR_NULL;
  if (B <= 0 || fanout < 1 || fanout > HILC_FORWARD_MAX_FANOUT || burst < 1 || burst > HILC_FORWARD_MAX_BURST || row_bytes <= HEAD ||
      row_bytes > HILC_SRTP_MAX_ROW_BYTES)
    return HILC_ERR_SHAPE;
  const int in_aligned = word_aligned(rows, row_bytes), out_aligned = word_aligned(out, row_bytes + TAG);
  const long n_routes = (long)B * fanout;
  const int per_wg = WG / burst;
  HILC_CLEAR_ERROR();
  hipLaunchKernelGGL(srtp_protect_routes_kernel, dim3((unsigned)((n_routes + per_wg - 1) / per_wg)), dim3(WG), 0, (hipStream_t)stream,
                     rows, nbytes, routes, new_routes, action, rekey_up, rekey_down, keys, route_rows, out, out_nbytes, B, fanout, burst,
                     row_bytes, in_aligned, out_aligned);
  HILC_CHECK_LAUNCH();
  return HILC_OK;
}
