"""SRTP packet protection of the graphed hops (graph_step.GraphedEncodeHop(srtp=SrtpConfig()), GraphedDecodeHop(srtp=SrtpConfig())):
the definition, bit for bit, of hilc_srtp_protect and hilc_srtp_unprotect (csrc/srtp.hip), and the only module that knows their rules.
Import it by name (`from hilcodec_amd import srtp`).  Pure Python and numpy: AES-128, SHA-1 and HMAC are written out here, the
standard library's `hmac` / `hashlib` serve the tests as a cross-check only.

The transform is SRTP's default, AES_CM_128_HMAC_SHA1_80 of RFC 3711: AES-128 in counter mode over the payload (§4.1.1), HMAC-SHA1
truncated to 80 bits over header || ciphertext || ROC (§4.2), a 48-bit packet index i = ROC 2^16 + SEQ from the transport header's
16-bit hop index SEQ and a per-slot rollover counter ROC (§3.3.1), a 64-packet replay window on the receiver (§3.3.2) and the AES-CM
key derivation with kdr = 0 (§4.3.1).

Packet.  A protected packet is a headed packet of wire.pack_transport: its first 3 bytes (SEQ big-endian, the flags byte with n) stay
clear, bytes [3, nbytes) are XORed with the keystream from keystream byte 0, and TAG_BYTES = 10 tag bytes follow.  The counter block
of AES block j is ((k_s 2^16) XOR (SSRC 2^64) XOR (i 2^16)) + j; the tag is the first 10 bytes of HMAC-SHA1(k_a, header || ciphertext
|| ROC as 4 bytes big-endian).

Key row (int32, KEY_WORDS words, what the kernels read: no kernel expands a key or hashes a pad): KEY_VALID (1: the slot has a key),
KEY_SSRC, KEY_ROC (the ROC a start gives the slot's row; 0 but for a late joiner), the 44 round-key words of k_e from KEY_RK, the salt
k_s as 4 big-endian words from KEY_SALT (14 bytes, then 2 zero bytes), and the HMAC midstates from KEY_INNER and KEY_OUTER, 5 words
each: the SHA-1 states after the blocks k_a XOR ipad and k_a XOR opad.  Every word is the big-endian uint32 held in an int32.

Sender rule (per slot and hop, behind hilc_packet_header; TX row, int32 TX_WORDS words: TX_ROC, TX_LAST (the last SEQ sent), TX_SENT
(0 until the slot has sent), the counters TX_PROTECTED, TX_NOKEY):
1. action != 0 (a start or a resume on this hop) clears the row; TX_ROC becomes the key row's KEY_ROC (0 without a key).
2. nb = min(nbytes, row bytes).  nb < 3 (held, stopped, DTX silent: nothing was sent) leaves the row as it is and moves nothing: the
   output row is zero with nbytes 0.
3. a slot without a valid key sends nothing: the output row is zero, nbytes 0, TX_NOKEY += 1.  Plaintext never leaves a keyed hop.
4. SEQ = the packet's bytes 0-1.  If TX_SENT and SEQ < TX_LAST (both unsigned 16 bit): TX_ROC += 1 (mod 2^32).  A slot never goes
   65 536 hops between two sent packets (DTX sends SIDs), so one comparison tells a wrap.  TX_LAST = SEQ, TX_SENT = 1.
5. the output row is the nb bytes protected under index TX_ROC 2^16 + SEQ, then the tag, zero past nb + 10 bytes; nbytes = nb + 10;
   TX_PROTECTED += 1.

Receiver rule (per slot, its arrivals of the hop in push order, in front of the jitter step; a protected record holds up to row
bytes + 10 bytes; RX row, int32 RX_WORDS words: RX_ROC, RX_SL (s_l, the highest authenticated SEQ), RX_SEEN, RX_WIN_LO, RX_WIN_HI (the
replay window: bit k of the 64 is the packet k below the highest authenticated index), the counters RX_OK, RX_AUTH_FAIL, RX_REPLAY,
RX_SHORT, RX_NOKEY):
0. action != 0 clears the row; RX_ROC becomes the key row's KEY_ROC (0 without a key).  Without a valid key every arrival counts
   RX_NOKEY and is rejected.
1. nbytes < 3 + 10, or more than the record holds (row bytes + 10): RX_SHORT.
2. v is estimated from (RX_SL, RX_ROC, SEQ) as in §3.3.1: with s_l < 32768, v = ROC - 1 if SEQ - s_l > 32768 else ROC; otherwise
   v = ROC + 1 if s_l - 32768 > SEQ else ROC.  The first packet of a slot (RX_SEEN = 0) takes v = RX_ROC.  v = -1: RX_REPLAY.
3. with i = v 2^16 + SEQ and top = RX_ROC 2^16 + RX_SL (when RX_SEEN): i more than 63 below top, or its window bit set: RX_REPLAY.
4. the tag over header || ciphertext || v must equal the packet's last 10 bytes, all 10 compared without an early exit; else
   RX_AUTH_FAIL.  A rejected arrival changes nothing but its counter.
5. otherwise the payload is decrypted under i, nbytes falls by 10, RX_OK += 1; i > top (or the first packet): the window moves up by
   i - top and gets bit 0, RX_SL = SEQ, RX_ROC = v, RX_SEEN = 1; else the window bit top - i is set.
A rejected arrival comes out as a record of 0 bytes, every word zero: the jitter step and hilc_rx_bwe count it malformed and drop it,
so nothing behind this launch knows about SRTP.  An accepted one comes out as the plain record (byte count, then the packet, zero
past it).

Not covered: key exchange (DTLS-SRTP belongs to the host), SRTCP (reports, NACKs and caps travel unprotected) and the timing of
table lookups on a GPU that others share.  graph_step.GraphedForwardHop(srtp=) trims packets, so it unprotects on ingress with this
module's receiver rule and protects per listener route under rules of its own: forward_srtp.py."""
from __future__ import annotations

import hashlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import wire

TAG_BYTES = wire.SRTP_TAG_BYTES
PROFILE = "AES_CM_128_HMAC_SHA1_80"
KEY_BYTES, SALT_BYTES, AUTH_BYTES = 16, 14, 20
WINDOW = 64

KEY_VALID, KEY_SSRC, KEY_ROC, KEY_RK = 0, 1, 2, 3
KEY_SALT = KEY_RK + 44
KEY_INNER = KEY_SALT + 4
KEY_OUTER = KEY_INNER + 5
KEY_WORDS = KEY_OUTER + 5

TX_ROC, TX_LAST, TX_SENT, TX_PROTECTED, TX_NOKEY = range(5)
TX_WORDS = 5
TX_NAMES = ("protected", "nokey")

RX_ROC, RX_SL, RX_SEEN, RX_WIN_LO, RX_WIN_HI, RX_OK, RX_AUTH_FAIL, RX_REPLAY, RX_SHORT, RX_NOKEY = range(10)
RX_WORDS = 10
RX_NAMES = ("ok", "auth_fail", "replay", "short", "nokey")

MAX_ROW_BYTES = 1 << 15


@dataclass(frozen=True)
class SrtpConfig:
    """packet protection of a graphed hop (the rules: this module's docstring).  The one transform is RFC 3711's default"""
    profile: str = PROFILE

    def __post_init__(self):
        if self.profile != PROFILE:
            raise ValueError(f"SrtpConfig.profile = {self.profile!r}: only {PROFILE!r}")


# ---------------------------------------------------------------- AES-128 (FIPS 197)
def _make_sbox():
    exp, log = [0] * 256, [0] * 256
    x = 1
    for i in range(255):
        exp[i], log[x] = x, i
        x ^= ((x << 1) ^ (0x11B if x & 0x80 else 0)) & 0xFF             # times 3, a generator of GF(2^8)*
    box = []
    for a in range(256):
        inv = 0 if a == 0 else exp[(255 - log[a]) % 255]
        s = inv
        for k in range(1, 5):
            s ^= ((inv << k) | (inv >> (8 - k))) & 0xFF
        box.append(s ^ 0x63)
    return box


SBOX = _make_sbox()


def _xtime(a: int) -> int:
    return ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF


# the one table of the kernels: TE0[x] = (2 S[x], S[x], S[x], 3 S[x]) as a big-endian word; the other three are its rotations and
# S[x] is its byte 1
TE0 = [(_xtime(s) << 24) | (s << 16) | (s << 8) | (_xtime(s) ^ s) for s in SBOX]


def aes_expand(key: bytes) -> list:
    """the 44 round-key words (big-endian uint32) of a 16-byte key"""
    key = bytes(key)
    if len(key) != KEY_BYTES:
        raise ValueError(f"an AES-128 key is {KEY_BYTES} bytes")
    w = [int.from_bytes(key[4 * i:4 * i + 4], "big") for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = w[i - 1]
        if i % 4 == 0:
            t = ((t << 8) | (t >> 24)) & 0xFFFFFFFF
            t = (SBOX[t >> 24] << 24) | (SBOX[(t >> 16) & 255] << 16) | (SBOX[(t >> 8) & 255] << 8) | SBOX[t & 255]
            t ^= rcon << 24
            rcon = _xtime(rcon)
        w.append(w[i - 4] ^ t)
    return w


def _ror(v: int, r: int) -> int:
    return ((v >> r) | (v << (32 - r))) & 0xFFFFFFFF


def aes_encrypt_words(rk, s) -> list:
    """one block: 4 big-endian words in, 4 out; the kernels' form (TE0 and its rotations, the last round from TE0's byte 1)"""
    s = [s[c] ^ rk[c] for c in range(4)]
    for r in range(1, 10):
        s = [TE0[s[c] >> 24] ^ _ror(TE0[(s[(c + 1) & 3] >> 16) & 255], 8) ^ _ror(TE0[(s[(c + 2) & 3] >> 8) & 255], 16)
             ^ _ror(TE0[s[(c + 3) & 3] & 255], 24) ^ rk[4 * r + c] for c in range(4)]
    return [(((TE0[s[c] >> 24] >> 8) & 255) << 24 | ((TE0[(s[(c + 1) & 3] >> 16) & 255] >> 8) & 255) << 16
             | ((TE0[(s[(c + 2) & 3] >> 8) & 255] >> 8) & 255) << 8 | ((TE0[s[(c + 3) & 3] & 255] >> 8) & 255)) ^ rk[40 + c]
            for c in range(4)]


def aes_encrypt(key: bytes, block: bytes) -> bytes:
    block = bytes(block)
    if len(block) != 16:
        raise ValueError("an AES block is 16 bytes")
    out = aes_encrypt_words(aes_expand(key), [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(4)])
    return b"".join(w.to_bytes(4, "big") for w in out)


def _keystream_words(rk, iv, nbytes: int) -> bytes:
    """`nbytes` of AES-CM keystream: blocks AES(iv + j), j = 0, 1, ...; iv: 4 big-endian words whose low 16 bits are zero"""
    out = bytearray()
    j = 0
    while len(out) < nbytes:
        if j > 0xFFFF:
            raise ValueError("AES-CM: more than 2^16 blocks under one index")
        for w in aes_encrypt_words(rk, [iv[0], iv[1], iv[2], iv[3] | j]):
            out += w.to_bytes(4, "big")
        j += 1
    return bytes(out[:nbytes])


def aes_cm_keystream(key: bytes, salt: bytes, ssrc: int, index: int, nbytes: int) -> bytes:
    """§4.1.1: `nbytes` of keystream for packet index `index` (48 bit) of `ssrc` under session key and 14-byte session salt"""
    return _keystream_words(aes_expand(key), _iv(_salt_words(salt), ssrc, index >> 16, index & 0xFFFF), nbytes)


def _salt_words(salt: bytes) -> list:
    salt = bytes(salt)
    if len(salt) != SALT_BYTES:
        raise ValueError(f"a salt is {SALT_BYTES} bytes")
    padded = salt + b"\0\0"
    return [int.from_bytes(padded[4 * i:4 * i + 4], "big") for i in range(4)]


def _iv(salt_words, ssrc: int, roc: int, seq: int) -> list:
    return [salt_words[0], salt_words[1] ^ (ssrc & 0xFFFFFFFF), salt_words[2] ^ (roc & 0xFFFFFFFF), salt_words[3] ^ ((seq & 0xFFFF) << 16)]


# ---------------------------------------------------------------- SHA-1 (FIPS 180), HMAC (RFC 2104)
SHA1_INIT = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)


def _rol(v: int, r: int) -> int:
    return ((v << r) | (v >> (32 - r))) & 0xFFFFFFFF


def sha1_compress(state, block: bytes) -> Tuple[int, ...]:
    """one 64-byte block into a 5-word state"""
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for t in range(16, 80):
        w.append(_rol(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = state
    for t in range(80):
        if t < 20:
            f, k = (b & c) | (~b & d), 0x5A827999
        elif t < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif t < 60:
            f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (_rol(a, 5) + (f & 0xFFFFFFFF) + e + k + w[t]) & 0xFFFFFFFF, a, _rol(b, 30), c, d
    return tuple((x + y) & 0xFFFFFFFF for x, y in zip(state, (a, b, c, d, e)))


def _sha1_finish(state, tail: bytes, total: int) -> bytes:
    """the digest of a message of `total` bytes whose whole blocks but `tail` are in `state`"""
    tail = bytes(tail) + b"\x80"
    tail += b"\0" * ((56 - len(tail)) % 64) + (8 * total).to_bytes(8, "big")
    for i in range(0, len(tail), 64):
        state = sha1_compress(state, tail[i:i + 64])
    return b"".join(x.to_bytes(4, "big") for x in state)


def hmac_midstates(k_a: bytes) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """the SHA-1 states after the blocks k_a XOR ipad and k_a XOR opad (k_a at most 64 bytes)"""
    k_a = bytes(k_a)
    if len(k_a) > 64:
        raise ValueError("hmac_midstates: a key of at most 64 bytes")
    pad = k_a + b"\0" * (64 - len(k_a))
    return (sha1_compress(SHA1_INIT, bytes(x ^ 0x36 for x in pad)), sha1_compress(SHA1_INIT, bytes(x ^ 0x5C for x in pad)))


def hmac_sha1_mid(inner, outer, msg: bytes) -> bytes:
    """HMAC-SHA1 from the two midstates: the packet path's form"""
    msg = bytes(msg)
    whole = len(msg) // 64 * 64
    state = tuple(inner)
    for i in range(0, whole, 64):
        state = sha1_compress(state, msg[i:i + 64])
    digest = _sha1_finish(state, msg[whole:], 64 + len(msg))
    return _sha1_finish(tuple(outer), digest, 64 + 20)


def hmac_sha1(k_a: bytes, msg: bytes) -> bytes:
    inner, outer = hmac_midstates(k_a)
    return hmac_sha1_mid(inner, outer, msg)


# ---------------------------------------------------------------- keys
def _check_key(master_key, master_salt) -> Tuple[bytes, bytes]:
    try:
        mk, ms = bytes(master_key), bytes(master_salt)
    except TypeError:
        raise ValueError("srtp: the master key and salt must be bytes") from None
    if isinstance(master_key, (int, str)) or isinstance(master_salt, (int, str)) or len(mk) != KEY_BYTES or len(ms) != SALT_BYTES:
        raise ValueError(f"srtp: a master key is {KEY_BYTES} bytes and a master salt {SALT_BYTES} bytes")      # never the key itself
    return mk, ms


def derive(master_key, master_salt) -> Tuple[bytes, bytes, bytes]:
    """§4.3.1 with kdr = 0: (k_e 16 bytes, k_a 20 bytes, k_s 14 bytes) from labels 0, 1, 2 and the AES-CM PRF"""
    mk, ms = _check_key(master_key, master_salt)
    rk = aes_expand(mk)
    out = []
    for label, size in ((0, KEY_BYTES), (1, AUTH_BYTES), (2, SALT_BYTES)):
        x = bytearray(ms)
        x[7] ^= label                                         # key_id = label 2^48 (r = 0), XORed into the 112-bit salt
        out.append(_keystream_words(rk, _salt_words(bytes(x)), size))
    return out[0], out[1], out[2]


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _u32(v) -> int:
    return int(v) & 0xFFFFFFFF


def _check_word(name: str, v, top: int = 0xFFFFFFFF) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top:
        raise ValueError(f"srtp: {name} = {v!r} outside [0, {top}]")
    return int(v)


def session_key_row(k_e: bytes, k_a: bytes, k_s: bytes, ssrc: int, roc: int = 0) -> np.ndarray:
    """the key row of a slot from its session keys (KEY_* layout)"""
    k_a = bytes(k_a)
    if len(k_a) != AUTH_BYTES:
        raise ValueError(f"srtp: an authentication key is {AUTH_BYTES} bytes")
    inner, outer = hmac_midstates(k_a)
    words = [1, _check_word("ssrc", ssrc), _check_word("roc", roc)] + aes_expand(k_e) + _salt_words(k_s) + list(inner) + list(outer)
    assert len(words) == KEY_WORDS
    return np.array([_i32(w) for w in words], dtype=np.int32)


def key_row(master_key, master_salt, ssrc: int, roc: int = 0) -> np.ndarray:
    """int32 [KEY_WORDS]: what the kernels read for one slot, derived from the master key and salt"""
    return session_key_row(*derive(master_key, master_salt), ssrc, roc)


class KeyTable:
    """the host's side of a hop's keys: `rows` int32 [B, KEY_WORDS] as the kernels read them, `dirty` since the last upload, and
    the two rules that keep a keystream from being used twice.  The transport header restarts SEQ at 0 on every start, so a start
    needs a set_key since the slot's previous start, and a set_key equal to the slot's previous one, or to any key the slot was
    started under since the last reset, is refused: set_key(A), start, set_key(B), set_key(A), start would otherwise run A's
    keystream from SEQ 0 twice.  It keeps digests of those keys (32 bytes per start), never a key."""

    def __init__(self, batch: int):
        self.B = int(batch)
        self.reset()

    def reset(self) -> None:
        self.rows = np.zeros((self.B, KEY_WORDS), dtype=np.int32)
        self.fresh = [False] * self.B
        self.last = [None] * self.B
        self.used = [set() for _ in range(self.B)]       # per slot: the digests of the keys it was started under
        self.dirty = True

    def _slot(self, slot) -> int:
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < self.B:
            raise ValueError(f"srtp: slot {slot!r} outside [0, {self.B})")
        return int(slot)

    def set_key(self, slot, master_key, master_salt, ssrc: Optional[int] = None, roc: int = 0) -> None:
        slot = self._slot(slot)
        mk, ms = _check_key(master_key, master_salt)
        ssrc = slot if ssrc is None else _check_word("ssrc", ssrc)
        roc = _check_word("roc", roc)
        mark = hashlib.sha256(mk + ms + ssrc.to_bytes(4, "big")).digest()
        if self.last[slot] == mark or mark in self.used[slot]:
            raise ValueError(f"srtp: slot {slot} was given the key it had before: a key is used for one start only")
        self.rows[slot] = key_row(mk, ms, ssrc, roc)
        self.last[slot], self.fresh[slot], self.dirty = mark, True, True

    def clear_key(self, slot) -> None:
        slot = self._slot(slot)
        self.rows[slot] = 0
        self.fresh[slot], self.dirty = False, True

    def started(self, slot) -> None:
        """a start of `slot`: ValueError unless it has a key set since its previous start"""
        slot = self._slot(slot)
        if not self.fresh[slot]:
            raise ValueError(f"srtp: slot {slot} needs a set_key since its previous start (the header restarts SEQ at 0)")
        self.fresh[slot] = False
        self.used[slot].add(self.last[slot])

    def __repr__(self):
        return f"KeyTable(batch={self.B}, keyed={int((self.rows[:, KEY_VALID] != 0).sum())})"


# ---------------------------------------------------------------- one packet
def _key_parts(row):
    rk = [_u32(w) for w in row[KEY_RK:KEY_RK + 44]]
    salt = [_u32(w) for w in row[KEY_SALT:KEY_SALT + 4]]
    inner = tuple(_u32(w) for w in row[KEY_INNER:KEY_INNER + 5])
    outer = tuple(_u32(w) for w in row[KEY_OUTER:KEY_OUTER + 5])
    return rk, salt, inner, outer


def _crypt(row, data: bytes, roc: int) -> bytes:
    """header kept, bytes [3, len) XORed with the keystream of index roc 2^16 + SEQ"""
    rk, salt, _, _ = _key_parts(row)
    seq = (data[0] << 8) | data[1]
    ks = _keystream_words(rk, _iv(salt, _u32(row[KEY_SSRC]), roc, seq), len(data) - wire.TRANSPORT_HEADER)
    return data[:wire.TRANSPORT_HEADER] + bytes(x ^ y for x, y in zip(data[wire.TRANSPORT_HEADER:], ks))


def _tag(row, data: bytes, roc: int) -> bytes:
    _, _, inner, outer = _key_parts(row)
    return hmac_sha1_mid(inner, outer, data + (roc & 0xFFFFFFFF).to_bytes(4, "big"))[:TAG_BYTES]


def protect_packet(row, packet: bytes, roc: int) -> bytes:
    """one headed packet (at least 3 bytes) under key row `row` and rollover counter `roc`"""
    packet = bytes(packet)
    if len(packet) < wire.TRANSPORT_HEADER:
        raise ValueError("protect_packet: a headed packet has at least 3 bytes")
    ct = _crypt(row, packet, roc)
    return ct + _tag(row, ct, roc)


class SenderModel:
    """numpy statement of hilc_srtp_protect for `batch` slots whose headed rows are `row_bytes` = wire.transport_bytes(n, m, T) bytes.
    `keys` (a KeyTable) holds the key rows, `state` int32 [B, TX_WORDS] the kernel's TX rows."""

    def __init__(self, batch: int, row_bytes: int):
        self.B, self.tb = int(batch), int(row_bytes)
        if not wire.TRANSPORT_HEADER < self.tb <= MAX_ROW_BYTES:
            raise ValueError(f"srtp.SenderModel: row_bytes = {row_bytes} outside ({wire.TRANSPORT_HEADER}, {MAX_ROW_BYTES}]")
        self.keys = KeyTable(self.B)
        self.state = np.zeros((self.B, TX_WORDS), dtype=np.int32)

    def protect(self, packets, nbytes, action=None) -> Dict[str, np.ndarray]:
        """one hop: `packets` uint8 [B, row_bytes] and `nbytes` int [B] as hilc_packet_header left them, `action` int [B] (None:
        zeros) -> packets (uint8 [B, row_bytes + 10]) and nbytes (int32 [B]); `state` is updated in place"""
        B, tb = self.B, self.tb
        packets = np.asarray(packets, dtype=np.uint8).reshape(B, tb)
        nbytes = np.asarray(nbytes, dtype=np.int64).reshape(-1)
        action = np.zeros(B, dtype=np.int64) if action is None else np.asarray(action).reshape(-1)
        out = np.zeros((B, tb + TAG_BYTES), dtype=np.uint8)
        out_nbytes = np.zeros(B, dtype=np.int32)
        for b in range(B):
            row, key = self.state[b], self.keys.rows[b]
            valid = key[KEY_VALID] != 0
            if action[b] != 0:
                row[:] = 0
                row[TX_ROC] = key[KEY_ROC] if valid else 0
            nb = min(int(nbytes[b]), tb)
            if nb < wire.TRANSPORT_HEADER:
                continue
            if not valid:
                row[TX_NOKEY] += 1
                continue
            seq = (int(packets[b, 0]) << 8) | int(packets[b, 1])
            if row[TX_SENT] != 0 and seq < (int(row[TX_LAST]) & 0xFFFF):
                row[TX_ROC] = _i32(_u32(row[TX_ROC]) + 1)
            row[TX_LAST], row[TX_SENT] = seq, 1
            blob = protect_packet(key, packets[b, :nb].tobytes(), _u32(row[TX_ROC]))
            out[b, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            out_nbytes[b] = len(blob)
            row[TX_PROTECTED] += 1
        return {"packets": out, "nbytes": out_nbytes}


def unprotect_packet(key, row, data: bytes, nbytes: int, row_bytes: int) -> Optional[bytes]:
    """one arrival against key row `key` and RX row `row` (updated in place): the plain packet, or None for a rejected one.
    `data`: the record's bytes (row_bytes + 10 of them at most), `nbytes`: its byte count"""
    if key[KEY_VALID] == 0:
        row[RX_NOKEY] += 1
        return None
    nbytes = int(nbytes)
    if nbytes < wire.TRANSPORT_HEADER + TAG_BYTES or nbytes > int(row_bytes) + TAG_BYTES or nbytes > len(data):
        row[RX_SHORT] += 1
        return None
    data = bytes(data[:nbytes])
    body, tag = data[:-TAG_BYTES], data[-TAG_BYTES:]
    seq = (body[0] << 8) | body[1]
    roc, s_l, seen = _u32(row[RX_ROC]), int(row[RX_SL]) & 0xFFFF, row[RX_SEEN] != 0
    if not seen:
        v = roc
    elif s_l < 32768:
        v = roc - 1 if seq - s_l > 32768 else roc
    else:
        v = (roc + 1) & 0xFFFFFFFF if s_l - 32768 > seq else roc
    if v < 0:
        row[RX_REPLAY] += 1
        return None
    window = _u32(row[RX_WIN_LO]) | _u32(row[RX_WIN_HI]) << 32
    delta = ((v << 16) | seq) - ((roc << 16) | s_l) if seen else 1
    if delta <= 0 and (-delta >= WINDOW or (window >> -delta) & 1):
        row[RX_REPLAY] += 1
        return None
    want = _tag(key, body, v)
    diff = 0
    for x, y in zip(want, tag):
        diff |= x ^ y
    if diff:
        row[RX_AUTH_FAIL] += 1
        return None
    if delta > 0:
        window = 1 if not seen or delta >= WINDOW else ((window << delta) | 1) & ((1 << WINDOW) - 1)
        row[RX_SL], row[RX_ROC], row[RX_SEEN] = seq, _i32(v), 1
    else:
        window |= 1 << -delta
    row[RX_WIN_LO], row[RX_WIN_HI] = _i32(window), _i32(window >> 32)
    row[RX_OK] += 1
    return _crypt(key, body, v)


class ReceiverModel:
    """numpy statement of hilc_srtp_unprotect for `batch` slots of a receiver whose plain rows are `row_bytes` bytes.  `keys` (a
    KeyTable) holds the key rows, `state` int32 [B, RX_WORDS] the kernel's RX rows."""

    def __init__(self, batch: int, row_bytes: int):
        self.B, self.tb = int(batch), int(row_bytes)
        if not wire.TRANSPORT_HEADER < self.tb <= MAX_ROW_BYTES:
            raise ValueError(f"srtp.ReceiverModel: row_bytes = {row_bytes} outside ({wire.TRANSPORT_HEADER}, {MAX_ROW_BYTES}]")
        self.keys = KeyTable(self.B)
        self.state = np.zeros((self.B, RX_WORDS), dtype=np.int32)

    def start(self, action) -> None:
        """rule 0 for the slots whose `action` is not 0"""
        for b in np.nonzero(np.asarray(action).reshape(-1))[0]:
            key = self.keys.rows[b]
            self.state[b] = 0
            self.state[b, RX_ROC] = key[KEY_ROC] if key[KEY_VALID] != 0 else 0

    def push(self, slot: int, packet: bytes) -> Optional[bytes]:
        """one arrival of `slot`: the plain packet or None"""
        return unprotect_packet(self.keys.rows[slot], self.state[slot], bytes(packet), len(packet), self.tb)

    def unprotect(self, records, offsets, action=None) -> np.ndarray:
        """one hop: `records` int32 [A, 1 + ceil((row_bytes + 10) / 4)] and `offsets` int [B + 1] (forward.arrival_records of the
        protected rows), `action` int [B] (None: zeros) -> the plain records int32 [A, 1 + ceil(row_bytes / 4)]; records outside
        every slot's range come out zero"""
        B, tb = self.B, self.tb
        pw = (tb + TAG_BYTES + 3) // 4
        records = np.ascontiguousarray(np.asarray(records, dtype=np.int32)).reshape(-1, 1 + pw)
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        A = records.shape[0]
        out = np.zeros((A, 1 + (tb + 3) // 4), dtype=np.int32)
        if action is not None:
            self.start(action)
        for b in range(B):
            a0 = min(max(int(offsets[b]), 0), A)
            a1 = min(max(int(offsets[b + 1]), a0), A)
            for a in range(a0, a1):
                data = records[a].view(np.uint8)[4:4 + tb + TAG_BYTES].tobytes()
                plain = unprotect_packet(self.keys.rows[b], self.state[b], data, int(records[a, 0]), tb)
                if plain is not None:
                    out[a, 0] = len(plain)
                    out[a].view(np.uint8)[4:4 + len(plain)] = np.frombuffer(plain, dtype=np.uint8)
        return out
