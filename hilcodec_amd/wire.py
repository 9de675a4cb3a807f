"""Wire / on-disk formats of the reference's streaming driver (`test_onnx.py`) — SURVEY.md §8(f) row 1.

* code indices: `int16 [n, B, T]` `.npy` (`test_onnx.py:96-100,105`), and a 10-bit-per-index packing
  (1024-entry codebooks = 0.75 kbps per codebook at 75 frames/s, `configs/hilcodec_music.yaml:31`);
* cache templates: `.npz` with `e_in{i}` / `d_in{i}` arrays (`test_onnx.py:71,119`, notebook cell 5);
* trained codebooks: the `embed [1024,128]` fp32 initializer of the reference's `onnx/*_deq{i}.onnx`
  (a single Gather node), read with a minimal protobuf walk — the `onnx` package is not needed.
Host-side helpers only: no arithmetic of the hot path lives here."""
from __future__ import annotations

import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor


# ---------------------------------------------------------------- indices
def save_indices_npy(path: str, indices: Tensor) -> None:
    """indices `[n,B,T]` (any integer dtype, values < 32768) -> int16 .npy, the reference's format."""
    a = indices.detach().cpu().numpy()
    if a.min() < 0 or a.max() > 32767:
        raise ValueError("index out of int16 range")
    np.save(path, a.astype(np.int16))


def load_indices_npy(path: str, device=None) -> Tensor:
    a = np.load(path)
    if a.dtype != np.int16 or a.ndim != 3:
        raise ValueError(f"expected int16 [n,B,T], got {a.dtype} {a.shape}")
    t = torch.from_numpy(a.astype(np.int64))
    return t.to(device) if device is not None else t


def pack_indices_10bit(indices: Tensor) -> bytes:
    """`[n,B,T]` indices in [0,1024) -> header (3 x uint32 LE) + ceil(n*B*T*10/8) bytes, MSB-first."""
    a = indices.detach().cpu().numpy().astype(np.int64)
    if a.ndim != 3 or a.min() < 0 or a.max() >= 1024:
        raise ValueError("indices must be [n,B,T] with values in [0,1024)")
    flat = a.reshape(-1)
    bits = ((flat[:, None] >> np.arange(9, -1, -1)) & 1).astype(np.uint8).reshape(-1)
    return struct.pack("<III", *a.shape) + np.packbits(bits).tobytes()


def unpack_indices_10bit(blob: bytes) -> Tensor:
    n, B, T = struct.unpack("<III", blob[:12])
    count = n * B * T
    bits = np.unpackbits(np.frombuffer(blob[12:], dtype=np.uint8))[: count * 10].reshape(count, 10)
    vals = (bits.astype(np.int64) << np.arange(9, -1, -1)).sum(axis=1)
    return torch.from_numpy(vals.reshape(n, B, T))


# ---------------------------------------------------------------- per-stream packets (graph_step.GraphedEncodeHop / GraphedDecodeHop)
# One stream's packet for one hop of T frames: its first n stages x T codes, stage-major, 10 bits each, MSB first, the last byte
# zero-padded — exactly the body of pack_indices_10bit(indices[:n, b:b+1, :]) without its header.  A batch of packets is a
# uint8 [B, packet_bytes(n_max, T)] tensor (row b zero past packet_bytes(n_b, T)) with an int32 [B] byte count.
MAX_STAGES = 32                                   # stages of one packet, primary + redundant


def packet_bytes(n: int, T: int) -> int:
    return (10 * int(n) * int(T) + 7) // 8


def packet_n(nbytes: int, T: int) -> int:
    """the n of a packet of `nbytes` bytes (unique: consecutive n differ by >= 1.25 bytes); ValueError when none matches"""
    n = (8 * int(nbytes)) // (10 * int(T))             # ceil(10 n T / 8) = nbytes  <=>  n = floor(8 nbytes / 10 T), if any
    if n >= 1 and packet_bytes(n, T) == nbytes:
        return n
    raise ValueError(f"no stage count gives a {nbytes}-byte packet of {T} frames")


def pack_stream_packet(codes: Tensor) -> bytes:
    """one stream's codes `[n, T]` in [0, 1024) -> its packet"""
    if codes.dim() != 2:
        raise ValueError("codes must be [n, T]")
    return pack_indices_10bit(codes.unsqueeze(1))[12:]


def unpack_stream_packet(blob: bytes, n: int, T: int) -> Tensor:
    """a packet of `n` stages x `T` frames -> its codes `[n, T]` int64 (bytes past packet_bytes(n, T) are ignored)"""
    if len(blob) < packet_bytes(n, T):
        raise ValueError(f"a packet of {n} x {T} codes needs {packet_bytes(n, T)} bytes, got {len(blob)}")
    return unpack_indices_10bit(struct.pack("<III", n, 1, T) + bytes(blob[:packet_bytes(n, T)]))[:, 0, :]



# Loss concealment of the receiver (graph_step.GraphedDecodeHop(conceal=True)): a lost hop is decoded from the codes of the last
# frame received, repeated over the hop, and faded.  These are the definitions the receiver's kernels follow.
# Concealment row of a slot (int32, n_max + CONCEAL_CODES words): hops lost in a row, has-codes, stored n, then the last frame's codes
CONCEAL_RUN, CONCEAL_HAS, CONCEAL_N, CONCEAL_CODES = 0, 1, 2, 3


def conceal_packet(packet: bytes, n: int, T: int) -> bytes:
    """the substitute packet for a stream whose last received packet is `packet` (`n` stages x `T` frames): that packet's last
    frame's n codes repeated over T frames, in the packet format"""
    codes = unpack_stream_packet(packet, n, T)
    return pack_stream_packet(codes[:, -1:].expand(int(n), int(T)).contiguous())


def conceal_tables(fade_hops: int, samples: int) -> Tuple[Tensor, Tensor]:
    """(G, W) fp32: G[k] = (F - k) / F for k = 0..F, the gain after k lost hops in a row, and W[s] = (s + 1) / S for s < S =
    `samples`, the weight of sample s on a hop's ramp; each computed in float64 and rounded once to fp32"""
    F, S = int(fade_hops), int(samples)
    if F < 1 or S < 1:
        raise ValueError("fade_hops and samples must be >= 1")
    G = ((F - torch.arange(F + 1, dtype=torch.float64)) / F).float()
    W = ((torch.arange(S, dtype=torch.float64) + 1) / S).float()
    return G, W


# In-band forward error correction (graph_step.GraphedEncodeHop / GraphedDecodeHop(fec_stages=m)): the packet of hop k of a
# stream with n_b stages is the packet of the [n_b + m, T] codes cat(idx_k[:n_b], idx_{k-1}[:m]) — the primary codes first,
# unchanged, then the first m stages of the stream's previous encoded hop, its redundant section.  A stream without a previous
# encoded hop (the first hop after a start, a resume, construction or reset) sends the plain packet_bytes(n_b, T) bytes.  The
# first m stages of a residual VQ encoding are themselves a valid m-stage encoding of that hop, so a receiver that lost packet k
# decodes hop k from the redundant section of packet k + 1 at n = m.  These are the definitions the kernels follow.
def fec_packet_bytes(n: int, m: int, T: int) -> int:
    """the length of an n-stage packet of T frames with an m-stage redundant section"""
    return packet_bytes(int(n) + int(m), T)


def pack_fec_packet(codes: Tensor, prev_codes=None) -> bytes:
    """one stream's codes `[n, T]` and its previous hop's first m stages `[m, T]` (None: no previous hop) -> its FEC packet"""
    if prev_codes is None:
        return pack_stream_packet(codes)
    if codes.dim() != 2 or prev_codes.dim() != 2 or prev_codes.shape[1] != codes.shape[1]:
        raise ValueError("codes must be [n, T] and prev_codes [m, T]")
    return pack_stream_packet(torch.cat([codes, prev_codes.to(codes.dtype)]))


def fec_primary(packet: bytes, n: int, T: int) -> bytes:
    """the primary section of an FEC packet with `n` primary stages: packet_bytes(n, T) bytes, the bits of the last byte that
    belong to the redundant section zeroed — byte for byte the packet of a sender without FEC"""
    return pack_stream_packet(unpack_stream_packet(packet, n, T))


def fec_redundant(packet: bytes, n: int, m: int, T: int) -> bytes:
    """the redundant section of an FEC packet (`n` primary stages, `m` redundant ones) re-packed as an m-stage packet"""
    return pack_stream_packet(unpack_stream_packet(packet, int(n) + int(m), T)[int(n):])


def fec_present(nbytes: int, n: int, m: int, T: int) -> bool:
    """whether a packet of `nbytes` bytes with `n` primary stages carries an m-stage redundant section; ValueError for a length
    that is neither packet_bytes(n, T) nor fec_packet_bytes(n, m, T)"""
    if int(m) < 1:
        raise ValueError(f"fec_present: m must be >= 1, got {m}")
    if int(nbytes) == fec_packet_bytes(n, m, T):
        return True
    if int(nbytes) == packet_bytes(n, T):
        return False
    raise ValueError(f"a {nbytes}-byte packet fits neither {n} nor {n} + {m} stages of {T} frames")


# Transport header of the graphed sender / receiver (graph_step.GraphedEncodeHop(header=True), GraphedDecodeHop(jitter=...)): a sent
# packet is 3 header bytes then its body.  Bytes 0-1: the hop index h mod 2^16, big-endian (the hops the sending slot's encoder
# advanced since its last start, before this hop); byte 2: bit 7 SID, bit 6 a redundant (FEC) section is present, bit 5 zero, bits
# 4..0 n (codes: 1..31; SID: 0).  The body is the packet_bytes(n, T) codes, the fec_packet_bytes(n, m, T) codes with bit 6, or a SID
# of dtx.sid_bytes(K) bytes.  Headed packets are not re-framed: the receiver's frames are the sender's T.
TRANSPORT_HEADER = 3
SID_BIT, FEC_BIT, RSV_BIT, N_MASK = 0x80, 0x40, 0x20, 0x1F


def transport_bytes(n: int, m: int, T: int) -> int:
    """the widest headed packet of a sender with n stages, m redundant ones and T frames (a SID always fits)"""
    return TRANSPORT_HEADER + packet_bytes(int(n) + int(m), T)


def pack_transport(hop: int, body: bytes, n: int, sid: bool = False, fec: bool = False) -> bytes:
    """header (hop mod 2^16, SID / FEC flags, n) + body; ValueError for an n outside 1..31 (codes), a SID with n != 0 or with the
    FEC flag"""
    n = int(n)
    if sid and (n != 0 or fec):
        raise ValueError("pack_transport: a SID has n = 0 and no redundant section")
    if not sid and not 1 <= n <= 31:
        raise ValueError(f"pack_transport: n = {n} outside [1, 31]")
    flags = (SID_BIT if sid else 0) | (FEC_BIT if fec else 0) | n
    h = int(hop) & 0xFFFF
    return bytes([h >> 8, h & 0xFF, flags]) + bytes(body)


def parse_transport(packet, nbytes: int, T: int, n_max: int, m: int, K) -> Tuple[int, bool, bool, int, bytes]:
    """(hop, sid, fec, n, body) of the first `nbytes` bytes of `packet`, for a receiver of n_max stages, m redundant ones (0: no
    FEC) and comfort noise of order K (None: none).  ValueError for a malformed packet: shorter than the header, bit 5 set, a codes
    packet with n = 0 or n > n_max, a SID without K or with n != 0, the FEC flag without m or with n < m, or a length that does not
    match the header"""
    from .dtx import sid_bytes
    nbytes = int(nbytes)
    data = bytes(packet[:max(nbytes, 0)])
    if nbytes < TRANSPORT_HEADER or len(data) < nbytes:
        raise ValueError(f"a {nbytes}-byte packet is shorter than its {TRANSPORT_HEADER}-byte header")
    hop, flags = (data[0] << 8) | data[1], data[2]
    sid, fec, n = bool(flags & SID_BIT), bool(flags & FEC_BIT), flags & N_MASK
    if flags & RSV_BIT:
        raise ValueError("header bit 5 is set")
    if fec and (int(m) < 1 or n < int(m)):
        raise ValueError(f"a redundant section with n = {n}, m = {m}")
    body = nbytes - TRANSPORT_HEADER
    if sid:
        if K is None:
            raise ValueError("a SID without comfort noise")
        if n != 0:
            raise ValueError(f"a SID with n = {n}")
        if body != sid_bytes(K):
            raise ValueError(f"a {body}-byte SID body, order {K} needs {sid_bytes(K)}")
    else:
        if not 1 <= n <= int(n_max):
            raise ValueError(f"n = {n} outside [1, {n_max}]")
        if int(m) >= 1:
            present = fec_present(body, n, m, T)           # ValueError: neither length
        elif body == packet_bytes(n, T):
            present = False
        else:
            raise ValueError(f"a {body}-byte body is not {n} stages of {T} frames")
        if present != fec:
            raise ValueError(f"a {body}-byte body disagrees with its header's FEC flag")
    return hop, sid, fec, n, data[TRANSPORT_HEADER:nbytes]


# Receiver report (hilcodec_amd/report.py: GraphedDecodeHop(report=...) emits it, GraphedEncodeHop(fec_adapt=...) takes it): feedback
# that travels beside the media, 3 bytes: a sequence number mod 256, then the loss and the residual loss of the receiver's window as
# fractions of 256 (loss_q8 counts the hops repaired from a redundant section as missing, residual_q8 only what the listener lost).
REPORT_BYTES = 3


def pack_report(seq: int, loss_q8: int, residual_q8: int) -> bytes:
    """(seq, loss_q8, residual_q8), one byte each in that order; ValueError for a field outside [0, 255]"""
    fields = (seq, loss_q8, residual_q8)
    for name, v in zip(("seq", "loss_q8", "residual_q8"), fields):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
            raise ValueError(f"pack_report: {name} = {v!r} outside [0, 255]")
    return bytes(int(v) for v in fields)


def parse_report(blob) -> Tuple[int, int, int]:
    """(seq, loss_q8, residual_q8) of a report; ValueError unless it is exactly REPORT_BYTES bytes"""
    data = bytes(blob)
    if len(data) != REPORT_BYTES:
        raise ValueError(f"a report is {REPORT_BYTES} bytes, got {len(data)}")
    return data[0], data[1], data[2]


# Negative acknowledgement (hilcodec_amd/rtx.py: GraphedDecodeHop(nack=...) emits it, GraphedEncodeHop(rtx=...) answers it): feedback
# that travels beside the media, 4 bytes: `base`, the first hop index asked for, big-endian in bytes 0-1, then a 16-bit bitmap,
# big-endian in bytes 2-3, whose bit j asks for hop (base + 1 + j) mod 2^16 as well.  `base` itself is always asked for.
NACK_BYTES = 4


def pack_nack(base: int, bitmap: int) -> bytes:
    """(base, bitmap), two bytes each, big-endian; ValueError for a field outside [0, 65535]"""
    for name, v in (("base", base), ("bitmap", bitmap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFF:
            raise ValueError(f"pack_nack: {name} = {v!r} outside [0, 65535]")
    base, bitmap = int(base), int(bitmap)
    return bytes([base >> 8, base & 0xFF, bitmap >> 8, bitmap & 0xFF])


def parse_nack(blob) -> Tuple[int, int]:
    """(base, bitmap) of a NACK; ValueError unless it is exactly NACK_BYTES bytes"""
    data = bytes(blob)
    if len(data) != NACK_BYTES:
        raise ValueError(f"a NACK is {NACK_BYTES} bytes, got {len(data)}")
    return (data[0] << 8) | data[1], (data[2] << 8) | data[3]


def nack_hops(base: int, bitmap: int) -> List[int]:
    """the hop indices a NACK asks for, in ascending order from `base` (mod 2^16): base, then base + 1 + j for every set bit j"""
    base, bitmap = int(base), int(bitmap)
    if not 0 <= base <= 0xFFFF or not 0 <= bitmap <= 0xFFFF:
        raise ValueError(f"nack_hops: base = {base} or bitmap = {bitmap} outside [0, 65535]")
    return [base] + [(base + 1 + j) & 0xFFFF for j in range(16) if (bitmap >> j) & 1]


# Rate cap (hilcodec_amd/bwe.py: GraphedDecodeHop(bwe=...) emits it, GraphedEncodeHop(cap=...) takes it): the receiver's delay-based
# bandwidth estimate, feedback that travels beside the media, 3 bytes: a sequence number mod 256, then the most bits per hop the
# sender should send, a big-endian uint16.
CAP_BYTES = 3


def pack_cap(seq: int, cap_bits: int) -> bytes:
    """(seq, cap_bits): one byte, then two bytes big-endian; ValueError for a seq outside [0, 255] or a cap outside [0, 65535]"""
    for name, v, top in (("seq", seq, 255), ("cap_bits", cap_bits, 0xFFFF)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top:
            raise ValueError(f"pack_cap: {name} = {v!r} outside [0, {top}]")
    return bytes([int(seq), int(cap_bits) >> 8, int(cap_bits) & 0xFF])


def parse_cap(blob) -> Tuple[int, int]:
    """(seq, cap_bits) of a rate cap; ValueError unless it is exactly CAP_BYTES bytes"""
    data = bytes(blob)
    if len(data) != CAP_BYTES:
        raise ValueError(f"a rate cap is {CAP_BYTES} bytes, got {len(data)}")
    return data[0], (data[1] << 8) | data[2]


# Packet protection (hilcodec_amd/srtp.py: GraphedEncodeHop(srtp=...) / GraphedDecodeHop(srtp=...)): a protected packet is the headed
# packet with its first 3 bytes clear, the rest encrypted, and an authentication tag of 10 bytes behind it.
SRTP_TAG_BYTES = 10


def srtp_bytes(n: int, m: int, T: int) -> int:
    """the widest protected packet of a sender with n stages, m redundant ones and T frames"""
    return transport_bytes(n, m, T) + SRTP_TAG_BYTES

# ---------------------------------------------------------------- caches
def save_cache_npz(path: str, caches: Sequence[Tensor], prefix: str) -> None:
    """prefix 'e_in' (encoder, 22 tensors) or 'd_in' (decoder, 30)."""
    np.savez(path, **{f"{prefix}{i}": c.detach().cpu().numpy() for i, c in enumerate(caches)})


def load_cache_npz(path: str, prefix: str, device=None, batch: int = None) -> List[Tensor]:
    z = np.load(path)
    out = []
    i = 0
    while f"{prefix}{i}" in z:
        t = torch.from_numpy(z[f"{prefix}{i}"].astype(np.float32))
        if batch is not None and t.shape[0] != batch:
            t = t.expand(batch, *t.shape[1:]).contiguous()      # templates are saved with batch 1
        out.append(t.to(device) if device is not None else t)
        i += 1
    if not out:
        raise KeyError(f"no '{prefix}0' in {path}")
    return out


# ---------------------------------------------------------------- ONNX initializer reader
def _varint(buf: bytes, pos: int) -> Tuple[int, int]:
    val = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        val |= (b & 0x7F) << shift
        if not b & 0x80:
            return val, pos
        shift += 7


def _fields(buf: bytes):
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
        elif wt == 1:
            val, pos = buf[pos:pos + 8], pos + 8
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            val, pos = buf[pos:pos + ln], pos + ln
        elif wt == 5:
            val, pos = buf[pos:pos + 4], pos + 4
        else:
            raise ValueError(f"unsupported protobuf wire type {wt}")
        yield num, wt, val


def read_onnx_initializers(path: str) -> Dict[str, np.ndarray]:
    """All fp32 initializers of an ONNX file: ModelProto.graph(7).initializer(5) -> TensorProto
    {dims(1), data_type(2)=1, float_data(4) | raw_data(9), name(8)}."""
    model = open(path, "rb").read()
    out: Dict[str, np.ndarray] = {}
    for num, wt, graph in _fields(model):
        if num != 7 or wt != 2:
            continue
        for gnum, gwt, tensor in _fields(graph):
            if gnum != 5 or gwt != 2:
                continue
            dims: List[int] = []
            dtype, name, raw, floats = None, "", None, None
            for tnum, twt, val in _fields(tensor):
                if tnum == 1 and twt == 0:
                    dims.append(val)
                elif tnum == 1 and twt == 2:               # packed dims
                    p = 0
                    while p < len(val):
                        d, p = _varint(val, p)
                        dims.append(d)
                elif tnum == 2:
                    dtype = val
                elif tnum == 8:
                    name = val.decode()
                elif tnum == 9:
                    raw = val
                elif tnum == 4 and twt == 2:
                    floats = np.frombuffer(val, dtype="<f4")
            if dtype != 1:
                continue
            data = np.frombuffer(raw, dtype="<f4") if raw is not None else floats
            if data is not None:
                out[name] = np.array(data, dtype=np.float32).reshape(dims)
    return out


def read_onnx_codebook(path: str) -> Tensor:
    """The `[K, C]` embed table of one `*_deq{i}.onnx` / `*_vq{i}.onnx` file."""
    inits = read_onnx_initializers(path)
    if "embed" in inits and inits["embed"].ndim == 2:        # the buffer's name in both exported graphs
        return torch.from_numpy(inits["embed"])
    cands = [v for v in inits.values() if v.ndim == 2]
    if len(cands) != 1:
        raise ValueError(f"{path}: no 'embed' initializer and {len(cands)} 2-D fp32 candidates")
    return torch.from_numpy(cands[0])
