"""What the hop features' tests share: the C header read back (for the one test that proves the ctypes binding against it, and for
each feature's "my entry points exist" test), the small helpers of the GPU hop tests, and what the tests of more than one feature
use: the adaptive receiver's traffic model, shapes, the VBR model and the host models of the FEC and concealment kernels.  A plain
module, imported as `from tests.hops import ...`; fixtures stay in the test modules."""
import ctypes
import math
import os
import re

import numpy as np
import torch

from hilcodec_amd import dtx, synth, vbr, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hilcodec_amd.h")
DEV = torch.device("cuda:0")
HOP = 320


# ---------------------------------------------------------------- include/hilcodec_amd.h
_KINDS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}


def _kind(decl):
    """the ctypes kind of one C parameter or field declaration: any pointer is a c_void_p, a scalar its own type"""
    return ctypes.c_void_p if "*" in decl else _KINDS[decl.replace("const ", " ").split()[0]]


def parse_header():
    """(prototypes, structs) of the header, comments stripped: {name: [kind per parameter]} of every `hilc_*(...);` prototype and
    {name: [(field, kind)]} of every `typedef struct hilc_*_params`, a list such as `float in_scale, out_scale;` split"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"^(?:int|const char\*)\s+(hilc_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        protos[name] = [] if args.strip() == "void" else [_kind(a) for a in args.split(",")]
    structs = {}
    for body, name in re.findall(r"typedef struct \w+\s*\{(.*?)\}\s*(hilc_\w+_params)\s*;", text, re.S):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            fields += [(piece.split()[-1].lstrip("*"), _kind(decl)) for piece in decl.split(",")]
    return protos, structs


def assert_entry_points(names, in_abi16_line=False):
    """each of `names` is declared at the start of a header line, (on request) named in the `#define HILC_ABI_VERSION 16` line,
    exported by the library and bound; that the binding's types are the header's is test_api_cpu's to prove, for all of them"""
    from hilcodec_amd import _lib
    assert _lib.ABI_VERSION == 16 and _lib.lib.hilc_abi_version() == 16
    header = open(HEADER).read()
    abi_line = re.search(r"#define HILC_ABI_VERSION 16\b.*", header).group(0)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert not in_abi16_line or name in abi_line, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


# ---------------------------------------------------------------- models
def bare_model(name="hil_speech"):
    """the streaming model as constructed, no weights loaded: for tests of layouts and queues, which never run it"""
    from hilcodec_amd.models.hilcodec.streaming import HILCodec
    return HILCodec(24000, **synth.streaming_kwargs(name)).eval()


def build_streaming(seed=7, name="hil_speech"):
    """(streaming model, offline kwargs, offline state dict): the last two are what the oracle's legs take"""
    sd = synth.synth_state_dict(name, seed)
    return synth.streaming_model(name, state_dict=sd), synth.model_kwargs(name), sd


# ---------------------------------------------------------------- hops, caches, packet rows
def chunk(x, h, hop=HOP):
    return x[:, :, hop * h:hop * (h + 1)].contiguous()


def same_indices(g_idx, e_idx):
    r = e_idx.shape[0]
    return torch.equal(g_idx[:r], e_idx) and bool((g_idx[r:] == -1).all())


def caches_equal(a_list, b_list):
    return all(torch.equal(a, b) for a, b in zip(a_list, b_list))


def row_bytes(packets, b, length=None):
    row = packets[b].tolist()
    return bytes(row if length is None else row[:length])


def put_row(packets, b, blob):
    packets[b] = 0
    packets[b, :len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)


def arrival_arrays(arrived, tbytes):
    """[(slot, bytes)] -> (slots, packets uint8 [A, tbytes], nbytes)"""
    packets = np.zeros((len(arrived), tbytes), dtype=np.uint8)
    for a, (_, p) in enumerate(arrived):
        packets[a, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return [s for s, _ in arrived], packets, [len(p) for _, p in arrived]


def arrival_records(slots, packets, nbytes, tbytes, B, max_a):
    """the device form of one hop's arrivals, as GraphedDecodeHop.play stages them: forward.arrival_records moved to the device.
    That function clips the byte counts to [-1, 2^20]; the counts given here lie inside that range, so the clip changes nothing"""
    from hilcodec_amd import forward
    counts = np.asarray(nbytes, dtype=np.int64)
    assert counts.size == 0 or (counts.min() >= -1 and counts.max() <= 1 << 20), counts
    rec, offs = forward.arrival_records(slots, packets, nbytes, tbytes, B, max_a)
    return torch.from_numpy(rec).to(DEV), torch.from_numpy(offs).to(DEV)


# ---------------------------------------------------------------- everything a hop object shows of one slot
def slot_views(hop):
    """the names of the per-slot device views a hop object's configuration has (an object that lacks one of them raises)"""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    names = []
    if isinstance(hop, GraphedEncodeHop):
        names += ["n_eff", "distortion"] * (hop.vbr is not None) + ["credit"] * (hop.vbr is not None and hop.vbr.cap_kbps is not None)
        names += ["kind"] * (hop.dtx is not None) + ["fec_on", "fec_adapt_state"] * (hop.fec_adapt is not None)
        names += ["hop_index"] * hop.header
    elif isinstance(hop, GraphedDecodeHop):
        names += ["concealed"] * hop.conceal + ["cng_state"] * (hop.cng_order is not None) + ["jitter_state"] * (hop.jitter is not None)
        names += ["jitter_adapt"] * (hop.jitter is not None and hop.jitter.adapt is not None)
        names += ["reports", "report_due", "report_state"] * (hop.report is not None)
        names += ["mixed", "speakers", "levels"] * (hop.mix is not None)
    return names


def observe(hop, slot):
    """clones of everything a sessions hop object exposes for slot `slot` after a hop, by name: the rows of what the last step()
    / play() returned, its indices, every per-slot view its configuration has (`slot_views`), and every tensor of export(slot)
    (a list).  The outputs are static views that the next-but-one call overwrites, hence the clones."""
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    out = hop.outs[hop.parity ^ 1]                           # the static outputs of the graph that ran last
    obs = {}
    if isinstance(hop, GraphedDecodeHop):
        obs["wav"], records = out[slot], [hop.export(slot)]
    elif isinstance(hop, GraphedEncodeHop):
        obs["indices"], obs["packet"], obs["nbytes"] = hop.indices[:, slot], out[1][slot], out[2][slot]
        records = [hop.export(slot)]
    else:
        obs["indices"], obs["wav"], records = out[0][:, slot], out[1][slot], hop.export(slot)
    for name in slot_views(hop):
        obs[name] = getattr(hop, name)[slot]
    obs = {k: v.clone() for k, v in obs.items()}
    obs["export"] = [t.clone() for rec in records for t in rec]
    return obs


def first_difference(a, b):
    """None when two observations are equal bit for bit (NaN never is), else "<attribute>: <where and what>" of the first that differs"""
    if a.keys() != b.keys():
        return f"attributes {sorted(a)} != {sorted(b)}"
    for name in a:
        xs, ys = (a[name], b[name]) if isinstance(a[name], list) else ([a[name]], [b[name]])
        if len(xs) != len(ys):
            return f"{name}: {len(xs)} tensors != {len(ys)}"
        for i, (x, y) in enumerate(zip(xs, ys)):
            if x.shape != y.shape or x.dtype != y.dtype:
                return f"{name}[{i}]: {tuple(x.shape)} {x.dtype} != {tuple(y.shape)} {y.dtype}"
            if not torch.equal(x, y):
                fx, fy = x.reshape(-1), y.reshape(-1)
                j = int(torch.nonzero(~(fx == fy))[0])
                which = f"[{i}]" if isinstance(a[name], list) else ""
                return f"{name}{which}: {int((~(fx == fy)).sum())} of {fx.numel()} differ, first at {j}: {fx[j].item()!r} != {fy[j].item()!r}"
    return None


def first_non_finite(obs):
    """None when every floating-point value of an observation is finite, else "<attribute>: ..." of the first that is not"""
    for name, v in obs.items():
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                return f"{name}[{i}]: {int((~torch.isfinite(t)).sum())} of {t.numel()} non-finite"
    return None


# ---------------------------------------------------------------- shared by the tests of more than one feature
class Network:
    """(of tests/test_gpu_jitter_adapt.py; the NACK, report, bandwidth and lifecycle tests drive their receivers with it too)
    seeded traffic of B senders: each hop every slot sends a codes packet, a SID (DTX) or nothing; packets are lost, delayed up
    to `delay` hops (reordered), duplicated or corrupted; `hold` / `start` rates give the host holds and the restarts of sender and
    receiver together, `restart` the rate of sender restarts the receiver is not told of.  Slot b drifts by b mod 3: 1 a slow
    sender (sends nothing on every `every`-th hop), 2 a fast one (two packets on that hop), 0 none; with `mild`, the slots with
    b // 3 even see a good network (nothing lost, duplicated or corrupted, a delay of at most one hop), so that their clock is
    moved by the windowed estimate and not by late arrivals."""

    def __init__(self, B, n, m, K, T, seed, loss=0.05, delay=3, dup=0.01, bad=0.0, hold=0.0, start=0.0, sid=0.0, restart=0.0, every=20,
                 mild=True):
        self.B, self.n, self.m, self.K, self.T = B, n, m, K, T
        self.rng = np.random.default_rng(seed)
        self.tbytes = wire.transport_bytes(n, m, T)
        self.h = self.rng.integers(0, 65536, B).astype(np.int64)
        self.dtx = np.zeros(B, dtype=bool)
        self.rates = dict(loss=loss, delay=delay, dup=dup, bad=bad, hold=hold, start=start, sid=sid, restart=restart)
        self.every, self.mild = every, mild
        self.flight = []                                     # (due hop, slot, packet bytes, byte count)
        self.k = 0

    def _packet(self, b):
        r, h = self.rng, int(self.h[b])
        if self.K is not None and (self.dtx[b] or r.random() < self.rates["sid"]):
            self.dtx[b] = r.random() < 0.8
            if r.random() < 0.4 or not self.dtx[b]:
                body = r.integers(0, 256, dtx.sid_bytes(self.K)).astype(np.uint8).tobytes()
                return wire.pack_transport(h, body, 0, sid=True) if self.dtx[b] else None
            return None                                      # silent: nothing sent
        nb = int(r.integers(max(self.m, 1), self.n + 1))
        fec = self.m >= 1 and r.random() < 0.7
        codes = torch.from_numpy(r.integers(0, 1024, (nb + (self.m if fec else 0), self.T)))
        return wire.pack_transport(h, wire.pack_stream_packet(codes), nb, fec=fec)

    def hop(self):
        """-> (slots, packets uint8 [A, tbytes], nbytes, action [B], hold [B]) of this hop"""
        r, B, k = self.rng, self.B, self.k
        action = (r.random(B) < self.rates["start"]).astype(np.int32)
        hold = (r.random(B) < self.rates["hold"]).astype(np.int32)
        for b in np.nonzero(action)[0]:
            self.h[b] = 0
            self.dtx[b] = False
        for b in np.nonzero(r.random(B) < self.rates["restart"])[0]:
            self.h[b] = int(r.integers(0, 65536))
        for b in range(B):
            if hold[b]:
                continue
            tick = k % self.every == self.every - 1
            good = self.mild and (b // 3) % 2 == 0
            for _ in range((0 if b % 3 == 1 else 2 if b % 3 == 2 else 1) if tick else 1):
                p = self._packet(b)
                self.h[b] = (self.h[b] + 1) & 0xFFFF
                if p is None or r.random() < (0.0 if good else self.rates["loss"]):
                    continue
                for _ in range(2 if r.random() < (0.0 if good else self.rates["dup"]) else 1):
                    q = bytearray(p)
                    nb = len(q)
                    if r.random() < (0.0 if good else self.rates["bad"]):
                        how = int(r.integers(0, 3))
                        if how == 0:
                            q[2] |= 0x20
                        elif how == 1:
                            nb -= 1
                        else:
                            nb = 2
                    self.flight.append((k + int(r.integers(0, (1 if good else self.rates["delay"]) + 1)), b, bytes(q), nb))
        now = [f for f in self.flight if f[0] <= k]
        self.flight = [f for f in self.flight if f[0] > k]
        now = [now[i] for i in r.permutation(len(now))]
        pk = np.zeros((len(now), self.tbytes), dtype=np.uint8)
        for a, f in enumerate(now):
            pk[a, :len(f[2])] = np.frombuffer(f[2], dtype=np.uint8)
        self.k += 1
        return [f[1] for f in now], pk, [f[3] for f in now], action, hold


# the three AES block edges (payloads of 16, 32 and 48 bytes: 19, 35, 51) and, for an HMAC message of nbytes + 4 bytes behind the pad
# block, its lengths 55, 56, 63 and 64 mod 64 (51, 52, 59, 60), one either side, nothing, no header, a bare header, the whole row
SRTP_LENGTHS = (0, 2, 3, 13, 18, 19, 20, 35, 51, 52, 59, 60, 61, 80)


def rooms_case(name):
    if name == "b6":
        return np.array([0, 0, 0, 1, -1, 1])
    if name == "b70":                                       # one room of 67 members: crosses a wave
        room = np.full(70, 5)
        room[[3, 40, 69]] = -1
        return room
    room = np.full(300, -1)                                 # two rooms of 130, interleaved: cross a 256-thread block; 40 slots in none
    perm = np.random.default_rng(300).permutation(300)
    room[perm[:130]] = 7
    room[perm[130:260]] = 299
    return room


def vbr_speech_model():
    """the streaming model with falling per-stage codebooks randn(1024, 128) g 0.95^s, g scaled to its latents, so that VBR decides
    (tests/test_gpu_vbr.py says why)"""
    model = synth.streaming_model()
    x = synth.synth_clips(8, HOP, seed=1).to(DEV)
    with torch.no_grad():
        z, _ = model.encoder(x, *[c.to(DEV) for c in model.initialize_cache(x)[0]])
    g = 0.05 * float(z.float().norm(dim=-1).median())
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for s, (ql, dl) in enumerate(zip(model.quantizer.layers, model.dequantizer.layers)):
            e = torch.randn(1024, 128, generator=gen) * g * 0.95 ** s
            ql.embed.copy_(e)
            dl.embed.copy_(e)
    return model


def target_from_reference(model, B, frames, n, x0):
    """the median over the slots of D[:, n / 2] / D[:, 0] at hop 0, as target_db"""
    with torch.no_grad():
        z, _ = model.encoder(x0, *[c.to(DEV) for c in model.initialize_cache(x0)[0]])
        idx = model.quantizer(z, n)
    D = vbr.distortions(z.cpu(), idx.cpu(), model.quantizer._tables(DEV).codebooks.cpu())
    rho = float(np.median(D[:, n // 2] / D[:, 0]))
    assert 0.0 < rho < 1.0
    return -10.0 * math.log10(rho)


# ---------------------------------------------------------------- host models of the FEC and concealment kernels
def pack_model(idx, n_slot, prev_in, action, hold, m):
    """hilc_pack_codes_10bit_fec per slot on host copies: (packets, nbytes, prev_out)"""
    n_max, B, T = idx.shape
    W = 1 + m * T
    packets = torch.zeros(B, wire.fec_packet_bytes(n_max, m, T), dtype=torch.uint8)
    nbytes = torch.zeros(B, dtype=torch.int32)
    prev_out = torch.zeros(B, W, dtype=torch.int32)
    codes = idx.clamp(0, 1023)
    for b in range(B):
        row = torch.zeros(W, dtype=torch.int32) if int(action[b]) else prev_in[b].clone()
        if int(hold[b]):
            prev_out[b] = row
            continue
        nb = min(max(int(n_slot[b]), m), n_max)
        prev = (row[1:].long() & 1023).view(m, T) if int(row[0]) else None
        blob = wire.pack_fec_packet(codes[:nb, b], prev)
        put_row(packets, b, blob)
        nbytes[b] = len(blob)
        prev_out[b, 0] = 1
        prev_out[b, 1:] = codes[:m, b].reshape(-1).to(torch.int32)
    return packets, nbytes, prev_out


def select_model(wide, fec, n_slot, n_max, m, T):
    B = wide.shape[0]
    out = torch.zeros(B, wire.packet_bytes(n_max, T), dtype=torch.uint8)
    n_out = n_slot.clone()
    for b in range(B):
        if int(fec[b]):
            nb = min(max(int(n_slot[b]), m), n_max)
            put_row(out, b, wire.fec_redundant(row_bytes(wide, b), nb, m, T))
            n_out[b] = m
        else:
            nb = min(max(int(n_slot[b]), 1), n_max)
            put_row(out, b, wire.fec_primary(row_bytes(wide, b), nb, T))
    return out, n_out


CONCEAL_FADE = 4          # hops of a concealment fade: `F` of hilc_conceal_prepare


def prepare_model(state, action, hold, lost, n_slot, packets, T, F):
    """the table of the issue, per slot, on host copies; returns (state, hold, n_slot, packets, ramp)"""
    state, hold, n_slot, packets = state.clone(), hold.clone(), n_slot.clone(), packets.clone()
    B, words = state.shape
    n_max = words - 3
    ramp = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        row = state[b]
        if int(action[b]) != 0:
            row.zero_()
        k = min(max(int(row[0]), 0), F)
        has = int(row[1]) != 0
        if int(hold[b]) != 0:
            continue
        if int(lost[b]) == 0:
            nb = min(max(int(n_slot[b]), 1), n_max)
            codes = wire.unpack_stream_packet(row_bytes(packets, b), nb, T)[:, -1]
            row.zero_()
            row[1], row[2] = 1, nb
            row[3:3 + nb] = codes.to(torch.int32)
            ramp[b] = -k
        elif has and k < F:
            nb = min(max(int(row[2]), 1), n_max)
            codes = (row[3:3 + nb].long() & 1023).view(nb, 1).expand(nb, T).contiguous()
            put_row(packets, b, wire.pack_stream_packet(codes))
            n_slot[b] = nb
            row[0] = k + 1
            ramp[b] = k + 1
        else:
            hold[b] = 1
    return state, hold, n_slot, packets, ramp
