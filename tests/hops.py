"""What the hop features' tests share: the C header read back (for the one test that proves the ctypes binding against it, and for
each feature's "my entry points exist" test), and the small helpers of the GPU hop tests.  A plain module, imported as
`from tests.hops import ...`; fixtures stay in the test modules."""
import ctypes
import os
import re

import numpy as np
import torch

from hilcodec_amd import synth

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
