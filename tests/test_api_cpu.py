"""CPU: host-side logic — the C-ABI library loads and exports every symbol of include/hilcodec_amd.h,
module trees carry the reference's state-dict keys, weight folding is bit-exact, and nothing falls
back to the CPU silently.  (No kernel is launched here.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from hilcodec_amd import synth
from tests.hops import parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from hilcodec_amd import _lib
    header = open(os.path.join(ROOT, "include", "hilcodec_amd.h")).read()
    declared = set(re.findall(r"\b(hilc_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 14
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/hilcodec_amd.h but not exported"
    for name in _lib.SIGNATURES:
        assert name in declared, f"{name} bound in _lib.py but not declared in the header"
    assert _lib.lib.hilc_abi_version() == _lib.ABI_VERSION
    assert b"num_quantizers" in _lib.lib.hilc_error_string(-5)


def test_binding_matches_header_type_for_type():
    """The ctypes binding is the one link to include/hilcodec_amd.h that no compiler checks (the .hip files include the header):
    every prototype's parameter kinds equal `_lib.SIGNATURES[name]` element for element (any pointer <-> c_void_p, int, long, float,
    double), every prototype is bound and every bound name declared, and the five `ctypes.Structure` mirrors have the fields of the
    header's `hilc_*_params` structs in name, order and kind."""
    from hilcodec_amd import _lib
    protos, structs = parse_header()
    apart = {"hilc_abi_version", "hilc_error_string", "hilc_last_hip_error"}          # bound one by one in _lib._load
    assert apart <= set(protos) and set(protos) - apart == set(_lib.SIGNATURES)
    assert len(protos) >= 67
    for name, kinds in _lib.SIGNATURES.items():
        assert kinds == protos[name], name
    mirrors = {"hilc_resblock_params": _lib.ResblockParams, "hilc_up_params": _lib.UpParams, "hilc_down_params": _lib.DownParams,
               "hilc_post_params": _lib.PostParams, "hilc_spec0_params": _lib.Spec0Params}
    assert set(structs) == set(mirrors)
    for name, mirror in mirrors.items():
        assert mirror._fields_ == structs[name], name


def test_layouts_match_header():
    """The per-slot row layouts, codes and limits are the other link between C and Python that no compiler checks: the kernels take
    them from include/hilcodec_amd.h, the bindings and the host models from the Python modules.  `#define HILC_<MODULE>_<NAME>` is
    `hilcodec_amd.<module>.<NAME>`, value for value, in both directions: every such define has its Python name, and every public
    upper-case int that one of those modules assigns has its define (HOST_ONLY: what a host model needs and no kernel row or code
    depends on).  Then the derived sizes that allocations rely on."""
    import ast
    import importlib
    modules = ("sessions", "wire", "resample", "dtx", "jitter", "mixer", "vbr", "report")
    HOST_ONLY = {"LANES", "BASE_RATE", "ZERO_CROSSINGS", "MAX_BURST_BITS"}    # a wave's lanes, the filter design, an int32 bound
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hilcodec_amd.h")).read(), flags=re.S)
    header, env = {}, {}
    for name, expr in re.findall(r"^#define (HILC_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        env[name] = eval(re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]\b", r"\1", expr), {"__builtins__": {}}, env)
        m = re.match(r"HILC_(%s)_(\w+)$" % "|".join(mod.upper() for mod in modules), name)
        if m:
            assert (m.group(1).lower(), m.group(2)) not in header, name
            header[m.group(1).lower(), m.group(2)] = env[name]
    python = {}
    for mod in modules:
        module = importlib.import_module("hilcodec_amd." + mod)
        for node in ast.parse(open(module.__file__).read()).body:
            if isinstance(node, ast.Assign):
                for leaf in ast.walk(node.targets[0]):
                    if isinstance(leaf, ast.Name) and leaf.id.isupper() and not leaf.id.startswith("_") and leaf.id not in HOST_ONLY:
                        value = getattr(module, leaf.id)
                        if isinstance(value, int) and not isinstance(value, bool):
                            python[mod, leaf.id] = value
    assert len(header) >= 90                                                # the regular expression found the section
    assert sorted(set(header) - set(python)) == [], "in the header, not in Python"
    assert sorted(set(python) - set(header)) == [], "in Python, not in the header"
    for key, value in header.items():
        assert python[key] == value, key
    from hilcodec_amd import dtx, report, wire
    for K in range(dtx.MAX_ORDER + 1):
        assert dtx.state_words(K) == env["HILC_DTX_ST_Q"] + 2 * K
    assert report.RP_WORDS == env["HILC_REPORT_RP_WORDS"] == env["HILC_REPORT_RP_RING"] + env["HILC_REPORT_RP_RING_WORDS"]
    assert 16 * report.RP_RING_WORDS == 256                                # the widest ReportConfig.window, 2 bits per hop
    # the conceal row: the three words before the codes, then one code per stage (GraphedDecodeHop allocates n + CONCEAL_CODES)
    assert (wire.CONCEAL_RUN, wire.CONCEAL_HAS, wire.CONCEAL_N) == tuple(range(env["HILC_WIRE_CONCEAL_CODES"]))
    # every row is a dense prefix of its width: no two words of a row share an index
    for mod, pre, width in (("jitter", ("ST_", "STAT_"), "ST_WORDS"), ("jitter", ("AD_",), "AD_WORDS"), ("report", ("FA_",), "FA_WORDS")):
        words = sorted(v for (m_, n_), v in header.items() if m_ == mod and n_.startswith(pre) and n_ != width)
        assert words == list(range(header[mod, width])), (mod, pre)


@pytest.mark.parametrize("name", ["hil_speech", "hil_music"])
def test_synth_streaming_model_is_the_one_recipe(name):
    """synth.streaming_model: eval mode, the same tensors on every call, the model stream_driver builds without a checkpoint,
    and a given state dict in place of the seed's"""
    from hilcodec_amd import stream_driver

    def same(a, b):
        a, b = a.state_dict(), b.state_dict()
        return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)

    m = synth.streaming_model(name)
    assert not m.training and not any(sub.training for sub in m.modules())
    assert same(m, synth.streaming_model(name))
    assert same(m, stream_driver.build_streaming_model(name, None, "cpu"))
    assert same(synth.streaming_model(name, state_dict=synth.synth_state_dict(name, 3)), synth.streaming_model(name, seed=3))
    assert not same(m, synth.streaming_model(name, seed=3))


def test_error_codes_without_gpu():
    """Argument validation happens before any launch, so it can be exercised on a CPU-only box."""
    from hilcodec_amd._lib import lib
    assert lib.hilc_pw_conv(None, None, None, None, None, 1, 8, 8, 8, 1.0, 0, 1.0, None) == -2      # NULL
    one = ctypes.c_void_p(16)
    assert lib.hilc_pw_conv(one, one, None, None, one, 0, 8, 8, 8, 1.0, 0, 1.0, None) == -1          # shape
    assert lib.hilc_pw_conv(one, one, None, None, one, 1, 8, 6, 8, 1.0, 0, 1.0, None) == -4          # unsupported
    assert lib.hilc_rvq_encode(one, one, one, one, one, None, None, 1, 128, 4, 1024, 8, 9, 0, 0, 0, None) == -5
    assert lib.hilc_rvq_encode(one, one, one, one, one, None, None, 1, 128, 4, 1024, 8, 0, 0, 0, 0, None) == -5
    # an unknown bit of `flags` (ABI 15) is refused, not ignored
    assert lib.hilc_rvq_encode(one, one, one, one, one, None, None, 1, 128, 4, 1024, 8, 8, 0, 0, 2, None) == -4
    assert lib.hilc_resblock_supported(96, 24000) == 1 and lib.hilc_resblock_supported(768, 600) == 1 and lib.hilc_resblock_supported(1024, 600) == 0
    from hilcodec_amd import ops
    for c in (32, 64, 80, 96, 128, 160, 192, 256, 768):          # the traceable Python mirror agrees with the library
        for t in (4, 75, 120, 600, 24000):
            assert ops.resblock_supported(c, t) == bool(lib.hilc_resblock_supported(c, t))
    for c in (32, 64, 96, 128, 192, 256, 320, 384, 512, 640, 768, 1024):       # ... and so does its streaming half
        for t in (1, 4, 8, 12, 16, 32, 40, 64, 160, 320):
            assert ops.resblock_supported(c, t, 4, streaming=True) == bool(lib.hilc_resblock_stream_supported(c, t)), (c, t)
    assert not ops.resblock_supported(768, 8, 1 << 18, streaming=True)          # flat 32-bit column space
    # the stage launches (round 4): chains, encoder / decoder stages, and the row split of their packed weights
    widths = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
    for c in widths:
        assert ops.resblock_chain_row_classes(c, True) == (lib.hilc_resblock_chain_row_classes(c) or 2), c
        assert ops.resblock_chain_row_classes(c, False) == (lib.hilc_resblock_chain_row_classes_offline(c) or 1), c
        for t in (4, 8, 20, 40, 75, 160, 320, 600, 3000):
            for n in (1, 2, 3, 4):
                for st in (0, 1):
                    assert ops.resblock_chain_supported(c, t, n, 2, streaming=bool(st)) == bool(lib.hilc_resblock_chain_supported(c, t, n, st)), (c, t, n, st)
                    for r in (2, 4, 5, 8):
                        assert ops.encoder_stage_supported(c, t, n, r, 2, streaming=bool(st)) == bool(lib.hilc_encoder_stage_supported(c, t, n, r, st)), (c, t, n, r, st)
                        assert ops.decoder_stage_supported(c, t, n, r, 2, streaming=bool(st)) == bool(lib.hilc_decoder_stage_supported(c, t, n, r, st)), (c, t, n, r, st)
    # ... and the round-5 forms that take the model's two ends into the first / last stage launch, plus their NULL / shape checks
    for c in (64, 96, 192):
        for t in (4, 75, 124, 24000):
            for n in (1, 2, 3):
                for r in (2, 4):
                    for k in (5, 7):
                        assert ops.decoder_stage_post_supported(c, t, n, r, k) == bool(lib.hilc_decoder_stage_post_supported(c, t, n, r, k)), (c, t, n, r, k)
                        for st in (0, 1):
                            assert ops.encoder_stage0_supported(t, n, r, c, 1, k, 1, bool(st)) == bool(lib.hilc_encoder_stage0_supported(t, n, r, c, 1, k, st)), (t, n, r, c, k, st)
    assert lib.hilc_decoder_stage_post(None, None, 3, None, 0, 1, 96, 8, None) == -2 and lib.hilc_encoder_stage0(None, None, 2, None, 0, 1, 8, None) == -2
    assert lib.hilc_resblock(one, one, one, one, one, one, one, one, 1, 96, 16, 1.0, 1.0, None) == -4  # y aliases x


def test_stage_limit_is_refused_at_33_and_passed_at_32():
    """csrc/slot.h MAX_N = 32 is the one staging limit of the packet kernels: every launcher that checks it answers unsupported (-4)
    to n_max + m = 33 (or n_max = 33) and lets 32 past that check.  Argument checks only, no kernel is launched: the 32-stage calls
    carry a hop of 2^25 frames, whose packet row the check behind the limit refuses as a shape (-1) — the same call with one frame
    and 33 stages reaches the limit, so nothing before it objects.  hilc_rvq_decode_packed and hilc_vbr_select check nothing behind
    the limit (32 stages would launch), so only their refusal of 33 is asserted."""
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)
    big = 1 << 25

    def fec_pack(n, m, T):
        return lib.hilc_pack_codes_10bit_fec(p, None, p, q, None, None, p, p, 1, T, n, m, None)

    def fec_select(n, m, T):
        return lib.hilc_fec_select(p, p, p, p, 1, T, n, m, None)

    def header(n, m, T):
        return lib.hilc_packet_header(p, p, None, None, None, None, p, q, p, p, 1, T, n, m, None)

    def jitter(n, m, T):
        return lib.hilc_jitter_step(p, p, 0, None, p, p, None, p, p, p, p, p, 1, T, n, m, -1, 0, 2, 8, None)

    def jitter_adapt(n, m, T):
        return lib.hilc_jitter_adapt_step(p, p, 0, None, p, p, None, p, p, p, p, p, 1, T, n, m, -1, 0, 2, 8, p, 1, 2, 4, 2, 0, None)

    for call in (fec_pack, fec_select, header, jitter, jitter_adapt):
        assert call(31, 2, 1) == -4, call.__name__
        assert call(30, 2, big) == -1, call.__name__
    assert lib.hilc_conceal_prepare(p, p, p, p, p, p, p, 1, 1, 33, 4, None) == -4
    assert lib.hilc_conceal_prepare(p, p, p, p, p, p, p, 1, big, 32, 4, None) == -1
    assert lib.hilc_rvq_decode_packed(p, None, p, p, 1, 128, 1, 1024, 33, 33, None) == -4
    assert lib.hilc_vbr_select(p, p, p, None, None, None, None, p, p, 1, 1, 128, 1024, 33, 33, 1, 0.5, 0, 0, 0, None) == -4


def test_cpu_tensors_raise():
    import hilcodec_amd
    from hilcodec_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pw_conv(torch.zeros(1, 8, 8), torch.zeros(8, 8))
    mk = synth.model_kwargs("hil_speech")
    m = hilcodec_amd.HILCodec(24000, 1, **mk).eval()
    with pytest.raises(RuntimeError):
        m.encoder(torch.zeros(1, 1, 640))


def test_offline_module_tree_matches_reference_keys():
    import hilcodec_amd
    for name in ("hil_speech", "hil_music"):
        mk = synth.model_kwargs(name)
        m = hilcodec_amd.HILCodec(24000, 1, **mk)
        own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith("_extra_state")}
        assert own == synth.offline_param_shapes(mk)          # same keys, same order, same shapes
        assert sum(p.numel() for p in m.parameters()) == 9577019
        assert m.encoder.hop_length == 320 and m.decoder.hop_length == 320 and m.sample_rate == 24000
        assert m.encoder.dimension == 128 and m.encoder.ratios == [2, 4, 5, 8] and m.decoder.ratios == [8, 5, 4, 2]
        # a freshly built model has kmeans_init codebooks marked un-initialised, like the reference
        assert not m.quantizer.layers[0].initted and m.quantizer.layers[0].get_extra_state() == {"initted": False}


def test_unsupported_options_fail_loudly():
    import hilcodec_amd
    mk = synth.model_kwargs("hil_speech")
    for bad in (dict(skip="1x1"), dict(causal=False), dict(dilation_base=2), dict(norm="spectral_norm"),
                dict(vq="ResidualGainShapeVQ"), dict(act_all=True)):
        with pytest.raises((NotImplementedError, ValueError, AssertionError)):
            hilcodec_amd.HILCodec(24000, 1, **{**mk, **bad})
    with pytest.raises(RuntimeError):
        hilcodec_amd.HILCodec(24000, 1, **{**mk, "expansion": 2, "groups": 4})


def test_weight_folds_bit_exact():
    from hilcodec_amd import fold
    from hilcodec_amd.models.hilcodec.modules import SConv1d
    from oracle import hilcodec_oracle as O
    v = torch.from_numpy(synth.normalish(1, 24 * 7 * 5)).view(24, 7, 5)
    g = torch.from_numpy(synth.uniform(2, 24, 0.5, 1.5)).view(24, 1, 1)
    assert torch.equal(fold.weight_norm_fold(v, g), torch._weight_norm(v, g, 0))
    assert torch.equal(fold.weight_standardization_fold(v, g, torch.tensor([1.3])),
                       O.fold_weight_standardization(v, g, torch.tensor([1.3])))
    m = SConv1d(7, 24, 1, norm="weight_norm", bias=True)
    with torch.no_grad():
        m.conv.conv.weight_v.copy_(v[:, :, :1]); m.conv.conv.weight_g.copy_(g)
    w0 = m.conv.conv.effective_weight()
    m.conv.conv.remove_reparameterization()
    assert "conv.conv.weight" in m.state_dict() and "conv.conv.weight_g" not in m.state_dict()
    assert torch.equal(m.conv.conv.effective_weight(), w0)
    basis = synth.stft_basis(64)
    bt = fold.stft_basis_layout(basis)
    assert bt.shape == (64, 96) and torch.equal(bt[:, 0], basis[0, 0]) and torch.equal(bt[:, 1], basis[33, 0])
    assert torch.equal(bt[:, 64], basis[32, 0]) and torch.equal(bt[:, 65], basis[65, 0]) and not bt[:, 66:].any()
    cb, cbt, norms = fold.codebook_tables([v[:, :, 0], v[:, :, 1]])
    assert cb.shape == (2, 24, 7) and torch.equal(cbt[1], v[:, :, 1].t()) and torch.equal(norms[0], v[:, :, 0].t().pow(2).sum(0))


def test_streaming_module_tree_and_mapping():
    from hilcodec_amd.models.hilcodec.streaming import HILCodec
    from oracle import hilcodec_oracle as O
    full = synth.model_kwargs("hil_speech")
    m = HILCodec(24000, **synth.streaming_kwargs("hil_speech")).eval()
    x = torch.zeros(5, 1)
    ce, cd = m.initialize_cache(x)
    enc_shapes, dec_shapes = O.stream_cache_shapes(full)
    assert [tuple(c.shape) for c in ce] == [(5, c, l) for c, l in enc_shapes]
    assert [tuple(c.shape) for c in cd] == [(5, c, l) for c, l in dec_shapes]
    assert m.encoder.num_cache == 22 and not any(c.any() for c in ce + cd)
    sd = synth.synth_state_dict("hil_speech", seed=7)
    m.load_offline_state_dict(sd)
    assert m.decoder.blocks[0][2].pre_scale == 1.0 and m.encoder.blocks[0][1].pre_scale == (1 + 2 * 0.5773502691896258 ** 2) ** -0.5
    m.remove_weight_reparameterizations()
    p = O.stream_prepare(sd, full)
    # merge_scaling reproduces the reference's algebra bit for bit (oracle == reference, tests/test_oracle_*)
    assert torch.equal(m.encoder.conv_pre.weight.data, p["enc.conv_pre.weight"])
    assert torch.equal(m.encoder.spec_post.layer.weight.data, p["enc.spec_post.layer.weight"])
    assert torch.equal(m.encoder.spec_post.layer.bias.data, p["enc.spec_post.layer.bias"])
    assert torch.equal(m.encoder.blocks[2][1].block[1].depthwise.weight.data, p["enc.blocks.2.1.1.dw.weight"])
    assert torch.equal(m.decoder.blocks[3][2].block[1].depthwise.bias.data, p["dec.blocks.3.2.1.dw.bias"])
    assert torch.equal(m.decoder.conv_post.weight.data, p["dec.post.weight"])
    assert torch.equal(m.decoder.conv_post.bias.data, p["dec.post.bias"])
    assert torch.equal(m.dequantizer.layers[3].embed, sd["quantizer.layers.3.embed"])


def test_legacy_rvq_matches_reference_constructor_and_state_dict():
    """`modules/vector_quantize.py` (row a9): same ctor signatures, buffers and return arity as the reference; a real
    reference state_dict's key/shape layout and the constructor signatures are the stored ones (tests/golden/vs_reference.npz),
    and the key/shape contract is checked against a literal too."""
    from hilcodec_amd.modules.vector_quantize import EuclideanCodebook, ResidualVQ, VectorQuantize
    kw = dict(num_quantizers=3, dropout=True, dropout_index=[1, 3], dim=16, codebook_size=32, kmeans_init=False,
              kmeans_iters=20, decay=0.9, eps=1e-7, ema_num_threshold=0.5, ema_num_initial=2.0, commitment=0.25,
              channel_last=False)
    own = ResidualVQ(**kw)
    keys = {k: tuple(v.shape) for k, v in own.state_dict().items()}
    want = {}
    for i in range(3):
        for name, shape in (("initted", (1,)), ("embed", (32, 16)), ("ema_embed", (32, 16)), ("ema_num", (32,))):
            want[f"layers.{i}._codebook.{name}"] = shape
    assert keys == want
    cbk = own.layers[0]._codebook
    assert torch.equal(cbk.ema_embed, cbk.embed * 2.0) and torch.equal(cbk.ema_num, torch.full((32,), 2.0))
    assert own.layers[0].commitment == 0.25 and own.layers[0].gradient_flow is False and own.dropout_index == [1, 3]
    # options this path does not implement are refused, unknown ones are a TypeError as in the reference
    with pytest.raises(NotImplementedError):
        VectorQuantize(use_shape_gain=True, dim=16, codebook_size=32)
    with pytest.raises(TypeError):
        VectorQuantize(dim=16, codebook_size=32, threshold_ema_dead_code=2.0)
    with pytest.raises(TypeError):
        EuclideanCodebook(16, 32, bogus=1)
    # un-initialised k-means codebooks never quantise against zeros silently
    lazy = ResidualVQ(num_quantizers=2, dim=16, codebook_size=32, kmeans_init=True).eval()
    assert not bool(lazy.layers[0]._codebook.initted)
    with pytest.raises(RuntimeError, match="not initialised"):
        lazy(torch.zeros(1, 16, 4))
    with pytest.raises(AssertionError):
        own.eval()(torch.zeros(1, 16, 4), 4)
    # the reference's own ResidualVQ(**kw) state_dict layout and constructor signatures (tests/golden/vs_reference.npz)
    import inspect
    import json
    ref = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "vs_reference.npz"))["meta_json"]))
    assert [[k, list(v.shape)] for k, v in own.state_dict().items()] == ref["legacy_vq_state_dict_shapes"]
    for cls in (EuclideanCodebook, VectorQuantize, ResidualVQ):
        pa, pb = inspect.signature(cls.__init__).parameters, {k: (has, d) for k, has, d in ref["legacy_vq_signatures"][cls.__name__]}
        assert list(pa) == list(pb), (cls.__name__, list(pa), list(pb))
        empty = inspect.Parameter.empty
        assert all((pa[k].default is not empty, None if pa[k].default is empty else pa[k].default) == pb[k]
                   for k in pa if k not in ("self", "kwargs")), cls.__name__
    assert list(inspect.signature(VectorQuantize.forward).parameters) == ref["legacy_vq_signatures"]["VectorQuantize.forward"]


def test_scalar_n_accepts_any_integer_like():
    """`n` from config arithmetic (numpy ints, 0-dim arrays / tensors) is a scalar n, not a per-clip list."""
    from hilcodec_amd import ops
    for n in (3, np.int64(3), np.int32(3), np.array(3), torch.tensor(3), True + 2):
        assert ops.per_clip_n(n, 5, 8, torch.device("cpu")) == (3, None)
    rows, per = ops.per_clip_n([1, 2, 8, 2, 1], 5, 8, torch.device("cpu"))
    assert rows == 8 and per.dtype == torch.int32 and per.tolist() == [1, 2, 8, 2, 1]
    rows, per = ops.per_clip_n(np.array([4]), 1, 8, torch.device("cpu"))       # a 1-element LIST is per-clip (B = 1)
    assert rows == 4 and per.tolist() == [4]
    with pytest.raises(AssertionError):
        ops.per_clip_n([1, 9], 2, 8, torch.device("cpu"))
    with pytest.raises(RuntimeError):
        ops.per_clip_n([1, 2], 3, 8, torch.device("cpu"))


def test_dws_conv_stream_mirror_knows_which_long_hops_take_a_shortcut():
    """ops.dws_conv_stream_supported(..., has_res): hilc_dws_conv_stream adds `res` on long hops (T > 128) only in its flat-tile form —
    stride <= 8, fewer than 2^31 outputs; the engine asks the mirror before it hands the SpecBlock branch to the layer."""
    from hilcodec_amd import ops
    assert ops.dws_conv_stream_supported(320, 4, 2, True, 1024, 128) and ops.dws_conv_stream_supported(160, 8, 4, True, 1024, 256)
    assert ops.dws_conv_stream_supported(320, 32, 16) and not ops.dws_conv_stream_supported(320, 32, 16, True)       # stride 16: no shortcut
    assert ops.dws_conv_stream_supported(360, 18, 9) and not ops.dws_conv_stream_profitable(360, 18, 9, True, 4, 64)
    assert not ops.dws_conv_stream_supported(320, 4, 2, True, 1 << 24, 128)                                           # 2^31 outputs
    assert ops.dws_conv_stream_supported(40, 10, 5, True) and ops.dws_conv_stream_supported(8, 16, 8, True)         # short hops: whole-clip tiles
    # long hops run on the linear-addressing core only: an x [B,K,T] of 2^32 bytes is refused (csrc/gemm.hip: lin_ok), with or without a shortcut
    assert ops.dws_conv_stream_supported(160, 8, 4, True, 419430, 32, 16) and not ops.dws_conv_stream_supported(160, 8, 4, True, 419431, 32, 16)
    assert ops.dws_conv_stream_supported(160, 8, 4, False, 419430, 32, 16) and not ops.dws_conv_stream_profitable(160, 8, 4, False, 419431, 32, 16)
    assert ops.dws_conv_stream_supported(8, 16, 8, True, 1 << 24, 1024, 512)                                         # short hops fall back to the generic core


def test_exec_options_are_launch_structure_only():
    """engine.ExecOptions: four booleans that select launches, never arithmetic (the split-bf16 decoder mode and the rejected launch
    variants left the library in round 5); nothing process-global."""
    import dataclasses
    from hilcodec_amd import engine
    fields = dataclasses.fields(engine.ExecOptions)
    assert [f.name for f in fields] == ["stage_launches", "wide_blocks", "decoder_stage_narrow", "stream_defer_spec"]
    assert all(f.type in (bool, "bool") and f.default is True for f in fields)
    assert not hasattr(engine, "DECODER_GEMM") and not hasattr(engine, "SIDE_STREAM")     # no process-global switches
    with engine.exec_overrides(decoder_stage_narrow=False):
        assert engine._effective(engine.ExecOptions()).decoder_stage_narrow is False
    assert engine._effective(engine.ExecOptions()).decoder_stage_narrow is True
    with pytest.raises(TypeError):
        with engine.exec_overrides(decoder_gemm="bf16x3"):
            engine._effective(engine.ExecOptions())


def test_clip_chunks_keep_activations_below_32bit_offsets():
    """engine: an offline batch whose largest activation would reach 4 GiB runs as the fewest equal clip chunks below it"""
    from hilcodec_amd import engine
    per_clip = 96 * 24000
    assert engine._clip_chunks(256, per_clip) == [(0, 256)]
    assert engine._clip_chunks(512, per_clip) == [(0, 256), (256, 512)]
    for b in (467, 1000, 2048):
        ch = engine._clip_chunks(b, per_clip)
        assert ch[0][0] == 0 and ch[-1][1] == b and all(a[1] == c[0] for a, c in zip(ch, ch[1:]))
        assert all((hi - lo) * per_clip * 4 < 2 ** 32 for lo, hi in ch) and max(hi - lo for lo, hi in ch) - min(hi - lo for lo, hi in ch) <= len(ch)
    assert engine._clip_chunks(4, 2 ** 31) == [(0, 1), (1, 2), (2, 3), (3, 4)]          # a single clip above the limit still runs: the fused offline stage launches take any size, the launches outside them the generic cores (tests/test_gpu_large.py)


def test_streaming_model_takes_a_weight_standardised_checkpoint(golden):
    """`load_offline_state_dict(sd, norm="weight_standardization", norm_kwargs=...)`: every conv folded to a plain weight
    with the reference's expression (`modules/weight_standardization.py:30-41`) — the streaming classes themselves know
    weight_norm only, like the reference's (`causal_layers.py:200-204`)."""
    import torch
    from hilcodec_amd import synth
    from hilcodec_amd.models.hilcodec.streaming import HILCodec as S
    g = golden("ws_hil_speech")
    mk = synth.streaming_kwargs("hil_speech")
    sd = synth.synth_state_dict("hil_speech", seed=int(g["weight_seed"]))
    with pytest.raises(ValueError):
        S(24000, norm="weight_standardization", **mk)
    m = S(24000, **mk).eval()
    with pytest.raises(ValueError):
        m.load_offline_state_dict(sd, norm="spectral_norm")
    m.load_offline_state_dict(sd, norm="weight_standardization", norm_kwargs={"eps": float(g["ws_eps"]), "scale": float(g["ws_scale"])})
    keys = m.state_dict()
    assert "decoder.upsample_depthwise.0.weight" in keys and "decoder.upsample_depthwise.0.weight_g" not in keys
    assert torch.equal(keys["decoder.upsample_depthwise.0.weight"], torch.from_numpy(g["fold_probe_convtr"]))
    assert torch.equal(keys["encoder.blocks.1.0.block.0.pointwise.1.weight"], torch.from_numpy(g["fold_probe_pw"]))
    m.remove_weight_reparameterizations()               # hooks are gone already; merge_scaling still runs
    assert "encoder.spec_post.layer.bias" in m.state_dict()
