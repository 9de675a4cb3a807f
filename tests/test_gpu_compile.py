"""GPU: the module classes are traceable — `torch.compile(fullgraph=True)` of the offline encoder / decoder and of a
streaming hop produces bit-identical outputs to eager execution (same custom ops, same launches), i.e. the boundary
really is "PyTorch-ROCm custom ops"  and not Python that only runs eagerly."""
import pytest
import torch

from hilcodec_amd import synth

pytestmark = pytest.mark.gpu


def _run(_unused, mod, *args, **kw):
    """inductor if this box can run it (the graph holds only custom ops, so it has nothing to fuse), else the
    reference-tracing backend: both go through dynamo + fake-tensor propagation with fullgraph=True."""
    last = None
    for backend in ("inductor", "aot_eager"):
        import torch._dynamo
        torch._dynamo.reset()
        c = torch.compile(mod, fullgraph=True, backend=backend)
        try:
            with torch.no_grad():
                return c(*args, **kw), backend
        except torch._dynamo.exc.BackendCompilerFailed as e:       # inductor toolchain missing on the box
            last = e
            continue
    raise last


def test_offline_encoder_decoder_compile_fullgraph():
    import hilcodec_amd
    dev = torch.device("cuda:0")
    mk = synth.model_kwargs("hil_speech")
    model = hilcodec_amd.HILCodec(24000, 1, **mk).eval()
    model.load_state_dict(synth.synth_state_dict("hil_speech", seed=7), strict=False)
    for l in model.quantizer.layers:
        l.initted = True
    x = synth.synth_clips(3, 9600, seed=5).to(dev)
    model.encoder.prepare(dev)
    model.decoder.prepare(dev)
    with torch.no_grad():
        z = model.encoder(x)
        q, _, _, idx = model.quantizer(z, None, return_indices=True)
        wav = model.decoder(q)
    z_c, be = _run(None, model.encoder, x)
    wav_c, bd = _run(None, model.decoder, q)
    print(f"backends: encoder {be}, decoder {bd}")
    assert torch.equal(z_c, z) and torch.equal(wav_c, wav)
    # another shape re-traces (static shapes) and still matches
    x2 = synth.synth_clips(2, 4800, seed=6).to(dev)
    with torch.no_grad():
        z2 = model.encoder(x2)
    z2_c, _ = _run(None, model.encoder, x2)
    assert torch.equal(z2_c, z2)


def test_streaming_hop_compile_fullgraph_with_state_block():
    from hilcodec_amd.graph_step import StateBlock
    dev = torch.device("cuda:0")
    m = synth.streaming_model()
    B = 4
    x = synth.synth_clips(B, 640, seed=9).to(dev)
    ce, cd = m.initialize_cache(x)
    with torch.no_grad():
        z0, ce1 = m.encoder(x[:, :, :320].contiguous(), *ce)                 # eager, fresh cache tensors
        z1, _ = m.encoder(x[:, :, 320:].contiguous(), *ce1)
    # compiled hop writing into a persistent state block (mutated custom-op arguments under functionalisation)
    a, b = StateBlock(m, B, dev), StateBlock(m, B, dev)

    def hop(xin, *caches_and_out):
        n = len(caches_and_out) // 2
        return m.encoder(xin, *caches_and_out[:n], cache_out=list(caches_and_out[n:]))

    (zc0, _), backend = _run(None, hop, x[:, :, :320].contiguous(), *a.enc, *b.enc)
    (zc1, _), _ = _run(None, hop, x[:, :, 320:].contiguous(), *b.enc, *a.enc)
    print("backend:", backend)
    assert torch.equal(zc0, z0) and torch.equal(zc1, z1)
    for got, want in zip(b.enc, ce1):
        assert torch.equal(got, want)
