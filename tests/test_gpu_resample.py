"""GPU: the sample-rate converter (csrc/resample.hip, hilcodec_amd/resample.py) and the graphed sender and receiver that run it.
The kernel against the torch statement of its definition (resample.reference) in every direction, streaming against offline, the
op under torch.compile and in a captured graph, GraphedEncodeHop(input_rate=) against a 24 kHz sender fed the reference's output,
GraphedDecodeHop(output_rate=) against a 24 kHz receiver followed by the streaming reference, the history in sessions, holds and
concealment, and the driver's resampling step — every comparison bit for bit (torch.equal)."""
import numpy as np
import pytest
import torch

from hilcodec_amd import ops, synth
from hilcodec_amd.resample import BASE_RATE, RATES, Resampler, design, device_taps, hop_samples, reference, resample

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HOP = 320
MULTIPLE = {8000: 3, 16000: 3, 22050: 1, 32000: 3, 44100: 1, 48000: 1}
DIRECTIONS = [(r, BASE_RATE) for r in RATES] + [(BASE_RATE, r) for r in RATES]


@pytest.fixture(scope="module")
def speech():
    return synth.streaming_model()


def hop_in(a, b, frames):
    return 320 * frames if a == BASE_RATE else hop_samples(frames, a)


def signal(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, T, generator=g) * 2 - 1).contiguous()


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("a,b", DIRECTIONS)
@pytest.mark.parametrize("B", [1, 3, 64])
def test_kernel_equals_reference(a, b, B):
    s = design(a, b)
    taps = device_taps(s, DEV)
    rate = a if a != BASE_RATE else b
    aligned = 2 * hop_in(a, b, MULTIPLE[rate])
    for T in (aligned, 1237, 5):
        x = signal(B, T, a + b + T + B)
        g = torch.Generator().manual_seed(T)
        hist = torch.randn(B, 1, s.Q - 1, generator=g) * 0.5
        for h in (None, hist):
            y_ref, h_ref = reference(x, s, h)
            hin = None if h is None else h.to(DEV)
            hout = torch.full((B, 1, s.Q - 1), 7.0, device=DEV)
            y = ops.resample_poly(x.to(DEV), taps, s.L, s.M, hist=hin, hist_out=hout)
            assert tuple(y.shape) == tuple(y_ref.shape), (T, h is None)
            assert torch.equal(y.cpu(), y_ref), (T, h is None)
            assert torch.equal(hout.cpu(), h_ref), (T, h is None)
            if hin is not None:
                assert torch.equal(hin.cpu(), hist)                    # read-only
            y2 = ops.resample_poly(x.to(DEV), taps, s.L, s.M, hist=hin)   # no hist_out: nothing else written
            assert torch.equal(y2.cpu(), y_ref)


@pytest.mark.parametrize("a,b", DIRECTIONS)
def test_streaming_equals_offline(a, b):
    s = design(a, b)
    rate = a if a != BASE_RATE else b
    n = hop_in(a, b, MULTIPLE[rate])
    B, hops = 3, 5
    x = signal(B, n * hops + 11, a * 3 + b).to(DEV)
    full = resample(x, a, b)
    r = Resampler(a, b, B, DEV)
    parts = [r(x[:, :, i * n:(i + 1) * n].contiguous()) for i in range(hops)] + [r(x[:, :, hops * n:].contiguous())]
    assert torch.equal(torch.cat(parts, dim=2), full)
    assert tuple(full.shape) == (B, 1, s.out_len(x.shape[-1]))
    assert torch.equal(r.history, x[:, :, x.shape[-1] - (s.Q - 1):])
    assert resample(x, BASE_RATE, BASE_RATE) is x


def test_op_compiles_and_captures():
    s = design(44100, BASE_RATE)
    taps = device_taps(s, DEV)
    B, T = 4, 588
    x = signal(B, T, 5).to(DEV)
    h0 = (torch.randn(B, 1, s.Q - 1) * 0.3).to(DEV)
    exp, exp_h = reference(x, s, h0)

    def fn(x, h, h_out):
        return ops.resample_poly(x * 1.0, taps, s.L, s.M, hist=h, hist_out=h_out) + 0.0

    h_out = torch.zeros_like(h0)
    y = torch.compile(fn, fullgraph=True)(x, h0, h_out)
    assert torch.equal(y.cpu(), exp) and torch.equal(h_out.cpu(), exp_h)

    xs, hs, ho = x.clone(), h0.clone(), torch.zeros_like(h0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.resample_poly(xs, taps, s.L, s.M, hist=hs, hist_out=ho)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = ops.resample_poly(xs, taps, s.L, s.M, hist=hs, hist_out=ho)
    x2 = signal(B, T, 6)
    xs.copy_(x2.to(DEV))
    ho.zero_()
    g.replay()
    torch.cuda.synchronize()
    e2, e2_h = reference(x2, s, h0)
    assert torch.equal(yg.cpu(), e2) and torch.equal(ho.cpu(), e2_h)


# ---------------------------------------------------------------- the graphed sender
@pytest.mark.parametrize("rate", [48000, 44100, 16000])
def test_sender_input_rate(speech, rate):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    frames = MULTIPLE[rate] if rate == 16000 else 1
    B, n_in = 3, hop_samples(frames, rate)
    s = design(rate, BASE_RATE)
    rs = GraphedEncodeHop(speech, B, HOP * frames, 8, DEV, input_rate=rate)
    plain = GraphedEncodeHop(speech, B, HOP * frames, 8, DEV)
    x = signal(B, n_in * 4, rate)
    hist = None
    for h in range(4):
        chunk = x[:, :, h * n_in:(h + 1) * n_in].contiguous()
        y24, hist = reference(chunk, s, hist)
        pk, nb = rs.step(chunk.to(DEV))
        pk0, nb0 = plain.step(y24.to(DEV))
        assert torch.equal(pk, pk0) and torch.equal(nb, nb0), h
        assert torch.equal(rs.indices, plain.indices), h
    assert torch.equal(rs.cache_enc[-1].cpu(), hist)
    with pytest.raises(ValueError, match="multiple of 3"):
        GraphedEncodeHop(speech, B, HOP, 8, DEV, input_rate=16000)
    with pytest.raises(ValueError):
        GraphedEncodeHop(speech, B, HOP, 8, DEV, input_rate=11025)


def random_packets(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 1024, (8, B, T), generator=g).to(DEV)
    return ops.pack_codes_10bit(idx)[0]


# ---------------------------------------------------------------- the graphed receiver
@pytest.mark.parametrize("rate", [48000, 16000])
def test_receiver_output_rate(speech, rate):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    frames = MULTIPLE[rate]
    B = 3
    s = design(BASE_RATE, rate)
    rs = GraphedDecodeHop(speech, B, frames, 8, DEV, output_rate=rate)
    plain = GraphedDecodeHop(speech, B, frames, 8, DEV)
    hist = None
    for h in range(4):
        pk = random_packets(B, frames, 100 * rate + h)
        y = rs.step(pk, [8] * B).cpu()
        exp, hist = reference(plain.step(pk, [8] * B), s, hist)
        assert tuple(y.shape) == (B, 1, hop_samples(frames, rate))
        assert torch.equal(y, exp), h
    assert torch.equal(rs.cache_dec[-1].cpu(), hist)
    with pytest.raises(ValueError, match="multiple of 3"):
        GraphedDecodeHop(speech, B, 1, 8, DEV, output_rate=8000)


def test_rate_24000_is_the_plain_graph(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop, GraphedEncodeHop
    B = 2
    a = GraphedEncodeHop(speech, B, HOP, 8, DEV, sessions=True, input_rate=24000)
    b = GraphedEncodeHop(speech, B, HOP, 8, DEV, sessions=True)
    ra = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, output_rate=24000)
    rb = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True)
    x = signal(B, HOP * 3, 77).to(DEV)
    for h in range(3):
        chunk = x[:, :, h * HOP:(h + 1) * HOP].contiguous()
        pa, na = a.step(chunk)
        pb, nb = b.step(chunk)
        assert torch.equal(pa, pb) and torch.equal(na, nb) and torch.equal(a.indices, b.indices)
        assert torch.equal(ra.step(pa, [8] * B), rb.step(pb, [8] * B))
    assert len(a.export(1)) == 22 and len(ra.export(1)) == 30
    assert a.x.shape[-1] == HOP and a.rs is None and ra.rs is None


# ---------------------------------------------------------------- sessions, holds and concealment
def test_sender_sessions_and_holds(speech):
    from hilcodec_amd.graph_step import GraphedEncodeHop
    rate, B = 48000, 4
    n_in = hop_samples(1, rate)
    s = GraphedEncodeHop(speech, B, HOP, 8, DEV, sessions=True, input_rate=rate)
    x = signal(B, n_in * 8, 12).to(DEV)

    def chunk(h):
        return x[:, :, h * n_in:(h + 1) * n_in].contiguous()

    for h in range(3):
        s.step(chunk(h))
    rec = s.export(1)
    assert len(rec) == 23 and tuple(rec[-1].shape) == (1, 1, design(rate, BASE_RATE).Q - 1)
    assert torch.equal(rec[-1], chunk(2)[1:2, :, n_in - rec[-1].shape[-1]:])
    # resume stream 1 at slot 3 mid-stream: from then on slot 3 fed stream 1's samples equals slot 1
    s.start(3, [c.cpu() for c in rec])
    for h in range(3, 6):
        c = chunk(h)
        c[3] = c[1]
        pk, nb = s.step(c)
        assert torch.equal(pk[3], pk[1]) and torch.equal(nb[3], nb[1]) and torch.equal(s.indices[:, 3], s.indices[:, 1]), h
    # hold and stop: every cache (the history included) unchanged, the output rows 0
    before0, before2 = s.export(0), s.export(2)
    s.stop(2)
    pk, nb = s.step(chunk(6), hold=[0])
    assert int(nb[0]) == 0 and int(nb[2]) == 0 and not pk[0].any() and not pk[2].any() and int(nb[1]) > 0
    for a_, b_ in ((s.export(0), before0), (s.export(2), before2)):
        assert len(a_) == 23 and all(torch.equal(p, q) for p, q in zip(a_, b_))
    s.start(2)
    s.step(chunk(7))
    assert not s.export(2)[-1].eq(0).all()
    s.start(2)
    s.step(chunk(7), hold=[2])                        # a fresh start held on its first hop: zero history
    assert s.export(2)[-1].eq(0).all()


def test_receiver_sessions_resume(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    rate, B = 16000, 3
    r = GraphedDecodeHop(speech, B, 3, 8, DEV, sessions=True, output_rate=rate)
    pks = [random_packets(B, 3, 500 + h) for h in range(6)]
    for h in range(3):
        r.step(pks[h], [8] * B)
    rec = r.export(0)
    assert len(rec) == 31
    r.start(2, rec)
    for h in range(3, 6):
        pk = pks[h].clone()
        pk[2] = pk[0]
        y = r.step(pk, [8] * B)
        assert torch.equal(y[2], y[0]), h


def test_concealing_receiver_with_output_rate(speech):
    from hilcodec_amd.graph_step import GraphedDecodeHop
    rate, B, F = 48000, 4, 2
    s = design(BASE_RATE, rate)
    rs = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True, fade_hops=F, output_rate=rate)
    plain = GraphedDecodeHop(speech, B, 1, 8, DEV, sessions=True, conceal=True, fade_hops=F)
    # slot 1: lost for 5 hops (concealed, faded out, then held by the device); slot 2: lost before anything arrived (held by the
    # device); slot 3: held by the host on hop 3
    lost = {h: [1] for h in range(2, 7)}
    lost[0] = [2]
    hold = {3: [3]}
    hist = [torch.zeros(1, 1, s.Q - 1) for _ in range(B)]
    received = [False] * B
    for h in range(9):
        pk = random_packets(B, 1, 900 + h)
        k_before = plain.concealed.cpu().tolist()
        gone, held = lost.get(h, []), hold.get(h, [])
        y = rs.step(pk, [8] * B, hold=held, lost=gone).cpu()
        w = plain.step(pk, [8] * B, hold=held, lost=gone).cpu()
        for b in range(B):
            device_held = b in gone and (not received[b] or k_before[b] == F)
            if b in held or device_held:
                assert not y[b].any(), (h, b)
                continue
            exp, hist[b] = reference(w[b:b + 1], s, hist[b])
            assert torch.equal(y[b:b + 1], exp), (h, b)
            if b not in gone:
                received[b] = True
        assert torch.equal(rs.concealed, plain.concealed)
        for b in range(B):
            assert torch.equal(rs.cache_dec[-1][b:b + 1].cpu(), hist[b]), (h, b)


# ---------------------------------------------------------------- the driver
def test_driver_reads_and_writes_other_rates(tmp_path):
    from hilcodec_amd import stream_driver as D
    from hilcodec_amd import wire
    x48 = synth.sweep_clip(48000, 48000).numpy().reshape(-1) * 0.5
    path = str(tmp_path / "in48.wav")
    D.write_wav(path, x48, 48000)
    wav, sr = D.read_wav_rate(path)
    assert sr == 48000 and wav.shape[0] == 48000
    D.main(["--enc", "--input", path, "--outdir", str(tmp_path)])
    got = wire.load_indices_npy(str(tmp_path / "hil_speech_quantized.npy"))
    model = D.build_streaming_model("hil_speech", None, DEV)
    x = torch.from_numpy(np.clip(wav, -1, 1)).view(1, 1, -1).to(DEV)
    exp, _ = D.encode_stream(model, resample(x, 48000, 24000), 8, 1)
    assert torch.equal(got.cpu().to(torch.int16), exp.cpu())
    D.main(["--dec", "--outdir", str(tmp_path), "--out_sr", "48000"])
    out, out_sr = D.read_wav_rate(str(tmp_path / "hil_speech_output.wav"))
    assert out_sr == 48000 and out.shape[0] == 2 * 320 * exp.shape[-1]
    with pytest.raises(ValueError):
        D.read_wav(path, 24000)
