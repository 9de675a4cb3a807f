"""CPU: the sample-rate converter's definition (hilcodec_amd/resample.py) — the filter table of every direction, its phases and
frequency response, the torch statement of the kernel against scipy's upfirdn, streaming with history against one offline call, the
argument checks, the C entry point's refusals and the state-layout records that carry the history.  (No kernel is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd.resample import BASE_RATE, RATES, design, hop_samples, reference
from tests.hops import assert_entry_points, bare_model

# other rate -> ((L, M, Q) into 24 kHz, (L, M, Q) out of 24 kHz, the smallest frame multiple of a hop)
TABLE = {
    8000: ((3, 1, 80), (1, 3, 240), 3),
    16000: ((3, 2, 80), (2, 3, 120), 3),
    22050: ((160, 147, 80), (147, 160, 88), 1),
    32000: ((3, 4, 107), (4, 3, 80), 3),
    44100: ((80, 147, 147), (147, 80, 80), 1),
    48000: ((1, 2, 160), (2, 1, 80), 1),
}
DIRECTIONS = [(r, BASE_RATE) for r in RATES] + [(BASE_RATE, r) for r in RATES]


def _full_filter(spec):
    h = np.zeros(spec.L * spec.Q)
    for p in range(spec.L):
        h[p::spec.L] = spec.taps[p].double().numpy()
    return h


def test_design_table():
    assert set(RATES) == set(TABLE)
    for rate, (into, out, _) in TABLE.items():
        for (a, b), want in (((rate, BASE_RATE), into), ((BASE_RATE, rate), out)):
            s = design(a, b)
            assert (s.L, s.M, s.Q) == want, (a, b)
            assert s.taps.dtype == torch.float32 and tuple(s.taps.shape) == (s.L, s.Q)
            assert s.history == s.Q - 1
            assert s.delay == (s.L * s.Q - 1) / (2 * s.L)
    assert abs(design(48000, BASE_RATE).delay_seconds - 1.66e-3) < 5e-6
    assert abs(design(BASE_RATE, 16000).delay_seconds - 2.49e-3) < 5e-6
    assert abs(design(8000, BASE_RATE).delay_seconds - 4.98e-3) < 5e-6


@pytest.mark.parametrize("a,b", DIRECTIONS)
def test_phases_sum_to_one(a, b):
    s = design(a, b)
    assert (s.taps.double().sum(dim=1) - 1.0).abs().max().item() <= 1e-4


@pytest.mark.parametrize("a,b", DIRECTIONS)
def test_frequency_response(a, b):
    from scipy.signal import freqz
    s = design(a, b)
    w, H = freqz(_full_filter(s), worN=1 << 16, fs=a * s.L)
    gain = 20 * np.log10(np.maximum(np.abs(H) / s.L, 1e-300))
    nyq = min(a, b) / 2
    assert np.abs(gain[w <= 0.85 * nyq]).max() <= 0.001
    assert gain[w >= nyq].max() <= -85.0


@pytest.mark.parametrize("a,b", DIRECTIONS)
def test_reference_matches_upfirdn(a, b):
    from scipy.signal import upfirdn
    s = design(a, b)
    gen = torch.Generator().manual_seed(a + 3 * b)
    T = 1237
    x = torch.rand(2, 1, T, generator=gen) * 2 - 1
    x[0, 0, :200] = torch.linspace(-1, 1, 200)
    y, hist = reference(x, s)
    assert tuple(y.shape) == (2, 1, -(-T * s.L // s.M)) and y.dtype == torch.float32
    h = _full_filter(s)
    for b_ in range(2):
        exp = upfirdn(h, x[b_, 0].double().numpy(), s.L, s.M)[:y.shape[-1]]
        assert np.abs(y[b_, 0].double().numpy() - exp).max() <= 5e-6
    assert torch.equal(hist, x[:, :, T - (s.Q - 1):])


@pytest.mark.parametrize("a,b", DIRECTIONS)
def test_streaming_reference_equals_offline(a, b):
    s = design(a, b)
    rate = a if a != BASE_RATE else b
    frames = TABLE[rate][2]
    hop_in = 320 * frames if a == BASE_RATE else hop_samples(frames, a)
    assert hop_in % s.M == 0
    gen = torch.Generator().manual_seed(a + b)
    rng = np.random.default_rng(a * 7 + b)
    hops = rng.integers(0, 4, size=6)                # chunks of 0 .. 3 hops
    T = int(hops.sum()) * hop_in + 37                # the last chunk is ragged
    x = torch.rand(3, 1, T, generator=gen) * 2 - 1
    full, full_hist = reference(x, s)
    outs, hist, at = [], None, 0
    for k in list(hops) + [None]:
        n = T - at if k is None else int(k) * hop_in
        if n == 0:
            continue
        y, hist = reference(x[:, :, at:at + n], s, hist)
        outs.append(y)
        at += n
    assert torch.equal(torch.cat(outs, dim=2), full)
    assert torch.equal(hist, full_hist)


def test_short_input_history():
    """fewer input samples than Q - 1: the new history keeps the tail of the old one"""
    s = design(48000, BASE_RATE)
    gen = torch.Generator().manual_seed(1)
    h0 = torch.randn(2, 1, s.Q - 1, generator=gen)
    x = torch.randn(2, 1, 10, generator=gen)
    _, h1 = reference(x, s, h0)
    assert torch.equal(h1, torch.cat([h0, x], dim=2)[:, :, 10:])


def test_unsupported_rates_and_frames():
    for a, b in ((44100, 48000), (24000, 24000), (12000, 24000), (24000, 96000), (48000, 16000)):
        with pytest.raises(ValueError):
            design(a, b)
    with pytest.raises(ValueError, match="multiple of 3"):
        hop_samples(1, 16000)
    with pytest.raises(ValueError, match="multiple of 3"):
        hop_samples(4, 8000)
    with pytest.raises(ValueError, match="multiple of 3"):
        hop_samples(2, 32000)
    with pytest.raises(ValueError):
        hop_samples(1, 11025)
    with pytest.raises(ValueError):
        hop_samples(0, 48000)
    assert hop_samples(1, 48000) == 640 and hop_samples(1, 44100) == 588 and hop_samples(1, 22050) == 294
    assert hop_samples(3, 16000) == 640 and hop_samples(3, 8000) == 320 and hop_samples(3, 32000) == 1280
    assert hop_samples(2, 24000) == 640


def test_public_names():
    import hilcodec_amd
    assert callable(hilcodec_amd.resample) and callable(hilcodec_amd.Resampler)
    with pytest.raises(ValueError):
        hilcodec_amd.resample(torch.zeros(1, 1, 8), 48000, 16000)


def test_c_entry_point_checks():
    from hilcodec_amd._lib import lib
    assert_entry_points(["hilc_resample_poly"])
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)
    # (x, hist_in, hist_out, y, taps, B, T_in, L, M, Q, stream)
    assert lib.hilc_resample_poly(None, None, None, p, p, 1, 640, 1, 2, 160, None) == -2
    assert lib.hilc_resample_poly(p, None, None, None, p, 1, 640, 1, 2, 160, None) == -2
    assert lib.hilc_resample_poly(p, None, None, p, None, 1, 640, 1, 2, 160, None) == -2
    assert lib.hilc_resample_poly(p, None, None, p, p, 0, 640, 1, 2, 160, None) == -1
    assert lib.hilc_resample_poly(p, None, None, p, p, 1, 0, 1, 2, 160, None) == -1
    assert lib.hilc_resample_poly(p, None, None, p, p, 1, 640, 1, 2, 1, None) == -1
    assert lib.hilc_resample_poly(p, q, q, p, p, 1, 640, 1, 2, 160, None) == -1        # hist_out must not be hist_in
    assert lib.hilc_resample_poly(p, None, None, p, p, 1, 640, 1, 2, 4000, None) == -4     # too long for the LDS tiles


def test_op_registered_with_fake_and_refuses_cpu():
    from hilcodec_amd import ops
    op = torch.ops.hilcodec.resample_poly.default
    assert "Tensor(a!)? hist_out" in str(op._schema)
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "Meta")
    s = design(44100, BASE_RATE)
    x = torch.empty(3, 1, 588, device="meta")
    y = ops.resample_poly(x, torch.empty(s.L, s.Q, device="meta"), s.L, s.M)
    assert y.device.type == "meta" and tuple(y.shape) == (3, 1, 320)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.resample_poly(torch.zeros(1, 1, 588), s.taps, s.L, s.M)


@pytest.mark.parametrize("side,rate", [("enc", 48000), ("dec", 16000)])
def test_state_layout_with_history(side, rate):
    from hilcodec_amd import graph_step as G
    model = bare_model()
    s = design(rate, BASE_RATE) if side == "enc" else design(BASE_RATE, rate)
    plain = G.state_layout(model, 5, side)
    layout = G.state_layout(model, 5, side, s.history)
    n = 22 if side == "enc" else 30
    assert len(plain.shapes) == n and len(layout.shapes) == n + 1
    assert layout.shapes[:n] == plain.shapes and layout.shapes[-1] == (5, 1, s.Q - 1)
    assert layout.n_enc == (n + 1 if side == "enc" else 0)
    assert layout.record_len == plain.record_len + s.Q - 1
    # a record is the codec's caches in order, then the history
    gen = torch.Generator().manual_seed(3)
    caches = [torch.randn((1,) + sh[1:], generator=gen) for sh in layout.shapes]
    rec = layout.record(caches, []) if side == "enc" else layout.record([], caches)
    assert torch.equal(rec[-(s.Q - 1):], caches[-1].reshape(-1))
    back = layout.split(rec)[0 if side == "enc" else 1]
    assert len(back) == n + 1 and all(torch.equal(a, b) for a, b in zip(back, caches))
    with pytest.raises(ValueError):
        layout.record(caches[:-1], []) if side == "enc" else layout.record([], caches[:-1])
    blk = G.StateBlock(model, 5, torch.device("cpu"), side, s.history)
    lst = blk.enc if side == "enc" else blk.dec
    codec = blk.codec_enc if side == "enc" else blk.codec_dec
    assert len(lst) == n + 1 and len(codec) == n and blk.hist is lst[-1] and tuple(blk.hist.shape) == (5, 1, s.Q - 1)
    with pytest.raises(ValueError):
        G.state_layout(model, 5, "both", s.history)
