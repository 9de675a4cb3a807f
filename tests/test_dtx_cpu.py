"""CPU: discontinuous transmission and comfort noise — the hilc_dtx_encode / hilc_cng_synth entry points (additive under ABI 16) and
their argument checks, their custom ops and fake kernels, DtxConfig, the SID wire helpers, the definitions of hilcodec_amd/dtx.py
(Levinson-Durbin, the sender's state machine, an analysis -> synthesis round trip) and the host checks of step(sid=, silent=).
(No kernel is launched here.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hilcodec_amd import dtx
from hilcodec_amd.graph_step import SessionQueue
from tests.hops import assert_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hilc_dtx_encode", "hilc_cng_synth")


def test_dtx_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)
    import hilcodec_amd
    assert not hasattr(hilcodec_amd, "dtx") or "dtx" not in open(os.path.join(ROOT, "hilcodec_amd", "__init__.py")).read()


def test_dtx_encode_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_dtx_encode
    # (x, action, hold, run, kind, packets, nbytes, indices, prev, level_thr, thr_vad, B, T, order, H, I, n_max, stride, prev_words, stream)
    ok = [p, None, None, p, p, p, p, p, None, p]
    for k in (0, 3, 4, 5, 6, 7, 9):                       # required pointers
        args = list(ok)
        args[k] = None
        assert f(*args, 1e-6, 4, 1, 8, 8, 8, 8, 10, 0, None) == -2, k
    assert f(*ok, 1e-6, 0, 1, 8, 8, 8, 8, 10, 0, None) == -1
    assert f(*ok, 1e-6, 4, 0, 8, 8, 8, 8, 10, 0, None) == -1
    assert f(*ok, 1e-6, 4, 1, 8, 8, 8, 0, 10, 0, None) == -1      # n_max
    assert f(*ok, 1e-6, 4, 1, 9, 8, 8, 8, 9, 0, None) == -1       # 1 + K > stride
    assert f(*ok, 1e-6, 4, 1, 17, 8, 8, 8, 30, 0, None) == -5
    assert f(*ok, 1e-6, 4, 1, -1, 8, 8, 8, 30, 0, None) == -5
    assert f(*ok, 1e-6, 4, 1, 8, -1, 8, 8, 30, 0, None) == -5     # hangover >= 0
    assert f(*ok, 1e-6, 4, 1, 8, 8, 0, 8, 30, 0, None) == -5      # sid_interval >= 1
    args = list(ok)
    args[8] = p
    assert f(*args, 1e-6, 4, 1, 8, 8, 8, 8, 10, 0, None) == -1    # prev without its width


def test_cng_synth_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_cng_synth
    # (packets, action, hold, state, wav, restore, gains, B, T, order, stride, stream)
    ok = [p, None, p, p, p, None, p]
    for k in (0, 2, 3, 4, 6):
        args = list(ok)
        args[k] = None
        assert f(*args, 4, 1, 8, 10, None) == -2, k
    assert f(*ok, 0, 1, 8, 10, None) == -1
    assert f(*ok, 4, 0, 8, 10, None) == -1
    assert f(*ok, 4, 1, 17, 30, None) == -5
    assert f(*ok, 4, 1, -1, 30, None) == -5
    assert f(*ok, 4, 1, 10, 10, None) == -1                       # 1 + K > stride


def test_dtx_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("dtx_encode", "cng_synth"):
        assert hasattr(torch.ops.hilcodec, name), name
    sch = str(torch.ops.hilcodec.dtx_encode.default._schema)
    assert "Tensor(a!) run" in sch and "Tensor(b!) packets" in sch and "Tensor(e!)? prev" in sch
    sch = str(torch.ops.hilcodec.cng_synth.default._schema)
    assert "Tensor(a!) hold" in sch and "Tensor(b!) state" in sch and "Tensor(c!) wav" in sch
    B, n, T, K = 5, 8, 1, 8
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        kind = torch.ops.hilcodec.dtx_encode(torch.empty(B, 1, 320), i32(B), i32(B), i32(B), torch.empty(B, 10, dtype=torch.uint8),
                                             i32(B), torch.empty(n, B, T, dtype=torch.int64), None,
                                             torch.empty(127, dtype=torch.float64), 1e-6, K, 8, 8)
        assert tuple(kind.shape) == (B,) and kind.dtype == torch.int32
        torch.ops.hilcodec.cng_synth(torch.empty(B, 10, dtype=torch.uint8), None, i32(B), i32(B, 3 + 2 * K), torch.empty(B, 1, 320),
                                     None, torch.empty(128), K)
    with pytest.raises(RuntimeError):                     # no CPU fallback
        torch.ops.hilcodec.cng_synth(torch.zeros(B, 10, dtype=torch.uint8), None, torch.zeros(B, dtype=torch.int32),
                                     torch.zeros(B, 3 + 2 * K, dtype=torch.int32), torch.zeros(B, 1, 320), None, torch.zeros(128), K)


def test_dtx_config_validation():
    c = dtx.DtxConfig()
    assert (c.threshold_db, c.hangover, c.sid_interval, c.order) == (-60.0, 8, 8, 8)
    assert c.thr_vad == 10.0 ** -6
    assert dtx.DtxConfig(threshold_db=-127, hangover=0, sid_interval=1, order=0).threshold_db == -127.0
    assert dtx.DtxConfig(threshold_db=0.0, order=16).order == 16
    for bad in (dict(threshold_db=1.0), dict(threshold_db=-127.5), dict(threshold_db=float("nan")), dict(threshold_db=float("-inf")),
                dict(threshold_db="x"), dict(threshold_db=True), dict(hangover=-1), dict(hangover=2.0), dict(hangover=True),
                dict(sid_interval=0), dict(sid_interval=1.5), dict(order=17), dict(order=-1), dict(order=None)):
        with pytest.raises(ValueError):
            dtx.DtxConfig(**bad)
    with pytest.raises(Exception):
        c.order = 3                                       # frozen
    dtx.check_order(9, 10, "x")
    with pytest.raises(ValueError, match="order must be <= 9"):
        dtx.check_order(10, 10, "x")


@pytest.mark.parametrize("K", [0, 1, 10, 16])
def test_sid_round_trip(K):
    rng = np.random.default_rng(K)
    for L in (0, 1, 64, 127):
        q = rng.integers(-128, 128, size=K)
        blob = dtx.pack_sid(L, q)
        assert len(blob) == dtx.sid_bytes(K) == 1 + K
        L2, q2 = dtx.parse_sid(blob + b"\0\0", K)
        assert L2 == L and q2.dtype == np.int8 and np.array_equal(q2, q)
    with pytest.raises(ValueError):
        dtx.pack_sid(128, [0] * K)
    with pytest.raises(ValueError):
        dtx.parse_sid(b"\0" * K, K)


def test_levinson_matches_normal_equations():
    rng = np.random.default_rng(0)
    for K in (1, 2, 5, 10, 16):
        for _ in range(5):
            x = rng.standard_normal(4096)
            x = np.convolve(x, rng.standard_normal(4) * 0.5 + np.array([1, 0, 0, 0]))[:4096]
            R = np.array([np.dot(x[k:], x[:len(x) - k]) for k in range(K + 1)])
            k, E = dtx.levinson(R[None, :])
            Rp = R.copy()
            Rp[0] *= dtx.NOISE_FLOOR
            toe = np.array([[Rp[abs(i - j)] for j in range(K)] for i in range(K)])
            a = np.linalg.solve(toe, -Rp[1:K + 1])
            # step-up of the reflection coefficients gives the direct form
            aa = np.zeros(K + 1)
            for i in range(1, K + 1):
                new = aa.copy()
                for j in range(1, i):
                    new[j] = aa[j] + k[0, i - 1] * aa[i - j]
                new[i] = k[0, i - 1]
                aa = new
            assert np.allclose(aa[1:], a, atol=1e-9, rtol=0), K
            assert abs(E[0] - (Rp[0] + np.dot(a, Rp[1:K + 1]))) <= 1e-9 * Rp[0]
    k, E = dtx.levinson(np.zeros((1, 9)))                 # digital silence: no coefficients, level 127
    assert not k.any() and E[0] == 0.0


def test_kind_sequence():
    cfg = dtx.DtxConfig(hangover=2, sid_interval=3)
    active = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    run, kinds = 0, []
    for a in active:
        run = dtx.next_run(run, bool(a), cfg)
        kinds.append(dtx.kind_of(run, bool(a), cfg))
    S, D, Q = dtx.SPEECH, dtx.SID, dtx.SILENT
    assert kinds == [S, S, S, D, Q, Q, D, Q, Q, D, S, S, S, D, S]
    cfg0 = dtx.DtxConfig(hangover=0, sid_interval=1)
    run, kinds = 0, []
    for a in (0, 0, 0):
        run = dtx.next_run(run, False, cfg0)
        kinds.append(dtx.kind_of(run, False, cfg0))
    assert kinds == [D, D, D]


def test_session_queue_cn_checks():
    q = SessionQueue(8, 8, 1, layout=None, one_sided=True)
    assert q.cn_slots([1, 2], [3], hold=[0], lost=[4], fec=[5]) == ([1, 2], [3])
    with pytest.raises(ValueError, match="in both"):
        q.cn_slots([1], [1])
    for kw in (dict(hold=[1]), dict(lost=[1]), dict(fec=[1])):
        with pytest.raises(ValueError):
            q.cn_slots([1], [], **kw)
        with pytest.raises(ValueError):
            q.cn_slots([], [1], **kw)
    with pytest.raises(IndexError):
        q.cn_slots([8], [])
    q.stop(6)
    with pytest.raises(ValueError, match="stopped"):
        q.cn_slots([6], [])
    with pytest.raises(ValueError, match="stopped"):
        q.cn_slots([], [6])
    with pytest.raises(ValueError):
        q.cn_slots(torch.tensor([1]).cuda() if torch.cuda.is_available() else torch.tensor([1]).to("meta"), [])


def ar2_noise(rng, n, a1, a2):
    e = rng.standard_normal(n + 512)
    y = np.zeros_like(e)
    for s in range(2, len(e)):
        y[s] = e[s] - a1 * y[s - 1] - a2 * y[s - 2]
    return y[512:]


@pytest.mark.parametrize("dbfs", [-30.0, -50.0])
def test_round_trip_level_and_envelope(dbfs):
    rng = np.random.default_rng(int(-dbfs))
    a1, a2 = -1.1, 0.45
    cfg = dtx.DtxConfig(threshold_db=-20.0, order=8)
    S, hops = 320, 8
    x = ar2_noise(rng, S, a1, a2)
    x = (x / np.sqrt(np.mean(x ** 2)) * 10 ** (dbfs / 20)).astype(np.float32)
    active, level, q, k, _ = dtx.analyze(x[None], cfg)
    assert not active[0]
    y = dtx.round_trip(x, cfg, hops)
    assert y.dtype == np.float32 and y.shape == (S * hops,)
    rms_in = 10 * np.log10(np.mean(x.astype(np.float64) ** 2))
    rms_out = 10 * np.log10(np.mean(y.astype(np.float64) ** 2))
    assert abs(rms_out - rms_in) < 2.0, (rms_in, rms_out)
    # reflection coefficients re-estimated from the noise agree with the input's
    R_in = dtx.autocorrelation(x[None], 2)
    R_out = np.array([[np.dot(y[j:].astype(np.float64), y[:len(y) - j]) for j in range(3)]])
    k_in, _ = dtx.levinson(R_in)
    k_out, _ = dtx.levinson(R_out)
    assert np.all(np.abs(k_in - k_out) < 0.1), (k_in, k_out)


def test_synthesis_is_stable_and_deterministic():
    q = np.array([-100, 60, -30, 20, -10, 5, 0, 0, 3, -3, 0, 0, 1, 0, 0, -1], dtype=np.int8)
    y1, m1 = dtx.synthesize(0, q, 3, 0, 320)
    y2, m2 = dtx.synthesize(0, q, 3, 0, 320)
    assert np.array_equal(y1, y2) and np.all(np.isfinite(y1))
    assert not np.array_equal(y1, dtx.synthesize(0, q, 4, 0, 320)[0])       # another slot: another excitation
    assert not np.array_equal(y1, dtx.synthesize(0, q, 3, 1, 320)[0])       # the next hop: another excitation
    u = dtx.excitation(0, 0, 100000)
    assert u.min() >= -1.0 and u.max() < 1.0 and abs(float(u.mean())) < 0.01
    assert dtx.gain_table().dtype == np.float32 and dtx.gain_table()[0] == np.float32(np.sqrt(3.0))
    thr = dtx.level_table()
    assert thr.shape == (127,) and np.all(np.diff(thr) < 0)


def test_step_checks_without_gpu():
    """sid / silent on a receiver without cng_order: RuntimeError before anything is launched (checked by the GPU tests too)"""
    from hilcodec_amd.graph_step import GraphedDecodeHop
    assert "sid" in GraphedDecodeHop.step.__code__.co_varnames and "silent" in GraphedDecodeHop.step.__code__.co_varnames
    import inspect
    assert inspect.signature(GraphedDecodeHop.__init__).parameters["cng_order"].default is None
    from hilcodec_amd.graph_step import GraphedEncodeHop
    assert inspect.signature(GraphedEncodeHop.__init__).parameters["dtx"].default is None


def test_diverging_sid_becomes_silence():
    """every q_i = -127 at K = 16: stable in exact arithmetic, but the fp32 direct form diverges; the hop is silence and the filter
    memory is cleared, never an overflow"""
    q = np.full(16, -127, dtype=np.int8)
    y, mem = dtx.synthesize(0, q, 3, 0, 320)
    assert not y.any() and not mem.any()
    rows, mems = dtx._synth_rows(np.array([0, 60]), np.stack([q, np.zeros(16, np.int8)]), np.array([3, 4]), np.array([0, 0]), 320,
                                 np.zeros((2, 16), np.float32))
    assert not rows[0].any() and not mems[0].any()
    assert rows[1].any() and np.all(np.abs(rows[1]) < dtx.NOISE_BOUND)
    st = torch.zeros(1, dtx.state_words(16), dtype=torch.int32)
    pk = torch.zeros(1, 17, dtype=torch.uint8)
    pk[0, 1:] = torch.from_numpy(q.view(np.uint8))
    st, hold, restore, noise = dtx.cng_model(st, pk, torch.tensor([2], dtype=torch.int32), None, 16, 1)
    assert int(restore[0]) == 1 and int(hold[0]) == 0 and not noise.any()
    assert int(st[0, dtx.ST_COUNT]) == 1 and not st[0, dtx.ST_Q + 16:].any()    # the hop counts, the memory is cleared
