"""CPU: per-speaker levelling and the limiter of the room mixer — LevelConfig / LimitConfig / MixConfig validation, the rules
(mixer.MixModel, mixer.update_gains, mixer.limit) on hand-built cases with literal expected values, the hilc_mix_gains /
hilc_mix_rooms_dyn entry points (additive under ABI 16) and their argument checks, their custom ops and fake kernels, and the errors of
mixer.Dynamics and hilcodec_amd.mix_rooms(dynamics=).  (No kernel is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd import mixer
from hilcodec_amd.mixer import Dynamics, LevelConfig, LimitConfig, MixConfig, MixModel
from tests.hops import assert_entry_points

NEW = ("hilc_mix_gains", "hilc_mix_rooms_dyn")
LIMIT_L = (1, 31, 32, 33, 70, 320, 960)


# ---------------------------------------------------------------- configuration
def test_level_config():
    c = LevelConfig()
    assert (c.target_rms, c.gate_rms, c.band, c.up, c.down, c.min_gain, c.max_gain, c.smooth) == (0.1, 0.01, 1.6, 1.01, 0.97, 0.125, 8.0, 0.25)
    assert c.gate2 == 0.01 * 0.01 and c.lo == 0.1 * 0.1 / 1.6 and c.hi == 0.1 * 0.1 * 1.6
    LevelConfig(min_gain=1, max_gain=1, smooth=1)                                # the closed ends
    bad = [dict(gate_rms=0), dict(gate_rms=-1.0), dict(target_rms=0), dict(target_rms=-0.1),
           dict(band=1), dict(band=0.5), dict(up=1), dict(up=0.9), dict(down=0), dict(down=1), dict(down=-0.5), dict(down=1.5),
           dict(min_gain=0), dict(min_gain=1.5), dict(max_gain=0.5), dict(min_gain=-1),
           dict(smooth=0), dict(smooth=1.5), dict(smooth=-0.1),
           dict(up=float("nan")), dict(band=float("inf")), dict(smooth="0.25"), dict(up=True), dict(target_rms=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            LevelConfig(**kw)


def test_limit_config():
    c = LimitConfig()
    assert (c.ceiling, c.release, c.sub) == (0.9, 0.99, 32)
    LimitConfig(ceiling=1, sub=16)
    LimitConfig(sub=np.int64(512))
    bad = [dict(ceiling=0), dict(ceiling=1.01), dict(ceiling=-0.5), dict(release=0), dict(release=1), dict(release=1.5),
           dict(sub=15), dict(sub=513), dict(sub=32.0), dict(sub=True), dict(sub=None), dict(ceiling=float("nan")), dict(release="0.9")]
    for kw in bad:
        with pytest.raises(ValueError):
            LimitConfig(**kw)


def test_mix_config_options():
    assert MixConfig(3) == MixConfig(3, None, None) and MixConfig().level is None and MixConfig().limit is None
    c = MixConfig(2, level=LevelConfig(), limit=LimitConfig())
    assert c.top_k == 2 and c.level == LevelConfig() and c.limit == LimitConfig()
    for kw in (dict(level=LimitConfig()), dict(limit=LevelConfig()), dict(level=True), dict(limit=0.9), dict(level=(0.1,))):
        with pytest.raises(ValueError):
            MixConfig(3, **kw)
    assert (mixer.MIN_SUB, mixer.MAX_SUB, mixer.MAX_LIMIT_L) == (16, 512, 8192)


# ---------------------------------------------------------------- the model without the options is the model as it was
def plain_step(score, x, room, top_k, action=None):
    """the mixer's rules before the options, from the module's own building blocks: (score, speakers, mixed)"""
    score = mixer.update_score(score, mixer.levels(x), action)
    speakers = mixer.select(room, score, top_k)
    B, L = x.shape
    out = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        terms = [t for t in range(B) if room[b] >= 0 and room[t] == room[b] and speakers[t] and t != b]
        if terms:
            acc = x[terms[0]].copy()
            for t in terms[1:]:
                acc = (acc + x[t]).astype(np.float32)
            out[b] = np.minimum(np.maximum(acc, np.float32(-1)), np.float32(1))
    return score, speakers, out


def test_model_without_options_is_unchanged():
    B, L = 7, 70
    rng = np.random.default_rng(1)
    a, b = MixModel(B, MixConfig(3)), MixModel(B, MixConfig(3, level=None, limit=None))
    assert a.gains is None and a.power is None and a.limiter is None
    score = np.zeros(B)
    for k in range(5):
        x = rng.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
        room = rng.integers(-1, 2, B)
        action = (rng.random(B) < 0.2).astype(np.int32)
        ma, sa = a.step(x, room, action)
        mb, sb = b.step(x, room, action)
        score, speakers, want = plain_step(score, x.reshape(B, L), room, 3, action)
        assert torch.equal(ma, mb) and torch.equal(sa, sb) and torch.equal(a.score, b.score)
        assert np.array_equal(ma.numpy().reshape(B, L), want) and np.array_equal(sa.numpy(), speakers)
        assert np.array_equal(a.score.numpy(), score)
    assert np.abs(want).max() == 1.0                                             # and it still clips


# ---------------------------------------------------------------- the leveller
def const_rows(*values, L=64):
    return torch.tensor(values, dtype=torch.float32).view(-1, 1, 1).repeat(1, 1, L).contiguous()


def test_leveller_rises_to_the_dead_band_and_holds():
    # a constant row of 2^-5: m = 2^-10 exactly; the dead band of target 0.1, band 1.6 is [0.00625, 0.016] = [6.4, 16.4] 2^-10.  As
    # heard the power is g^2 2^-10: under the band at g = 1, 1.5 and 2.25 (g^2 = 5.06), inside it at g = 1.5^3 = 3.375 (g^2 = 11.39)
    cfg = LevelConfig(up=1.5, down=0.7)
    m = MixModel(1, MixConfig(1, level=cfg))
    assert m.gains.tolist() == [[1.0, 1.0]] and m.power.tolist() == [0.0]
    trace = []
    for k in range(6):
        m.step(const_rows(2.0 ** -5), [0])
        trace.append(m.gains[0].tolist())
        assert m.power.tolist() == [2.0 ** -10]                                  # pw = m on the first hop, then m + s (m - m)
    assert trace == [[1.0, 1.5], [1.5, 2.25], [2.25, 3.375], [3.375, 3.375], [3.375, 3.375], [3.375, 3.375]]
    assert cfg.lo <= 3.375 * 3.375 * 2.0 ** -10 <= cfg.hi


def test_leveller_gate_leaves_power_and_gain_alone():
    cfg = LevelConfig(up=1.5, down=0.7)
    m = MixModel(2, MixConfig(1, level=cfg))
    m.step(const_rows(2.0 ** -5, 2.0 ** -5), [0, 0])
    assert m.gains.tolist() == [[1.0, 1.5]] * 2
    # slot 0: 2^-7 (m = 2^-14 < gate2 = 1e-4), slot 1: silence — neither counts: the power stays, the gain holds at its end value
    for k in range(3):
        m.step(const_rows(2.0 ** -7, 0.0), [0, 0])
        assert m.gains.tolist() == [[1.5, 1.5]] * 2 and m.power.tolist() == [2.0 ** -10] * 2
    # just above the gate: m = 2^-12 > 1e-4 counts, and the power moves by smooth (m - pw)
    m.step(const_rows(2.0 ** -6, 0.0), [0, 0])
    assert m.power.tolist() == [2.0 ** -10 + 0.25 * (2.0 ** -12 - 2.0 ** -10), 2.0 ** -10]
    assert m.gains.tolist() == [[1.5, 2.25], [1.5, 1.5]]


def test_leveller_falls_to_min_gain_and_rises_to_max_gain():
    cfg = LevelConfig(up=1.5, down=0.7, min_gain=0.25, max_gain=4.0)
    m = MixModel(2, MixConfig(1, level=cfg))
    ends = []
    for k in range(12):
        m.step(const_rows(1.0, 2.0 ** -6), [0, 0])                               # m = 1 (far above hi) and 2^-12 (far under lo)
        ends.append(m.gains[:, 1].tolist())
        assert m.gains[:, 0].tolist() == ([1.0, 1.0] if k == 0 else ends[k - 1])  # a hop starts where the last one ended
    down, up = [e[0] for e in ends], [e[1] for e in ends]
    g, want_down = 1.0, []
    for k in range(12):
        g = max(g * 0.7, 0.25)
        want_down.append(g)
    assert down == want_down and down[3] == 0.25 and down[2] > 0.25 and down[-1] == 0.25     # 0.7^4 = 0.2401 < 0.25
    assert up == [1.5, 2.25, 3.375, 4.0] + [4.0] * 8                             # 1.5^4 = 5.06 > 4: capped


def test_leveller_action_resets_gain_and_power():
    cfg = LevelConfig(up=1.5, down=0.7)
    m = MixModel(2, MixConfig(1, level=cfg))
    for k in range(2):
        m.step(const_rows(2.0 ** -5, 2.0 ** -5), [0, 0])
    assert m.gains.tolist() == [[1.5, 2.25]] * 2
    m.step(const_rows(2.0 ** -4, 2.0 ** -4), [0, 0], action=[0, 1])              # slot 1 starts again: g0 = 1, pw = 0 -> m
    assert m.gains.tolist() == [[2.25, 2.25], [1.0, 1.5]]                        # slot 0: 2.25^2 pw = 0.0087, inside the dead band
    assert m.power.tolist() == [2.0 ** -10 + 0.25 * (2.0 ** -8 - 2.0 ** -10), 2.0 ** -8]
    m.step(const_rows(0.0, 0.0), [0, 0], action=[0, 2])                          # a reset on a silent hop: the cleared row
    assert m.gains.tolist() == [[2.25, 2.25], [1.0, 1.0]] and m.power[1].item() == 0.0


def test_levelled_terms_ramp_over_the_hop():
    # slots 0 and 1 speak, slot 2 listens: it hears fp32(x0 (g0 + (g1 - g0)(i + 1)/L)) + fp32(x1 ...), the select is on the raw score
    cfg = LevelConfig(up=1.5, down=0.7)
    m = MixModel(3, MixConfig(2, level=cfg))
    L = 4
    x = const_rows(2.0 ** -5, 2.0 ** -6, 0.0, L=L)
    mixed, sp = m.step(x, [0, 0, 0])
    assert sp.tolist() == [1, 1, 0] and m.gains.tolist() == [[1.0, 1.5], [1.0, 1.5], [1.0, 1.0]]
    ramp = [1.0 + 0.5 * (i + 1) / L for i in range(L)]
    assert mixed[2, 0].tolist() == [2.0 ** -5 * r + 2.0 ** -6 * r for r in ramp]
    assert mixed[0, 0].tolist() == [2.0 ** -6 * r for r in ramp]                 # a speaker hears the other one only
    mixed, _ = m.step(x, [0, 0, 0])                                              # the next hop starts at 1.5: no step at the seam
    assert mixed[0, 0, 0].item() == 2.0 ** -6 * (1.5 + 0.75 / L)


# ---------------------------------------------------------------- the limiter
def noise_hops(L, hops=12):
    """the hops of the bound's check: uniform noise at 2.4 and 0.5 in turn, one listener's sums"""
    rng = np.random.default_rng(L)
    return [((2.4 if k % 2 == 0 else 0.5) * rng.uniform(-1, 1, (1, L))).astype(np.float32) for k in range(hops)]


@pytest.mark.parametrize("L", LIMIT_L)
def test_limiter_never_exceeds_the_ceiling(L):
    cfg = LimitConfig()
    ceil32 = np.float32(cfg.ceiling)
    state = np.array([[0.0, 1.0]])
    over, peak = 0, np.float32(0)
    for acc in noise_hops(L):
        out, state = mixer.limit(acc, state, cfg)
        assert out.dtype == np.float32 and out.shape == acc.shape
        over += int((np.abs(acc) > 1).sum())
        peak = max(peak, np.abs(out).max())
        # g <= ceiling / p_s in every sub-frame: |acc g| <= ceiling (1 + 2^-52)^2 in float64, so at most one fp32 ulp over fp32(ceiling)
        assert np.abs(out).max() <= np.nextafter(ceil32, np.float32(2)), (L, np.abs(out).max())
    assert over > 0 and peak >= ceil32                                           # the raw sums clip, and the limiter was at work


def test_limiter_releases_by_release_per_subframe():
    cfg = LimitConfig(ceiling=0.5, release=0.5, sub=16)
    loud = np.full((1, 32), 2.0, dtype=np.float32)
    out, state = mixer.limit(loud, np.array([[0.0, 1.0]]), cfg)
    assert state.tolist() == [[2.0, 0.25]] and out.tolist() == [[0.5] * 32]      # an immediate attack: G = 0.5 / 2 from sample 0
    # 40 samples of silence: sub-frames of 16, 16 and 8; e = 1, 0.5, 0.25 and G = 0.5, 1, 1
    quiet = np.zeros((1, 40), dtype=np.float32)
    out, state = mixer.limit(quiet, state, cfg)
    assert state.tolist() == [[0.25, 1.0]] and not out.any()
    # the same release under a quiet signal: the gain moves linearly over each sub-frame, (k + 1) / n_s of the way at offset k
    soft = np.full((1, 40), 0.125, dtype=np.float32)
    out, state = mixer.limit(soft, np.array([[2.0, 0.25]]), cfg)
    want = [0.125 * (0.25 + 0.25 * (k + 1) / 16) for k in range(16)] + [0.125 * (0.5 + 0.5 * (k + 1) / 16) for k in range(16)] + [0.125] * 8
    assert out[0].tolist() == [float(np.float32(w)) for w in want]
    assert state.tolist() == [[0.25, 1.0]]
    # over many sub-frames the envelope is the last peak times release^s exactly (each product rounded: powers of two here)
    out, state = mixer.limit(np.zeros((1, 16 * 9), dtype=np.float32), np.array([[2.0, 0.25]]), cfg)
    assert state.tolist() == [[2.0 * 0.5 ** 9, 1.0]]


def test_limiter_runs_on_a_zero_row_and_resets_on_action():
    cfg = MixConfig(1, limit=LimitConfig(ceiling=0.5, release=0.5, sub=16))
    m = MixModel(3, cfg)
    assert m.limiter.tolist() == [[0.0, 1.0]] * 3
    mixed, sp = m.step(const_rows(2.0, 0.0, 0.0, L=16), [0, 0, -1])
    assert sp.tolist() == [1, 0, 0]
    assert mixed[:, 0, 0].tolist() == [0.0, 0.5, 0.0]                            # slot 1 hears slot 0 limited; 0 and 2 hear nothing
    assert m.limiter.tolist() == [[0.0, 1.0], [2.0, 0.25], [0.0, 1.0]]
    mixed, _ = m.step(const_rows(0.0, 0.0, 0.0, L=16), [0, -1, -1])              # slot 1 has left: its zero row still releases
    assert not mixed.any() and m.limiter.tolist() == [[0.0, 1.0], [1.0, 0.5], [0.0, 1.0]]
    m.step(const_rows(0.0, 0.0, 0.0, L=16), [0, -1, -1], action=[0, 1, 0])
    assert m.limiter.tolist() == [[0.0, 1.0]] * 3
    with pytest.raises(ValueError):
        m.step(torch.zeros(3, 1, mixer.MAX_LIMIT_L + 1), [0, 0, 0])


def test_level_and_limit_together():
    # two speakers at 2^-5 whose gains rise from 1 by 1.5 per hop: listener 2's sum is 2^-4 g, over the ceiling 2^-4 as soon as g > 1
    cfg = MixConfig(2, level=LevelConfig(up=1.5, down=0.7), limit=LimitConfig(ceiling=2.0 ** -4, release=0.5, sub=16))
    m = MixModel(3, cfg)
    x = const_rows(2.0 ** -5, 2.0 ** -5, 0.0, L=16)
    mixed, sp = m.step(x, [0, 0, 0])
    assert sp.tolist() == [1, 1, 0] and m.gains.tolist() == [[1.0, 1.5], [1.0, 1.5], [1.0, 1.0]]
    # the hop's last sample has the end gain exactly: the one sub-frame's peak is e = 2 (2^-5 1.5), the limiter's gain ceiling / e from
    # its first sample on (an immediate attack), and the last sample lands on the ceiling
    G = 2.0 ** -4 / 0.09375
    assert m.limiter[2].tolist() == [0.09375, G]
    assert mixed[2, 0].tolist() == [float(np.float32(2.0 ** -4 * (1.0 + 0.5 * (i + 1) / 16) * G)) for i in range(16)]
    assert mixed[2].abs().max().item() == mixed[2, 0, 15].item() == 2.0 ** -4
    assert mixed[0, 0].tolist() == [2.0 ** -5 * (1.0 + 0.5 * (i + 1) / 16) for i in range(16)]     # one term stays under the ceiling
    assert m.limiter[0].tolist() == [2.0 ** -5 * 1.5, 1.0]


# ---------------------------------------------------------------- the entry points
def test_mix_dyn_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)


def test_mix_gains_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_mix_gains
    c = LevelConfig()
    rule = [c.gate2, c.lo, c.hi, c.up, c.down, c.min_gain, c.max_gain, c.smooth]
    # (wav, gains, power, action, gate2, lo, hi, up, down, min_gain, max_gain, smooth, B, L, stream)
    for k in range(3):
        args = [p, p, p, None]
        args[k] = None
        assert f(*args, *rule, 4, 320, None) == -2, k
    assert f(None, p, p, p, *rule, 4, 320, None) == -2
    assert f(p, p, p, None, *rule, 0, 320, None) == -1
    assert f(p, p, p, p, *rule, 4, 0, None) == -1
    for k, v in ((0, 0.0), (1, 0.0), (2, c.lo), (3, 1.0), (4, 1.0), (4, 0.0), (5, 0.0), (5, 2.0), (6, 0.5), (7, 0.0), (7, 1.5),
                 (0, float("nan"))):
        args = list(rule)
        args[k] = v
        assert f(p, p, p, None, *args, 4, 320, None) == -4, (k, v)


def test_mix_rooms_dyn_argument_checks():
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    f = lib.hilc_mix_rooms_dyn
    # (wav, room, score, top_k, gains, limiter, ceiling, release, sub, action, mixed, speakers, B, L, stream)
    ok = [p, p, p, 3, p, p, 0.9, 0.99, 32, None, q, p]
    for k in (0, 1, 2, 10, 11):
        for rows in ((p, p), (None, p), (p, None), (None, None)):
            args = list(ok)
            args[4], args[5] = rows
            args[k] = None
            assert f(*args, 4, 320, None) == -2, k
    assert f(*ok, 0, 320, None) == -1
    assert f(*ok, 4, 0, None) == -1
    for top_k in (0, 9, -1):
        args = list(ok)
        args[3] = top_k
        assert f(*args, 4, 320, None) == -4, top_k
    for k, v in ((8, 15), (8, 513), (8, 0), (6, 0.0), (6, 1.5), (7, 0.0), (7, 1.0), (6, float("nan"))):
        args = list(ok)
        args[k] = v
        assert f(*args, 4, 320, None) == -4, (k, v)
    assert f(*ok, 4, mixer.MAX_LIMIT_L + 1, None) == -4                          # the limiter's longest hop


def test_mix_dyn_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hilcodec_amd.ops  # noqa: F401  (registers the ops)
    for name in ("mix_gains", "mix_rooms_dyn"):
        assert hasattr(torch.ops.hilcodec, name), name
    sch = str(torch.ops.hilcodec.mix_gains.default._schema)
    assert "Tensor(a!) gains" in sch and "Tensor(b!) power" in sch
    sch = str(torch.ops.hilcodec.mix_rooms_dyn.default._schema)
    assert "Tensor(a!)? limiter" in sch and "Tensor(b!) mixed" in sch and "Tensor(c!) speakers" in sch and "Tensor? gains" in sch
    B, L = 5, 294
    c, lim = LevelConfig(), LimitConfig()
    rule = (c.gate2, c.lo, c.hi, c.up, c.down, c.min_gain, c.max_gain, c.smooth)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with FakeTensorMode():
        wav, mixed = torch.empty(B, 1, L), torch.empty(B, 1, L)
        gains, power, limiter, score = f64(B, 2), f64(B), f64(B, 2), f64(B)
        assert torch.ops.hilcodec.mix_gains(wav, gains, power, None, *rule) is None
        assert torch.ops.hilcodec.mix_gains(wav, gains, power, i32(B), *rule) is None
        for g, l in ((gains, limiter), (None, limiter), (gains, None), (None, None)):
            assert torch.ops.hilcodec.mix_rooms_dyn(wav, i32(B), score, 3, g, l, lim.ceiling, lim.release, lim.sub, None, mixed,
                                                    i32(B)) is None
        assert gains.shape == (B, 2) and gains.dtype == torch.float64 and limiter.shape == (B, 2) and mixed.shape == (B, 1, L)
    with pytest.raises(RuntimeError):                      # no CPU fallback
        torch.ops.hilcodec.mix_gains(torch.zeros(B, 1, L), f64(B, 2), f64(B), None, *rule)
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.mix_rooms_dyn(torch.zeros(B, 1, L), i32(B), f64(B), 3, f64(B, 2), f64(B, 2), 0.9, 0.99, 32, None,
                                         torch.zeros(B, 1, L), i32(B))
    with pytest.raises(RuntimeError):                      # the state row and its rule come together
        hilcodec_amd.ops.mix_rooms_dyn(torch.zeros(B, 1, L), i32(B), f64(B), 3, torch.zeros(B, 1, L), i32(B), limiter=f64(B, 2))


# ---------------------------------------------------------------- Dynamics and mix_rooms(dynamics=)
def test_dynamics_and_mix_rooms_errors():
    import hilcodec_amd
    for batch in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            Dynamics(batch, device="cpu")
    for kw in (dict(level=LimitConfig()), dict(limit=LevelConfig()), dict(level=1.0)):
        with pytest.raises(ValueError):
            Dynamics(2, device="cpu", **kw)
    d = Dynamics(3, LevelConfig(), LimitConfig(), device="cpu")
    assert d.gains.tolist() == [[1.0, 1.0]] * 3 and d.power.tolist() == [0.0] * 3 and d.limiter.tolist() == [[0.0, 1.0]] * 3
    assert d.gains.dtype == d.power.dtype == d.limiter.dtype == torch.float64
    d.gains += 1
    d.power += 1
    d.limiter += 1
    d.reset([1])
    assert d.gains.tolist() == [[2.0, 2.0], [1.0, 1.0], [2.0, 2.0]] and d.power.tolist() == [1.0, 0.0, 1.0]
    assert d.limiter.tolist() == [[1.0, 2.0], [0.0, 1.0], [1.0, 2.0]]
    d.reset()
    assert d.gains.tolist() == [[1.0, 1.0]] * 3 and d.power.tolist() == [0.0] * 3 and d.limiter.tolist() == [[0.0, 1.0]] * 3
    only = Dynamics(2, limit=LimitConfig(), device="cpu")
    assert only.gains is None and only.power is None and only.limiter.shape == (2, 2)
    wav, room = torch.zeros(3, 1, 8), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        hilcodec_amd.mix_rooms(wav, room, dynamics=LimitConfig())                # the state object, not a config
    with pytest.raises(ValueError):
        hilcodec_amd.mix_rooms(wav, room, dynamics=only)                         # 2 slots for 3 rows
    with pytest.raises(RuntimeError):                                            # no CPU fallback
        hilcodec_amd.mix_rooms(wav, room, dynamics=d)
