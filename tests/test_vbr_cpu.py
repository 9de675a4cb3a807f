"""CPU: quality-targeted variable bitrate of the sender — the hilc_vbr_select entry point (additive under ABI 16) and its argument
checks, its custom op and fake kernel, VbrConfig, the constructor checks of GraphedEncodeHop(vbr=), and the rules (vbr.VbrModel) on
hand-built cases with literal expected values.  (No kernel is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd import vbr
from hilcodec_amd.vbr import VbrConfig, VbrModel
from tests.hops import assert_entry_points

NAME = "hilc_vbr_select"


def test_vbr_symbol_exported_and_declared():
    assert_entry_points([NAME], in_abi16_line=True)


def test_vbr_select_argument_checks():
    """every call here returns before the launch"""
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    f = lib.hilc_vbr_select
    # (z, indices, codebooks, n_per_stream, action, hold, credit, n_eff, distortion, B, T, C, K, Nq, n, n_lo, rho, stage_bits,
    #  rate_bits, burst_bits, stream)
    ptrs = [p, q, p, None, None, None, None, q, q]
    dims = dict(B=4, T=1, C=128, K=1024, Nq=12, n=8, n_lo=1)
    tail = dict(rho=0.01, stage_bits=10, rate_bits=0, burst_bits=0)

    def call(ptr_list=ptrs, **kw):
        d = dict(dims, **{k: v for k, v in kw.items() if k in dims})
        t = dict(tail, **{k: v for k, v in kw.items() if k in tail})
        return f(*ptr_list, *d.values(), *t.values(), None)

    for k in (0, 1, 2, 7, 8):                               # the required pointers
        bad = list(ptrs)
        bad[k] = None
        assert call(bad) == -2, k
    assert call(rate_bits=80, burst_bits=640) == -2         # a cap without a credit row
    for name in ("B", "T", "C", "K", "Nq"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(n=0) == -5 and call(n=13) == -5             # outside [1, Nq]
    assert call(n_lo=0) == -5 and call(n_lo=9) == -5        # outside [1, n]
    for rho in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(rho=rho) == -5, rho
    capped = list(ptrs)
    capped[6] = q
    assert call(capped, n_lo=2, rate_bits=19, burst_bits=80) == -5         # the rate does not pay for the floor
    assert call(capped, rate_bits=80, burst_bits=79) == -5                # a burst below the rate
    assert call(capped, stage_bits=0, rate_bits=80, burst_bits=80) == -5
    assert call(capped, rate_bits=1 << 30, burst_bits=(1 << 30) + 1) == -5
    assert call(C=96) == -4 and call(C=576) == -4           # not a multiple of 64; more than 512
    assert call(Nq=40, n=33) == -4                          # more than 32 stages


def test_vbr_op_registered_with_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hilcodec_amd.ops  # noqa: F401  (registers the ops)
    assert hasattr(torch.ops.hilcodec, "vbr_select")
    sch = str(torch.ops.hilcodec.vbr_select.default._schema)
    assert "Tensor(a!) indices" in sch and "Tensor(b!)? credit" in sch
    B, T, C, n = 5, 3, 128, 8
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        z, idx, cb = torch.empty(B, T, C), torch.empty(n, B, T, dtype=torch.int64), torch.empty(12, 1024, C)
        for rows in ((None, None, None, None), (i32(B), i32(B), i32(B), i32(B))):
            n_eff, D = torch.ops.hilcodec.vbr_select(z, idx, cb, *rows, 1, 0.01, 10 * T, 0, 0)
            assert n_eff.shape == (B,) and n_eff.dtype == torch.int32
            assert D.shape == (B, n + 1) and D.dtype == torch.float64
    with pytest.raises(RuntimeError):                      # no CPU fallback
        torch.ops.hilcodec.vbr_select(torch.zeros(B, T, C), torch.zeros(n, B, T, dtype=torch.int64), torch.zeros(12, 1024, C), None, None,
                                      None, None, 1, 0.01, 10 * T, 0, 0)
    with pytest.raises(RuntimeError):
        hilcodec_amd.ops.vbr_select(torch.zeros(B, T, C), torch.zeros(n, B, T, dtype=torch.int64), torch.zeros(12, 1024, C), 1, 0.01)


def test_vbr_config():
    c = VbrConfig(20.0)
    assert (c.n_min, c.cap_kbps, c.burst_hops) == (1, None, 8)
    assert isinstance(c.rho, float) and c.rho == 10.0 ** (-2.0)
    assert VbrConfig(10, n_min=np.int64(2), cap_kbps=6, burst_hops=1).cap_kbps == 6.0
    for bad in (0, 0.0, -3.0, True, "20", None, float("nan"), float("inf"), 4000.0):
        with pytest.raises(ValueError):
            VbrConfig(bad)
    for bad in (0, -1, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            VbrConfig(20.0, n_min=bad)
        with pytest.raises(ValueError):
            VbrConfig(20.0, burst_hops=bad)
    for bad in (0, 0.0, -6.0, True, "6", float("nan")):
        with pytest.raises(ValueError):
            VbrConfig(20.0, cap_kbps=bad)


def test_bucket_bits():
    assert vbr.bucket_bits(VbrConfig(20.0), 3) == (30, 0, 0)
    assert vbr.bucket_bits(VbrConfig(20.0, cap_kbps=6.0), 1) == (10, 80, 640)                # 6 kbit/s of 13.3 ms hops: 80 bits
    assert vbr.bucket_bits(VbrConfig(20.0, cap_kbps=6.0, burst_hops=3), 2) == (20, 160, 480)
    assert vbr.bucket_bits(VbrConfig(20.0, cap_kbps=1.0), 1) == (10, 13, 104)                # floor(13.33)
    assert vbr.bucket_bits(VbrConfig(20.0, cap_kbps=1.5, n_min=2), 1) == (10, 20, 160)       # exactly the floor's price
    with pytest.raises(ValueError, match="floor"):
        vbr.bucket_bits(VbrConfig(20.0, cap_kbps=1.4, n_min=2), 1)
    with pytest.raises(ValueError, match="floor"):
        vbr.bucket_bits(VbrConfig(20.0, cap_kbps=1.5), 1, fec_stages=3)
    with pytest.raises(ValueError, match="floor"):
        VbrModel(4, VbrConfig(20.0, cap_kbps=0.5), 8, 1)
    with pytest.raises(ValueError):
        vbr.bucket_bits(VbrConfig(20.0, cap_kbps=1e9, burst_hops=1000), 1)


def test_graphed_encode_hop_constructor_checks():
    """the checks come before anything touches the model or the device"""
    from hilcodec_amd.graph_step import GraphedEncodeHop
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="VbrConfig"):
        GraphedEncodeHop(None, 2, 320, 8, dev, vbr=20.0)
    with pytest.raises(ValueError, match="header=True"):
        GraphedEncodeHop(None, 2, 320, 8, dev, fec_stages=2, vbr=VbrConfig(20.0))
    with pytest.raises(ValueError, match="multiple of 320"):
        GraphedEncodeHop(None, 2, 160, 8, dev, vbr=VbrConfig(20.0))
    with pytest.raises(ValueError, match="floor"):
        GraphedEncodeHop(None, 2, 320, 8, dev, vbr=VbrConfig(20.0, cap_kbps=1.0, n_min=2))
    with pytest.raises(ValueError, match="floor"):
        GraphedEncodeHop(None, 2, 320, 8, dev, fec_stages=2, header=True, vbr=VbrConfig(20.0, cap_kbps=1.0))


# ---------------------------------------------------------------- the rules
C = 64
STEPS = (4.0, 2.0, 1.5, 0.25)


def books():
    """4 stages of 2 codewords over 64 channels: codeword 0 is zero, codeword 1 of stage s is STEPS[s] on channel 0"""
    cb = torch.zeros(4, 2, C)
    for s, v in enumerate(STEPS):
        cb[s, 1, 0] = v
    return cb


def hop(codes):
    """z [B, 1, 64] = 8 on channel 0, idx [4, B, 1]: slot b takes codeword codes[b] at every stage"""
    B = len(codes)
    z = torch.zeros(B, 1, C)
    z[:, 0, 0] = 8.0
    idx = torch.tensor(codes, dtype=torch.int64).view(1, B, 1).repeat(4, 1, 1)
    return z, idx


FALLING = [64.0, 16.0, 4.0, 0.25, 0.0625]                  # 8 -> 4 -> 2 -> 0.5 -> 0.25, squared


def test_model_distortion_is_the_lane_ordered_float64_sum():
    # lane 0 holds z[0]^2 + z[64]^2 = (1 + 1.5625) 2^-54 = 0.64 ulp(1), lane 1 holds z[1]^2 = 1: D[0] = 1 + 2^-52.  In channel order
    # both small squares (0.25 and 0.39 ulp) would be rounded away one by one and D[0] would be 1
    z = torch.zeros(1, 1, 128)
    z[0, 0, 0], z[0, 0, 1], z[0, 0, 64] = 2.0 ** -27, 1.0, 1.25 * 2.0 ** -27
    idx = torch.zeros(1, 1, 1, dtype=torch.int64)
    cb = torch.zeros(1, 2, 128)
    cb[0, 0, 1] = 1.0
    D = vbr.distortions(z, idx, cb)
    assert D.dtype == np.float64 and D.shape == (1, 2)
    assert D[0].tolist() == [1.0 + 2.0 ** -52, 2.5625 * 2.0 ** -54]
    # frames add in ascending order after the lane sums; a code outside [0, K) is clamped
    z2 = torch.zeros(1, 3, 128)
    z2[0, 0, 1], z2[0, 1, 5], z2[0, 2, 7] = 1.0, 1.25 * 2.0 ** -27, 1.25 * 2.0 ** -27
    small = 1.5625 * 2.0 ** -54                            # 0.39 ulp(1): (1 + small) + small = 1, but (small + small) + 1 = 1 + 2^-52
    D = vbr.distortions(z2, torch.tensor([[[1, 5, 1]]]), cb)               # 5 -> codeword 1, the zero one
    assert D[0].tolist() == [1.0, 1.0]
    D = vbr.distortions(z2, torch.tensor([[[-1, 1, 1]]]), cb)              # -1 -> codeword 0: frame 0 becomes zero
    assert D[0].tolist() == [1.0, small + small]


def test_model_quality_rule_fires_at_stage_3():
    z, idx = hop([1, 0])
    m = VbrModel(2, VbrConfig(20.0), 4, 1)                 # the bar is 0.64: D[2] = 4 is above it, D[3] = 0.25 below
    n_eff, D, out = m.step(z, idx, books())
    assert n_eff.dtype == torch.int32 and n_eff.tolist() == [3, 4]         # slot 1 never gets there: all 4
    assert D.dtype == torch.float64 and D.tolist() == [FALLING, [64.0] * 5]
    assert out.dtype == torch.int64 and out[:, 0, 0].tolist() == [1, 1, 1, -1] and out[:, 1, 0].tolist() == [0, 0, 0, 0]
    assert idx[:, 0, 0].tolist() == [1, 1, 1, 1]           # the input is not touched
    assert m.credit.dtype == torch.int32 and m.credit.tolist() == [0, 0]
    # <=, with one rounded product on the right: 16 <= 0.25 * 64
    assert vbr.choose(np.array([FALLING]), np.array([4]), np.array([1]), 0.25).tolist() == [1]
    assert vbr.choose(np.array([FALLING]), np.array([4]), np.array([1]), np.nextafter(0.25, 0)).tolist() == [2]


def test_model_floor_and_ceiling():
    z, idx = hop([1, 1, 1])
    cb = books()
    easy = VbrConfig(3.0)                                  # the bar is 32: stage 1 is enough
    assert VbrModel(3, easy, 4, 1).step(z, idx, cb)[0].tolist() == [1, 1, 1]
    assert VbrModel(3, VbrConfig(3.0, n_min=2), 4, 1).step(z, idx, cb)[0].tolist() == [2, 2, 2]
    assert VbrModel(3, easy, 4, 1, fec_stages=3).step(z, idx, cb)[0].tolist() == [3, 3, 3]
    assert VbrModel(3, VbrConfig(3.0, n_min=2), 4, 1, fec_stages=3).step(z, idx, cb)[0].tolist() == [3, 3, 3]
    # the ceiling n_b wins over the floor, and over a rule that has not fired; D repeats past it
    n_eff, D, out = VbrModel(3, VbrConfig(20.0, n_min=3), 4, 1).step(z, idx, cb, n_b=[2, 4, 9])
    assert n_eff.tolist() == [2, 3, 3]
    assert D.tolist() == [[64.0, 16.0, 4.0, 4.0, 4.0], FALLING, FALLING]
    assert out[:, :, 0].t().tolist() == [[1, 1, -1, -1], [1, 1, 1, -1], [1, 1, 1, -1]]
    n_eff, D, _ = VbrModel(3, VbrConfig(20.0), 4, 1).step(z, idx, cb, n_b=torch.tensor([1, 0, 3], dtype=torch.int32))
    assert n_eff.tolist() == [1, 1, 3]                     # n_b is clamped to [1, n]
    assert D[1].tolist() == [64.0, 16.0, 16.0, 16.0, 16.0]


def test_model_bucket_over_several_hops():
    cb = books()
    z, idx = hop([0, 1])                                   # slot 0 always wants all 4 stages, slot 1 one (the bar is 20.2)
    cfg = VbrConfig(5.0, cap_kbps=1.5, burst_hops=2)       # 20 bits per hop = 2 stages, a bucket of 40
    m = VbrModel(2, cfg, 4, 1)
    assert (m.stage_bits, m.rate_bits, m.burst_bits) == (10, 20, 40)
    assert m.credit.tolist() == [40, 40]
    want = [([4, 1], [0, 30]),                             # full buckets stay at 40 (the burst clamp): 40 - 40, 40 - 10
            ([2, 1], [0, 30]),                             # 0 + 20 pays for 2; min(30 + 20, 40) - 10
            ([2, 1], [0, 30])]
    for n_want, credit_want in want:
        n_eff, D, out = m.step(z, idx, cb)
        assert n_eff.tolist() == n_want and m.credit.tolist() == credit_want
        assert D.tolist() == [[64.0] * 5, FALLING]         # the cap does not change what is measured
        assert out[:, 0, 0].tolist() == [0] * n_want[0] + [-1] * (4 - n_want[0])
    # an action refills the bucket before the hop
    n_eff, _, _ = m.step(z, idx, cb, action=[-1, 0])
    assert n_eff.tolist() == [4, 1] and m.credit.tolist() == [0, 30]
    # a held slot keeps its credit, reports n_b and a zero row; the other slot goes on
    n_eff, D, out = m.step(z, idx, cb, n_b=[3, 4], hold=[1, 0])
    assert n_eff.tolist() == [3, 1] and m.credit.tolist() == [0, 30]
    assert D.tolist() == [[0.0] * 5, FALLING]
    assert out[:, 0, 0].tolist() == [0, 0, 0, -1]
    n_eff, _, _ = m.step(z, idx, cb, hold=torch.tensor([0, 2], dtype=torch.int32))
    assert n_eff.tolist() == [2, 4] and m.credit.tolist() == [0, 30]
    # held and started on the same hop: the refill stays
    n_eff, _, _ = m.step(z, idx, cb, action=[3, 0], hold=[1, 0])
    assert n_eff.tolist() == [4, 1] and m.credit.tolist() == [40, 30]
    # the cap never cuts below the floor: n_min = 2 at 20 bits per hop
    m = VbrModel(1, VbrConfig(5.0, n_min=2, cap_kbps=1.5, burst_hops=1), 4, 1)
    for _ in range(3):
        n_eff, _, _ = m.step(z[:1], idx[:, :1], cb)
        assert n_eff.tolist() == [2] and m.credit.tolist() == [0]
    # without a cap the credit row is unused
    m = VbrModel(2, VbrConfig(5.0), 4, 1)
    assert m.step(z, idx, cb)[0].tolist() == [4, 1] and m.credit.tolist() == [0, 0]
