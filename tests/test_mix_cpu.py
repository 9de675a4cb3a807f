"""CPU: the room mixer — the hilc_mix_levels / hilc_mix_rooms entry points (additive under ABI 16) and their argument checks, their
custom ops and fake kernels, MixConfig, and the rules (mixer.MixModel) on hand-built cases with literal expected values.  (No kernel
is launched here.)"""
import ctypes

import numpy as np
import pytest
import torch

from hilcodec_amd import mixer
from hilcodec_amd.mixer import MixConfig, MixModel
from tests.hops import assert_entry_points

NEW = ("hilc_mix_levels", "hilc_mix_rooms")


def test_mix_symbols_exported_and_declared():
    assert_entry_points(NEW, in_abi16_line=True)


def test_mix_levels_argument_checks():
    from hilcodec_amd._lib import lib
    p = ctypes.c_void_p(16)
    f = lib.hilc_mix_levels
    # (wav, score, action, B, L, stream)
    assert f(None, p, None, 4, 320, None) == -2
    assert f(p, None, None, 4, 320, None) == -2
    assert f(None, p, p, 4, 320, None) == -2
    assert f(p, p, None, 0, 320, None) == -1
    assert f(p, p, None, 4, 0, None) == -1
    assert f(p, p, p, -1, 320, None) == -1


def test_mix_rooms_argument_checks():
    from hilcodec_amd._lib import lib
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    f = lib.hilc_mix_rooms
    # (wav, room, score, top_k, mixed, speakers, B, L, stream)
    ok = [p, p, p, 3, q, p]
    for k in (0, 1, 2, 4, 5):
        args = list(ok)
        args[k] = None
        assert f(*args, 4, 320, None) == -2, k
    assert f(*ok, 0, 320, None) == -1
    assert f(*ok, 4, 0, None) == -1
    for top_k in (0, 9, -1, 64):
        args = list(ok)
        args[3] = top_k
        assert f(*args, 4, 320, None) == -4, top_k


def test_mix_ops_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hilcodec_amd.ops  # noqa: F401  (registers the ops)
    for name in ("mix_levels", "mix_rooms"):
        assert hasattr(torch.ops.hilcodec, name), name
    assert "Tensor(a!) score" in str(torch.ops.hilcodec.mix_levels.default._schema)
    sch = str(torch.ops.hilcodec.mix_rooms.default._schema)
    assert "Tensor(a!) mixed" in sch and "Tensor(b!) speakers" in sch
    B, L = 5, 294
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        wav, score = torch.empty(B, 1, L), torch.empty(B, dtype=torch.float64)
        mixed, speakers = torch.empty(B, 1, L), i32(B)
        assert torch.ops.hilcodec.mix_levels(wav, score, None) is None
        assert torch.ops.hilcodec.mix_levels(wav, score, i32(B)) is None
        assert torch.ops.hilcodec.mix_rooms(wav, i32(B), score, 3, mixed, speakers) is None
        # the outputs are the caller's buffers: their shapes and dtypes are what the kernels write
        assert mixed.shape == (B, 1, L) and mixed.dtype == torch.float32
        assert speakers.shape == (B,) and speakers.dtype == torch.int32 and score.dtype == torch.float64
    with pytest.raises(RuntimeError):                      # no CPU fallback
        torch.ops.hilcodec.mix_levels(torch.zeros(B, 1, L), torch.zeros(B, dtype=torch.float64), None)
    with pytest.raises(RuntimeError):
        torch.ops.hilcodec.mix_rooms(torch.zeros(B, 1, L), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.float64), 3,
                                     torch.zeros(B, 1, L), torch.zeros(B, dtype=torch.int32))


def test_public_names():
    import hilcodec_amd
    assert hilcodec_amd.MixConfig is MixConfig and callable(hilcodec_amd.mix_rooms)
    with pytest.raises(ValueError):
        hilcodec_amd.mix_rooms(torch.zeros(2, 1, 8), torch.zeros(2, dtype=torch.int32), top_k=9)
    with pytest.raises(RuntimeError):                      # no CPU fallback
        hilcodec_amd.mix_rooms(torch.zeros(2, 1, 8), torch.zeros(2, dtype=torch.int32))


def test_mix_config():
    assert MixConfig().top_k == 3
    for k in range(1, 9):
        assert MixConfig(k).top_k == k
    assert MixConfig(np.int64(2)).top_k == 2
    for bad in (0, 9, -1, True, False, 2.0, "3", None):
        with pytest.raises(ValueError):
            MixConfig(bad)
    assert mixer.MAX_TOP_K == 8


# ---------------------------------------------------------------- the rules
def rows(*values, L=4):
    """wav [B, 1, L]: row b constant at values[b]"""
    return torch.tensor(values, dtype=torch.float32).view(-1, 1, 1).repeat(1, 1, L).contiguous()


def flat(mixed):
    """a mix of constant rows, as one value per row"""
    assert torch.equal(mixed, mixed[:, :, :1].expand_as(mixed))
    return mixed[:, 0, 0].tolist()


def test_model_level_is_the_lane_ordered_float64_sum():
    # lane 0 holds x[0]^2 + x[64]^2 = (1 + 1.5625) 2^-54 = 0.64 ulp(1), lane 1 holds x[1]^2 = 1: E = 1 + 2^-52.  In index order both
    # small squares (0.25 and 0.39 ulp) would be rounded away one by one and E would be 1
    x = torch.zeros(1, 1, 65)
    x[0, 0, 0], x[0, 0, 1], x[0, 0, 64] = 2.0 ** -27, 1.0, 1.25 * 2.0 ** -27
    m = MixModel(1, MixConfig(1))
    m.step(x, [0])
    assert m.score.dtype == torch.float64 and m.score.tolist() == [1.0 + 2.0 ** -52]
    m = MixModel(1, MixConfig(1))
    m.step(x[:, :, :64], [0])
    assert m.score.tolist() == [1.0]                                             # 2^-54 + 1 rounds to 1 in float64
    m = MixModel(2, MixConfig(1))
    m.step(torch.tensor([[[0.5]], [[-3.0]]]), [-1, -1])                          # L = 1; every slot is scored, whatever its room
    assert m.score.tolist() == [0.25, 9.0]


def test_model_ties_go_to_the_lowest_slot():
    m = MixModel(4, MixConfig(2))
    mixed, sp = m.step(rows(0.25, 0.25, 0.25, 0.25), [0, 0, 0, 0])
    assert sp.dtype == torch.int32 and sp.tolist() == [1, 1, 0, 0]
    assert mixed.dtype == torch.float32 and mixed.shape == (4, 1, 4)
    assert flat(mixed) == [0.25, 0.25, 0.5, 0.5]
    # score first, slot second: the louder slot 3 comes before the tied 0 and 1
    m = MixModel(4, MixConfig(2))
    mixed, sp = m.step(rows(0.25, 0.25, 0.125, 0.5), [0, 0, 0, 0])
    assert sp.tolist() == [1, 0, 0, 1]
    assert flat(mixed) == [0.5, 0.75, 0.75, 0.25]


def test_model_top_k_larger_than_the_room():
    m = MixModel(5, MixConfig(8))
    mixed, sp = m.step(rows(0.125, 0.25, 0.5, 0.0625, 0.75), [1, 1, 4, 1, 4])
    assert sp.tolist() == [1, 1, 1, 1, 1]
    assert flat(mixed) == [0.3125, 0.1875, 0.75, 0.375, 0.5]


def test_model_lone_member_hears_zero():
    m = MixModel(3, MixConfig(3))
    mixed, sp = m.step(rows(0.5, 0.25, 0.125), [2, 0, 0])
    assert sp.tolist() == [1, 1, 1]
    assert flat(mixed) == [0.0, 0.125, 0.25]


def test_model_top_k_1():
    m = MixModel(4, MixConfig(1))
    mixed, sp = m.step(rows(0.125, 0.5, 0.25, 0.75), [0, 0, 0, -1])
    assert sp.tolist() == [0, 1, 0, 0]
    assert flat(mixed) == [0.5, 0.0, 0.5, 0.0]                                   # the speaker hears 0, the others hear the speaker


def test_model_all_zero_room_has_no_speakers():
    m = MixModel(4, MixConfig(3))
    mixed, sp = m.step(rows(0.0, 0.0, 0.5, 0.0), [0, 0, 1, 0])
    assert sp.tolist() == [0, 0, 1, 0]
    assert flat(mixed) == [0.0, 0.0, 0.0, 0.0]
    assert m.score.tolist() == [0.0, 0.0, 1.0, 0.0]


def test_model_clamp():
    m = MixModel(4, MixConfig(3))
    mixed, sp = m.step(rows(0.9, 0.9, 0.9, 0.0), [0, 0, 0, 0])
    assert sp.tolist() == [1, 1, 1, 0]
    want_two = float(np.float32(0.9) + np.float32(0.9))                          # 1.8 in fp32: clamped too
    assert want_two > 1.0
    assert flat(mixed) == [1.0, 1.0, 1.0, 1.0]                                   # three speakers at 0.9 give 1.0
    mixed, _ = m.step(rows(-0.9, -0.9, -0.9, 0.0), [0, 0, 0, 0])
    assert flat(mixed) == [-1.0, -1.0, -1.0, -1.0]
    # the sum is rounded in fp32 term by term, in ascending slot order: (0.75 + 2^-25) + -0.75 = 0 (the tie rounds to even), while
    # 0.75 + (2^-25 + -0.75) would be 2^-25
    m = MixModel(4, MixConfig(3))
    mixed, _ = m.step(rows(0.75, 2.0 ** -25, -0.75, 0.0), [0, 0, 0, 0])
    assert flat(mixed)[3] == 0.0


def test_model_no_room_gives_a_zero_row():
    m = MixModel(3, MixConfig(3))
    mixed, sp = m.step(rows(0.5, 0.25, 0.125), [-1, 0, 0])
    assert sp.tolist() == [0, 1, 1]
    assert flat(mixed) == [0.0, 0.125, 0.25]                                     # slot 0 hears nothing and nobody hears it
    assert m.score.tolist() == [1.0, 0.25, 0.0625]                               # but it is scored


def test_model_score_halves_and_action_resets():
    m = MixModel(3, MixConfig(1))
    loud = rows(0.5, 0.25, 0.0)
    quiet = rows(0.0, 0.25, 0.0)
    room = [0, 0, 0]
    _, sp = m.step(loud, room)
    assert m.score.tolist() == [1.0, 0.25, 0.0] and sp.tolist() == [1, 0, 0]
    _, sp = m.step(quiet, room)                                                  # slot 0 falls silent: its score halves per hop
    assert m.score.tolist() == [0.5, 0.25, 0.0] and sp.tolist() == [1, 0, 0]
    mixed, sp = m.step(quiet, room)                                              # a tie at 0.25: the lowest slot
    assert m.score.tolist() == [0.25, 0.25, 0.0] and sp.tolist() == [1, 0, 0]
    assert flat(mixed) == [0.0, 0.0, 0.0]                                        # the held speaker's row is silent
    mixed, sp = m.step(quiet, room)
    assert m.score.tolist() == [0.125, 0.25, 0.0] and sp.tolist() == [0, 1, 0]
    assert flat(mixed) == [0.25, 0.0, 0.25]
    # an action clears the previous score on that hop
    m = MixModel(3, MixConfig(1))
    m.step(loud, room)
    _, sp = m.step(quiet, room, action=[1, 0, 0])
    assert m.score.tolist() == [0.0, 0.25, 0.0] and sp.tolist() == [0, 1, 0]
    _, sp = m.step(quiet, room, action=torch.tensor([0, -1, 0], dtype=torch.int32))   # any non-zero action; E still counts
    assert m.score.tolist() == [0.0, 0.25, 0.0] and sp.tolist() == [0, 1, 0]
