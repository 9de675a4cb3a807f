"""`tests.alignment.skew`: the misaligned-but-contiguous views the GPU alignment sweep (tests/test_gpu_alignment.py) hands to the
library really are what they claim — contiguous, equal to the original, and 4 * k bytes behind a 16-byte boundary."""
import pytest
import torch

from tests.alignment import skew, skew_bytes


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
def test_skew_offsets_and_contents(k, dtype):
    t = (torch.arange(2 * 3 * 5) * 7 - 40).to(dtype).view(2, 3, 5)
    v = skew(t, k)
    assert v.dtype == dtype and v.shape == t.shape and v.is_contiguous() and torch.equal(v, t)
    assert v.data_ptr() % 16 == skew_bytes(dtype, k) and v.data_ptr() % 16 != 0
    assert v.data_ptr() % v.element_size() == 0                    # still a legal pointer of its own type
    if dtype != torch.int64:
        assert v.data_ptr() % 16 == 4 * k
    v.add_(1)                                                      # a copy: the original does not move
    assert torch.equal(v, t + 1) and t[0, 0, 0] == -40


def test_skew_of_scalar_sized_and_empty_tail():
    for n in (1, 4, 17):
        t = torch.arange(n, dtype=torch.float32)
        for k in (1, 2, 3):
            v = skew(t, k)
            assert torch.equal(v, t) and v.data_ptr() % 16 == 4 * k


@pytest.mark.parametrize("k", [1, 2, 3])
def test_single_clip_slice_is_contiguous_and_misaligned(k):
    """The ordinary case the sweep stands for: one recording trimmed at the front.  With B = 1 the slice is `is_contiguous()` — size-1
    dimensions do not count — so `.contiguous()` returns it unchanged and its pointer is 4 * k bytes off."""
    T = 1280
    rec = torch.arange(T + 8, dtype=torch.float32).view(1, 1, T + 8)
    assert rec.data_ptr() % 16 == 0
    s = rec[:, :, k:k + T]
    assert s.is_contiguous() and s.contiguous() is s and s.contiguous().float() is s
    assert s.data_ptr() % 16 == 4 * k
    assert torch.equal(skew(s, k), s) and skew(s, k).data_ptr() % 16 == s.data_ptr() % 16
    two = torch.zeros(2, 1, T + 8)[:, :, k:k + T]                   # B = 2: the same slice is NOT contiguous, `.contiguous()` copies it
    assert not two.is_contiguous() and two.contiguous().data_ptr() % 16 == 0
