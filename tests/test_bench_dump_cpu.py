"""CPU: bench.py --dump-outputs writes float32 .npy files of at most 64 MB in all, keeping the same seeded sample of batch rows
of every array beyond that."""
import numpy as np
import torch

import bench


def test_dump_small_is_whole_float32(tmp_path):
    idx = torch.randint(0, 1024, (4, 8, 75), dtype=torch.int64)
    wav = torch.randn(4, 1, 320)
    info = bench.dump_outputs(str(tmp_path), {"indices": (idx, 0), "wav": (wav, 0)})
    assert info["rows"] == "all" and info["arrays"] == {"indices": [4, 8, 75], "wav": [4, 1, 320]}
    a, w = np.load(tmp_path / "indices.npy"), np.load(tmp_path / "wav.npy")
    assert a.dtype == np.float32 and w.dtype == np.float32
    assert np.array_equal(a, idx.numpy().astype(np.float32)) and np.array_equal(w, wav.numpy())


def test_dump_large_is_a_fixed_sample_of_the_same_rows(tmp_path):
    B, limit = 64, 1 << 16
    idx = torch.arange(8 * B * 3).view(8, B, 3)                      # streaming layout: batch on axis 1
    wav = torch.arange(B, dtype=torch.float32).view(B, 1, 1).expand(B, 1, 320).contiguous()
    infos = [bench.dump_outputs(str(tmp_path / str(k)), {"indices": (idx, 1), "wav": (wav, 0)}, suffix="_rank1", limit=limit)
             for k in range(2)]
    w = np.load(tmp_path / "0" / "wav_rank1.npy")
    a = np.load(tmp_path / "0" / "indices_rank1.npy")
    assert infos[0]["bytes"] <= limit and w.nbytes + a.nbytes == infos[0]["bytes"] and 0 < w.shape[0] < B
    rows = w[:, 0, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0)                                # sorted, distinct
    assert np.array_equal(a, idx.numpy()[:, rows].astype(np.float32))
    assert np.array_equal(w, np.load(tmp_path / "1" / "wav_rank1.npy")) and infos[0] == {**infos[1], "dir": infos[0]["dir"]}
