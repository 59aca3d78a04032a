"""bench.py's output dump without a GPU: the sample of windows `--dump-outputs` writes is fixed, seeded and within the
size budget, the arrays are float32 and hold exactly the sampled windows' rows."""
import os
import sys

import numpy as np
import torch

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_a_fixed_seeded_sample_within_the_budget(tmp_path):
    import bench

    g = torch.Generator().manual_seed(3)
    out = {"note": torch.rand((256, 172, 88), generator=g), "onset": torch.rand((256, 172, 88), generator=g),
           "contour": torch.rand((256, 172, 264), generator=g)}
    dumps = []
    for run in ("a", "b"):
        bench.dump_outputs(torch, out, str(tmp_path / run))
        dumps.append({k: np.load(str(tmp_path / run / f"{k}.npy")) for k in out})
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["contour.npy", "note.npy", "onset.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f"{k}.npy")) for k in out) <= 64_000_000
    a, b = dumps
    n = a["note"].shape[0]
    assert 128 < n < 256
    # the sampled windows are the same for every array and every run, in order: find them through the note map
    idx = [int(np.flatnonzero((out["note"].numpy() == a["note"][i]).all(axis=(1, 2)))[0]) for i in range(n)]
    assert idx == sorted(set(idx))
    for k in out:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], out[k].numpy()[idx]), k


def test_dump_outputs_keeps_a_small_batch_whole(tmp_path):
    import bench

    out = {"note": torch.rand((16, 172, 88)), "onset": torch.rand((16, 172, 88)), "contour": torch.rand((16, 172, 264))}
    bench.dump_outputs(torch, out, str(tmp_path))
    for k in out:
        assert np.array_equal(np.load(str(tmp_path / f"{k}.npy")), out[k].numpy()), k
