"""bench.py --dump-outputs without a GPU: the snapshot of a step's outputs is float32, stays within the size budget, keeps small
arrays whole, and samples larger ones at the same elements on every run (so that two builds can be compared output for output)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return {"loss": torch.rand((), generator=g), "image": torch.rand(8, 3, 1024, 1024, generator=g),
            "radii": torch.randint(0, 60, (8, 98562), generator=g, dtype=torch.int32), "grad_xyz": torch.randn(98562, 3, generator=g),
            "grad_shs": torch.randn(98562, 16, 3, generator=g), "grad_color_w": torch.randn(48, generator=g), "grad_unused": None}


def test_small_outputs_are_written_whole(tmp_path):
    a = {"loss": torch.tensor(0.25), "image": torch.rand(2, 3, 64, 48), "radii": torch.arange(10, dtype=torch.int32)}
    bench.write_outputs(str(tmp_path), bench.snapshot_outputs(a))
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "loss.npy", "radii.npy"]
    for k, v in a.items():
        x = np.load(tmp_path / (k + ".npy"))
        assert x.dtype == np.float32 and x.shape == tuple(v.shape) and np.array_equal(x, v.float().numpy())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    a = _arrays(0)
    s1, s2 = bench.snapshot_outputs(a), bench.snapshot_outputs(_arrays(0))
    assert set(s1) == {"loss", "image", "radii", "grad_xyz", "grad_shs", "grad_color_w"}
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    bench.write_outputs(str(tmp_path), s1)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(s1["grad_color_w"], a["grad_color_w"].numpy())          # small arrays stay whole
    img = a["image"].reshape(-1).numpy()
    assert 0 < s1["image"].size < img.size and np.isin(s1["image"], img).all()
    # the sample size depends on the shapes only; other inputs give other values
    s3 = bench.snapshot_outputs(_arrays(1))
    assert s3["image"].shape == s1["image"].shape and not np.array_equal(s3["image"], s1["image"])
