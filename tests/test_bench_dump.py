"""bench.py --dump-outputs and --full (host logic only, no GPU): a small output is
written whole, a large one as the same fixed sample in every run, both as float32
within the value budget; --full is off by default."""
import os
import sys

import numpy as np
import torch

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_full_and_dump_are_off_by_default():
    args = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None
    args = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert args.full is True and args.dump_outputs == "d"


def test_small_output_is_dumped_whole(tmp_path):
    y = torch.arange(2 * 3 * 5, dtype=torch.float64).reshape(2, 3, 5)
    bench.dump_outputs(str(tmp_path / "a"), y, 0, 1)
    got = np.load(tmp_path / "a" / "y.npy")
    assert got.dtype == np.float32 and np.array_equal(got, y.reshape(-1).numpy())


def test_large_output_is_the_same_sample_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    y = torch.randn(7, 11, 13, 5, generator=torch.Generator().manual_seed(3))
    for d, rank in (("a", 0), ("b", 0), ("c", 1)):
        bench.dump_outputs(str(tmp_path / d), y, rank, 2)
    a = np.load(tmp_path / "a" / "y_rank0.npy")
    assert a.dtype == np.float32 and a.shape == (500,)
    assert np.array_equal(a, np.load(tmp_path / "b" / "y_rank0.npy"))
    assert np.array_equal(a, np.load(tmp_path / "c" / "y_rank1.npy"))
    # every dumped value is an element of the output, and the sample is spread over it
    flat = y.reshape(-1).numpy()
    assert np.isin(a, flat).all() and len(np.unique(a)) > 400
    assert sorted(os.listdir(tmp_path / "a")) == ["y_rank0.npy"]
