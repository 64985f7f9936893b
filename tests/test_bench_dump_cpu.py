"""bench.py's --dump-outputs writer and its new options (no GPU needed).

dump_outputs writes small arrays whole and a larger one as a fixed sample at
seeded flat indices of its logical (row-major) order, whatever its strides,
so two dumps of the same shape hold the same elements.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_small_whole_large_sampled(tmp_path):
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    # larger than the sample, and a transposed (strided) view like the DP
    # table's (B, n_int, Q, L) view of a site-major buffer
    shape = (3, 5, 700, 500)
    assert int(np.prod(shape)) > bench.DUMP_SAMPLE
    base = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    big = base.transpose(2, 3)
    assert not big.is_contiguous()
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), {"small": small, "big": big})
    a_small = np.load(tmp_path / "a" / "small.npy")
    assert a_small.dtype == np.float32 and a_small.shape == (3, 4)
    np.testing.assert_array_equal(a_small, small.numpy())
    a_big = np.load(tmp_path / "a" / "big.npy")
    assert a_big.dtype == np.float32 and a_big.shape == (bench.DUMP_SAMPLE,)
    np.testing.assert_array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    # the sample is the logical array's elements at the documented indices
    flat = np.sort(np.random.default_rng(0).integers(0, big.numel(), size=bench.DUMP_SAMPLE))
    np.testing.assert_array_equal(a_big, big.numpy().reshape(-1)[flat])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 64 * 1024 * 1024


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
