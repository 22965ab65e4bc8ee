"""bench.py --dump-outputs without a GPU: the sample of an output is the same from run to run, stays inside its budget, keeps
float32 / float64 and converts trees to float32; the options parse with the side measurements off by default."""
import os
import sys

import numpy as np
import torch

import bench


def _colmajor(a):
    """numpy (Julia shape) -> column-major torch tensor, as the workloads hold them"""
    t = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(a).T))
    return t.permute(*reversed(range(a.ndim))) if a.ndim > 1 else t


def test_small_outputs_are_written_whole():
    a = np.random.default_rng(0).standard_normal((64, 13, 5))
    s = bench.dump_sample(_colmajor(a), 1 << 20)
    assert s.dtype == np.float64 and s.shape == a.shape and np.array_equal(s, a)
    f = bench.dump_sample(_colmajor(a.astype(np.float32)), 1 << 20)
    assert f.dtype == np.float32 and np.array_equal(f, a.astype(np.float32))


def test_large_outputs_are_sampled_by_columns_of_the_batch():
    a = np.random.default_rng(1).standard_normal((32, 4, 300))
    budget = 32 * 4 * 8 * 20 + 5                        # 20 columns fit
    s = bench.dump_sample(_colmajor(a), budget)
    assert s.shape == (32, 4, 20) and s.nbytes <= budget
    assert np.array_equal(s, bench.dump_sample(_colmajor(a), budget))
    cols = [j for j in range(300) if any(np.array_equal(s[..., k], a[..., j]) for k in range(20))]
    assert len(cols) == 20 and cols == sorted(cols)


def test_outputs_with_huge_columns_are_sampled_by_elements_in_column_major_order():
    a = np.random.default_rng(2).standard_normal((1000, 3))
    budget = 8 * 200                                    # not even 8 columns: elements
    s = bench.dump_sample(_colmajor(a), budget)
    assert s.ndim == 1 and 0 < s.size <= 200 and s.nbytes <= budget
    assert np.array_equal(s, bench.dump_sample(_colmajor(a), budget))
    flat = a.reshape(-1, order="F")
    pos = [int(np.flatnonzero(flat == v)[0]) for v in s]
    assert pos == sorted(pos)
    sliced = _colmajor(np.asfortranarray(np.random.default_rng(3).standard_normal((1000, 5))))[:, :3]   # a view, as a shard is
    assert bench.dump_sample(sliced, budget).size > 0


def test_trees_become_float32():
    t = torch.from_numpy(np.array([True, False, True]))
    s = bench.dump_sample(t, 1 << 10)
    assert s.dtype == np.float32 and s.tolist() == [1.0, 0.0, 1.0]


def test_dump_outputs_writes_one_npy_per_output_within_64_mb(tmp_path):
    big = _colmajor(np.zeros((4096, 13, 200)))           # 85 MB
    small = _colmajor(np.ones((4096, 400)))
    bench.dump_outputs({"wpdall": big, "iwpdall": small}, str(tmp_path / "out"))
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == ["iwpdall.npy", "wpdall.npy"]
    assert sum(os.path.getsize(tmp_path / "out" / n) for n in names) <= 64_000_000
    for n in names:
        assert np.load(tmp_path / "out" / n).dtype in (np.float32, np.float64)


def test_options_default_to_a_lean_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"

