"""bench.py's command line and --dump-outputs writer (CPU only): what a run without --full leaves out is
behind --full, and a dumped output is float32, bounded in size and the same positions from run to run."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    b = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert b.full is True and b.dump_outputs == "somewhere"


def test_write_checksums_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--write-checksums")
    assert _parse(monkeypatch, "--full", "--write-checksums").write_checksums is True


def test_dump_outputs_whole_and_sampled(tmp_path):
    small = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    n_big = 3 * (bench.DUMP_MAX_ELEMS // 2 + 7)  # an odd multiple of 3 above the limit
    big = (torch.arange(n_big, dtype=torch.int64) % 251).to(torch.bfloat16).reshape(-1, 3)  # exact in bf16
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    info = bench.dump_outputs(d1, [("small", small), ("big", big)])
    bench.dump_outputs(d2, [("small", small), ("big", big)])
    s, b = np.load(os.path.join(d1, "small.npy")), np.load(os.path.join(d1, "big.npy"))
    assert s.dtype == np.float32 and b.dtype == np.float32
    np.testing.assert_array_equal(s, small.numpy())                      # whole, in its own shape
    idx = bench.dump_sample_index("big", n_big)
    assert b.shape == (bench.DUMP_MAX_ELEMS,) and idx.shape == (bench.DUMP_MAX_ELEMS,)
    assert int(idx.min()) >= 0 and int(idx.max()) < n_big and bool((idx[1:] >= idx[:-1]).all())
    np.testing.assert_array_equal(b, (idx % 251).to(torch.float32).numpy())  # the values at the drawn positions
    np.testing.assert_array_equal(b, np.load(os.path.join(d2, "big.npy")))   # the same positions every run
    assert info["small.npy"] == {"elements": 30, "written": 30, "sampled": False}
    assert info["big.npy"] == {"elements": n_big, "written": bench.DUMP_MAX_ELEMS, "sampled": True}
    # at most 6 outputs per workload (conv training: 5), each at most 8 MB + the .npy header: under 64 MB in all
    assert 6 * os.path.getsize(os.path.join(d1, "big.npy")) < 64 * 10 ** 6


def test_dump_outputs_names_ranks_apart_and_shares_the_limit(tmp_path):
    """N ranks: <name>_rank<r>.npy each, a rank's share of the limit DUMP_MAX_ELEMS // N elements per output, so
    6 outputs x 8 ranks stay under 64 MB together."""
    world = 8
    big = torch.ones(bench.DUMP_MAX_ELEMS // world + 1)
    fits = torch.ones(bench.DUMP_MAX_ELEMS // world)
    for r in range(world):
        info = bench.dump_outputs(str(tmp_path), [("out", big), ("fits", fits)], world=world, rank=r)
        assert info[f"out_rank{r}.npy"] == {"elements": big.numel(), "written": bench.DUMP_MAX_ELEMS // world,
                                            "sampled": True}
        assert info[f"fits_rank{r}.npy"]["sampled"] is False
    files = sorted(os.listdir(str(tmp_path)))
    assert files == sorted([f"out_rank{r}.npy" for r in range(world)] + [f"fits_rank{r}.npy" for r in range(world)])
    per_output = sum(os.path.getsize(os.path.join(str(tmp_path), f"out_rank{r}.npy")) for r in range(world))
    assert 6 * per_output < 64 * 10 ** 6
