"""bench.py's command line and its --dump-outputs writer (no GPU needed)."""
import os
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_full_and_dump_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_whole_small_arrays_and_a_fixed_sample_of_large_ones(tmp_path,
                                                                                  monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    small = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    big = np.arange(5000, dtype=np.float32).reshape(5, 1000) * 0.5
    losses = np.array([0.25, 1.5], dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "losses": losses})
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "losses.npy", "small.npy"]
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "big", "losses")}
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], small)
    assert got["losses"].dtype == np.float64 and np.array_equal(got["losses"], losses)
    s = got["big"]
    assert s.dtype == np.float32 and s.shape == (1000,)
    idx = (s * 2).astype(np.int64)                 # big[i] = i / 2: the sampled indices
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 5000
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))   # the same sample every run
