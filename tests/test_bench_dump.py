"""bench.py --dump-outputs and --steps on the CPU: the dump helper writes float32 .npy files, keeps the total under its cap with the same
seeded sample every time, and the argument parser refuses a run without timed steps."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_small_outputs_are_written_whole(tmp_path):
    bench = _bench()
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    info = bench.dump_outputs(str(tmp_path / "out"), {"audio": a})
    got = np.load(tmp_path / "out" / "audio.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4) and np.array_equal(got, a)
    assert info["arrays"]["audio"] == {"shape": [3, 4], "dtype": "float32", "sampled": False}


def test_large_outputs_are_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    a = np.random.default_rng(3).standard_normal(10_000).astype(np.float32)
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), {"audio": a})
        assert info["arrays"]["audio"]["sampled"]
    x, y = np.load(tmp_path / "a" / "audio.npy"), np.load(tmp_path / "b" / "audio.npy")
    assert x.dtype == np.float32 and 0 < x.nbytes <= 4096 and np.array_equal(x, y)
    assert np.isin(x, a).all()
    assert os.path.getsize(tmp_path / "a" / "audio.npy") < 4096 + 256


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_a_run_needs_timed_steps(argv):
    bench = _bench()
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(argv)
