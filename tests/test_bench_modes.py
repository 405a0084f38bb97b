"""What a plain `bench.py --gpus 1 --steps K --warmup W` does and what only `--full` adds: the plain line carries the headline figure and
its configuration, nothing that takes runs of its own (cpu_baseline, roofline + traffic, legs, cfg3's stage split); `--full` brings them back."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

EXTRAS = ("cpu_baseline", "roofline", "legs")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_full_is_off_by_default():
    bench = _bench()
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def _run(*extra, timeout):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *extra], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("workload", ["cfg2", "cfg3"])
def test_plain_run_is_the_headline_only(workload):
    out = _run("--steps", "2", "--warmup", "1", "--workload", workload, timeout=240)
    assert out["metric"] == "utterances_per_sec" and out["unit"] == "utt/s" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert out["dtype"] == {"cfg2": "f32", "cfg3": "bf16"}[workload]
    assert not [k for k in EXTRAS if k in out], sorted(out)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_full_run_adds_the_other_measurements():
    """--full with every part but the rocprofv3 counter passes (kept short: a small CPU sample, one step per leg)."""
    out = _run("--steps", "2", "--warmup", "1", "--full", "--no-traffic", "--cpu-utts", "8", "--leg-steps", "1", "--leg-warmup", "1", timeout=540)
    assert out["metric"] == "utterances_per_sec" and out["value"] > 0 and out["dtype"] == "f32"
    assert out["cpu_baseline"]["value"] > 0, out["cpu_baseline"]
    assert out["roofline"]["achieved"] > 0 and out["roofline"]["traffic"] is None
    legs = out["legs"]
    assert sorted(legs) == ["cfg2_f32_matrix_cores", "cfg3_full_chain", "cfg4_strong", "cfg5_strong"], legs
    assert all(leg.get("value", 0) > 0 for leg in legs.values()), legs
    assert legs["cfg3_full_chain"]["roofline"]["frame_rate"]["ms"] > 0
