"""The alignment, duration and difference scores' C entry points under AddressSanitizer + UBSan: tests/asan/align_scores_driver.cpp, a stand-alone
program linked against the HIP stub (nothing is loaded into python, nothing runs on a device)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_align_scores_entry_points_under_asan_ubsan(tmp_path):
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "align_scores_build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-6000:]
    assert r.returncode == 0, tail
    assert "align scores driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    for what in ("ctc_nll P = 0", "ctc_nll P = 511", "ctc_nll T = 0", "ctc_nll blank outside the classes", "ctc_nll null output", "ctc_confidence_sums T = 0",
                 "ctc_confidence_sums null output", "ctc_prior_sums one byte below the workspace", "ctc_prior_sums null output", "ctc_prior_sums T = 0",
                 "val_duration_sums 65 classes", "val_duration_sums P = 0", "val_duration_sums null output", "val_diff_sums kind 2", "val_diff_sums an empty utterance",
                 "val_diff_sums null output"):
        assert f"rejected {what} : " in r.stdout, (what, tail)
    traces = {ln.split(" : ")[0][6:]: ln.split(" : ")[1] for ln in r.stdout.splitlines() if ln.startswith("trace ")}
    assert len(traces) == 8
    assert traces["ctc_nll ragged"] == traces["ctc_nll ragged with priors"] == "1x ctc_forward_kernel (4,1,1)(1024,1,1)"  # one workgroup per utterance
    assert traces["ctc_confidence_sums ragged"] == "1x ctc_confidence_kernel (4,1,1)(256,1,1)"
    assert traces["ctc_prior_sums ragged"] == "1x ctc_prior_part_kernel (9,1,1)(256,1,1) | 1x ctc_prior_merge_kernel (1,1,1)(256,1,1)"  # 564 rows: 9 chunks of 64
    assert traces["val_duration_sums ragged, 16 classes"] == traces["val_duration_sums ragged, 64 classes"] == "1x val_duration_kernel (4,1,1)(256,1,1)"
    assert traces["val_diff_sums ragged, absolute"] == "1x val_diff_kernel<0> (4,1,1)(256,1,1)" and traces["val_diff_sums ragged, squared"] == "1x val_diff_kernel<1> (4,1,1)(256,1,1)"
