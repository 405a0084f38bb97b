"""The Viterbi pitch decoding's C entry points under AddressSanitizer + UBSan: tests/asan/rmvpe_viterbi_driver.cpp, a stand-alone program linked
against the HIP stub (nothing is loaded into python, nothing runs on a device)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_rmvpe_viterbi_entry_points_under_asan_ubsan(tmp_path):
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "rmvpe_viterbi_build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-6000:]
    assert r.returncode == 0, tail
    assert "rmvpe viterbi driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    for what in ("viterbi a short workspace", "viterbi a tiny workspace", "viterbi T = 0", "viterbi no utterances", "viterbi null table", "viterbi no output",
                 "viterbi null workspace", "viterbi ld 359", "viterbi eps 0", "viterbi a misaligned workspace", "decode_at null centres", "decode_at no rows"):
        assert f"rejected {what} : " in r.stdout, (what, tail)
    traces = {ln.split(" : ")[0][6:]: ln.split(" : ")[1] for ln in r.stdout.splitlines() if ln.startswith("trace ")}
    assert len(traces) == 6
    both = "1x rv_viterbi_kernel (7,1,1)(384,1,1) | 1x rv_decode_at_kernel (118,1,1)(256,1,1)"  # one workgroup per utterance; 472 rows, four per block
    assert traces["viterbi ragged, all outputs"] == traces["viterbi ragged, f0 only"] == traces["viterbi with a caller's path, workspace less the path"] == both
    assert traces["viterbi ragged, path only"] == "1x rv_viterbi_kernel (7,1,1)(384,1,1)"  # no f0: no decode launch
    assert traces["viterbi one frame"] == "1x rv_viterbi_kernel (1,1,1)(384,1,1) | 1x rv_decode_at_kernel (1,1,1)(256,1,1)"
    assert traces["decode_at"] == "1x rv_decode_at_kernel (118,1,1)(256,1,1)"
