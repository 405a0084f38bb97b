"""The posterior encoder's C entry points under AddressSanitizer + UBSan: tests/asan/posterior_driver.cpp, a stand-alone program linked against the
HIP stub (nothing is loaded into python, nothing runs on a device)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_posterior_entry_points_under_asan_ubsan(tmp_path):
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "posterior_build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-6000:]
    assert r.returncode == 0, tail
    assert "posterior driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    assert "finalized : STTS_W_POSTERIOR alone, and after STTS_W_ALL" in r.stdout
    for what in ("not finalized", "below the least workspace", "capacity segments", "mel_out without STTS_W_FLOW", "an utterance of 13 rows", "ld_har 1024"):
        assert f"rejected {what} : " in r.stdout, (what, tail)
    traces = [ln for ln in r.stdout.splitlines() if ln.startswith("trace ")]
    assert len(traces) == 15
    for ln in traces:
        forced = ln.split("STTS_POST_WN=")[1].split(" ")[0]
        if forced == "0":
            assert "wn_post_kernel" not in ln, ln
        elif forced in ("16", "32", "64"):
            assert f"11x wn_post_kernel<{int(forced) // 16}, false>" in ln and f"1x wn_post_kernel<{int(forced) // 16}, true>" in ln, ln
