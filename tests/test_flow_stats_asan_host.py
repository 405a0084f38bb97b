"""The flow statistics' C entry points under AddressSanitizer + UBSan: tests/asan/flow_stats_driver.cpp, a stand-alone program linked against the
HIP stub (nothing is loaded into python, nothing runs on a device)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_flow_stats_entry_points_under_asan_ubsan(tmp_path):
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "flow_stats_build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-6000:]
    assert r.returncode == 0, tail
    assert "flow stats driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    assert "finalized : STTS_W_FLOW_STATS alone, and after STTS_W_ALL, and again" in r.stdout
    for what in ("flow not finalized", "prior not finalized", "one byte below the workspace", "capacity segments", "capacity segments (prior)", "an output that is an input",
                 "reverse 2", "ld_x 256", "KL kind 2", "KL width 256 in rows of 128", "KL workspace of 8 bytes"):
        assert f"rejected {what} : " in r.stdout, (what, tail)
    traces = [ln for ln in r.stdout.splitlines() if ln.startswith("trace ")]
    assert len(traces) == 30
    for ln in traces:  # (the trace joins consecutive launches of one kernel: a coupling layer is "3x <plain> | 1x <last>")
        forced = ln.split("STTS_FSTAT_WN=")[1].split(" ")[0]
        if forced == "0":  # per coupling layer 10 contractions and the coupling row kernel
            assert "wn_stats_kernel" not in ln and ln.count("1x flow_stats_couple_kernel") == 8, ln
            continue
        assert "flow_stats_couple_kernel" not in ln, ln
        rts = [int(forced) // 16] if forced in ("16", "32", "64") else [rt for rt in (1, 2, 4) if f"wn_stats_kernel<{rt}, " in ln]
        assert len(rts) == 1, ln
        assert ln.count(f"3x wn_stats_kernel<{rts[0]}, false>") == 8 and ln.count(f"1x wn_stats_kernel<{rts[0]}, true>") == 8, ln
