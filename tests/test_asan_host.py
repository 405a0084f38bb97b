"""CPU sanitizer pass over the library's host side.

The host code of csrc/ (weight-norm folding, row / Winograd / MFMA-fragment packing, style tables, the workspace closed forms,
arena carving, the launch planning of every contraction) is compiled with -fsanitize=address,undefined against a stub of the
HIP runtime (tests/asan/hip_stub.cpp: device memory = host heap, launches validated and counted, nothing executed) and driven
over the shapes of BASELINE's configs (cfg2, cfg3's phoneme batch, cfg4's 256 mixed utterances, cfg5's 64 x 10 s per GPU,
token-count extremes), in fp32 and fp16 operand modes.  GPU AddressSanitizer is not available on this pool; the kernels
themselves are covered by the -m gpu parity tests.

The driver also finalizes every component (text-to-speech, the voice-conversion models, AdaptiveHubert, the CFM estimator) in the f32, f16
and f32_native precisions and prints a digest of the packed device bytes after each; a second context per precision finalizes them in
another order around a finalize that fails, and must end at the same digest (tests/asan/asan_driver.cpp).  No digest is an expected value
here: two builds of the library pack the same bytes exactly when their digest lines agree.

The driver also traces which kernels the reverse flow launches (`flowtrace <precision> <case> <switches> : <kernel, grid, block in issue order,
run-length encoded>`), in all four precisions, over the batch shapes around the thresholds of the kernel choice (csrc/flow.hip.h plan_flow) and
under the STTS_WN_* switches.  Every case must be there, and the choice with no switch set is pinned without a constant: its trace must equal
the trace under the switches that force the intended kernel (PINS).  No trace is an expected value here either: two builds plan the same
launches exactly when their flowtrace lines agree."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_X3 = [f"STTS_WN_M=2,STTS_WN_X3={rt},STTS_WN_X3_WAVES={nw}" for rt in (1, 2, 4) for nw in (8, 4)]
_VARIANTS = _X3 + ["STTS_WN_M=2,STTS_WN_X3=2,STTS_WN_X3B=3", "STTS_WN_M=2,STTS_WN_X3=2,STTS_WN_X3B=4"] + [f"STTS_WN_M={m},STTS_WN_X3=-1" for m in (1, 2, 4, 16)]
_HALF = [(b, "-") for b in ("8x960", "23x960", "24x960", "64x3200")] + [("ragged", f"STTS_WN_RT={rt}") for rt in (-1, 4, 8, 16)]
# (precision, case, switches) of every flowtrace line but the forced halves of PINS; tests/test_hip_flow_layers.py has the ragged / many lists and VARIANTS
FLOW_CASES = ([(0, b, "-") for b in ("1x960", "8x960", "16x960", "64x3200", "ragged", "many")] + [(0, "ragged", v) for v in _VARIANTS]
              + [(0, "ragged", f"STTS_WN_DEBUG={k}") for k in (0, 3, -3, 4, -4, 32, -32)]
              + [(3, b, "-") for b in ("1x960", "8x960", "16x960")] + [(3, "ragged", f"STTS_WN_M={m}") for m in (1, 2, 4, 16)]
              + [(p, b, sw) for p in (1, 2) for b, sw in _HALF])
# the kernel that is meant to run with no switch set: (precision, case) -> the switches that force it
PINS = {(0, "1x960"): "STTS_WN_M=1,STTS_WN_X3=1", (0, "8x960"): "STTS_WN_M=2,STTS_WN_X3=2", (0, "16x960"): "STTS_WN_M=4,STTS_WN_X3=4",
        (3, "1x960"): "STTS_WN_M=1", (3, "8x960"): "STTS_WN_M=2", (3, "16x960"): "STTS_WN_M=4",
        (1, "23x960"): "STTS_WN_RT=4", (1, "24x960"): "STTS_WN_RT=16", (2, "23x960"): "STTS_WN_RT=4", (2, "24x960"): "STTS_WN_RT=16"}


@pytest.mark.timeout(900)
def test_host_side_under_asan_ubsan(tmp_path):
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert "asan driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    assert r.stdout.count("cfg5 per GPU") == 2  # both precisions reached the largest case
    for prec in (0, 2, 3):
        assert f"order {prec}: the second order and the failed finalize end at the same digest" in r.stdout, tail
        for what in ("tts", "hubert", "mel_style", "cfm_pitch_net", "ssl", "cfm"):
            assert re.search(rf"^digest {prec} {what} [0-9a-f]{{16}}$", r.stdout, re.M), (prec, what, tail)
    traces = {(int(p), b, sw): t for p, b, sw, t in re.findall(r"^flowtrace (\d) (\S+) (\S+) : (.+)$", r.stdout, re.M)}
    missing = [k for k in FLOW_CASES + [(p, b, sw) for (p, b), sw in PINS.items()] if k not in traces]
    assert not missing, missing
    for (prec, batch), forced in PINS.items():
        assert traces[(prec, batch, "-")] == traces[(prec, batch, forced)], (prec, batch, forced, traces[(prec, batch, "-")])
    # (the pins say something only while the forced traces differ from one another)
    assert len({traces[(0, "ragged", v)] for v in _VARIANTS}) == len(_VARIANTS)
    assert all(len({traces[(p, "ragged", f"STTS_WN_RT={rt}")] for rt in (-1, 4, 8, 16)}) == 4 for p in (1, 2))
