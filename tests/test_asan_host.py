"""CPU sanitizer pass over the library's host side.

The host code of csrc/ (weight-norm folding, row / Winograd / MFMA-fragment packing, style tables, the workspace queries - dry runs of
the stages' own arena carving - the launch planning of every contraction) is compiled with -fsanitize=address,undefined against a stub of the
HIP runtime (tests/asan/hip_stub.cpp: device memory = host heap, launches validated and counted, nothing executed) and driven
over the shapes of BASELINE's configs (cfg2, cfg3's phoneme batch, cfg4's 256 mixed utterances, cfg5's 64 x 10 s per GPU,
token-count extremes, two skewed batches whose per-utterance statistics buffers outgrow an average-length bound), in fp32 and fp16
operand modes.  Every stage outside the frame path is walked on a workspace of the size its query returns and then once more one
256-byte unit below the smallest size it accepts: that call must be refused with "workspace too small" before anything is launched
(`refusal <precision> <case> <stage> : ...`, STAGE_WALKS).  GPU AddressSanitizer is not available on this pool; the kernels
themselves are covered by the -m gpu parity tests.

The driver also finalizes every component (text-to-speech, the voice-conversion models, AdaptiveHubert, the CFM estimator) in the f32, f16
and f32_native precisions and prints a digest of the packed device bytes after each; a second context per precision finalizes them in
another order around a finalize that fails, and must end at the same digest (tests/asan/asan_driver.cpp).  No digest is an expected value
here: two builds of the library pack the same bytes exactly when their digest lines agree.

The driver also traces which kernels the reverse flow launches (`flowtrace <precision> <case> <switches> : <kernel, grid, block in issue order,
run-length encoded>`), in all four precisions, over the batch shapes around the thresholds of the kernel choice (csrc/flow.hip.h plan_flow) and
under the STTS_WN_* switches.  Every case must be there, and the choice with no switch set is pinned without a constant: its trace must equal
the trace under the switches that force the intended kernel (PINS).  No trace is an expected value here either: two builds plan the same
launches exactly when their flowtrace lines agree.

The same for the dense contractions (csrc/gemm_plan.hip.h plan_conv_gemm): `gemmtrace <precision> <case> <force_tile> : <trace>` for every tile of the tile
table forced in each operand form it exists in, the shapes around every threshold of the plan with the tile left to it, and the remainder launch; and
`launchtrace <precision> <case> : <trace>` around every stage walk, and `flowtrace <precision> generic96* -` for a second model whose flow is 96 channels wide
(every coupling layer as plain contractions with the gate / split-accumulate / couple epilogues).  The tile the plan is meant to take is pinned the same way: against the forced trace on the
same shape.  build_and_run.py repeats the gemmtrace cases under each experiment switch (lines prefixed `[NAME=value]`, compared between builds only).

And for the AdaptiveDecoderBlock chains (csrc/adain_block.hip.h plan_adain_chain / plan_adain_block): `blocktrace <precision> <case> <switches> : <trace>` of the decoder, the
frame path, the pitch/energy predictors and stts_op_adain_block on the batch shapes around every threshold of the plan (2 500 rows fold -> Winograd, 96 .. 384 bridge
blocks, 3 840 / 4 096 rows in the 16-bit modes, 12 000 rows for the side lane), under STTS_ADAIN_BRIDGE (read per call) and, one process per setting, under the block's
process-wide switches.  The unforced trace must equal the forced one on its side of a threshold and differ from it on the other (check_blocktraces).

And for the vocoder and the frame path: `frametrace <precision> <call>_<rows> <switches> : <stts_frame_workspace_bytes> | <launches on the caller's stream>+<launches on
any other stream> | <trace>` of one stts_frame_path and one stts_vocoder_forward call on the two thresholds this code owns: 3 000 rows against 3 001 (fp32: the source ->
STFT -> prior-conv chain goes to a side stream above), with and without STTS_NO_SIDE_STREAM (read per call), and 3 839 rows against 3 840 (16-bit rows in the 16-bit
modes) (check_frametraces)."""
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

# gemmtrace cases: (precision, case, force_tile); tests/asan/asan_driver.cpp gemm_section has the shapes
_SPLIT, _PRESPLIT, _NATIVE = (2, 3, 4, 5, 6, 8, 20, 21, 22), (25, 26, 27, 28), (2, 3, 4, 5, 6, 8, 11, 13)
_HALF_TILES = (2, 3, 4, 5, 6, 8, 14, 15) + tuple(100 + t for t in (2, 3, 4, 5, 6, 14, 15, 16, 17, 18))
FORCED = {0: _SPLIT + _PRESPLIT, 3: _NATIVE, 1: _HALF_TILES, 2: _HALF_TILES}  # per form: traces pairwise distinct
_AUTO = ("auto32x1025", "auto33x130", "auto578x512", "auto1536x64", "splitK", "tile22", "300x20")
GEMM_CASES = ([(p, "forced", t) for p, ts in FORCED.items() for t in ts] + [(0, "forced", 7), (1, "forced", 119), (2, "forced", 119)]
              + [(p, c, 0) for p in (0, 3) for c in _AUTO] + [(3, "tile8_257", 0)] + [(0, f"tile22_{b}", f) for b in (439, 440, 459, 460, 639, 640) for f in (0, 22)]
              + [(p, c, 100) for p in (1, 2) for c in ("tile15_127", "tile15_128", "tile14_95", "tile14_96", "gemm16_191", "gemm16_192")])
# the tile that is meant to run with no tile forced (no split-K, no remainder launch in these): (precision, case, unforced) -> the force that selects it
GEMM_PINS = {(0, "auto33x130", 0): 4, (3, "auto33x130", 0): 4, (0, "auto32x1025", 0): 6, (3, "auto32x1025", 0): 6, (0, "tile22", 0): 22, (3, "tile8_256", 0): 8,
             (0, "tile22_460", 0): 22, (0, "tile22_640", 0): 22}
GEMM_PINS.update({(p, c, 100): f for p in (1, 2) for c, f in (("tile15_128", 115), ("tile14_95", 115), ("tile14_96", 114), ("gemm16_192", 119))})
# ... and just below each threshold the forced tile must NOT be what runs
GEMM_OFF = ([(0, f"tile22_{b}", 0, 22) for b in (439, 440, 459, 639)]
            + [(p, c, 100, f) for p in (1, 2) for c, f in (("tile15_127", 115), ("tile14_95", 114), ("gemm16_191", 119))])
# the walks of the stages outside the frame path: case -> the stages whose refusal line must be there (asan_driver.cpp main)
_PHONEME = ("text_encoder", "text_style", "duration", "pitch_energy")
_HUBERT = ("speaker_style", "hubert_encoder", "hubert_pitch_energy")
STAGE_WALKS = {"cfg3:_64_x_50_tokens": _PHONEME, "token-count_extremes": _PHONEME, "skew256:_1_x_4000_+_255_x_20_frames": _PHONEME,
               "skew24:_1_x_2400_+_23_x_8_frames": _PHONEME, "hubert:_3_utterances": _HUBERT, "hubert_skew256": _HUBERT, "hubert_skew24": _HUBERT,
               "ssl:_3_utterances": ("ssl",), "cfm:_3_utterances": ("cfm_estimator",), "cfm_skew24": ("cfm_estimator",),
               "aligner:_3_utterances": ("aligner",), "aligner,_one_tdnn_layer": ("aligner",), "rmvpe:_3_utterances": ("rmvpe",)}
STAGE_WALKS.update({f"{c}_{e}": ("mel_style",) for c in ("mel:_3_utterances", "mel_skew24") for e in ("pe_mel_style", "spk_emb")})
STAGE_WALKS.update({f"{c}_cfm_pitch": ("cfm_pitch",) for c in ("mel:_3_utterances", "mel_skew24")})
# blocktrace cases: (precision, case, switches); tests/asan/asan_driver.cpp block_section has the shapes
_BRIDGE = ("-", "STTS_ADAIN_BRIDGE=0", "STTS_ADAIN_BRIDGE=1")
BRIDGE_ON, BRIDGE_OFF, BRIDGE_TOO_LONG = ("3x960", "4x700", "12x960"), ("2x1300", "13x960"), "1537+2x960"  # what the rule of plan_adain_chain takes with the switch unset
BLOCK_CASES = ([(p, f"dec_1x{n}", "-") for p in (0, 3) for n in (300, 2500, 2501)]
               + [(p, f"dec_{b}", sw) for p in (0, 3) for b in BRIDGE_ON + BRIDGE_OFF + (BRIDGE_TOO_LONG,) for sw in _BRIDGE]
               + [(p, f"dec_{c}", "-") for p in (1, 2) for c in ("1x300", "3839rows", "3840rows", "4096rows", "4097rows", "110utt", "100utt")]
               + [(0, f"frame_{b}x960", sw) for b in (12, 13) for sw in _BRIDGE[:2]] + [(p, c, "-") for p in (0, 1, 2, 3) for c in ("op_1x300", "op_2x2049")]
               + [(p, f"chain_{r}rows", "-") for p in (0, 1, 2, 3) for r in (300, 301, 500, 501)]
               + [(p, c, "-") for p in (0, 2, 3) for c in ("pe_2500frames", "pe_2501frames", "hubert_353frames", "hubert_2600frames")])
# the block's process-wide switches (tests/asan/build_and_run.py BLOCK_SETTINGS): setting -> the (precision, case, switches) whose trace it must change and those it
# must leave alone.  STTS_FOLD_ROWS=0 forces the Winograd form and STTS_SC_SIDE_MIN_ROWS=0 the side lane, so what they leave alone is the unforced choice pinned.
BLOCK_SETTINGS = {
    "STTS_FOLD_ROWS=0": ([(0, "dec_1x2500", "-"), (0, "pe_2500frames", "-"), (0, "dec_1x300", "-")], [(0, "dec_1x2501", "-"), (0, "pe_2501frames", "-"), (0, "dec_13x960", "-")]),
    "STTS_SC_SIDE_MIN_ROWS=0": ([(0, "frame_12x960", sw) for sw in _BRIDGE[:2]], [(0, "frame_13x960", sw) for sw in _BRIDGE[:2]] + [(0, "dec_13x960", "-")]),
    "STTS_NO_WINO_STATS=1": ([(0, "dec_2x1300", "-"), (0, "dec_3x960", "-"), (0, "pe_2501frames", "-")], [(0, "dec_1x2500", "-"), (0, "hubert_2600frames", "-"), (1, "dec_110utt", "-")]),
    "STTS_NO_STAT_FUSE=1": ([(1, "dec_110utt", "-")], [(1, "dec_100utt", "-"), (0, "dec_2x1300", "-")]),
    "STTS_NO_WINO_CONV2SC=1": ([(0, "dec_2x1300", "-")], [(0, "dec_1x2500", "-"), (0, "pe_2501frames", "-")]),
    "STTS_AFFINE_SERIAL=1": ([(0, "dec_1x300", "-"), (0, "op_1x300", "-")], [(0, "op_2x2049", "-")]),
}


def check_blocktraces(stdout):
    """The blocktrace lines of a driver run: every case there and accepted, the unforced choice equal to the forced one on its side of each threshold."""
    block = {(int(p), c, sw): t for p, c, sw, t in re.findall(r"^blocktrace (\d) (\S+) (\S+) : (.*)$", stdout, re.M)}
    missing = [k for k in BLOCK_CASES if k not in block]
    assert not missing, missing
    assert not [k for k, t in block.items() if t.startswith("error") or not t.strip()], block
    for p in (0, 3):
        auto, off, on = ({b: block[(p, f"dec_{b}", sw)] for b in BRIDGE_ON + BRIDGE_OFF + (BRIDGE_TOO_LONG,)} for sw in _BRIDGE)
        for b in BRIDGE_ON:  # 96 <= utterances x 32 <= 384: the bridge, as forced on
            assert auto[b] == on[b] != off[b], (p, b, auto[b])
        for b in BRIDGE_OFF:  # outside: three launches, as forced off; the kernel could run
            assert auto[b] == off[b] != on[b], (p, b, auto[b])
        assert auto[BRIDGE_TOO_LONG] == off[BRIDGE_TOO_LONG] == on[BRIDGE_TOO_LONG], p  # an utterance beyond a bridge block: not even forced
        assert "winograd_bridge_kernel" in on["3x960"] and "winograd_bridge_kernel" not in off["3x960"], on["3x960"]
        # fold -> Winograd above 2 500 rows
        assert "winograd" not in block[(p, "dec_1x2500", "-")] and "winograd_input_kernel" in block[(p, "dec_1x2501", "-")], p
    assert "winograd" not in block[(0, "pe_2500frames", "-")] and "winograd_input_kernel" in block[(0, "pe_2501frames", "-")]
    for p in (1, 2):  # 4 400 rows: conv_gemm16_kernel with the statistics from its epilogues; 3 960 rows: folded, no apply pass
        assert "conv_gemm16_kernel<" in block[(p, "dec_110utt", "-")] and "conv_gemm16_kernel<" not in block[(p, "dec_100utt", "-")], p
        assert "adain_apply_kernel" in block[(p, "dec_4097rows", "-")] and "adain_apply_kernel" not in block[(p, "dec_4096rows", "-")], p
        # 3 840 .. 4 096 rows: folded means fp32 rows throughout, so nothing is cast to 16-bit rows there (no rounded copy of x for the shortcuts, no rounded y);
        # from 4 097 rows on the blocks read and write them
        for rows in (3839, 3840, 4096):
            assert "cast_rows_kernel" not in block[(p, f"dec_{rows}rows", "-")], (p, rows)
        assert "cast_rows_kernel" in block[(p, "dec_4097rows", "-")], p
    # stts_op_adain_chain's returned plans (8 integers of the chain plan, 16 per block: conv1, conv2, rows16, ... shortcut at 8, cast_x16 at 9, y16 at 10), with
    # fold_rows = 300, the 16-bit fold limit at 500 and 16-bit rows from 300: a block is folded on fp32 rows with the shortcut a segment on x, or it runs
    # on 16-bit rows throughout - never 16-bit rows under folded contractions
    plans = {(int(p), c): [int(v) for v in t.split()] for p, c, t in re.findall(r"^blockplan (\d) (\S+) :(.*)$", stdout, re.M)}
    assert sorted(plans) == sorted((p, f"chain_{r}rows") for p in (0, 1, 2, 3) for r in (300, 301, 500, 501)), sorted(plans)
    for (p, c), v in plans.items():
        rows, chain, blk = int(c[6:-4]), v[:8], [v[8:24], v[24:40]]
        for b in blk:
            assert b[2] == 0 or (b[0] != 0 and b[1] != 0), (p, c, "16-bit rows under a folded contraction", b)
        if p in (0, 3):
            assert [b[0] for b in blk] == ([0, 0] if rows <= 300 else [2, 2]) and chain[2] == 0, (p, c, v)  # CONV_FOLD | CONV_WINO
        else:
            folded = rows <= 500
            assert [b[:3] for b in blk] == ([[0, 0, 0]] * 2 if folded else [[1, 1, p]] * 2), (p, c, v)  # CONV_FOLD on fp32 rows | CONV_APPLY on 16-bit rows
            assert chain[2] == (0 if folded else 1) and [b[8] for b in blk] == [1, 1], (p, c, v)         # the chain plan agrees; SC_SEGMENT
            assert blk[0][10] == (2 if folded else 1) and blk[1][9] == 0, (p, c, v)                       # y16: a cast pass | conv2's epilogue; B's copy is there
    per_setting = {}
    for sw, p, c, s, t in re.findall(r"^\[(STTS_\w+=\d+)\] blocktrace (\d) (\S+) (\S+) : (.*)$", stdout, re.M):
        per_setting.setdefault(sw, {})[(int(p), c, s)] = t
    assert sorted(per_setting) == sorted(BLOCK_SETTINGS), sorted(per_setting)
    n_cases = len([k for k in block if k[0] in (0, 1)])
    for sw, (changed, same) in BLOCK_SETTINGS.items():
        forced = per_setting[sw]
        assert len(forced) == n_cases and not [k for k, t in forced.items() if t.startswith("error")], (sw, len(forced), n_cases)
        assert not [k for k in changed if forced[k] == block[k]], (sw, "changes nothing in", [k for k in changed if forced[k] == block[k]])
        assert not [k for k in same if forced[k] != block[k]], (sw, "changes", [k for k in same if forced[k] != block[k]])
    assert len({tuple(sorted(f.items())) for f in per_setting.values()}) == len(per_setting)  # (the settings differ from one another)


# frametrace cases: (precision, call_rows, switches); tests/asan/asan_driver.cpp frametrace_section has the shapes
_NO_SIDE = "STTS_NO_SIDE_STREAM=1"
FRAME_CASES = ([(p, f"{call}_{rows}", sw) for p in (0, 2) for call in ("frame_path", "vocoder_forward") for rows in (3000, 3001) for sw in ("-", _NO_SIDE)]
               + [(p, f"{call}_{rows}", "-") for p in (0, 2) for call in ("frame_path", "vocoder_forward") for rows in (3839, 3840)])


def check_frametraces(stdout):
    """The frametrace lines of a driver run: every case there; the side stream taken above 3 000 rows in fp32 only, and not under the switch, with the same kernels in
    the same order either way; 16-bit rows in the vocoder from 3 840 rows on."""
    frame = {(int(p), c, sw): (int(b), int(m), int(s), t) for p, c, sw, b, m, s, t in
             re.findall(r"^frametrace (\d) (\S+) (\S+) : (\d+) \| (\d+)\+(\d+) \| (.*)$", stdout, re.M)}
    assert sorted(frame) == sorted(FRAME_CASES), sorted(frame)
    assert not [k for k, v in frame.items() if v[0] == 0 or v[1] == 0 or not v[3].strip()], frame
    on, below, off = frame[(0, "frame_path_3001", "-")], frame[(0, "frame_path_3000", "-")], frame[(0, "frame_path_3001", _NO_SIDE)]
    assert on[2] > 0 and below[2] == 0 and off[2] == 0, (on[:3], below[:3], off[:3])
    assert on[3] == off[3] and on[1] + on[2] == off[1] and on[0] == off[0], (on, off)  # same kernels, same order, same workspace
    # nothing else leaves the caller's stream: only stts_frame_path, only fp32, only above 3 000 rows
    assert sorted(k for k, v in frame.items() if v[2]) == [(0, f"frame_path_{rows}", "-") for rows in (3001, 3839, 3840)], frame
    for k in FRAME_CASES:  # the switch changes nothing else
        if k[2] == _NO_SIDE and k != (0, "frame_path_3001", _NO_SIDE):
            assert frame[k] == frame[(k[0], k[1], "-")], k
    # 3 840 rows: the 16-bit modes run the vocoder on 16-bit rows (mel gets a rounded copy; the prior convs read a rounded copy of the spectra), fp32 does not
    lo, hi = frame[(2, "vocoder_forward_3839", "-")][3], frame[(2, "vocoder_forward_3840", "-")][3]
    assert lo != hi and "cast_rows_kernel" in hi and "cast_rows_kernel" not in lo, (lo, hi)
    assert frame[(2, "frame_path_3839", "-")][3] != frame[(2, "frame_path_3840", "-")][3]
    assert "cast_rows_kernel" not in frame[(0, "vocoder_forward_3840", "-")][3]


LAUNCH_CASES = [(p, c) for p in (0, 2) for c in ("cfg2:_8_x_3_s", "B_=_1_x_3_s", "short_ragged_utterances", "cfg5_per_GPU:_64_x_10_s", "cfg3:_64_x_50_tokens",
                                                 "token-count_extremes")] + [(0, "cfg4:_256_utterances_of_0.25-10_s")]


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
        for what in ("tts", "hubert", "mel_style", "cfm_pitch_net", "ssl", "cfm", "aligner", "rmvpe"):
            assert re.search(rf"^digest {prec} {what} [0-9a-f]{{16}}$", r.stdout, re.M), (prec, what, tail)
    traces = {(int(p), b, sw): t for p, b, sw, t in re.findall(r"^flowtrace (\d) (\S+) (\S+) : (.+)$", r.stdout, re.M)}
    missing = [k for k in FLOW_CASES + [(p, b, sw) for (p, b), sw in PINS.items()] if k not in traces]
    assert not missing, missing
    for (prec, batch), forced in PINS.items():
        assert traces[(prec, batch, "-")] == traces[(prec, batch, forced)], (prec, batch, forced, traces[(prec, batch, "-")])
    # (the pins say something only while the forced traces differ from one another)
    assert len({traces[(0, "ragged", v)] for v in _VARIANTS}) == len(_VARIANTS)
    assert all(len({traces[(p, "ragged", f"STTS_WN_RT={rt}")] for rt in (-1, 4, 8, 16)}) == 4 for p in (1, 2))

    # ---- the dense contractions
    gemm = {(int(p), c, int(f)): t for p, c, f, t in re.findall(r"^gemmtrace (\d) (\S+) (-?\d+) : (.*)$", r.stdout, re.M)}
    missing = [k for k in GEMM_CASES + [(p, c, f) for (p, c, _), f in GEMM_PINS.items()] + [(p, c, f) for p, c, _, f in GEMM_OFF] if k not in gemm]
    assert not missing, missing
    launch = {(int(p), c): t for p, c, t in re.findall(r"^launchtrace (\d) (\S+) : (.+)$", r.stdout, re.M)}
    assert not [k for k in LAUNCH_CASES if k not in launch], sorted(launch)
    # every stage walk ran on the workspace its query sized (a launchtrace line: the driver stops at a call that fails), and was refused just below the
    # smallest workspace the stage accepts, before its first launch (the driver prints the line only then)
    refusals = set(re.findall(r"^refusal (\d) (\S+) (\S+) : query \d+ bytes, least accepted \d+, refused below it with nothing launched$", r.stdout, re.M))
    for prec in (0, 2):
        for case, stages in STAGE_WALKS.items():
            assert (prec, case) in launch, (prec, case)
            assert not [s for s in stages if (str(prec), case, s) not in refusals], (prec, case, sorted(refusals))
    for (prec, case, unforced), forced in GEMM_PINS.items():
        assert not gemm[(prec, case, forced)].startswith("error") and gemm[(prec, case, unforced)] == gemm[(prec, case, forced)], (prec, case, forced, gemm[(prec, case, unforced)])
    for prec, case, unforced, forced in GEMM_OFF:
        assert gemm[(prec, case, unforced)] != gemm[(prec, case, forced)], (prec, case, forced)
    assert "(1024,1,1)" in gemm[(3, "tile8_256", 0)] and "(1024,1,1)" not in gemm[(3, "tile8_257", 0)]  # (tile 8 alone has blocks of 16 waves)
    for prec, tiles in FORCED.items():  # (the pins say something only while the forced traces differ from one another)
        forced = [gemm[(prec, "forced", t)] for t in tiles]
        assert len(set(forced)) == len(tiles) and not any(t.startswith("error") for t in forced), (prec, forced)
    # whole rounds + split-K remainder: two contraction launches (the second with K cut: grid.z > 1) and one reduce pass on the f32 matrix cores, one launch in split fp32
    rem = gemm[(3, "300x20", 0)].split(" | ")
    assert len(rem) == 3 and all(t.startswith("1x conv_gemm_f32<") for t in rem[:2]) and rem[2].startswith("1x splitk_reduce_kernel "), rem
    assert re.search(r"\(1,256,1\)\(", rem[0]) and re.search(r"\(1,44,3\)\(", rem[1]), rem
    whole = gemm[(0, "300x20", 0)]
    assert whole.startswith("1x conv_gemm_f32<") and " | " not in whole and "splitk_reduce_kernel" not in whole, whole
    # a tile id without a row is an error and launches nothing; tile 19 on a contraction conv_gemm16_kernel cannot take (130 channels out) fails after the row cast
    assert gemm[(0, "forced", 7)] == "error ", gemm[(0, "forced", 7)]
    assert all(gemm[(p, "forced", 119)].startswith("error ") and "conv_gemm" not in gemm[(p, "forced", 119)] for p in (1, 2))
    # the paired and the split-accumulate epilogues (conv_gemm_f32's fifth template argument): the prior conv (EPI_PRIOR = 4) is in every frame-path walk; gate (1),
    # split-accumulate (2) and couple (3) are the coupling layers of a flow that is not 128 channels wide (the driver's second model: 96), on tile 3 below 24 blocks
    # of 128 x 128 and on tile 2 above (split-accumulate is unpaired: tile 4, then 5 / 6 / 8)
    for prec in (0, 2):
        assert re.search(r"conv_gemm_f32<128, (64, 2, 2|32, 2, 1), 4,", launch[(prec, "cfg2:_8_x_3_s")]), prec
    for prec in (0, 2, 3):
        small, large = traces[(prec, "generic96", "-")], traces[(prec, "generic96_8x960", "-")]
        for epi in (1, 3):
            assert re.search(rf"conv_gemm_f32<128, 32, 2, 1, {epi},", small) and re.search(rf"conv_gemm_f32<128, 64, 2, 2, {epi},", large), (prec, epi)
        assert re.search(r"conv_gemm_f32<128, 32, 4, 1, 2,", small) and re.search(r"conv_gemm_f32<128, (128|64), 4, 2, 2,", large), prec
        assert "wn_" not in small and "wn_" not in large, prec
    # stts_op_conv1d_epi's host side (asan_driver.cpp epi_section): the three launches run the kernel they name, a refused combination launches NOTHING
    epi = dict(re.findall(r"^epitrace (\S+) : (.*)$", r.stdout, re.M))
    assert "conv_gemm16_kernel<" in epi["two_segments"] and "conv_gemm16_kernel<" in epi["capacity"] and "conv_gemm_f32<" in epi["windows_tile15"], epi
    assert not any(epi[k].startswith("error") for k in ("two_segments", "capacity", "windows_tile15")), epi
    refused = [k for k in epi if k.startswith("refuse_")]
    assert len(refused) == 6 and all(epi[k].strip() == "error" for k in refused), epi
    # the operators of the kernels between the contractions and of the 2-D convolution (asan_driver.cpp norm_section): each accepted call launches the kernels it names, each refused one NOTHING
    norm = dict(re.findall(r"^normtrace (\S+) : (.*)$", r.stdout, re.M))
    accepted = {"adain_reduce_apply": ("adain_partial_reduce_kernel", "adain_apply_kernel"), "adain_lanes24": ("adain_partial_kernel", "adain_affine_lanes_kernel"),
                "wino_stat": ("winograd_output_kernel<8, true>",), "row_layernorm": ("row_utt_kernel", "row_layernorm_kernel"), "dwconv_form0": ("dwconv_kernel<31>",),
                "dwconv_form1": ("dwconv_ln_kernel<15, 16>",), "dwconv_form2": ("dwconv_kernel<31>", "row_layernorm_kernel"), "grn_mode1": ("grn_gx_kernel", "grn_xaff_kernel"),
                "grn_mode2": ("grn_gx_kernel", "scale_weight_kernel<1>"), "conv2d_sliced": ("conv2d_kernel<2, 2, 2, 2, true>", "(11,1,3)", "conv2d_reduce_kernel")}
    for case, kernels in accepted.items():
        assert not norm[case].startswith("error") and all(k in norm[case] for k in kernels), (case, norm[case])
    refused = [k for k in norm if k.startswith("refuse_")]
    assert sorted(refused) == sorted(["refuse_" + k for k in accepted] + ["refuse_dwconv_form1_k5"]) and all(norm[k].strip() == "error" for k in refused), norm
    # the operators of the flow-matching estimator's row kernels (asan_driver.cpp cfm_ops_section): the product's grids - capped at 2048 / 1024 blocks where the
    # shapes exceed them -, each refused call launches NOTHING
    cfm = dict(re.findall(r"^cfmtrace (\S+) : (.*)$", r.stdout, re.M))
    cfm_accepted = {"elem_mish": ("mish_kernel", "(2048,1,1)(256,1,1)"), "elem_swiglu": ("swiglu_kernel", "(2048,1,1)(256,1,1)"), "elem_gated": ("gated_residual_kernel", "(1024,3,1)(256,1,1)"),
                    "rms_adaln": ("rms_adaln_kernel", "(275,3,1)(256,1,1)"), "rope_axial": ("axial_rope_kernel", "(1024,3,1)(256,1,1)"), "rope_sequence": ("rope_kernel", "(1100,3,1)(256,1,1)"),
                    "small_kind0": ("small_linear_kernel", "(4,1,1)(256,1,1)"), "small_kind1": ("small_layernorm_kernel", "(3,1,1)(64,1,1)"),
                    "small_kind2": ("cfm_time_embed_kernel", "(1,1,1)(256,1,1)"), "source": ("cfm_source_kernel", "(3,1,1)(256,1,1)")}
    for case, parts in cfm_accepted.items():
        assert not cfm[case].startswith("error") and cfm[case].startswith("1x ") and " | " not in cfm[case] and all(k in cfm[case] for k in parts), (case, cfm[case])
    refused = [k for k in cfm if k.startswith("refuse_")]
    assert sorted(refused) == ["refuse_elem", "refuse_rms_adaln", "refuse_rope", "refuse_small", "refuse_source"] and all(cfm[k].strip() == "error" for k in refused), cfm
    check_blocktraces(r.stdout)
    check_frametraces(r.stdout)
    # every switch setting ran every case
    per_setting = {}
    for sw in re.findall(r"^\[(STTS_\w+=\d+)\] gemmtrace ", r.stdout, re.M):
        per_setting[sw] = per_setting.get(sw, 0) + 1
    assert len(per_setting) == 11 and set(per_setting.values()) == {len(gemm)}, per_setting
