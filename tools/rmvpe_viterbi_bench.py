#!/usr/bin/env python3
"""RMVPE's Viterbi pitch decoding on the engine, ms per call: RmvpePitchExtractor.decode(decoder="viterbi") (the shim: pack, stts_rmvpe_viterbi,
unpack), HipModel.rmvpe_viterbi alone (the path-search workgroups and the decode launch), and the default argmax decode beside them.  The
baseline is the same recursion as a torch loop on the same device in fp64 - one max over a [B, 360, 360] tensor per frame and one gather per
frame on the way back - which is what a user of the reference could run on a GPU (the reference's own decoder is a host loop).  Reported, not
barred.  Shapes: B utterances of SECONDS at 100 frames / s (+ 1 frame).  Writes the JSON lines and a summary to --out.

    python tools/rmvpe_viterbi_bench.py [--iters 20] [--shapes 1x3,8x3,16x10] [--out profiles/rmvpe_viterbi_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES_PER_SECOND = 100  # hop 160 at 16 kHz


def timed(fn, iters: int, warmup: int = 3) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def salience(B: int, T: int, seed: int) -> np.ndarray:
    """A pitch-like salience [B, T, 360]: a bump on a moving track, its octave harmonic, a noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[None, :, None]
    j = np.arange(360)[None, None, :]
    track = 140.0 + 30.0 * np.sin(t / 37.0 + rng.random((B, 1, 1)) * 6.0) + 5.0 * np.sin(t / 4.7)
    s = 0.9 * np.exp(-0.5 * ((j - track) / 2.2) ** 2) + 0.6 * rng.random((B, T, 1)) * np.exp(-0.5 * ((j - track - 60.0) / 2.2) ** 2) + 0.02 * rng.random((B, T, 360))
    return np.clip(s, 0.0, 1.0).astype(np.float32)


def torch_loop(sal: torch.Tensor, lt: torch.Tensor, eps: float):
    """The objective of DESIGN.md section 5s as eager torch in fp64: (path [B, T], logp [B])."""
    s = torch.nan_to_num(sal.double(), nan=0.0).clamp_min(0.0)
    e = torch.log(s / s.sum(-1, keepdim=True) + eps)
    v = e[:, 0] + math.log(1.0 / 360 + eps)
    ptr = []
    for t in range(1, e.shape[1]):
        m, i = (v[:, :, None] + lt[None]).max(dim=1)
        v = e[:, t] + m
        ptr.append(i)
    logp, st = v.max(dim=1)
    path = [st]
    for i in reversed(ptr):
        st = i.gather(1, st[:, None])[:, 0]
        path.append(st)
    return torch.stack(path[::-1], dim=1), logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS at 100 salience frames per second")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmvpe_viterbi_bench.txt"))
    a = ap.parse_args()
    from stylish_tts_amd import modules, rmvpe
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    m = modules.RmvpePitchExtractor(config=dict(n_blocks=1, inter_layers=1, en_out_channels=8), engine=eng)  # decode needs no weights
    lt = torch.from_numpy(rmvpe.viterbi_transition()).to(eng.device)
    eps = rmvpe.VITERBI_EPS
    lines = []
    with torch.no_grad():
        for k, shape in enumerate(a.shapes.split(",")):
            B, sec = [int(v) for v in shape.split("x")]
            T = FRAMES_PER_SECOND * sec + 1
            hid = torch.from_numpy(salience(B, T, k)).to(eng.device)
            rows, seg = hid.reshape(-1, 360), Segments([T] * B, eng.device)
            f0, path, logp = eng.rmvpe_viterbi(seg, rows, path=True, logp=True)
            t_path, t_logp = torch_loop(hid, lt, eps)
            shim_ms = timed(lambda: m.decode(hid, decoder="viterbi"), a.iters)
            eng_ms = timed(lambda: eng.rmvpe_viterbi(seg, rows), a.iters)
            search_ms = timed(lambda: eng.rmvpe_viterbi(seg, rows, path=True, logp=True), a.iters)
            argmax_ms = timed(lambda: m.decode(hid), a.iters)
            loop_ms = timed(lambda: torch_loop(hid, lt, eps), max(2, a.iters // 10), warmup=1)
            rec = dict(batch=B, seconds=sec, frames=T, decode_viterbi_ms=round(shim_ms, 3), rmvpe_viterbi_ms=round(eng_ms, 3), rmvpe_viterbi_with_path_ms=round(search_ms, 3),
                       rmvpe_viterbi_us_per_frame=round(1e3 * eng_ms / T, 3), decode_argmax_ms=round(argmax_ms, 3), torch_loop_fp64_ms=round(loop_ms, 3),
                       torch_loop_us_per_frame=round(1e3 * loop_ms / T, 3), torch_loop_over_rmvpe_viterbi=round(loop_ms / eng_ms, 1),
                       viterbi_over_argmax=round(shim_ms / argmax_ms, 1), frames_off_the_argmax=int((path.view(B, T) != hid.argmax(-1)).sum()),
                       frames_path_differs_from_torch_loop=int((path.view(B, T) != t_path).sum()), max_abs_logp_diff_vs_torch_loop=float((logp - t_logp).abs().max()))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/rmvpe_viterbi_bench.py --iters {a.iters} --shapes {a.shapes}: ms per call (host-timed launches included), {torch.cuda.get_device_name(0)}\n")
        for r in lines:
            f.write(json.dumps(r) + "\n")
        f.write("# rmvpe_viterbi is bound by its serial loop over the frames (rmvpe_viterbi_us_per_frame), not by bandwidth or by the batch: one workgroup per utterance "
                "(a batch of 1 uses one CU), and per frame one barrier, 59 taps of an LDS read, an fp64 add, an fp64 compare and three selects per state, one fp64 divide "
                "and log for the next emission and the six-step wave maximum for the guard, all on the dependent chain; six waves on four SIMDs put two waves on two of "
                "them (read from the code, no counters).  Backtracking adds T dependent LDS reads by one thread.  The torch loop pays about five launches per frame.\n")


if __name__ == "__main__":
    main()
