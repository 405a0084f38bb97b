#!/usr/bin/env python3
"""The log-mel front end on the engine (csrc/log_mel.hip.h): ms per call of the one launch (packed recordings -> normalised log-mel rows, with
and without the energy and raw outputs) and of the statistics pair, beside a plain torch eager fp32 run of the same arithmetic on the same GPU in
the same run: torch.stft (center, reflect, periodic Hann) -> |.|^2 -> matmul with the mel filters -> log(1e-5 + .) -> normalise.  The eager time is
the yardstick to report against, not a bar.  Kernel by kernel: ``rocprofv3 --kernel-trace --stats -- python tools/log_mel_bench.py --no-eager``.
Prints one JSON line per shape.

    python tools/log_mel_bench.py [--iters 50] [--shapes 1x3,8x3,16x10] [--geometry 2048,1200,300,80,24000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS")
    ap.add_argument("--geometry", default="2048,1200,300,80,24000", help="n_fft,win_length,hop_length,n_mels,sample_rate")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    import logmel64 as L64
    from stylish_tts_amd import log_mel
    from stylish_tts_amd.runtime import HipModel, Segments

    geom = tuple(int(v) for v in a.geometry.split(","))
    n_fft, win, hop, n_mels, sr = geom
    mean, std = -4.0, 4.0
    eng = HipModel(None, 0)
    fb = torch.from_numpy(log_mel.filter_table(n_fft, n_mels, sr)[0]).cuda()  # [n_mels, bins]
    window = torch.hann_window(win, periodic=True, device="cuda")

    def eager(x):  # [B, samples] -> [B, n_mels, frames]
        spec = torch.stft(x, n_fft, hop, win, window, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        return (torch.log(1e-5 + torch.matmul(fb, spec.abs().pow(2.0))) - mean) / std

    with torch.no_grad():
        for shape in a.shapes.split(","):
            B, sec = [int(v) for v in shape.split("x")]
            n = sec * sr
            one = L64.signal(f"bench.{sec}", n, sr)
            x = torch.from_numpy(np.stack([np.roll(one, 997 * b) for b in range(B)])).cuda()
            flat, seg = x.reshape(-1).contiguous(), Segments([n] * B, eng.device)
            rows, seg_m = eng.log_mel(seg, flat, *geom, mean=mean, std=std, frames="all")
            T = seg_m.lengths[0]
            mel_ms = timed(lambda: eng.log_mel(seg, flat, *geom, mean=mean, std=std, frames="all"), a.iters)
            all_ms = timed(lambda: eng.log_mel(seg, flat, *geom, mean=mean, std=std, frames="all", energy=True, raw=True), a.iters)
            part = torch.empty(seg_m.rows, 2, dtype=torch.float64, device=eng.device)
            st = torch.empty(3, dtype=torch.float64, device=eng.device)
            import ctypes as C

            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def stats():  # the kernel pair alone, without the host read of HipModel.log_mel_stats
                assert eng.lib.stts_log_mel_stats(eng.ctx, stream, seg.n, seg.host_ptr, p(seg.dev), seg_m.host_ptr, p(seg_m.dev), p(flat), *geom, p(part), p(st)) == 0

            stats_ms = timed(stats, a.iters)
            rec = dict(batch=B, seconds=sec, geometry=list(geom), frames=T, rows=seg_m.rows, log_mel_ms=round(mel_ms, 4), with_energy_and_raw_ms=round(all_ms, 4),
                       stats_pair_ms=round(stats_ms, 4), us_per_frame=round(1e3 * mel_ms / seg_m.rows, 4), audio_seconds_per_second=round(B * sec / (mel_ms * 1e-3), 1),
                       launches=1, transform="fp32" if os.environ.get("STTS_LOG_MEL_F32", "0") not in ("", "0") else "fp64")
            if not a.no_eager:
                ref = eager(x)
                rec["eager_fp32_ms"] = round(timed(lambda: eager(x), a.iters), 4)
                rec["speedup_vs_eager"] = round(rec["eager_fp32_ms"] / mel_ms, 3)
                rec["max_abs_diff_vs_eager"] = float((ref.permute(0, 2, 1).reshape(B * T, n_mels) - rows).abs().max())
            print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
