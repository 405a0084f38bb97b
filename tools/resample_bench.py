#!/usr/bin/env python3
"""The windowed-sinc resampler on the engine (csrc/resample.hip.h), packed recordings in, packed recordings out.  Two times per shape:
``resample_ms`` is a call of HipModel.resample as a user makes it, which also builds the output's Segments (a small host-to-device copy of the
offsets) and allocates the output; ``library_call_ms`` is stts_resample_forward alone on buffers made once - the host checks and the one kernel
launch.  At the small shapes both are host issue cost, not kernel time.  Beside them a plain torch eager fp32 run of what
torchaudio.transforms.Resample runs, on the same GPU in the same run: the kernel built in float64 and rounded to fp32, F.pad + F.conv1d at stride o, the output cut to ceil(n length / o).  The eager time is the yardstick to report against, not a
bar.  Kernel by kernel: ``rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py --no-eager``.  Prints one JSON line per shape.

    python tools/resample_bench.py [--iters 50] [--shapes 1x3,8x3,16x10] [--rates 24000:16000:6,24000:16000:128,44100:16000:6,44100:16000:128]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
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


def eager_kernel(o: int, n: int, lpw: int, rolloff: float = 0.99):
    """torchaudio's sinc_interp_hann kernel [n, 1, taps] as it builds it with dtype=None: float64 arithmetic, p / n in fp32, rounded to fp32."""
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1)[:, None, None] / n + idx
    t = (t * base).clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t) * window * (base / o)
    return k.to(torch.float32), width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS")
    ap.add_argument("--rates", default="24000:16000:6,24000:16000:128,44100:16000:6,44100:16000:128", help="ORIG:NEW:LOWPASS_FILTER_WIDTH")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    import resample64 as R64
    from stylish_tts_amd import resample
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    with torch.no_grad():
        for rate in a.rates.split(","):
            orig, new, lpw = [int(v) for v in rate.split(":")]
            o, n, width, taps = resample.geometry(orig, new, lpw)
            kern, kw = eager_kernel(o, n, lpw)
            kern = kern.cuda()

            def eager(x):  # [B, samples] -> [B, ceil(n samples / o)]
                y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (kw, kw + o))[:, None], kern, stride=o)
                return y.transpose(1, 2).reshape(x.shape[0], -1)[:, : resample.out_length(x.shape[1], orig, new)]

            for shape in a.shapes.split(","):
                B, sec = [int(v) for v in shape.split("x")]
                s = sec * orig
                one = R64.signal(f"bench.{sec}", s, orig)
                x = torch.from_numpy(np.stack([np.roll(one, 997 * b) for b in range(B)])).cuda()
                flat, seg = x.reshape(-1).contiguous(), Segments([s] * B, eng.device)
                out, seg_o = eng.resample(seg, flat, orig, new, lpw)
                ms = timed(lambda: eng.resample(seg, flat, orig, new, lpw), a.iters)
                p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def library_call():
                    assert eng.lib.stts_resample_forward(eng.ctx, stream, orig, new, lpw, 0.99, 0, 0.0, seg.n, seg.host_ptr, p(seg.dev), seg_o.host_ptr, p(seg_o.dev),
                                                         p(flat), p(out)) == 0

                lib_ms = timed(library_call, a.iters)
                fma = seg_o.rows * taps
                rec = dict(batch=B, seconds=sec, orig_freq=orig, new_freq=new, lowpass_filter_width=lpw, o=o, n=n, taps=taps, tile=resample.tile(orig, new),
                           samples_out=seg_o.rows, resample_ms=round(ms, 4), library_call_ms=round(lib_ms, 4), fp64_gflops=round(2e-6 * fma / lib_ms, 1),
                           audio_seconds_per_second=round(B * sec / (ms * 1e-3), 1))
                if not a.no_eager:
                    ref = eager(x)
                    rec["eager_fp32_ms"] = round(timed(lambda: eager(x), a.iters), 4)
                    rec["speedup_vs_eager"] = round(rec["eager_fp32_ms"] / ms, 3)
                    rec["max_abs_diff_vs_eager"] = float((ref.reshape(-1) - out).abs().max())
                print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
