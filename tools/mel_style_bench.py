#!/usr/bin/env python3
"""MelStyleEncoder on the engine: ms per call and 2-D convolution TFLOP/s (algorithmic flops, 2 x MAC) at B x 3-s mels (240 frames),
both configurations, with torch F.conv2d (MIOpen, fp32) on the same GPU as a yardstick.  The yardstick is measurement only; it is never
in the product path.  Prints one JSON line per case.

    python tools/mel_style_bench.py [--iters 30] [--batches 1,8,64]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"pe": ((80, 64, 384, True), "pe_mel_style_encoder"), "cfm": ((80, 256, 1024, True), "cfm_pitch_predictor.spk_emb")}
PEAK_F32 = 157.3  # TFLOP/s, f32 matrix cores (MI355X)


def conv_flops(args, T: int, B: int) -> float:
    dim_in, _, max_conv, skip = args
    Fq, t, c = dim_in, T, dim_in
    fl = 2.0 * c * 9 * Fq * t  # shared.0
    for i in range(4):
        co = min(2 * c, max_conv)
        down = not (i == 3 and skip)
        fl += 2.0 * c * c * 9 * Fq * t  # conv1
        Fo, to = (Fq // 2, (t + 1) // 2) if down else (Fq, t)
        if down:
            fl += 2.0 * c * 9 * Fo * to  # depthwise
        if c != co:
            fl += 2.0 * c * co * Fq * t  # the reference's 1x1 (before the pool)
        fl += 2.0 * c * co * 9 * Fo * to  # conv2
        Fq, t, c = Fo, to, co
    fl += 2.0 * c * c * 25 * (Fq - 4) * (t - 4)
    return B * fl


def timed(fn, iters: int, warmup: int = 5) -> float:
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


def miopen_forward(sd, args, x):
    from stylish_tts_amd import params

    dev = x.device

    def w(p):
        return torch.from_numpy(params.fold_spectral_norm(sd[p + ".weight_orig"].numpy(), sd[p + ".weight_u"].numpy(), sd[p + ".weight_v"].numpy())).float().to(dev)

    W = {k[: -len(".weight_orig")]: w(k[: -len(".weight_orig")]) for k in sd if k.endswith(".weight_orig")}
    Bv = {k[: -len(".bias")]: v.to(dev) for k, v in sd.items() if k.endswith(".bias")}
    dim_in, _, max_conv, skip = args
    lr = lambda t: F.leaky_relu(t, 0.2)  # noqa: E731

    def fwd():
        h = F.conv2d(x, W["shared.0"], Bv["shared.0"], padding=1)
        c = dim_in
        for i in range(4):
            co, q = min(2 * c, max_conv), f"shared.{i + 1}."
            down = not (i == 3 and skip)
            s = F.conv2d(h, W[q + "conv1x1"]) if c != co else h
            if down:
                s = F.avg_pool2d(s, 2)  # (T even here)
            r = F.conv2d(lr(h), W[q + "conv1"], Bv[q + "conv1"], padding=1)
            if down:
                r = F.conv2d(r, W[q + "downsample_res.conv"], Bv[q + "downsample_res.conv"], stride=2, padding=1, groups=c)
            h = (s + F.conv2d(lr(r), W[q + "conv2"], Bv[q + "conv2"], padding=1)) / np.sqrt(2.0)
            c = co
        h = lr(F.conv2d(lr(h), W["shared.6"], Bv["shared.6"]).mean(dim=(2, 3)))
        return F.linear(h, sd["unshared.weight"].to(dev), Bv["unshared"])

    return fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--frames", type=int, default=240)
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel

    eng = HipModel(None, 0)
    T = a.frames
    for cfg, (args, comp) in CONFIGS.items():
        enc = modules.MelStyleEncoder(*args, engine=eng, component=comp).load_synthetic(0)
        for B in [int(b) for b in a.batches.split(",")]:
            x = torch.from_numpy(synth.normal(f"bench{B}", (B, 1, 80, T))).cuda()
            enc(x)
            ms = timed(lambda: enc(x), a.iters)
            y = miopen_forward(enc.state_dict(), args, x)
            y()
            ms_ref = timed(y, a.iters)
            fl = conv_flops(args, T, B)
            print(json.dumps(dict(config=cfg, batch=B, frames=T, ms=round(ms, 4), conv_gflop=round(fl * 1e-9, 2), tflops=round(fl / ms * 1e-9, 2),
                                  frac_f32_peak=round(fl / ms * 1e-9 / PEAK_F32, 3), miopen_fp32_ms=round(ms_ref, 4),
                                  speedup_vs_miopen=round(ms_ref / ms, 3))), flush=True)


if __name__ == "__main__":
    main()
