#!/usr/bin/env python3
"""CfmPitchPredictor on the engine: ms per call at B x T asr frames (80 frames per second: 3 s = 240, 10 s = 800), the speaker branch
(spk_emb MelStyleEncoder on a mel of the same length) split from the frame-rate network by events inside one serialised call, and a
torch-eager comparator of the same math on the same GPU (MIOpen convs; measurement only, never in the product path).  Prints one JSON
line per case.

    python tools/cfm_pitch_bench.py [--iters 20] [--cases 1x240,8x240,16x800]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def eager_frame_net(sd, x, spk):
    """asr_emb + 4 ConvNeXt blocks + out_proj in torch eager, fp32 (x [B, asr_dim, T], spk [B, 256])."""
    h = F.conv1d(F.mish(F.conv1d(x, sd["asr_emb.0.weight"], sd["asr_emb.0.bias"])), sd["asr_emb.2.weight"], sd["asr_emb.2.bias"])
    for i in range(4):
        q = f"blocks.{i}."
        y = F.conv1d(h, sd[q + "dwconv.weight"], sd[q + "dwconv.bias"], padding=3, groups=256).transpose(1, 2)
        g = F.linear(spk, sd[q + "norm.fc.weight"], sd[q + "norm.fc.bias"])[:, None]
        y = (1 + g[..., :256]) * F.layer_norm(y, (256,), eps=1e-6) + g[..., 256:]
        y = F.silu(F.linear(y, sd[q + "pwconv1.weight"], sd[q + "pwconv1.bias"]))
        gx = torch.norm(y, p=2, dim=1, keepdim=True)
        y = sd[q + "grn.gamma"] * (y * (gx / (gx.mean(dim=-1, keepdim=True) + 1e-6))) + sd[q + "grn.beta"] + y
        h = h + F.linear(y, sd[q + "pwconv2.weight"], sd[q + "pwconv2.bias"]).transpose(1, 2)
    return F.conv1d(h, sd["out_proj.weight"], sd["out_proj.bias"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="1x240,8x240,16x800")
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    m = modules.CfmPitchPredictor(768, 80, engine=eng).load_synthetic(0)
    sd = {k: v.cuda() for k, v in m.state_dict().items()}
    stats = (7.4, 0.45)
    for case in a.cases.split(","):
        B, T = (int(v) for v in case.split("x"))
        x = torch.from_numpy(synth.normal(f"cpb.asr{B}x{T}", (B, 768, T))).cuda()
        mel = torch.from_numpy(synth.normal(f"cpb.mel{B}x{T}", (B, 80, T))).cuda()
        L = [T] * B
        m.run(x, mel, f0_log2_stats=stats)
        ms_call = timed(lambda: m.run(x, mel, f0_log2_stats=stats), a.iters)
        # stage split inside one serialised call, packed inputs prepared outside the events
        seg = Segments(L, eng.device)
        rows = modules._pack_rows(eng, x, L)
        mel_rows = torch.cat([mel[b].t() for b in range(B)]).contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def staged():
            ev[0].record()
            spk = eng.mel_style(modules.W_CFM_PITCH, seg, mel_rows, 256)
            ev[1].record()
            eng.cfm_pitch(seg, rows, spk, f0_log2_stats=stats)
            ev[2].record()

        spk_ms = net_ms = 0.0
        for _ in range(5):
            staged()
        for _ in range(a.iters):
            staged()
            torch.cuda.synchronize()
            spk_ms += ev[0].elapsed_time(ev[1]) / a.iters
            net_ms += ev[1].elapsed_time(ev[2]) / a.iters
        spk = eng.mel_style(modules.W_CFM_PITCH, seg, mel_rows, 256)
        with torch.no_grad():
            ref = eager_frame_net(sd, x, spk)
            eager_ms = timed(lambda: eager_frame_net(sd, x, spk), a.iters)
        got = m(x, mel)
        err = float((got - ref).abs().max() / ref.abs().max())
        # algorithmic flops of the frame-rate network (2 x MAC): asr_emb, per block dwconv + pwconv1 + pwconv2, out_proj
        fl = 2.0 * B * T * (768 * 1024 + 1024 * 256 + 4 * (256 * 7 + 2 * 256 * 1024) + 256)
        print(json.dumps(dict(batch=B, frames=T, ms_per_call=round(ms_call, 4), speaker_branch_ms=round(spk_ms, 4), frame_net_ms=round(net_ms, 4),
                              frame_net_gflop=round(fl * 1e-9, 3), frame_net_tflops=round(fl / net_ms * 1e-9, 2), eager_frame_net_ms=round(eager_ms, 4),
                              frame_net_speedup_vs_eager=round(eager_ms / net_ms, 3), rel_err_vs_eager=float(f"{err:.2e}"))), flush=True)


if __name__ == "__main__":
    main()
