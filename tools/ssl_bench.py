#!/usr/bin/env python3
"""AdaptiveHubert (the HuBERT content encoder) on the engine: ms per call and achieved TFLOP/s (algorithmic flops, 2 x MAC) against the
peak of the fp32 form the dense contractions use (split fp32 on the bf16 matrix cores: 6 bf16 MFMAs per 16 channels, 3/8 of the f32
matrix-core cycles), at B x seconds of 16 kHz audio.  Beside it a plain torch eager fp32 run of the same graph on the same GPU, total and
per stage from stream events (no ``transformers`` import: the graph is restated here with torch.nn.functional).  The engine's own split
per kernel comes from a kernel trace of this script (``rocprofv3 --kernel-trace --stats -- python tools/ssl_bench.py --shapes 8x3``).
The yardstick is measurement only; it is never in the product path.  Prints one JSON line per shape.

    python tools/ssl_bench.py [--iters 20] [--shapes 1x3,8x3,16x10]
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

PEAK_F32 = 157.3            # TFLOP/s, f32 matrix cores (MI355X)
PEAK_X3 = PEAK_F32 * 8 / 3  # the split-fp32 form: 16 f32 MFMAs' work in 6 bf16 MFMAs


def flops(a, samples: int, B: int) -> dict:
    from stylish_tts_amd import hubert_ssl

    n, cin, fe = samples, 1, 0.0
    for c, k, s in zip(a["conv_dim"], a["conv_kernel"], a["conv_stride"]):
        n = (n - k) // s + 1
        fe += 2.0 * n * c * cin * k
        cin = c
    Fr, H, I = hubert_ssl.frames(samples, a), a["hidden_size"], a["intermediate_size"]
    proj = 2.0 * Fr * cin * H
    pos = 2.0 * Fr * H * (H // a["num_conv_pos_embedding_groups"]) * a["num_conv_pos_embeddings"]
    layer = 2.0 * Fr * (4 * H * H + 2 * H * I) + 4.0 * Fr * Fr * H
    return dict(feature_extractor=B * fe, projection=B * proj, pos_conv=B * pos, transformer=B * a["num_hidden_layers"] * layer)


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


def eager_graph(sd, a, x, time_dim):
    """The same network in plain torch on the device of x: returns (forward, staged forward that also returns per-stage event times)."""
    from stylish_tts_amd import hubert_ssl

    dev = x.device
    W = {k[len("model."):]: v.to(dev) for k, v in sd.items()}
    q = "encoder.pos_conv_embed.conv."
    wpos = torch.from_numpy(hubert_ssl.fold_pos_conv_weight(sd["model." + q + "parametrizations.weight.original0"].numpy(),
                                                            sd["model." + q + "parametrizations.weight.original1"].numpy())).to(dev)
    H, heads, eps = a["hidden_size"], a["num_attention_heads"], a["layer_norm_eps"]
    kpos, G = a["num_conv_pos_embeddings"], a["num_conv_pos_embedding_groups"]

    def features(x):
        h = x[:, None]
        for i, s in enumerate(a["conv_stride"]):
            h = F.conv1d(h, W[f"feature_extractor.conv_layers.{i}.conv.weight"], stride=s)
            if i == 0:
                h = F.group_norm(h, h.shape[1], W["feature_extractor.conv_layers.0.layer_norm.weight"], W["feature_extractor.conv_layers.0.layer_norm.bias"], eps)
            h = F.gelu(h)
        return h.transpose(1, 2)

    def project(h):
        h = F.layer_norm(h, (h.shape[-1],), W["feature_projection.layer_norm.weight"], W["feature_projection.layer_norm.bias"], eps)
        return F.linear(h, W["feature_projection.projection.weight"], W["feature_projection.projection.bias"])

    def positional(h):
        p = F.conv1d(h.transpose(1, 2), wpos, W[q + "bias"], padding=kpos // 2, groups=G)
        if kpos % 2 == 0:
            p = p[:, :, :-1]
        h = h + F.gelu(p).transpose(1, 2)
        return F.layer_norm(h, (H,), W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps)

    def layers(h):
        B, T, _ = h.shape
        for i in range(a["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            lin = lambda n, t: F.linear(t, W[p + n + ".weight"], W[p + n + ".bias"])  # noqa: E731
            sp = lambda t: t.view(B, T, heads, H // heads).transpose(1, 2)  # noqa: E731
            o = F.scaled_dot_product_attention(sp(lin("attention.q_proj", h)), sp(lin("attention.k_proj", h)), sp(lin("attention.v_proj", h)))
            h = h + lin("attention.out_proj", o.transpose(1, 2).reshape(B, T, H))
            h = F.layer_norm(h, (H,), W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], eps)
            h = h + lin("feed_forward.output_dense", F.gelu(lin("feed_forward.intermediate_dense", h)))
            h = F.layer_norm(h, (H,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps)
        return h

    def resample(h):
        return F.interpolate(h.transpose(1, 2), size=time_dim, mode="nearest")

    stages = [("feature_extractor", features), ("projection", project), ("pos_conv", positional), ("transformer", layers), ("resample", resample)]

    def fwd():
        h = x
        for _, f in stages:
            h = f(h)
        return h

    def staged():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        h = x
        ev[0].record()
        for i, (_, f) in enumerate(stages):
            h = f(h)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return {n: ev[i].elapsed_time(ev[i + 1]) for i, (n, _) in enumerate(stages)}

    return fwd, staged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS at 16 kHz; time_dim = 80 frames per second")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel

    eng = HipModel(None, 0)
    m = modules.AdaptiveHubert(engine=eng).load_synthetic(0)
    sd = m.state_dict()
    with torch.no_grad():
        for shape in a.shapes.split(","):
            B, sec = [int(v) for v in shape.split("x")]
            S, T = 16000 * sec, 80 * sec
            x = torch.from_numpy((synth.normal(f"ssl.bench{B}", (B, S)) * 0.3).astype(np.float32)).cuda()
            y = m(x, T)
            ms = timed(lambda: m.packed(x, [T] * B), a.iters)
            if a.no_eager:
                print(json.dumps(dict(batch=B, seconds=sec, engine_ms=round(ms, 3))), flush=True)
                continue
            fwd, staged = eager_graph(sd, m.arch, x, T)
            ref = fwd()
            err = float((ref - y).abs().max())
            ms_ref = timed(fwd, a.iters)
            staged()
            st = staged()
            fl = flops(m.arch, S, B)
            tot = sum(fl.values())
            print(json.dumps(dict(batch=B, seconds=sec, samples=S, frames=m.frames(S), time_dim=T, engine_ms=round(ms, 3), gflop=round(tot * 1e-9, 1),
                                  gflop_by_stage={k: round(v * 1e-9, 2) for k, v in fl.items()}, tflops=round(tot / ms * 1e-9, 2),
                                  frac_split_fp32_peak=round(tot / ms * 1e-9 / PEAK_X3, 3), frac_f32_peak=round(tot / ms * 1e-9 / PEAK_F32, 3),
                                  eager_fp32_ms=round(ms_ref, 3), eager_stage_ms={k: round(v, 3) for k, v in st.items()},
                                  speedup_vs_eager=round(ms_ref / ms, 3), max_abs_diff_vs_eager=err)), flush=True)


if __name__ == "__main__":
    main()
