#!/usr/bin/env python3
"""The WavLM perceptual distance ("slm", modules.WavLMLoss) on the engine: ms per call at B pairs x seconds of 16 kHz audio (one call = both
waveforms of every pair through WavLM-base with synthetic weights and the L1 sums of all 13 hidden states), 10 calls after 3 warm-up, from device
events.  Beside it the same graph in torch eager fp32 on the same GPU in the same process: ``transformers``' WavLMModel where ``import
transformers`` succeeds (the line says so: "comparator": "transformers"), otherwise the graph restated here with torch.nn.functional
("comparator": "restated").  The comparator runs the 2 B waveforms as one batch and takes the l1_loss of the stacked states, as the reference's
WavLMLoss does.  The engine's own split per kernel comes from a kernel trace of this script, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wavlm_bench.py --no-eager --shapes 8x3

The yardstick is measurement only; it is never in the product path.  Prints one JSON line per shape.

    python tools/wavlm_bench.py [--iters 10] [--shapes 1x3,8x3,16x10]
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


def restated(sd, a, dev):
    """WavLMModel's hidden states in plain torch: x [B, samples] -> list of 13 [B, frames, hidden]."""
    from stylish_tts_amd import hubert_ssl, wavlm

    W = {k: v.to(dev) for k, v in sd.items()}
    q = "encoder.pos_conv_embed.conv."
    wpos = torch.from_numpy(hubert_ssl.fold_pos_conv_weight(sd[q + "parametrizations.weight.original0"].numpy(), sd[q + "parametrizations.weight.original1"].numpy())).to(dev)
    H, heads, eps = a["hidden_size"], a["num_attention_heads"], a["layer_norm_eps"]
    kpos, G = a["num_conv_pos_embeddings"], a["num_conv_pos_embedding_groups"]

    def fwd(x):
        h = x[:, None]
        for i, s in enumerate(a["conv_stride"]):
            h = F.conv1d(h, W[f"feature_extractor.conv_layers.{i}.conv.weight"], stride=s)
            if i == 0:
                h = F.group_norm(h, h.shape[1], W["feature_extractor.conv_layers.0.layer_norm.weight"], W["feature_extractor.conv_layers.0.layer_norm.bias"], eps)
            h = F.gelu(h)
        h = h.transpose(1, 2)
        h = F.layer_norm(h, (h.shape[-1],), W["feature_projection.layer_norm.weight"], W["feature_projection.layer_norm.bias"], eps)
        h = F.linear(h, W["feature_projection.projection.weight"], W["feature_projection.projection.bias"])
        p = F.conv1d(h.transpose(1, 2), wpos, W[q + "bias"], padding=kpos // 2, groups=G)
        if kpos % 2 == 0:
            p = p[:, :, :-1]
        h = F.layer_norm(h + F.gelu(p).transpose(1, 2), (H,), W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps)
        B, T, _ = h.shape
        t = np.arange(T)
        bk = torch.from_numpy(wavlm.bucket(t[None, :] - t[:, None], a["num_buckets"], a["max_bucket_distance"])).to(dev)
        bias = W["encoder.layers.0.attention.rel_attn_embed.weight"][bk].permute(2, 0, 1)  # [heads, T, T]
        states = [h]
        for i in range(a["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            lin = lambda n, t: F.linear(t, W[p + n + ".weight"], W[p + n + ".bias"])  # noqa: E731
            sp = lambda t: t.view(B, T, heads, H // heads).transpose(1, 2)  # noqa: E731
            g = lin("attention.gru_rel_pos_linear", sp(h)).view(B, heads, T, 2, 4).sum(-1)
            ga, gb = torch.sigmoid(g).chunk(2, dim=-1)
            gate = ga * (gb * W[p + "attention.gru_rel_pos_const"] - 1.0) + 2.0
            o = F.scaled_dot_product_attention(sp(lin("attention.q_proj", h)), sp(lin("attention.k_proj", h)), sp(lin("attention.v_proj", h)), attn_mask=gate * bias[None])
            h = h + lin("attention.out_proj", o.transpose(1, 2).reshape(B, T, H))
            h = F.layer_norm(h, (H,), W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], eps)
            h = h + lin("feed_forward.output_dense", F.gelu(lin("feed_forward.intermediate_dense", h)))
            h = F.layer_norm(h, (H,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps)
            states.append(h)
        return states

    return fwd


def comparator(sd, a, dev):
    """(name, x -> hidden states) of the eager fp32 comparator."""
    try:
        os.environ.setdefault("HF_HUB_OFFLINE", "1")
        from transformers import WavLMConfig, WavLMModel
    except Exception:  # not installed (or not importable) where this runs: the restated graph
        return "restated", restated(sd, a, dev)
    m = WavLMModel(WavLMConfig(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in a.items()}))
    m.load_state_dict(sd, strict=True)
    m = m.eval().to(dev)
    return "transformers", lambda x: m(input_values=x, output_hidden_states=True).hidden_states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="PAIRSxSECONDS at 16 kHz")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel

    eng = HipModel(None, 0)
    m = modules.WavLM(engine=eng).load_synthetic(0)
    loss = modules.WavLMLoss(m, 16000)
    sd = m.state_dict()
    with torch.no_grad():
        name, states = (None, None) if a.no_eager else comparator(sd, m.arch, eng.device)
        for shape in a.shapes.split(","):
            B, sec = [int(v) for v in shape.split("x")]
            S = 16000 * sec
            x = torch.from_numpy((synth.normal(f"wavlm.bench{B}", (B, S)) * 0.3).astype(np.float32)).cuda()
            y = (x + 0.01 * torch.from_numpy(synth.normal(f"wavlm.benchn{B}", (B, S)).astype(np.float32)).cuda()).contiguous()
            mine = float(loss(x, y))
            ms = timed(lambda: loss.sums(x, y), a.iters)
            if a.no_eager:
                print(json.dumps(dict(pairs=B, seconds=sec, engine_ms=round(ms, 3), slm=mine)), flush=True)
                continue
            xy = torch.cat([x, y])

            def eager():
                hs = torch.stack(list(states(xy)))
                return F.l1_loss(hs[:, :B], hs[:, B:])

            ref = float(eager())
            ms_ref = timed(eager, a.iters)
            print(json.dumps(dict(pairs=B, seconds=sec, samples=S, frames=m.frames(S), engine_ms=round(ms, 3), comparator=name, eager_fp32_ms=round(ms_ref, 3),
                                  speedup_vs_eager=round(ms_ref / ms, 3), slm_engine=mine, slm_eager=ref)), flush=True)


if __name__ == "__main__":
    main()
