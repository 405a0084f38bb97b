#!/usr/bin/env python3
"""The RMVPE pitch extractor on the engine: ms per call (mel -> salience -> f0) against a plain torch eager fp32 run of the same network on the
same GPU in the same run, the convolution part's fraction of the f32 matrix-core peak (69.4 MFLOP per 10 ms frame at full size, counted from
the layer shapes below), and the GRU recurrence's time per step (a call with only that kernel's share comes from a kernel trace of this
script: ``rocprofv3 --kernel-trace --stats -- python tools/rmvpe_bench.py --no-eager --shapes 8x3``).  The torch restatement here is written
from the network's description, with torch.nn.functional only; it is the yardstick and the CPU tests' cross-check, never in the
product path.  Prints one JSON line per shape.

    python tools/rmvpe_bench.py [--iters 10] [--shapes 1x3,8x3,16x10]
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

PEAK_F32 = 157.3  # TFLOP/s, f32 matrix cores (MI355X)
BN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------ the network in plain torch
def _bn(x, W, p):
    shape = (1, -1, 1, 1)
    return (x - W[p + ".running_mean"].view(shape)) / torch.sqrt(W[p + ".running_var"].view(shape) + BN_EPS) * W[p + ".weight"].view(shape) + W[p + ".bias"].view(shape)


def _res_block(x, W, p):
    """relu(bn(conv3x3)) twice, then + shortcut(x): a 1 x 1 conv with bias where the channel count changes, x itself otherwise."""
    y = F.relu(_bn(F.conv2d(x, W[p + ".conv.0.weight"], padding=1), W, p + ".conv.1"))
    y = F.relu(_bn(F.conv2d(y, W[p + ".conv.3.weight"], padding=1), W, p + ".conv.4"))
    if p + ".shortcut.weight" in W:
        x = F.conv2d(x, W[p + ".shortcut.weight"], W[p + ".shortcut.bias"])
    return y + x


def unet_taps(W, d, x):
    """x [B, 1, T, 128] with T a multiple of 32 -> dict of the taps (enc0 .. 4 pooled, inter, dec0 .. 4, cnn, gru, hidden)."""
    nb, out = d["n_blocks"], {}
    x = _bn(x, W, "unet.encoder.bn")
    skips = []
    for l in range(5):
        for b in range(nb):
            x = _res_block(x, W, f"unet.encoder.layers.{l}.conv.{b}")
        skips.append(x)
        x = F.avg_pool2d(x, 2)
        out[f"enc{l}"] = x
    for i in range(d["inter_layers"]):
        for b in range(nb):
            x = _res_block(x, W, f"unet.intermediate.layers.{i}.conv.{b}")
    out["inter"] = x
    for i in range(5):
        q = f"unet.decoder.layers.{i}"
        x = F.relu(_bn(F.conv_transpose2d(x, W[q + ".conv1.0.weight"], stride=2, padding=1, output_padding=1), W, q + ".conv1.1"))
        x = torch.cat((x, skips[4 - i]), dim=1)
        for b in range(nb):
            x = _res_block(x, W, f"{q}.conv2.{b}")
        out[f"dec{i}"] = x
    x = F.conv2d(x, W["cnn.weight"], W["cnn.bias"], padding=1)
    out["cnn"] = x
    B, _, T, M = x.shape
    seq = x.permute(0, 2, 1, 3).reshape(B, T, 3 * M)  # feature index c * 128 + f
    if "gru_module" in W:  # the benchmark's comparator: torch's own fused GRU
        h = W["gru_module"](seq)[0]
    else:
        h = torch.cat((_gru_dir(seq, W, ""), _gru_dir(seq.flip(1), W, "_reverse").flip(1)), dim=2)
    out["gru"] = h
    out["hidden"] = torch.sigmoid(F.linear(h, W["fc.1.weight"], W["fc.1.bias"]))
    return out


def _gru_dir(seq, W, sfx):
    """One direction of a GRU layer, gates in the order (r, z, n): n = tanh(W_in x + b_in + r * (W_hn h + b_hn)), h' = (1 - z) n + z h."""
    wi, wh = W["fc.0.gru.weight_ih_l0" + sfx], W["fc.0.gru.weight_hh_l0" + sfx]
    bi, bh = W["fc.0.gru.bias_ih_l0" + sfx], W["fc.0.gru.bias_hh_l0" + sfx]
    H = wh.shape[1]
    gi = F.linear(seq, wi, bi)
    h = seq.new_zeros(seq.shape[0], H)
    outs = []
    for t in range(seq.shape[1]):
        gh = F.linear(h, wh, bh)
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H : 2 * H] + gh[:, H : 2 * H])
        n = torch.tanh(gi[:, t, 2 * H :] + r * gh[:, 2 * H :])
        h = (1 - z) * n + z * h
        outs.append(h)
    return torch.stack(outs, dim=1)


def attach_gru(W):
    """torch.nn.GRU with the network's weights, used by unet_taps in place of the step-by-step loop (a Python loop would flatter the engine)."""
    wi = W["fc.0.gru.weight_ih_l0"]
    g = torch.nn.GRU(wi.shape[1], wi.shape[0] // 3, 1, batch_first=True, bidirectional=True).to(device=wi.device, dtype=wi.dtype)
    g.load_state_dict({k[len("fc.0.gru."):]: v for k, v in W.items() if k.startswith("fc.0.gru.")})
    W["gru_module"] = g.eval()
    return W


def mel2hidden(W, d, mel, taps: bool = False):
    """mel [B, 128, T] (one length for the batch) -> salience [B, T, 360]: reflect padding to the next multiple of 32 frames, the network, the crop."""
    T = mel.shape[-1]
    Tp = 32 * ((T - 1) // 32 + 1)
    x = F.pad(mel, (0, Tp - T), mode="reflect") if Tp > T else mel
    t = unet_taps(W, d, x.transpose(1, 2)[:, None])
    return t if taps else t["hidden"][:, :T]


def decode(hidden, thred: float = 0.03):
    """Salience [..., 360] -> f0 in Hz: the salience-weighted mean of the bins' cents (20 i + 1997.379...) over the nine bins around the argmax
    (clipped to the table), 10 * 2^(cents / 1200); 0 where the largest salience is below thred."""
    from stylish_tts_amd.rmvpe import CENTS_0

    n = hidden.shape[-1]
    idx = torch.arange(n, device=hidden.device)
    cents = (idx * 20 + CENTS_0).to(torch.float32)
    c = hidden.argmax(dim=-1, keepdim=True)
    mask = (idx >= (c - 4).clamp(min=0)) & (idx < (c + 5).clamp(max=n))
    w = hidden * mask
    ws = w.sum(-1)
    f0 = 10 * 2 ** ((w * cents).sum(-1) / (ws + (ws == 0)) / 1200)
    return f0 * ~(hidden.max(dim=-1)[0] < thred)


def log_mel(audio, basis, linear: bool = False):
    """audio [B, samples] at 16 kHz -> log-mel [B, 128, samples // 160 + 1] (centred 1024-point STFT, hop 160, periodic Hann, magnitude)."""
    spec = torch.stft(audio, 1024, hop_length=160, win_length=1024, window=torch.hann_window(1024, dtype=audio.dtype, device=audio.device), center=True,
                      return_complex=True)
    mel = torch.matmul(basis.to(audio.dtype), spec.abs())
    return mel if linear else torch.log(torch.clamp(mel, min=1e-5))


def to_dtype(sd, dtype, device="cpu"):
    return {k: torch.as_tensor(v).to(device=device, dtype=dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


# ------------------------------------------------------------------------------------------------ the benchmark
def conv_flops_per_frame(d) -> float:
    """2 x MACs of every convolution per 10 ms frame (128 mel bins per frame at level 0)."""
    nb, c0, fl = d["n_blocks"], d["en_out_channels"], 0.0

    def block(cin, cout, pos):
        return 2.0 * pos * (9 * cin * cout + 9 * cout * cout + (cin * cout if cin != cout else 0))

    cin, cout = 1, c0
    for l in range(5):
        pos = 128.0 / 4**l
        for b in range(nb):
            fl += block(cin if b == 0 else cout, cout, pos)
        cin, cout = cout, cout * 2
    pos = 128.0 / 4**5
    for i in range(d["inter_layers"]):
        for b in range(nb):
            fl += block(cin if (i == 0 and b == 0) else cout, cout, pos)
    dc = cout
    for i in range(5):
        oc, pos_out = dc // 2, 128.0 / 4 ** (4 - i)
        fl += 2.0 * pos_out * 2.25 * dc * oc
        for b in range(nb):
            fl += block(2 * oc if b == 0 else oc, oc, pos_out)
        dc = oc
    return fl + 2.0 * 128 * 9 * c0 * 3


def timed(fn, iters: int, warmup: int = 2) -> float:
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS at 100 frames per second")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel

    eng = HipModel(None, 0)
    m = modules.RmvpePitchExtractor(engine=eng).load_synthetic(0)
    per_frame = conv_flops_per_frame(m.dims)
    with torch.no_grad():
        W = None if a.no_eager else attach_gru(to_dtype(m.state_dict(), torch.float32, "cuda"))
        for shape in a.shapes.split(","):
            B, sec = [int(v) for v in shape.split("x")]
            T = 100 * sec
            mel = torch.from_numpy((synth.normal(f"rmvpe.bench{B}", (B, 128, T)) * 2 - 5).astype(np.float32)).cuda()
            f0 = m(mel)
            ms = timed(lambda: m.packed(mel), a.iters)
            Tp = 32 * ((T - 1) // 32 + 1)
            fl = per_frame * Tp * B
            rec = dict(batch=B, seconds=sec, frames=T, padded_frames=Tp, engine_ms=round(ms, 3), conv_gflop=round(fl * 1e-9, 2),
                       conv_mflop_per_frame=round(per_frame * 1e-6, 1), whole_call_frac_f32_peak=round(fl / ms * 1e-9 / PEAK_F32, 3))
            if not a.no_eager:
                ref = decode(mel2hidden(W, m.dims, mel))
                rec["eager_fp32_ms"] = round(timed(lambda: decode(mel2hidden(W, m.dims, mel)), max(2, a.iters // 3), 1), 3)
                rec["speedup_vs_eager"] = round(rec["eager_fp32_ms"] / ms, 3)
                rec["voiced_pattern_equal"] = bool(((ref == 0) == (f0 == 0)).all())
                v = (ref > 0) & (f0 > 0)
                rec["max_rel_f0_diff_vs_eager"] = float(((ref - f0).abs() / ref.clamp(min=1))[v].max()) if bool(v.any()) else 0.0
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
