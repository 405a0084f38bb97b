#!/usr/bin/env python3
"""The text aligner and the CTC forced alignment on the engine: ms per call of the network (packed mel rows -> log-probs) and of the alignment
(log-probs + targets -> path, scores, durations, boundary probabilities), the network against a plain torch eager fp32 run of the same layers
built here from torch.nn on the same GPU in the same run, and the alignment against tests/aligner64.py on the host (float64 numpy, one
utterance after the other: the only other implementation there is; reported, not barred).  The alignment is also timed with the path given, so
that only the post-processing kernel runs: the difference is the Viterbi kernel, whose loop over the frames is serial.  Kernel by kernel:
``rocprofv3 --kernel-trace --stats -- python tools/aligner_bench.py --no-eager --no-host --shapes 8x3``.  Prints one JSON line per shape.

    python tools/aligner_bench.py [--iters 20] [--shapes 1x3x50,8x3x50,16x10x160]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

FRAMES_PER_SECOND = 80  # hop 300 at 24 kHz
PEAK_F32 = 157.3            # TFLOP/s, f32 matrix cores (MI355X)
PEAK_X3 = PEAK_F32 * 8 / 3  # the split-fp32 form: 16 f32 MFMAs' work in 6 bf16 MFMAs


def eager_network(d, sd):
    """CTCModel's layers in eval mode from torch.nn: (Conv1d, ReLU, BatchNorm1d(affine=False)) per TDNN layer, the Ffn with its skip, the output
    layer and log_softmax; dense batches of equal lengths (the mask is all ones)."""
    H = d["hidden"]

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.tdnn = nn.ModuleList()
            cin = d["n_mels"]
            for k in d["tdnn_kernel"]:
                self.tdnn.append(nn.Sequential(nn.Conv1d(cin, H, k, padding=(k - 1) // 2), nn.ReLU(), nn.BatchNorm1d(H, affine=False)))
                cin = H
            self.ffn = nn.Sequential(*[m for _ in range(d["ffn_layers"]) for m in (nn.Linear(H, H), nn.ReLU())])
            self.out = nn.Linear(H, d["classes"])

        def forward(self, x):  # [B, T, n_mels]
            x = x.permute(0, 2, 1)
            for layer in self.tdnn:
                x = layer(x)
            x = x.permute(0, 2, 1)
            x = self.ffn(x) + x
            return torch.log_softmax(self.out(x), dim=-1)

    net = Net().eval()
    n = len(d["tdnn_kernel"])
    with torch.no_grad():
        for i in range(n):
            q = f"encoder.layers.{i}"
            net.tdnn[i][0].weight.copy_(sd[q + ".0.weight"])
            net.tdnn[i][0].bias.copy_(sd[q + ".0.bias"])
            net.tdnn[i][2].running_mean.copy_(sd[q + ".2.running_mean"])
            net.tdnn[i][2].running_var.copy_(sd[q + ".2.running_var"])
        for j in range(d["ffn_layers"]):
            net.ffn[2 * j].weight.copy_(sd[f"encoder.layers.{n}.ffn.{3 * j}.weight"])
            net.ffn[2 * j].bias.copy_(sd[f"encoder.layers.{n}.ffn.{3 * j}.bias"])
        net.out.weight.copy_(sd["encoder_output_layer.weight"])
        net.out.bias.copy_(sd["encoder_output_layer.bias"])
    return net.cuda()


def flops_per_frame(d) -> float:
    """2 x MACs of every contraction per mel frame (un-padded sizes)."""
    H, fl, cin = d["hidden"], 0.0, d["n_mels"]
    for k in d["tdnn_kernel"]:
        fl += 2.0 * k * cin * H
        cin = H
    return fl + 2.0 * d["ffn_layers"] * H * H + 2.0 * H * d["classes"]


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x3x50,8x3x50,16x10x160", help="BxSECONDSxTOKENS at 80 mel frames per second")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    ap.add_argument("--no-host", action="store_true", help="skip the float64 alignment on the host")
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    m = modules.TextAligner(engine=eng).load_synthetic(0)
    m.engine
    d = m.dims
    per_frame = flops_per_frame(d)
    n_launch_net = 1 + len(d["tdnn_kernel"]) + 1 + d["ffn_layers"] + 1 + 1  # prepare, TDNN, last BatchNorm, Ffn, output layer, log-softmax
    with torch.no_grad():
        net = None if a.no_eager else eager_network(d, m.state_dict())
        for shape in a.shapes.split(","):
            B, sec, P = [int(v) for v in shape.split("x")]
            T = FRAMES_PER_SECOND * sec
            mel = torch.from_numpy(synth.normal(f"aligner.bench{B}x{sec}", (B, T, d["n_mels"])).astype(np.float32)).cuda()
            tok = np.clip((synth.uniform(f"aligner.bench.tok{B}x{sec}", (B, P)).astype(np.float64) * d["num_symbols"]).astype(np.int64), 0, d["num_symbols"] - 1)
            seg, seg_p = Segments([T] * B, eng.device), Segments([P] * B, eng.device)
            rows = mel.reshape(B * T, d["n_mels"]).contiguous()
            tg = torch.from_numpy(tok.reshape(-1).astype(np.int32)).cuda()
            lp = eng.text_aligner(seg, rows)
            r = eng.ctc_align(seg, lp, seg_p, tg, m.blank)
            net_ms = timed(lambda: eng.text_aligner(seg, rows), a.iters)
            align_ms = timed(lambda: eng.ctc_align(seg, lp, seg_p, tg, m.blank), a.iters)
            post_ms = timed(lambda: eng.ctc_align(seg, lp, seg_p, tg, m.blank, path=r["path"]), a.iters)
            both_ms = timed(lambda: eng.ctc_align(seg, eng.text_aligner(seg, rows), seg_p, tg, m.blank), a.iters)
            fl = per_frame * T * B
            rec = dict(batch=B, seconds=sec, frames=T, tokens=P, network_ms=round(net_ms, 3), align_ms=round(align_ms, 3), post_processing_only_ms=round(post_ms, 3),
                       viterbi_share_of_align=round(max(0.0, 1 - post_ms / align_ms), 3), network_plus_align_ms=round(both_ms, 3),
                       viterbi_share_of_call=round(max(0.0, align_ms - post_ms) / both_ms, 3), viterbi_us_per_frame=round(1e3 * max(0.0, align_ms - post_ms) / T, 3),
                       launches_network=n_launch_net, launches_align=2, network_gflop=round(fl * 1e-9, 2), mflop_per_frame=round(per_frame * 1e-6, 2),
                       network_tflops=round(fl / net_ms * 1e-9, 2), network_frac_split_fp32_peak=round(fl / net_ms * 1e-9 / PEAK_X3, 4),
                       network_frac_f32_peak=round(fl / net_ms * 1e-9 / PEAK_F32, 4))
            if not a.no_eager:
                ref = net(mel)
                rec["eager_fp32_ms"] = round(timed(lambda: net(mel), a.iters), 3)
                rec["network_speedup_vs_eager"] = round(rec["eager_fp32_ms"] / net_ms, 3)
                rec["max_abs_log_prob_diff_vs_eager"] = float((ref.reshape(B * T, -1) - lp).abs().max())
            if not a.no_host:
                import aligner64 as A

                lph = lp.cpu().double().numpy().reshape(B, T, -1)
                t0 = time.perf_counter()
                same = 0
                for b in range(B):
                    path, best = A.viterbi(lph[b], tok[b], m.blank)
                    dur = A.durations(path, P, m.blank)
                    A.boundaries(lph[b], tok[b], dur)
                    mine = r["path"][b * T : (b + 1) * T].cpu().numpy()
                    same += int(abs(A.path_score(lph[b], mine) - best) <= 1e-3)
                rec["host_float64_align_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["align_speedup_vs_host_float64"] = round(rec["host_float64_align_ms"] / align_ms, 1)
                rec["paths_within_1e-3_of_the_float64_optimum"] = f"{same}/{B}"
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
