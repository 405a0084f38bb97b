#!/usr/bin/env python3
"""The alignment scores on the engine, ms per call: ctc_nll (the CTC likelihood, one workgroup per utterance, fp64), the three reductions beside
it (confidence sums, label-prior sums, duration sums), the Viterbi launch of ctc_align for scale, and TextAligner.alignment_scores end to end
(aligner forward + ctc_align + ctc_nll + confidence + the one host read).  Beside them torch's own F.ctc_loss on the same device in the same run,
in fp32 and in fp64 - reported, not barred: where eager torch is faster the report says so.  Shapes as tools/aligner_bench.py.  Writes the
JSON lines and a summary to --out.

    python tools/align_scores_bench.py [--iters 20] [--shapes 1x3x50,8x3x50,16x10x160] [--out profiles/align_scores_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES_PER_SECOND = 80  # hop 300 at 24 kHz


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_scores_bench.txt"))
    a = ap.parse_args()
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    m = modules.TextAligner(engine=eng).load_synthetic(0)
    m.engine
    d = m.dims
    F = torch.nn.functional
    lines = []
    with torch.no_grad():
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
            pri = torch.full((d["classes"],), -3.0, dtype=torch.float64, device=eng.device)
            logits = torch.randn(B * P, 16, device=eng.device)
            classes16, w16 = tg % 16, torch.ones(16, device=eng.device)
            texts = torch.from_numpy(tok)
            nll = eng.ctc_nll(seg, lp, seg_p, tg, m.blank)
            nll_ms = timed(lambda: eng.ctc_nll(seg, lp, seg_p, tg, m.blank), a.iters)
            nll_pri_ms = timed(lambda: eng.ctc_nll(seg, lp, seg_p, tg, m.blank, log_priors=pri, prior_scale=0.3), a.iters)
            conf_ms = timed(lambda: eng.ctc_confidence_sums(seg, r["scores"]), a.iters)
            prior_ms = timed(lambda: eng.ctc_prior_sums(seg, lp), a.iters)
            dur_ms = timed(lambda: eng.duration_sums(seg_p, logits, classes16, w16), a.iters)
            align_ms = timed(lambda: eng.ctc_align(seg, lp, seg_p, tg, m.blank), a.iters)
            post_ms = timed(lambda: eng.ctc_align(seg, lp, seg_p, tg, m.blank, path=r["path"]), a.iters)
            e2e_ms = timed(lambda: m.alignment_scores(mel, [T] * B, texts, [P] * B), max(3, a.iters // 2))
            # torch's own CTC loss on the same log-probs, same device
            lp_tnc = lp.view(B, T, -1).permute(1, 0, 2).contiguous()
            tl, pl, tgt = torch.full((B,), T, dtype=torch.long), torch.full((B,), P, dtype=torch.long), torch.from_numpy(tok).cuda()
            lp64 = lp_tnc.double()
            t32 = F.ctc_loss(lp_tnc, tgt, tl, pl, blank=m.blank, reduction="none")
            t64 = F.ctc_loss(lp64, tgt, tl, pl, blank=m.blank, reduction="none")
            t32_ms = timed(lambda: F.ctc_loss(lp_tnc, tgt, tl, pl, blank=m.blank, reduction="none"), a.iters)
            t64_ms = timed(lambda: F.ctc_loss(lp64, tgt, tl, pl, blank=m.blank, reduction="none"), a.iters)
            rec = dict(batch=B, seconds=sec, frames=T, tokens=P, states=2 * P + 1, ctc_nll_ms=round(nll_ms, 3), ctc_nll_with_priors_ms=round(nll_pri_ms, 3),
                       ctc_nll_us_per_frame=round(1e3 * nll_ms / T, 3), confidence_sums_ms=round(conf_ms, 3), prior_sums_ms=round(prior_ms, 3),
                       duration_sums_ms=round(dur_ms, 3), viterbi_launch_ms=round(max(0.0, align_ms - post_ms), 3), ctc_align_ms=round(align_ms, 3),
                       alignment_scores_end_to_end_ms=round(e2e_ms, 3), torch_ctc_loss_fp32_ms=round(t32_ms, 3), torch_ctc_loss_fp64_ms=round(t64_ms, 3),
                       ctc_nll_vs_torch_fp32=round(t32_ms / nll_ms, 3), ctc_nll_vs_torch_fp64=round(t64_ms / nll_ms, 3),
                       max_rel_diff_vs_torch_fp64=float(((nll - t64).abs() / t64.abs()).max()), max_rel_diff_torch_fp32_vs_fp64=float(((t32.double() - t64).abs() / t64.abs()).max()))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    faster = [f"{r['batch']}x{r['seconds']}s: torch fp32 {r['torch_ctc_loss_fp32_ms']} ms / fp64 {r['torch_ctc_loss_fp64_ms']} ms against ctc_nll {r['ctc_nll_ms']} ms"
              for r in lines if min(r["torch_ctc_loss_fp32_ms"], r["torch_ctc_loss_fp64_ms"]) < r["ctc_nll_ms"]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/align_scores_bench.py --iters {a.iters} --shapes {a.shapes}: ms per call (host-timed launches included), {torch.cuda.get_device_name(0)}\n")
        for r in lines:
            f.write(json.dumps(r) + "\n")
        f.write("# eager torch's F.ctc_loss is faster than ctc_nll at: " + ("; ".join(faster) if faster else "no shape of this run") + "\n")
        f.write("# ctc_nll is bound by its serial loop over the frames: one barrier and, per state, up to two fp64 exp and one fp64 log per frame "
                "(ctc_nll_us_per_frame); one workgroup per utterance, so a batch of 1 uses one CU.\n")


if __name__ == "__main__":
    main()
