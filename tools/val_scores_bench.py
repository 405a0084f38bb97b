#!/usr/bin/env python3
"""The validation scores on the engine (csrc/val_scores.hip.h): ms per call of pipeline.validation_scores - "mel" alone (three fused launches and
their reductions, one host read) and "mel" + "mag" / "phase" (the vocoder's time-major rows as the prediction) - beside a plain torch eager fp32 run
of the same arithmetic on the same GPU in the same process: torch.stft per resolution -> |.| -> matmul with the mel filters -> log1p -> L1 norms; and
torch.stft at the model geometry -> log / mask / angle -> the three anti-wrapping means.  Both sides end in one host read.  The eager time is the
yardstick to report against, not a bar.  Also what the choice between the two forms of the phase loss' time difference rests on: the whole
mag/phase call beside one transform per frame at its geometry (HipModel.multi_spectrogram, fft_mag only) - recomputing the neighbour's transform in
the same wave would add one of those; the scratch rows and the second launch cost the call's remainder.  Prints one JSON line per shape.

    python tools/val_scores_bench.py [--iters 50] [--shapes 1x3,8x3,16x10]
"""
from __future__ import annotations

import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="1x3,8x3,16x10", help="BxSECONDS")
    ap.add_argument("--no-eager", action="store_true", help="engine only (for a kernel trace of the engine's own launches)")
    a = ap.parse_args()
    import logmel64 as L64
    from stylish_tts_amd import log_mel, val_scores
    from stylish_tts_amd.pipeline import validation_scores
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(None, 0)
    sr, n_fft, win, hop, nb = eng.cfg.sample_rate, eng.n_fft, eng.win_length, eng.hop4, eng.n_bins
    res = [val_scores.as_tuple(r) for r in val_scores.resolutions]
    fbs = [torch.from_numpy(log_mel.filter_table(fft, val_scores.N_MELS, sr)[0]).cuda() for fft, _, _ in res]
    wins = [torch.hann_window(w, periodic=True, device="cuda") for _, _, w in res]
    win_mp = torch.hann_window(win, periodic=True, device="cuda")
    wk = torch.from_numpy(val_scores.phase_weights(nb).astype(np.float32)).cuda().reshape(1, nb, 1)
    two_pi = 2.0 * math.pi

    def eager_mel(gt, pr):
        loss = 0.0
        for (fft, h, w), fb, window in zip(res, fbs, wins):
            t, p = (torch.log1p(torch.matmul(fb, torch.stft(x, fft, h, w, window, return_complex=True).abs())) for x in (gt, pr))
            loss = loss + (t - p).abs().sum() / (t.abs().sum() + 1e-6)
        return loss / len(res)

    def eager_magphase(gt, la, ph):  # la, ph [B, bins, F]
        y = torch.stft(gt, n_fft, hop, win, win_mp, return_complex=True)
        tm = y.abs() + 1e-14
        on = tm > 1e-3
        mag = (la - torch.log(tm + 1e-9)).abs().mean()
        tp, pp = on * torch.angle(y), on * ph
        aw = lambda d: ((d - two_pi * torch.round(d / two_pi)).abs() * wk).mean()  # noqa: E731
        df = lambda x: torch.cat([-x[:, :1], x[:, :-1] - x[:, 1:]], dim=1)  # noqa: E731
        dt = lambda x: torch.cat([-x[:, :, :1], x[:, :, :-1] - x[:, :, 1:]], dim=2)  # noqa: E731
        return mag, aw(pp - tp) + aw(df(pp) - df(tp)) + aw(dt(pp) - dt(tp))

    with torch.no_grad():
        for shape in a.shapes.split(","):
            B, sec = [int(v) for v in shape.split("x")]
            n = sec * sr
            one = L64.signal(f"bench.{sec}", n, sr)
            gt = torch.from_numpy(np.stack([np.roll(one, 997 * b) for b in range(B)])).cuda()
            pr = (0.9 * gt + 0.01 * torch.randn_like(gt)).contiguous()
            T4 = n // hop
            la = torch.randn(B * T4, eng.ld_lp, device="cuda") * 1.5 - 4.5
            ph = (torch.rand(B * T4, eng.ld_lp, device="cuda") * 2.0 - 1.0) * math.pi
            seg = Segments([n] * B, eng.device)
            flat = gt.reshape(-1).contiguous()
            got = validation_scores(eng, pr, gt, prediction=(la, ph))
            mel_ms = timed(lambda: validation_scores(eng, pr, gt), a.iters)
            all_ms = timed(lambda: validation_scores(eng, pr, gt, prediction=(la, ph)), a.iters)
            # the mag/phase call on rows already padded to samples // hop + 1, and one transform per frame at its geometry
            rows = Segments([T4 + 1] * B, eng.device)
            idx = torch.cat([torch.cat([torch.arange(b * T4, (b + 1) * T4), torch.tensor([(b + 1) * T4 - 1])]) for b in range(B)]).cuda()
            la1, ph1 = la.index_select(0, idx).contiguous(), ph.index_select(0, idx).contiguous()
            mp_ms = timed(lambda: eng.magphase_sums(seg, flat, rows, la1, ph1, eng.ld_lp, n_fft, win, hop), a.iters)
            one_ms = timed(lambda: eng.multi_spectrogram(seg, flat, n_fft, win, hop, val_scores.N_MELS, sr, mag=False, fft_mag=True), a.iters)
            rec = dict(batch=B, seconds=sec, frames_per_resolution=[n // h + 1 for _, h, _ in res], magphase_frames=T4 + 1, mel_ms=round(mel_ms, 4),
                       mel_magphase_ms=round(all_ms, 4), magphase_kernels_ms=round(mp_ms, 4), one_transform_per_frame_ms=round(one_ms, 4),
                       audio_seconds_per_second_mel=round(B * sec / (mel_ms * 1e-3), 1), mel=got["mel"], mag=got["mag"], phase=got["phase"])
            if not a.no_eager:
                la3 = torch.cat([la[:, :nb].reshape(B, T4, nb), la[:, :nb].reshape(B, T4, nb)[:, -1:]], dim=1).permute(0, 2, 1).contiguous()
                ph3 = torch.cat([ph[:, :nb].reshape(B, T4, nb), ph[:, :nb].reshape(B, T4, nb)[:, -1:]], dim=1).permute(0, 2, 1).contiguous()
                e_mel = float(eager_mel(gt, pr))
                e_mag, e_phase = (float(v) for v in eager_magphase(gt, la3, ph3))

                def eager_all():
                    m = eager_mel(gt, pr)
                    g, p = eager_magphase(gt, la3, ph3)
                    return torch.stack([m, g, p]).cpu()

                rec["eager_fp32_mel_ms"] = round(timed(lambda: eager_mel(gt, pr).cpu(), a.iters), 4)
                rec["eager_fp32_mel_magphase_ms"] = round(timed(eager_all, a.iters), 4)
                rec["speedup_vs_eager_mel"] = round(rec["eager_fp32_mel_ms"] / mel_ms, 3)
                rec["speedup_vs_eager_mel_magphase"] = round(rec["eager_fp32_mel_magphase_ms"] / all_ms, 3)
                rec["eager_fp32"] = dict(mel=e_mel, mag=e_mag, phase=e_phase)
            print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
