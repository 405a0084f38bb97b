#!/usr/bin/env python3
"""The reference's "mel" validation score between two sets of waveforms, on the engine (pipeline.validation_scores: MultiSpectrogram ->
MultiResolutionSTFTLoss of train/multi_spectrogram.py / train/losses.py, fused, fp64): A is the target, B the prediction.  The files are what
``bench.py --dump-outputs DIR`` writes (DIR/audio.npy): [utterances, samples], or one row of samples cut by --lengths.  Two runs with the same
arguments but another --precision compare output for output:

    python bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs out_f32
    python bench.py --gpus 1 --steps 2 --warmup 1 --precision bf16 --dump-outputs out_bf16
    python tools/compare_audio.py out_f32/audio.npy out_bf16/audio.npy

Prints the score per resolution, their mean, the worst utterance and the waveform max-abs difference, then one JSON line.

    python tools/compare_audio.py A.npy B.npy [--sample-rate 24000] [--lengths 72000,72000] [--slm DIR]

--slm DIR adds the reference's "slm" score (WavLMLoss, train/losses.py:408-426: the mean absolute difference of WavLM's 13 hidden states, both
files resampled from --sample-rate to 16 kHz on the engine) from the LOCAL WavLM checkpoint directory DIR (config.json + model.safetensors or
pytorch_model.bin; nothing is downloaded, no weights ship with the engine).  ``--slm synthetic`` runs the base network with the engine's synthetic
weights: the arithmetic of the score, not a perceptual number.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def utterances(a: np.ndarray, lengths):
    a = np.asarray(a, np.float32)
    if lengths:
        flat = a.reshape(-1)
        if sum(lengths) != flat.size:
            raise SystemExit(f"--lengths add up to {sum(lengths)} samples, the file holds {flat.size}")
        off = np.concatenate([[0], np.cumsum(lengths)])
        return [flat[off[i] : off[i + 1]] for i in range(len(lengths))]
    if a.ndim == 1:
        return [a]
    if a.ndim != 2:
        raise SystemExit(f"expected [utterances, samples] or [samples], got shape {a.shape}")
    return [row for row in a]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="the target waveforms (.npy)")
    ap.add_argument("b", help="the waveforms scored against them (.npy)")
    ap.add_argument("--sample-rate", type=int, default=None, help="of both files (default: the model config's)")
    ap.add_argument("--lengths", default="", help="comma-separated sample counts of the utterances in a flat file")
    ap.add_argument("--slm", default=None, metavar="DIR", help="also print the WavLM distance, from this local checkpoint directory ('synthetic': synthetic weights)")
    args = ap.parse_args()
    import torch

    from stylish_tts_amd import val_scores
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.modules import mel_score
    from stylish_tts_amd.runtime import HipModel, Segments

    lengths = [int(v) for v in args.lengths.split(",") if v]
    A, B = utterances(np.load(args.a), lengths), utterances(np.load(args.b), lengths)
    val_scores.check_pair([w.size for w in A], [w.size for w in B])
    eng = HipModel(load_model_config(), 0)
    sr = eng.cfg.sample_rate if args.sample_rate is None else args.sample_rate
    seg = Segments([w.size for w in A], eng.device)
    sums = eng.mel_sums(seg, torch.from_numpy(np.concatenate(A)), torch.from_numpy(np.concatenate(B)), sample_rate=sr)
    mel, mel_r, mel_utt = mel_score(sums.cpu().tolist())
    extra = {}
    if args.slm:
        from stylish_tts_amd import modules

        net = modules.WavLM(engine=eng).load_synthetic(0) if args.slm == "synthetic" else modules.WavLM(model_path=args.slm, engine=eng)
        slm, slm_utt = modules.WavLMLoss(net, sr).scores([torch.from_numpy(w) for w in A], [torch.from_numpy(w) for w in B])
        extra = dict(slm=slm, slm_utt_max=max(slm_utt))
    eng.close()
    for (fft, hop, window), v in zip((val_scores.as_tuple(r) for r in val_scores.resolutions), mel_r):
        print(f"mel at fft {fft:4d} hop {hop:3d} window {window:4d}: {v:.6e}")
    worst = int(np.argmax(mel_utt))
    max_abs = max(float(np.abs(x - y).max()) for x, y in zip(A, B))
    print(f"mel: {mel:.6e}   worst utterance {worst}: {mel_utt[worst]:.6e}   waveform max-abs difference: {max_abs:.3e}")
    if extra:
        print(f"slm: {extra['slm']:.6e}   worst utterance: {extra['slm_utt_max']:.6e}")
    print(json.dumps(dict(mel=mel, mel_r=mel_r, mel_utt_max=mel_utt[worst], utterances=len(A), sample_rate=sr, max_abs=max_abs, **extra)))


if __name__ == "__main__":
    main()
