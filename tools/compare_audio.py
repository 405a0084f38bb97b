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

    python tools/compare_audio.py recordings.npy [resynth_out.npy] --resynth JOB.npz --checkpoint DIR [--lengths ...] [--slm DIR]

--resynth JOB.npz resynthesises the recordings of A on the engine and scores the result against them in the same command (copy-synthesis,
pipeline.Synthesizer.resynthesize: the posterior encoder's latent of each recording through post_flow and the vocoder - how good the vocoder half
of a checkpoint is, with the text half taken out of the question).  JOB.npz holds, for the utterances of A in order: ``tokens`` (all token ids, one
after the other), ``token_lengths`` [utterances], ``durations`` (mel frames per token, one per token) and ``pitch`` (Hz per mel frame, one after the
other); a recording must hold at least hop_length samples per mel frame and is cut to that.  --checkpoint is the reference's accelerate checkpoint
directory or a packed safetensors file (checkpoint.py) whose speech_predictor holds the posterior_encoder.* keys; ``synthetic`` runs the synthetic
weights.  With a second file name the resynthesised waveforms are also written there (one flat row; their lengths are printed).
When JOB.npz also holds ``energy`` (per mel frame, like ``pitch``) the command prints kl_text and kl_audio as well - NormalizingFlowLoss's two scores
(train/losses.py:205-222) from SpeechPredictor.forward(audio_gt=, flow_stats=True): how well the text prior and the audio posterior of the checkpoint
meet in latent space, the flow half of the question the mel score leaves open.
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


def flow_scores(sp, toks, durs, f0, energy, recordings):
    """kl_text / kl_audio of the batch: the module's training forward on padded tensors (a ragged batch comes back as lists per utterance)."""
    import torch

    from stylish_tts_amd import modules

    B, P, T = len(toks), max(len(t) for t in toks), max(sum(d) for d in durs)
    texts, al = torch.zeros(B, P, dtype=torch.int64), torch.zeros(B, P, T)
    pitch, en = torch.zeros(B, T), torch.zeros(B, T)
    for b in range(B):
        texts[b, : len(toks[b])] = torch.tensor(toks[b])
        t0 = 0
        for p_, d in enumerate(durs[b]):
            al[b, p_, t0 : t0 + d] = 1
            t0 += d
        pitch[b, :t0], en[b, :t0] = f0[b], energy[b]
    pred = sp(texts, torch.tensor([len(t) for t in toks]), al, pitch, en, audio_gt=[torch.from_numpy(w) for w in recordings], flow_stats=True)
    return modules.NormalizingFlowLoss(sp.cfg, engine=sp.engine).scores(pred)


def resynthesize(eng, recordings, job, checkpoint):
    """-> (the recordings cut to their alignments, the resynthesised waveforms, the KL scores or None), numpy rows."""
    import torch

    from stylish_tts_amd import checkpoint as ckpt
    from stylish_tts_amd import modules, pipeline

    sp = modules.SpeechPredictor(eng.cfg, engine=eng)
    if checkpoint == "synthetic":
        sp.load_synthetic(0).attach_posterior(modules.PosteriorEncoder.from_config(eng.cfg, engine=eng).load_synthetic(0))
    else:
        sds = ckpt.load_accelerate_checkpoint(checkpoint, ("speech_predictor",)) if os.path.isdir(checkpoint) else ckpt.load_packed(checkpoint)
        sp.load_state_dict(sds["speech_predictor"])
    if not sp.has_posterior:
        raise SystemExit("the checkpoint's speech_predictor holds no complete posterior_encoder.* set")
    sp.engine, sp.posterior.engine  # noqa: B018 - packs both
    tl = np.asarray(job["token_lengths"], np.int64)
    to = np.concatenate([[0], np.cumsum(tl)])
    if len(tl) != len(recordings):
        raise SystemExit(f"the job describes {len(tl)} utterances, A holds {len(recordings)}")
    toks = [[int(v) for v in job["tokens"][to[i] : to[i + 1]]] for i in range(len(tl))]
    durs = [[int(v) for v in job["durations"][to[i] : to[i + 1]]] for i in range(len(tl))]
    fo = np.concatenate([[0], np.cumsum([sum(d) for d in durs])])
    f0 = [torch.from_numpy(np.asarray(job["pitch"][fo[i] : fo[i + 1]], np.float32)) for i in range(len(tl))]
    out = pipeline.Synthesizer(eng).resynthesize(toks, [torch.from_numpy(w) for w in recordings], durs, f0)
    out = [w.cpu().numpy() for w in out]
    kl = None
    if "energy" in job:
        en = [torch.from_numpy(np.asarray(job["energy"][fo[i] : fo[i + 1]], np.float32)) for i in range(len(tl))]
        kl = flow_scores(sp, toks, durs, f0, en, recordings)
    return [r[: w.size] for r, w in zip(recordings, out)], out, kl


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="the target waveforms (.npy)")
    ap.add_argument("b", nargs="?", default=None, help="the waveforms scored against them (.npy); with --resynth: where the resynthesised waveforms are written (optional)")
    ap.add_argument("--sample-rate", type=int, default=None, help="of both files (default: the model config's)")
    ap.add_argument("--lengths", default="", help="comma-separated sample counts of the utterances in a flat file")
    ap.add_argument("--slm", default=None, metavar="DIR", help="also print the WavLM distance, from this local checkpoint directory ('synthetic': synthetic weights)")
    ap.add_argument("--resynth", default=None, metavar="JOB.npz", help="resynthesise A's recordings (tokens, token_lengths, durations, pitch) and score the result against them")
    ap.add_argument("--checkpoint", default="synthetic", help="with --resynth: checkpoint directory or packed file holding speech_predictor with posterior_encoder.* ('synthetic')")
    args = ap.parse_args()
    if args.b is None and args.resynth is None:
        ap.error("give B, or --resynth JOB.npz")
    import torch

    from stylish_tts_amd import val_scores
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.modules import mel_score
    from stylish_tts_amd.runtime import HipModel, Segments

    lengths = [int(v) for v in args.lengths.split(",") if v]
    A = utterances(np.load(args.a), lengths)
    eng = HipModel(load_model_config(), 0)
    if args.resynth:
        A, B, kl = resynthesize(eng, A, np.load(args.resynth), args.checkpoint)
        print("resynthesised lengths:", ",".join(str(w.size) for w in B))
        if args.b:
            np.save(args.b, np.concatenate(B))
    else:
        B = utterances(np.load(args.b), lengths)
    val_scores.check_pair([w.size for w in A], [w.size for w in B])
    sr = eng.cfg.sample_rate if args.sample_rate is None else args.sample_rate
    seg = Segments([w.size for w in A], eng.device)
    sums = eng.mel_sums(seg, torch.from_numpy(np.concatenate(A)), torch.from_numpy(np.concatenate(B)), sample_rate=sr)
    mel, mel_r, mel_utt = mel_score(sums.cpu().tolist())
    extra = {}
    if args.resynth and kl is not None:
        extra.update(kl_text=kl["kl_text"], kl_audio=kl["kl_audio"])
    if args.slm:
        from stylish_tts_amd import modules

        net = modules.WavLM(engine=eng).load_synthetic(0) if args.slm == "synthetic" else modules.WavLM(model_path=args.slm, engine=eng)
        slm, slm_utt = modules.WavLMLoss(net, sr).scores([torch.from_numpy(w) for w in A], [torch.from_numpy(w) for w in B])
        extra.update(slm=slm, slm_utt_max=max(slm_utt))
    eng.close()
    for (fft, hop, window), v in zip((val_scores.as_tuple(r) for r in val_scores.resolutions), mel_r):
        print(f"mel at fft {fft:4d} hop {hop:3d} window {window:4d}: {v:.6e}")
    worst = int(np.argmax(mel_utt))
    max_abs = max(float(np.abs(x - y).max()) for x, y in zip(A, B))
    print(f"mel: {mel:.6e}   worst utterance {worst}: {mel_utt[worst]:.6e}   waveform max-abs difference: {max_abs:.3e}")
    if "kl_text" in extra:
        print(f"kl_text: {extra['kl_text']:.6e}   kl_audio: {extra['kl_audio']:.6e}")
    if "slm" in extra:
        print(f"slm: {extra['slm']:.6e}   worst utterance: {extra['slm_utt_max']:.6e}")
    print(json.dumps(dict(mel=mel, mel_r=mel_r, mel_utt_max=mel_utt[worst], utterances=len(A), sample_rate=sr, max_abs=max_abs, **extra)))


if __name__ == "__main__":
    main()
