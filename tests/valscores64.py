"""Float64 numpy restatement of the validation scores (csrc/val_scores.hip.h): MultiSpectrogram (train/multi_spectrogram.py), MultiResolutionSTFTLoss
and MagPhaseLoss (train/losses.py:14-154) and smooth_l1_loss of the reference, from their definitions.  Own DFT (numpy.fft); the mel filters are the
float64 HTK triangles rounded once to fp32 and widened again - the values the engine sums (stylish_tts_amd.log_mel.filter_table, bit for bit), so
that filter rounding is part of no error.  tests/golden/gen_golden_valscores.py pins it against the reference's modules run in float64
(tests/test_val_scores_cpu.py: to 1e-12 relative); the GPU tests compare against it, since the fixtures hold a sample of the tensors only.
Also the deterministic recipes of the test signals, shared with the generator."""
from __future__ import annotations

import numpy as np

SR, N_MELS, MASK = 24000, 128, 1e-3
RESOLUTIONS = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))  # (fft, hop, window): train/multi_spectrogram.py:13-20
MAGPHASE = (2048, 1200, 75)  # (n_fft, win_length, hop_length // 4): model.yml
TWO_PI = 2.0 * np.pi
SEED = 1  # of the signals' noise; the generator raises it if a bin lands on the mask threshold or a scalar's fp32 error cancels to nothing

# ragged batch A: 1025 is one sample more than the 2048 resolution's reflect padding accepts; 4800 and 3300 are 300 T (mag/phase rows 4 T + 1);
# 4800 / 50 + 1 = 97 frames is no multiple of a waves-per-block.  Equal-length batch B: 3157 is no multiple of any hop.
BATCHES = {"A": (4800, 3300, 1025), "B": (3157, 3157)}
IDENTICAL = {"A": 1, "B": None}  # the utterance whose prediction is its target


def signal(name: str, n: int, shift: float = 0.0, seed: int = SEED) -> np.ndarray:
    """A vibrato harmonic tone plus noise (fp32) in one loud block; around it the same at 1e-6, a stretch of exact zeros, and a 150-sample sinusoid
    at amplitude 1e-4, whose main lobe stands above the 1e-3 mask over a floor far below it.  shift: the tone's phase offset in radians.
    The layout answers the generator's condition (a), no bin within 1e3 fp32-run errors of the mask, which a frame with a floor NEAR 1e-3 breaks in
    every draw (an fp32 transform is wrong by ~3e-7 of the frame's largest bin):
      - the loud block begins and ends on multiples of 600 samples: under all three resolutions the last frame to overlap it does so by 20, 60 and
        120 or 240 samples, enough for a floor far above the mask, and the next frame not at all;
      - its noise is strong (0.5 beside a tone of 0.3), so that such a frame's Rayleigh floor is thin at 1e-3;
      - the first 600 samples, and a long signal's end, stay at 1e-6: a frame centred on a reflected edge is symmetric, its spectrum real, and a real
        Gaussian has its density AT 0.  There the magnitudes, wholly below the mask, still test the reflected indexing; the 1025-sample signal keeps
        a loud right edge, on which no frame is centred;
      - the sinusoid sits where the half window of the fft-2048 frame 0 has all but left it (weights below 0.15), so that frame keeps no bin: a
        kept bin of a real spectrum has an angle of 0 to rounding, an exact 0 in one transform and a 1e-15 in another, and the generator's
        condition (c) wants every kept angle exactly 0 or far from it, for the phase's zero pattern to be compared exactly."""
    from stylish_tts_amd import synth

    t = np.arange(n, dtype=np.float64) / SR
    f0 = 140.0 * (1.0 + 0.04 * np.sin(2.0 * np.pi * 5.5 * t))
    ph = 2.0 * np.pi * np.cumsum(f0) / SR + shift
    tone = sum(np.sin(k * ph) / k for k in range(1, 13))
    x = 0.3 * tone + 0.5 * synth.normal("valscores.noise." + name, (n,), seed).astype(np.float64)
    g = np.full(n, 1e-6)
    if n < 3000:  # quiet with the zeros and the sinusoid inside, then loud to the end
        g[600:] = 1.0
        g[80:280] = 0.0
        burst = 450
    else:  # quiet with the sinusoid inside, loud, zeros, quiet
        g[1200:2400] = 1.0
        g[2400:3000] = 0.0
        burst = 500
    x *= g
    u = synth.uniform("valscores.burst." + name, (2,), seed).astype(np.float64)
    i = np.arange(150)
    x[burst : burst + 150] += 1e-4 * np.sin(2.0 * np.pi * (600.0 + 2400.0 * u[0]) * i / SR + 2.0 * np.pi * u[1])
    return x.astype(np.float32)


def batch(key: str, seed: int = SEED):
    """(targets, predictions): lists of fp32 recordings; a prediction is a phase-shifted, differently-seeded copy, or the target itself."""
    tg = [signal(f"{key}.t{i}", n, 0.0, seed) for i, n in enumerate(BATCHES[key])]
    pr = [tg[i].copy() if i == IDENTICAL[key] else signal(f"{key}.p{i}", n, 0.4 + 0.1 * i, seed) for i, n in enumerate(BATCHES[key])]
    return tg, pr


def perturbed(x: np.ndarray, name: str) -> np.ndarray:
    """A waveform near x (fp32): 0.9 x plus noise at 0.01, for scoring a synthesised waveform against something that is not itself."""
    from stylish_tts_amd import synth

    x = np.asarray(x, np.float64)
    return (0.9 * x + 0.01 * synth.normal("valscores.perturb." + name, x.shape).astype(np.float64)).astype(np.float32)


def pred_spectra(key: str, i: int, frames: int, bins: int, seed: int = SEED):
    """The prediction's (log-magnitude, phase) [frames, bins] fp32 for MagPhaseLoss: values around log(1e-2) and angles in [-pi, pi), from the
    name-keyed generator (exactly reproducible, unlike a transform's last bits)."""
    from stylish_tts_amd import synth

    la = -4.5 + 1.5 * synth.normal(f"valscores.la.{key}.{i}", (frames, bins), seed).astype(np.float64)
    ph = np.pi * (2.0 * synth.uniform(f"valscores.ph.{key}.{i}", (frames, bins), seed).astype(np.float64) - 1.0)
    return la.astype(np.float32), ph.astype(np.float32)


def curves(key: str, n: int = 777, seed: int = SEED):
    """A pair of fp32 vectors whose differences straddle |d| = 1, with |d| exactly 1 and exactly 0 among them."""
    from stylish_tts_amd import synth

    a = (2.0 * synth.normal(f"valscores.curve.a.{key}", (n,), seed)).astype(np.float32)
    b = (a + 1.2 * synth.normal(f"valscores.curve.b.{key}", (n,), seed)).astype(np.float32)
    a[:4] = np.array([0.5, 3.0, -2.0, 7.25], np.float32)
    b[:4] = np.array([0.5, 2.0, -1.0, 7.25], np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------ arithmetic
def filters(n_fft: int, n_mels: int = N_MELS, sample_rate: int = SR) -> np.ndarray:
    """The fp32 filter values every run sums, [n_mels, n_fft // 2 + 1]: the library's host-side table (no GPU), which is formula_filters rounded once
    (two float64 builds of the formula can differ in a last bit, so the values are taken from one place)."""
    from stylish_tts_amd import log_mel

    return log_mel.filter_table(n_fft, n_mels, sample_rate)[0]


def formula_filters(n_fft: int, n_mels: int = N_MELS, sample_rate: int = SR) -> np.ndarray:
    """torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, 0, sample_rate // 2, n_mels, sample_rate, norm=None, mel_scale="htk") in float64,
    rounded once to fp32: [n_mels, n_fft // 2 + 1] float32."""
    f_max, bins = float(sample_rate // 2), n_fft // 2 + 1
    freqs = f_max * np.arange(bins, dtype=np.float64) / (bins - 1)
    m_max = 2595.0 * np.log10(1.0 + f_max / 700.0)
    f_pts = 700.0 * (np.power(10.0, (m_max * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1)) / 2595.0) - 1.0)
    down = (freqs[None, :] - f_pts[:-2, None]) / (f_pts[1:-1] - f_pts[:-2])[:, None]
    up = (f_pts[2:, None] - freqs[None, :]) / (f_pts[2:] - f_pts[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(down, up)).astype(np.float32)


def stft(x: np.ndarray, n_fft: int, hop: int, win: int) -> np.ndarray:
    """torch.stft(x, n_fft, hop, win, periodic Hann(win)) (center=True, reflect, one-sided, unnormalised) as [samples // hop + 1, n_fft // 2 + 1]."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.size > n_fft // 2
    xp = np.pad(x, n_fft // 2, mode="reflect")
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo : lo + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    T = x.size // hop + 1
    return np.fft.rfft(np.stack([xp[hop * f : hop * f + n_fft] for f in range(T)]) * w, axis=1)


def anti_wrap(d):
    return np.abs(d - TWO_PI * np.round(d / TWO_PI))


def multi_spectrogram(x: np.ndarray, res, fb=None):
    """calculate_single as time-major rows: (mag [F, 128], phase [F, bins], fft_mag [F, bins])."""
    fft, hop, win = res
    X = stft(x, fft, hop, win)
    fft_mag = np.abs(X)
    phase = (fft_mag > MASK) * np.angle(X)
    fb = filters(fft) if fb is None else fb
    return np.log1p(fft_mag @ fb.astype(np.float64).T), phase, fft_mag


def mel_sums(targets, preds, resolutions=RESOLUTIONS) -> np.ndarray:
    """[R, B, 2]: (sum |t - p|, sum |t|) of every utterance's log1p mel spectrogram at every resolution."""
    out = np.zeros((len(resolutions), len(targets), 2))
    for r, res in enumerate(resolutions):
        fb = filters(res[0])
        for u, (t, p) in enumerate(zip(targets, preds)):
            mt, mp = multi_spectrogram(t, res, fb)[0], multi_spectrogram(p, res, fb)[0]
            out[r, u] = np.abs(mt - mp).sum(), np.abs(mt).sum()
    return out


def mel_score(sums: np.ndarray):
    """(mel, mel_r [R], mel_utt [B]) of sums [R, B, 2]: the batch score per resolution is sum numerators / (sum denominators + 1e-6)."""
    mel_r = sums[:, :, 0].sum(axis=1) / (sums[:, :, 1].sum(axis=1) + 1e-6)
    mel_utt = (sums[:, :, 0] / (sums[:, :, 1] + 1e-6)).mean(axis=0)
    return float(mel_r.mean()), mel_r, mel_utt


def phase_weights(bins: int) -> np.ndarray:
    return np.power(np.exp(np.log(2.5) / (bins // 2)), np.arange(bins, dtype=np.float64))


def masked_target(gt: np.ndarray, geom=MAGPHASE):
    """(log(target_mag + 1e-9), mask, masked target phase) of MagPhaseLoss as [F, bins] rows."""
    n_fft, win, hop = geom
    Y = stft(gt, n_fft, hop, win)
    tm = np.abs(Y) + 1e-14
    on = tm > MASK
    return np.log(tm + 1e-9), on, on * np.angle(Y)


def magphase_sums(gts, logamps, phases, geom=MAGPHASE) -> np.ndarray:
    """[B, 4]: the L1 sum of "mag" and the three weighted anti-wrapping sums of "phase" (instantaneous, along the bins, along the frames); logamps /
    phases: the prediction's [F, bins] rows per utterance."""
    out = np.zeros((len(gts), 4))
    for u, (gt, la, ph) in enumerate(zip(gts, logamps, phases)):
        lt, on, tp = masked_target(gt, geom)
        la, pp = np.asarray(la, np.float64), on * np.asarray(ph, np.float64)
        assert la.shape == lt.shape == pp.shape
        w = phase_weights(lt.shape[1])[None, :]
        dfreq = lambda x: np.concatenate([-x[:, :1], x[:, :-1] - x[:, 1:]], axis=1)  # noqa: E731
        dtime = lambda x: np.concatenate([-x[:1], x[:-1] - x[1:]], axis=0)  # noqa: E731
        out[u] = (np.abs(la - lt).sum(), (w * anti_wrap(pp - tp)).sum(), (w * anti_wrap(dfreq(pp) - dfreq(tp))).sum(),
                  (w * anti_wrap(dtime(pp) - dtime(tp))).sum())
    return out


def magphase_score(sums: np.ndarray, rows: int, bins: int):
    """(mag, phase, the three phase terms): means over every (utterance, bin, frame)."""
    tot = sums.sum(axis=0) / (float(rows) * bins)
    return float(tot[0]), float(tot[1] + tot[2] + tot[3]), tot[1:]


def smooth_l1_sum(a, b) -> float:
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(np.where(d < 1.0, 0.5 * d * d, d - 0.5).sum())
