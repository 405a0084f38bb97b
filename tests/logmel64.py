"""Float64 numpy restatement of the log-mel front end (csrc/log_mel.hip.h): torchaudio.transforms.MelSpectrogram at its defaults, from its documented
definition, followed by calculate_mel / preprocess / log_norm / compute_log_mel_stats of the reference (train/stage_type.py:1023-1032,
train/dataprep/align_text.py:112-117, train/utils.py:71-148).  Own DFT (numpy.fft), own filter table.  tests/golden/gen_golden_logmel.py pins it
against the reference's functions run in float64 (tests/test_log_mel_cpu.py: to 1e-12 of scale); the GPU tests compare against it where no fixture
exists.  Also the recipes of the test signals, shared with the generator."""
from __future__ import annotations

import numpy as np

# (n_fft, win_length, hop_length, n_mels, sample_rate), (mean, std) of the normalisation
CASES = {
    "g2048": ((2048, 1200, 300, 80, 24000), (-4.0, 4.0)),
    "g512": ((512, 400, 100, 48, 16000), (-3.2, 3.7)),
    "g4096": ((4096, 2400, 600, 128, 48000), (-4.0, 4.0)),
    "g256": ((256, 256, 64, 80, 24000), (-5.5, 2.25)),
}


def lengths(geom):
    """Three utterances: the shortest legal one (n_fft / 2 + 1 samples), about 0.4 s as an exact multiple of the hop, about 0.3 s that is not."""
    n_fft, _, hop, _, sr = geom
    return [n_fft // 2 + 1, int(round(0.4 * sr / hop)) * hop, int(round(0.3 * sr / hop)) * hop + hop // 2 + 1]


def signal(name: str, n: int, sample_rate: int) -> np.ndarray:
    """A vibrato harmonic tone under a slow envelope plus noise at 0.02 (fp32, from the name-keyed generator)."""
    from stylish_tts_amd import synth

    t = np.arange(n, dtype=np.float64) / sample_rate
    f0 = 140.0 * (1.0 + 0.04 * np.sin(2.0 * np.pi * 5.5 * t))
    ph = 2.0 * np.pi * np.cumsum(f0) / sample_rate
    tone = sum(np.sin(k * ph) / k for k in range(1, 13))
    env = 0.15 + 0.85 * (0.5 - 0.5 * np.cos(2.0 * np.pi * 3.1 * t + 0.7))
    return (0.3 * env * tone + 0.02 * synth.normal("logmel.noise." + name, (n,)).astype(np.float64)).astype(np.float32)


def signals(case: str):
    """The case's three recordings: u0 scaled by 1e-3, the second half of u1 exactly zero, u2 as it is."""
    geom, _ = CASES[case]
    out = [signal(f"{case}.{i}", n, geom[4]) for i, n in enumerate(lengths(geom))]
    out[0] = (out[0].astype(np.float64) * 1e-3).astype(np.float32)
    out[1][out[1].size // 2 :] = 0.0
    return out


def filters(n_fft: int, n_mels: int, sample_rate: int) -> np.ndarray:
    """torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, 0, sample_rate // 2, n_mels, sample_rate, norm=None, mel_scale="htk") as
    [n_mels, n_fft // 2 + 1] float64: triangles between the points 700 (10^(m / 2595) - 1) of a uniform grid in m = 2595 log10(1 + f / 700)."""
    f_max = float(sample_rate // 2)
    freqs = np.linspace(0.0, f_max, n_fft // 2 + 1)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + f_max / 700.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
    return np.maximum(0.0, np.minimum(down, up)).T.copy()


def frames(samples: int, hop: int, policy: str) -> int:
    n = samples // hop + 1
    return {"even": n - n % 2, "drop_last": n - 1, "all": n}[policy]


def power(x: np.ndarray, n_fft: int, win: int, hop: int) -> np.ndarray:
    """|torch.stft(center=True, pad_mode="reflect", window=periodic Hann(win) centred in n_fft)|^2 as re^2 + im^2: [samples // hop + 1, n_fft // 2 + 1]."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.size > n_fft // 2
    xp = np.pad(x, n_fft // 2, mode="reflect")
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo : lo + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    T = x.size // hop + 1
    fr = np.stack([xp[hop * f : hop * f + n_fft] for f in range(T)]) * w
    X = np.fft.rfft(fr, axis=1)
    return X.real**2 + X.imag**2


def raw_log_mel(x: np.ndarray, geom, policy: str = "all") -> np.ndarray:
    """log(1e-5 + mel) as time-major rows [frames, n_mels]."""
    n_fft, win, hop, n_mels, sr = geom
    mel = power(x, n_fft, win, hop) @ filters(n_fft, n_mels, sr).T
    return np.log(1e-5 + mel)[: frames(np.asarray(x).size, hop, policy)]


def log_mel(x: np.ndarray, geom, mean: float, std: float, policy: str = "even") -> np.ndarray:
    return (raw_log_mel(x, geom, policy) - mean) / std


def energy(x: np.ndarray, geom, mean: float, std: float, policy: str = "even") -> np.ndarray:
    """log_norm of the normalised mel, summed over the mel axis: [frames]."""
    return (np.exp(log_mel(x, geom, mean, std, policy) * std + mean) ** 0.33).sum(axis=1)


def partials(x: np.ndarray, geom) -> np.ndarray:
    """Per-frame (sum, sum of squares) of the raw log-mel over the mel axis, all frames: [frames, 2]."""
    r = raw_log_mel(x, geom, "all")
    return np.stack([r.sum(axis=1), (r * r).sum(axis=1)], axis=1)


def stats(xs, geom):
    """compute_log_mel_stats over the recordings: (mean, std, count), unbiased variance clamped at 1e-12."""
    count, s1, s2 = 0, 0.0, 0.0
    for x in xs:
        r = raw_log_mel(x, geom, "all")
        count += r.size
        s1 += r.sum()
        s2 += (r * r).sum()
    mean = s1 / count
    var = (s2 - count * mean * mean) / (count - 1) if count > 1 else 16.0
    return float(mean), float(np.sqrt(max(var, 1e-12))), int(count)
