"""Float64 numpy restatement of the windowed-sinc resampler (csrc/resample.hip.h): torchaudio.transforms.Resample / functional.resample from its
published definition, by direct sums - no convolution call.  tests/golden/gen_golden_resample.py pins it against a restatement of torchaudio's own
code on F.conv1d run in float64 (tests/test_resample_cpu.py: to 1e-12 of the output scale); the GPU tests compare against it.  Also the recipes of the
test signals, shared with the generator."""
from __future__ import annotations

import math

import numpy as np

KAISER_BETA = 14.769656459379492

# name -> (orig_freq, new_freq, lowpass_filter_width, rolloff, method, beta): the cases of tests/test_hip_resample.py; the first two are the
# resamplers of the reference's AdaptiveHubert (24 kHz model) and RMVPE.infer_from_audio
CASES = {
    "r24_16_w6": (24000, 16000, 6, 0.99, "sinc_interp_hann", None),
    "r24_16_w128": (24000, 16000, 128, 0.99, "sinc_interp_hann", None),
    "r441_160": (44100, 16000, 6, 0.99, "sinc_interp_hann", None),
    "r441_160_w128": (44100, 16000, 128, 0.99, "sinc_interp_hann", None),  # 1155 taps: three staging passes of the kernel's tap loop
    "r160_441": (16000, 44100, 6, 0.99, "sinc_interp_hann", None),  # 441 phases: two phase chunks per input step
    "r16_24": (16000, 24000, 6, 0.99, "sinc_interp_hann", None),
    "r48_16": (48000, 16000, 6, 0.99, "sinc_interp_hann", None),
    "r8_16": (8000, 16000, 6, 0.99, "sinc_interp_hann", None),
    "kaiser": (24000, 16000, 6, 0.99, "sinc_interp_kaiser", None),
    "kaiser_b9": (44100, 16000, 6, 0.99, "sinc_interp_kaiser", 9.0),
    "rolloff09": (24000, 16000, 6, 0.9, "sinc_interp_hann", None),
}


def reduced(orig_freq: int, new_freq: int):
    d = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // d, int(new_freq) // d


def geometry(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99):
    """(o, n, width, taps)"""
    o, n = reduced(orig_freq, new_freq)
    width = math.ceil(lpw * o / (min(o, n) * rolloff))
    return o, n, width, 2 * width + o


def out_length(samples: int, orig_freq: int, new_freq: int) -> int:
    o, n = reduced(orig_freq, new_freq)
    return (n * int(samples) + o - 1) // o


def _i0(x: np.ndarray) -> np.ndarray:
    """I0 by its power series (all terms positive)."""
    x = np.asarray(x, np.float64)
    h = 0.25 * x * x
    term, total = np.ones_like(x), np.ones_like(x)
    for k in range(1, 1000):
        term = term * h / (k * k)
        total = total + term
        if (term <= total * 1e-18).all():
            break
    return total


def table(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99, method: str = "sinc_interp_hann", beta=None) -> np.ndarray:
    """Coefficients [n, taps] in float64: row p, column j standing for tap j - width."""
    o, n, width, taps = geometry(orig_freq, new_freq, lpw, rolloff)
    base = min(o, n) * rolloff
    j = np.arange(-width, width + o, dtype=np.float64)[None, :]
    p = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip((-p / n + j / o) * base, -lpw, lpw)
    if method == "sinc_interp_hann":
        win = np.cos(t * math.pi / lpw / 2.0) ** 2
    elif method == "sinc_interp_kaiser":
        b = KAISER_BETA if beta is None else float(beta)
        win = _i0(b * np.sqrt(np.maximum(0.0, 1.0 - (t / lpw) ** 2))) / _i0(np.float64(b))
    else:
        raise ValueError(method)
    a = t * math.pi
    safe = np.where(a == 0.0, 1.0, a)
    return np.where(a == 0.0, 1.0, np.sin(safe) / safe) * win * (base / o)


def resample(x: np.ndarray, orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99, method: str = "sinc_interp_hann", beta=None) -> np.ndarray:
    """One utterance [samples] -> [ceil(n samples / o)] in float64: output q n + p = sum_j table[p][j] x[q o - width + j], zeros outside x."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.size >= 1
    o, n, width, taps = geometry(orig_freq, new_freq, lpw, rolloff)
    if o == n:
        return x.copy()
    tab = table(orig_freq, new_freq, lpw, rolloff, method, beta)
    M = out_length(x.size, orig_freq, new_freq)
    Q = (M + n - 1) // n
    xp = np.zeros(width + (Q - 1) * o + taps + x.size)
    xp[width : width + x.size] = x
    out = np.zeros((Q, n))
    for jj in range(taps):  # the direct sum, tap by tap: out[q, p] += tab[p, jj] * x[q o - width + jj]
        out += xp[jj : jj + (Q - 1) * o + 1 : o][:, None] * tab[None, :, jj]
    return out.reshape(-1)[:M]


def signal(name: str, n: int, sample_rate: int) -> np.ndarray:
    """logmel64.signal: the vibrato harmonic tone under a slow envelope plus noise at 0.02 (fp32)."""
    import logmel64

    return logmel64.signal("resample." + name, n, sample_rate)


def lengths(orig_freq: int, new_freq: int, tile: int):
    """The test lengths at these rates: 1 sample; 5 (shorter than the width); o k - 1, o k, o k + 1; the input counts whose output counts are exactly
    ``tile`` and ``tile`` + 1; about 0.3 s."""
    o, n = reduced(orig_freq, new_freq)
    k = 37

    def samples_for(m):  # the smallest input count with at least m outputs (exactly m when o >= n; upsampling skips some counts)
        s = ((m - 1) * o) // n + 1
        assert out_length(s, o, n) >= m > out_length(s - 1, o, n), (s, m)
        return s

    return [1, 5, o * k - 1, o * k, o * k + 1, samples_for(tile), samples_for(tile + 1), int(round(0.3 * orig_freq))]


def signals(case: str, tile: int):
    """The case's recordings at ``lengths``: the fourth scaled by 1e-3, the second half of the last exactly zero."""
    orig = CASES[case][0]
    out = [signal(f"{case}.{i}", n, orig) for i, n in enumerate(lengths(orig, CASES[case][1], tile))]
    out[3] = (out[3].astype(np.float64) * 1e-3).astype(np.float32)
    out[-1][out[-1].size // 2 :] = 0.0
    return out
