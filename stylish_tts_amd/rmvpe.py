"""Shapes and host-side rules of the RMVPE pitch extractor (the reference's train/dataprep/rmvpe/: E2E0, mel2hidden, the log-mel front end):
the constructor arguments the engine reads, the padding rule, the BatchNorm fold and the sub-pixel repacking of the transposed convolutions
(float64, what csrc/rmvpe.hip.h does at finalize), and the default mel filter bank.  No GPU here.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Mapping, Optional

import numpy as np

# E2E0(4, 1, (2, 2)) (rmvpe/inference.py:15) with the class defaults en_de_layers = 5, inter_layers = 4, en_out_channels = 16
DIMS_DEFAULTS = {"n_blocks": 4, "inter_layers": 4, "en_out_channels": 16, "en_de_layers": 5, "kernel_size": (2, 2), "n_gru": 1, "n_mels": 128}
_FIXED = {"en_de_layers": 5, "kernel_size": (2, 2), "n_gru": 1, "n_mels": 128}
N_MELS, N_CLASS, GRU_HIDDEN = 128, 360, 256
SAMPLE_RATE, N_FFT, HOP, MEL_FMIN, MEL_FMAX = 16000, 1024, 160, 30.0, 8000.0
N_BINS = N_FFT // 2 + 1
CENTS_0 = 1997.3794084376191  # rmvpe/constants.py CONST
MIN_FRAMES = 17   # reflect padding to a multiple of 32 frames needs pad < frames
MIN_SAMPLES = N_FFT // 2 + 1  # reflect padding of the STFT needs pad = 512 < samples
MAX_BLOCKS, MAX_INTER, MAX_C0 = 8, 8, 64


class RmvpeDims(C.Structure):
    """stts_rmvpe_dims (include/stylish_hip.h)."""

    _fields_ = [(n, C.c_int32) for n in ("n_blocks", "inter_layers", "en_out_channels", "en_de_layers", "kernel_h", "kernel_w", "n_gru", "n_mels")]


def dims(config: Optional[Mapping[str, Any]] = None) -> dict:
    """E2E0's constructor arguments from ``config`` over the defaults, validated: ValueError naming the argument for a network the engine does not run."""
    d = dict(DIMS_DEFAULTS)
    for k, v in (config or {}).items():
        if k not in d:
            raise ValueError(f"rmvpe: unknown argument {k!r} (E2E0 takes {sorted(d)})")
        d[k] = tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else int(v)
    for k, want in _FIXED.items():
        if d[k] != want:
            raise ValueError(f"rmvpe: {k} = {d[k]!r} is not supported (the engine runs {k} = {want!r})")
    if not 1 <= d["n_blocks"] <= MAX_BLOCKS:
        raise ValueError(f"rmvpe: n_blocks = {d['n_blocks']} is outside [1, {MAX_BLOCKS}]")
    if not 1 <= d["inter_layers"] <= MAX_INTER:
        raise ValueError(f"rmvpe: inter_layers = {d['inter_layers']} is outside [1, {MAX_INTER}]")
    if not 2 <= d["en_out_channels"] <= MAX_C0:
        raise ValueError(f"rmvpe: en_out_channels = {d['en_out_channels']} is outside [2, {MAX_C0}]")
    return d


def dims_struct(d: Mapping[str, Any]) -> RmvpeDims:
    return RmvpeDims(d["n_blocks"], d["inter_layers"], d["en_out_channels"], d["en_de_layers"], d["kernel_size"][0], d["kernel_size"][1], d["n_gru"], d["n_mels"])


def padded_frames(n: int) -> int:
    """mel2hidden's length: the next multiple of 32 (rmvpe/inference.py:28-35); ValueError where the reference's reflect F.pad raises."""
    n = int(n)
    if n < MIN_FRAMES:
        raise ValueError(f"RMVPE needs at least {MIN_FRAMES} mel frames per utterance (reflect padding to a multiple of 32), got {n}")
    return 32 * ((n - 1) // 32 + 1)


def mel_frames(samples: int) -> int:
    """Frames of the centred STFT (hop 160): samples // 160 + 1; ValueError at 512 samples or fewer (the reflect padding)."""
    samples = int(samples)
    if samples < MIN_SAMPLES:
        raise ValueError(f"RMVPE's log-mel needs more than {N_FFT // 2} samples per utterance (reflect padding), got {samples}")
    return samples // HOP + 1


# ------------------------------------------------------------------------------------------------ Viterbi decoding (rmvpe/utils.py:134-150)
VITERBI_BAND = 29          # max(30 - |i - j|, 0) is nonzero for |i - j| <= 29
VITERBI_EPS = 2.0 ** -126  # the smallest normal fp32: what the reference's sequence decoder adds inside every logarithm of an fp32 input
_VITERBI_TABLES = None


def viterbi_transition() -> np.ndarray:
    """[360, 360] float64: lt[i][j] = log(A[i][j] + eps), A = w / w.sum(axis=1) with w[i][j] = max(30 - |i - j|, 0) (to_viterbi_f0's transition)."""
    idx = np.arange(N_CLASS)
    w = np.maximum(30 - np.abs(idx[:, None] - idx[None, :]), 0).astype(np.float64)
    return np.log(w / w.sum(axis=1, keepdims=True) + VITERBI_EPS)


def viterbi_tables():
    """(lt_band [360, 59] float64, lt_out, eps): the transition log-probabilities in the form stts_rmvpe_viterbi reads.  lt_band[j][k] =
    lt[j - 29 + k][j], -inf where that predecessor does not exist; lt_out = log(eps), the value of every lt[i][j] outside the band.  Built once."""
    global _VITERBI_TABLES
    if _VITERBI_TABLES is None:
        lt = viterbi_transition()
        band = np.full((N_CLASS, 2 * VITERBI_BAND + 1), -np.inf, np.float64)
        for j in range(N_CLASS):
            lo, hi = max(0, j - VITERBI_BAND), min(N_CLASS, j + VITERBI_BAND + 1)
            band[j, lo - (j - VITERBI_BAND) : hi - (j - VITERBI_BAND)] = lt[lo:hi, j]
        band.setflags(write=False)
        out = float(lt[0, N_CLASS - 1])  # read from the matrix itself: the same bits as every other out-of-band entry
        assert (lt[np.abs(np.arange(N_CLASS)[:, None] - np.arange(N_CLASS)[None, :]) > VITERBI_BAND] == out).all()
        _VITERBI_TABLES = (band, out, VITERBI_EPS)
    return _VITERBI_TABLES


# ------------------------------------------------------------------------------------------------ mel filter bank
def _hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def _mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def default_mel_basis() -> np.ndarray:
    """[128, 513] fp32: triangular filters with HTK-scale centres between 30 Hz and 8 kHz over the 513 bins of a 1024-point transform at 16 kHz,
    each scaled by 2 / (its band's width in Hz) (Slaney's area normalisation) - the construction the reference asks its audio library for
    (rmvpe/spec.py:22-29).  Built in float64 and rounded once.  Its values are NOT pinned against that library."""
    freqs = np.linspace(0.0, SAMPLE_RATE / 2.0, N_BINS)
    pts = _mel_to_hz_htk(np.linspace(_hz_to_mel_htk(MEL_FMIN), _hz_to_mel_htk(MEL_FMAX), N_MELS + 2))
    fdiff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    w = np.zeros((N_MELS, N_BINS), np.float64)
    for i in range(N_MELS):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return w.astype(np.float32)


def basis_band(basis: np.ndarray) -> np.ndarray:
    """[128, 2] int32: first and one-past-last nonzero bin of every filter (an all-zero filter: 0, 0)."""
    b = np.asarray(basis)
    if b.shape != (N_MELS, N_BINS):
        raise ValueError(f"mel_basis must be [{N_MELS}, {N_BINS}], got {tuple(b.shape)}")
    out = np.zeros((N_MELS, 2), np.int32)
    for m in range(N_MELS):
        nz = np.nonzero(b[m])[0]
        if nz.size:
            out[m] = (nz[0], nz[-1] + 1)
    return out


# ------------------------------------------------------------------------------------------------ folds (float64; csrc/rmvpe.hip.h, finalize_rmvpe)
def fold_conv_bn(w, gamma, beta, mean, var, eps: float = 1e-5):
    """Conv2d without bias followed by BatchNorm2d in eval mode as one conv: (w * scale[:, None, None, None], beta - mean * scale), float64."""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return np.asarray(w, np.float64) * scale[:, None, None, None], np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


def _axis_taps(parity: int):
    """ConvTranspose(3, stride 2, padding 1, output_padding 1) along one axis: out[2 j] = x[j] w[1]; out[2 j + 1] = x[j] w[2] + x[j + 1] w[0]."""
    return [(0, 1)] if parity == 0 else [(0, 2), (1, 0)]


def subpixel_weights(w, scale=None):
    """The four sub-pixel convolutions of ConvTranspose2d(3 x 3, stride 2, padding 1, output_padding 1) with weight w [cin, cout, 3, 3]:
    {(pt, pf): (offsets [(dt, df)], weights [ntap, cin, cout])}, out[2 t + pt, 2 f + pf] = sum_tap x[t + dt, f + df] @ weights[tap] (x = 0 past
    the end).  ``scale`` [cout] (a folded BatchNorm) multiplies the output channels.  float64."""
    w = np.asarray(w, np.float64)
    if scale is not None:
        w = w * np.asarray(scale, np.float64)[None, :, None, None]
    out = {}
    for pt in (0, 1):
        for pf in (0, 1):
            offs, ws = [], []
            for dt, kt in _axis_taps(pt):
                for df, kf in _axis_taps(pf):
                    offs.append((dt, df))
                    ws.append(w[:, :, kt, kf])
            out[(pt, pf)] = (offs, np.stack(ws))
    return out


def interp_linear_index(n_in: int, n_out: int):
    """F.interpolate(mode="linear", align_corners=True): (i0, i1, lambda) in float64 for every output position."""
    pos = np.arange(n_out, dtype=np.float64) * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros(n_out)
    i0 = np.minimum(pos.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), pos - i0
