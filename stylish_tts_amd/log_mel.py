"""Host side of the log-mel front end (csrc/log_mel.hip.h): geometry rules, frame-count policies and the mel filter table the kernel uses.

The transform is torchaudio.transforms.MelSpectrogram(n_mels, n_fft, win_length, hop_length, sample_rate) at its defaults: power 2, center=True
with reflect padding, periodic Hann, HTK scale, f_min 0, f_max sample_rate / 2, norm None.  Nothing else is built.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib

POLICIES = ("even", "drop_last", "all")
MAX_MELS = 256


def check_geometry(n_fft: int, win_length: int, hop_length: int, n_mels: int, sample_rate: int) -> None:
    """config.geometry's rules for n_fft / win_length, any hop >= 1, 1 <= n_mels <= 256.  ValueError naming the broken rule."""
    n_fft, win, hop, n_mels, sr = int(n_fft), int(win_length), int(hop_length), int(n_mels), int(sample_rate)
    if n_fft <= 0 or n_fft & (n_fft - 1):
        raise ValueError(f"n_fft {n_fft} is not a power of two")
    if not 256 <= n_fft <= 4096:
        raise ValueError(f"n_fft {n_fft} is outside [256, 4096]")
    if not 1 <= win <= n_fft:
        raise ValueError(f"win_length {win} is outside [1, n_fft = {n_fft}]")
    if hop < 1:
        raise ValueError(f"hop_length {hop} is not positive")
    if not 1 <= n_mels <= MAX_MELS:
        raise ValueError(f"n_mels {n_mels} is outside [1, {MAX_MELS}]")
    if sr < 2:
        raise ValueError(f"sample_rate {sr} is not positive")


def frames(samples: int, hop_length: int, policy: str = "even") -> int:
    """Frames of an utterance of ``samples`` samples: "even" = samples // hop + 1 rounded down to even (calculate_mel, train/stage_type.py:1027-1028),
    "drop_last" = samples // hop (preprocess, train/dataprep/align_text.py:116), "all" = samples // hop + 1 (torch.stft, center=True)."""
    if policy not in POLICIES:
        raise ValueError(f"frames must be one of {POLICIES}, got {policy!r}")
    n = int(samples) // int(hop_length) + 1
    return n - n % 2 if policy == "even" else n - 1 if policy == "drop_last" else n


def frame_counts(lengths: Sequence[int], n_fft: int, hop_length: int, policy: str = "even") -> List[int]:
    """Frame counts of a ragged batch; ValueError for an utterance torch.stft refuses (n_fft / 2 samples or fewer) or one left without a frame."""
    out = []
    for u, n in enumerate(lengths):
        n = int(n)
        if n <= n_fft // 2:
            raise ValueError(f"utterance {u} has {n} samples; the reflect padding needs more than n_fft / 2 = {n_fft // 2}")
        fr = frames(n, hop_length, policy)
        if fr < 1:
            raise ValueError(f"utterance {u}: {n} samples at hop {hop_length} leave no frame under the {policy!r} policy")
        out.append(fr)
    return out


def filter_table(n_fft: int, n_mels: int, sample_rate: int):
    """(weights [n_mels, n_fft / 2 + 1] float32, band [n_mels, 2] int32): the filters the kernel sums, from the library's own host-side builder
    (include/stylish_hip.h, stts_log_mel_filters; no GPU): torchaudio's melscale_fbanks (HTK, norm None, f_min 0, f_max sample_rate // 2) in float64,
    rounded once to fp32; band = the nonzero bins [first, one past the last) of every filter."""
    check_geometry(n_fft, n_fft, 1, n_mels, sample_rate)
    w = np.zeros((int(n_mels), int(n_fft) // 2 + 1), np.float32)
    band = np.zeros((int(n_mels), 2), np.int32)
    _lib.check(_lib.load().stts_log_mel_filters(int(n_fft), int(n_mels), int(sample_rate), band.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)))
    return w, band
