"""Host side of the validation scores (csrc/val_scores.hip.h): the reference's resolutions, the geometry and length rules, the buffer sizes.

MultiSpectrogram (train/multi_spectrogram.py) -> MultiResolutionSTFTLoss "mel" (train/losses.py:14-35), MagPhaseLoss "mag" / "phase"
(losses.py:38-154), smooth_l1_loss "pitch" / "energy": what every validate_* of the reference logs (train/stage_type.py).  No GPU is needed here.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib, log_mel

N_MELS = 128
MASK = 1e-3


class Resolution:
    """train/multi_spectrogram.py:6-10."""

    def __init__(self, *, fft, hop, window):
        self.fft = fft
        self.hop = hop
        self.window = window


resolutions = [Resolution(fft=512, hop=50, window=240), Resolution(fft=1024, hop=120, window=600), Resolution(fft=2048, hop=240, window=1200)]
multi_spectrogram_count = len(resolutions)


def as_tuple(item) -> Tuple[int, int, int]:
    """(fft, hop, window) of a Resolution or of a 3-tuple in that order."""
    if hasattr(item, "fft"):
        return int(item.fft), int(item.hop), int(item.window)
    fft, hop, window = item
    return int(fft), int(hop), int(window)


def check_geometry(n_fft: int, win_length: int, hop_length: int, n_mels: int = 1, sample_rate: int = 2) -> None:
    """log_mel.check_geometry's rules; ValueError naming the broken one."""
    log_mel.check_geometry(n_fft, win_length, hop_length, n_mels, sample_rate)


def frame_counts(lengths: Sequence[int], n_fft: int, hop_length: int) -> List[int]:
    """samples // hop + 1 frames of every utterance; ValueError naming an utterance of n_fft / 2 samples or fewer."""
    return log_mel.frame_counts(lengths, n_fft, hop_length, "all")


def check_pair(target_lengths: Sequence[int], pred_lengths: Sequence[int]) -> None:
    """The target and the prediction of an utterance must have equal sample counts; ValueError naming the utterance."""
    if len(target_lengths) != len(pred_lengths):
        raise ValueError(f"{len(target_lengths)} target utterances, {len(pred_lengths)} predictions")
    for u, (a, b) in enumerate(zip(target_lengths, pred_lengths)):
        if int(a) != int(b):
            raise ValueError(f"utterance {u}: the target has {int(a)} samples, the prediction {int(b)}")


def check_rows(lengths: Sequence[int], rows: Sequence[int], hop_length: int) -> None:
    """MagPhaseLoss: the prediction rows of an utterance must equal samples // hop + 1; ValueError naming the utterance."""
    if len(lengths) != len(rows):
        raise ValueError(f"{len(lengths)} recordings, {len(rows)} predictions")
    for u, (n, r) in enumerate(zip(lengths, rows)):
        if int(r) != int(n) // int(hop_length) + 1:
            raise ValueError(f"utterance {u} has {int(r)} prediction rows; its {int(n)} samples at hop {int(hop_length)} make {int(n) // int(hop_length) + 1} frames")


def sizes(lengths: Sequence[int], n_fft: int, hop_length: int) -> Dict[str, int]:
    """What the Python side allocates for a packed batch: rows, doubles of the mel partials, of the mag/phase partials and of its scratch."""
    rows = sum(frame_counts(lengths, n_fft, hop_length))
    return dict(rows=rows, mel_partials=2 * rows, magphase_partials=4 * rows, magphase_scratch=rows * (int(n_fft) // 2 + 1))


def lib_sizes(lengths: Sequence[int], n_fft: int, hop_length: int) -> Dict[str, int]:
    """The same from the library's host-only helper (include/stylish_hip.h, stts_val_sizes); ValueError with its message."""
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum([int(n) for n in lengths])
    out = np.zeros(4, np.int64)
    lib = _lib.load()
    if lib.stts_val_sizes(len(lengths), off.ctypes.data_as(C.c_void_p), int(n_fft), int(hop_length), out.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError((lib.stts_last_error() or b"?").decode("utf-8", "replace"))
    return dict(zip(("rows", "mel_partials", "magphase_partials", "magphase_scratch"), (int(v) for v in out)))


def phase_weights(n_bins: int) -> np.ndarray:
    """w_k = base^k, base = exp(ln 2.5 / (n_bins // 2)) (differential_phase_loss, losses.py:43-48), float64."""
    base = math.exp(math.log(2.5) / (int(n_bins) // 2))
    return np.power(base, np.arange(int(n_bins), dtype=np.float64))
