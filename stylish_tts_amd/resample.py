"""Host side of the windowed-sinc resampler (csrc/resample.hip.h): the reduced rates, the filter width, output lengths and the interface limits.

The operation is torchaudio.transforms.Resample / functional.resample from its published definition; the engine's target is its float64 result (the
coefficients stay fp64 and unrounded on the device).  ``librosa.resample`` (soxr / kaiser_best) is a different filter and is not built.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence, Tuple

from . import _lib

METHODS = {"sinc_interp_hann": 0, "sinc_interp_kaiser": 1}
KAISER_BETA = 14.769656459379492  # torchaudio's default
MAX_FREQ = 1024  # o, n after the gcd reduction
MAX_TABLE = 1 << 20  # phases * taps
MAX_WIDTH = 256  # lowpass_filter_width
MAX_BETA = 512.0


def reduced(orig_freq: int, new_freq: int) -> Tuple[int, int]:
    """(o, n): the two rates divided by their gcd."""
    o, n = int(orig_freq), int(new_freq)
    if o != orig_freq or n != new_freq or o < 1 or n < 1:
        raise ValueError(f"orig_freq {orig_freq} / new_freq {new_freq} must be positive integers")
    d = math.gcd(o, n)
    return o // d, n // d


def width(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[int, int]:
    """(width, taps): width = ceil(lowpass_filter_width * o / (min(o, n) * rolloff)) samples on either side, taps = 2 width + o per phase."""
    o, n = reduced(orig_freq, new_freq)
    w = math.ceil(int(lowpass_filter_width) * o / (min(o, n) * float(rolloff)))
    return w, 2 * w + o


def out_length(samples: int, orig_freq: int, new_freq: int) -> int:
    """ceil(n * samples / o), in integers."""
    o, n = reduced(orig_freq, new_freq)
    return (n * int(samples) + o - 1) // o


def out_lengths(lengths: Sequence[int], orig_freq: int, new_freq: int) -> List[int]:
    """Output sample counts of a ragged batch; ValueError for an utterance without a sample."""
    out = []
    for u, s in enumerate(lengths):
        if int(s) < 1:
            raise ValueError(f"utterance {u} has {int(s)} samples; the resampler needs at least 1")
        out.append(out_length(s, orig_freq, new_freq))
    return out


def method_id(resampling_method: str) -> int:
    if resampling_method not in METHODS:
        raise ValueError(f"resampling_method must be one of {sorted(METHODS)}, got {resampling_method!r}")
    return METHODS[resampling_method]


def check(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, resampling_method: str = "sinc_interp_hann", beta=None):
    """The interface limits; ValueError naming the offending number.  -> (o, n, width, taps, method id, beta)."""
    o, n = reduced(orig_freq, new_freq)
    lpw, ro = int(lowpass_filter_width), float(rolloff)
    if lpw != lowpass_filter_width or not 1 <= lpw <= MAX_WIDTH:
        raise ValueError(f"lowpass_filter_width {lowpass_filter_width} is outside [1, {MAX_WIDTH}]")
    if not 0.0 < ro <= 1.0:
        raise ValueError(f"rolloff {rolloff} is outside (0, 1]")
    if o > MAX_FREQ:
        raise ValueError(f"orig_freq {orig_freq} reduces to {o}, above {MAX_FREQ}")
    if n > MAX_FREQ:
        raise ValueError(f"new_freq {new_freq} reduces to {n}, above {MAX_FREQ}")
    w, taps = width(o, n, lpw, ro)
    if n * taps > MAX_TABLE:
        raise ValueError(f"{n} phases x {taps} taps = {n * taps} coefficients are above {MAX_TABLE}")
    m = method_id(resampling_method)
    b = KAISER_BETA if beta is None else float(beta)
    if m == 1 and not 0.0 <= b <= MAX_BETA:  # also refuses a NaN
        raise ValueError(f"beta {beta} is outside [0, {MAX_BETA}]")
    return o, n, w, taps, m, b


def geometry(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[int, int, int, int]:
    """(o, n, width, taps) from the library's own host code (include/stylish_hip.h, stts_resample_geometry; no GPU); RuntimeError with the library's
    message outside the limits."""
    v = [C.c_int(0) for _ in range(4)]
    _lib.check(_lib.load().stts_resample_geometry(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def tile(orig_freq: int, new_freq: int) -> int:
    """Outputs per block of the resampling kernel at these rates (include/stylish_hip.h, stts_resample_tile)."""
    return int(_lib.load().stts_resample_tile(int(orig_freq), int(new_freq)))
