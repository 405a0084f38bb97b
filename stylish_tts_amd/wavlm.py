"""Shapes and host-side rules of WavLM, the network of the reference's perceptual distance (WavLMLoss, train/losses.py:408-426; model.yml
``slm: model: microsoft/wavlm-base-plus``, ``sr: 16000``; logged as "slm"): the ``transformers`` WavLMConfig fields the engine reads, the
relative-position bucket rule and the score's normalisation.  The feature extractor, the projection, the positional conv and the layer body
are HuBERT's (hubert_ssl.py); the gated relative-position bias is what differs.  No GPU and no ``transformers`` import here; the engine side
is csrc/wavlm.hip.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Mapping, Optional

import numpy as np

from . import hubert_ssl

# WavLMConfig() defaults = WavLM-base / base-plus
ARCH_DEFAULTS = {k: v for k, v in hubert_ssl.ARCH_DEFAULTS.items() if k != "classifier_proj_size"}
ARCH_DEFAULTS.update({"num_buckets": 320, "max_bucket_distance": 800})
HEAD_SIZE = 64  # gru_rel_pos_linear is a Linear(head size, 8); the gated attention is built for heads of 64
MAX_BUCKET_DISTANCE = 2048  # a head's bias-by-distance table (2 D + 1 floats) sits in LDS next to the attention's stages
DEFAULT_SR = 16000
# graph switches of WavLMConfig the engine does not run (their default is the supported value)
_UNSUPPORTED = {"add_adapter": False, "conv_bias": False}


class WavlmDims(C.Structure):
    """stts_wavlm_dims (include/stylish_hip.h)."""

    _fields_ = [("ssl", hubert_ssl.SslDims), ("num_buckets", C.c_int32), ("max_bucket_distance", C.c_int32)]


def arch(config: Optional[Mapping[str, Any]] = None) -> dict:
    """The WavLMConfig fields of ``config`` (a mapping: a checkpoint's config.json or a model config's ``slm.arch`` section) over the base
    defaults, validated.  ValueError naming the field for anything the engine would have to run as a different graph."""
    cfg = dict(config or {})
    for k, want in _UNSUPPORTED.items():
        if k in cfg and cfg[k] != want:
            raise ValueError(f"wavlm.arch.{k} = {cfg[k]!r} is not supported (the engine runs {k} = {want!r})")
    try:
        a = hubert_ssl.arch({k: v for k, v in cfg.items() if k in hubert_ssl.ARCH_DEFAULTS})
    except ValueError as e:
        raise ValueError(str(e).replace("hubert.arch.", "wavlm.arch.")) from None
    a.pop("classifier_proj_size", None)
    nb, md = int(cfg.get("num_buckets", 320)), int(cfg.get("max_bucket_distance", 800))
    if a["hidden_size"] // a["num_attention_heads"] != HEAD_SIZE:
        raise ValueError(f"wavlm.arch.num_attention_heads = {a['num_attention_heads']}: hidden_size / heads must be {HEAD_SIZE}")
    if nb < 4 or nb % 4:
        raise ValueError(f"wavlm.arch.num_buckets = {nb} must be a positive multiple of 4")
    if not nb // 4 < md <= MAX_BUCKET_DISTANCE:
        raise ValueError(f"wavlm.arch.max_bucket_distance = {md} is outside (num_buckets / 4, {MAX_BUCKET_DISTANCE}]")
    a["num_buckets"], a["max_bucket_distance"] = nb, md
    return a


def arch_from_model_config(cfg) -> tuple:
    """(slm.sr, arch) of a model config: ``slm.sr`` (16000 when absent) and the optional ``slm.arch`` (WavLMConfig fields over the base values)."""
    node = (cfg.get("slm") if hasattr(cfg, "get") else None) or {}
    return int(node.get("sr", DEFAULT_SR)), arch(dict(node.get("arch") or {}))


def dims_struct(a: Mapping[str, Any]) -> WavlmDims:
    d = WavlmDims()
    d.ssl = hubert_ssl.dims_struct(a)
    d.num_buckets, d.max_bucket_distance = int(a["num_buckets"]), int(a["max_bucket_distance"])
    return d


def frames(samples: int, a: Optional[Mapping[str, Any]] = None) -> int:
    return hubert_ssl.frames(samples, a or ARCH_DEFAULTS)


def min_samples(a: Optional[Mapping[str, Any]] = None) -> int:
    return hubert_ssl.min_samples(a or ARCH_DEFAULTS)


def bucket(d, num_buckets: int = 320, max_bucket_distance: int = 800) -> np.ndarray:
    """WavLMAttention._relative_positions_bucket of distances ``d`` = key - query: bidirectional (the upper half of the buckets for d > 0), exact
    below num_buckets / 4, logarithmic above, saturating.  The logarithmic part in double, as the engine builds its table (csrc/wavlm.hip.h)."""
    d = np.asarray(d, np.int64)
    nb = num_buckets // 2
    me = nb // 2
    a = np.abs(d)
    big = me + np.log(np.maximum(a, 1) / me) / math.log(max_bucket_distance / me) * (nb - me)
    big = np.minimum(big.astype(np.int64), nb - 1)
    return np.where(d > 0, nb, 0) + np.where(a < me, a, big)


def score(sums, frame_counts, hidden: int) -> tuple:
    """(slm, [per-utterance slm]) from the per-state sums [B][states] of |difference| and the frame counts [B]: the mean over states, real frames
    and channels - torch.nn.functional.l1_loss of the stacked hidden states for a batch without padding."""
    sums = [[float(v) for v in row] for row in sums]
    fr = [int(n) for n in frame_counts]
    ns = len(sums[0])
    utt = [math.fsum(row) / (ns * n * hidden) for row, n in zip(sums, fr)]
    return math.fsum(math.fsum(row) for row in sums) / (ns * sum(fr) * hidden), utt
