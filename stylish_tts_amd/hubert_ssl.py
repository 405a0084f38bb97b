"""Shapes and host-side rules of the HuBERT content encoder (the reference's AdaptiveHubert, train/models/ssl.py:16-31): the
``transformers`` HubertConfig fields the engine reads, the frame count of the conv feature extractor, F.interpolate's nearest index
rule and the weight-norm fold of the positional conv.  No GPU and no ``transformers`` import here; the engine side is csrc/ssl.hip.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Mapping, Optional

import numpy as np

# HubertConfig() defaults = HuBERT-base (model.yml:68-71, hubert.model "dr87/spinv2_rvc", hidden_dim 768)
ARCH_DEFAULTS = {
    "hidden_size": 768,
    "num_hidden_layers": 12,
    "num_attention_heads": 12,
    "intermediate_size": 3072,
    "conv_dim": (512, 512, 512, 512, 512, 512, 512),
    "conv_kernel": (10, 3, 3, 3, 3, 2, 2),
    "conv_stride": (5, 2, 2, 2, 2, 2, 2),
    "conv_bias": False,
    "feat_extract_norm": "group",
    "feat_extract_activation": "gelu",
    "hidden_act": "gelu",
    "do_stable_layer_norm": False,
    "num_conv_pos_embeddings": 128,
    "num_conv_pos_embedding_groups": 16,
    "layer_norm_eps": 1e-5,
    "classifier_proj_size": 256,
}
# the one graph the engine runs: any other value of these fields is a different network
_FIXED = {"feat_extract_norm": "group", "do_stable_layer_norm": False, "conv_bias": False, "feat_extract_activation": "gelu", "hidden_act": "gelu"}
MAX_CONV_LAYERS = 8
HEAD_SIZES = (16, 32, 40, 64, 96, 128, 160)
DEFAULT_SR = 16000


class SslDims(C.Structure):
    """stts_ssl_dims (include/stylish_hip.h)."""

    _fields_ = [(n, C.c_int32) for n in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "num_feat_extract_layers")] + [
        ("conv_dim", C.c_int32 * 8), ("conv_kernel", C.c_int32 * 8), ("conv_stride", C.c_int32 * 8),
        ("num_conv_pos_embeddings", C.c_int32), ("num_conv_pos_embedding_groups", C.c_int32), ("layer_norm_eps", C.c_float)]


def arch(config: Optional[Mapping[str, Any]] = None) -> dict:
    """The HubertConfig fields of ``config`` (a mapping: a model config's ``hubert.arch`` section or a checkpoint's config.json) over the
    base defaults, validated.  ValueError naming the field for anything the engine would have to run as a different graph."""
    a = dict(ARCH_DEFAULTS)
    for k, v in (config or {}).items():
        if k in a:
            a[k] = tuple(v) if isinstance(v, (list, tuple)) else v
    for k, want in _FIXED.items():
        if a[k] != want:
            raise ValueError(f"hubert.arch.{k} = {a[k]!r} is not supported (the engine runs {k} = {want!r})")
    n = len(a["conv_dim"])
    if not (len(a["conv_kernel"]) == len(a["conv_stride"]) == n) or not 1 <= n <= MAX_CONV_LAYERS:
        raise ValueError(f"hubert.arch.conv_dim / conv_kernel / conv_stride must be lists of one length in [1, {MAX_CONV_LAYERS}]")
    for i in range(n):
        if a["conv_dim"][i] <= 0 or a["conv_dim"][i] % 32 or a["conv_dim"][i] > 2048:
            raise ValueError(f"hubert.arch.conv_dim[{i}] = {a['conv_dim'][i]} must be a multiple of 32, at most 2048")
        if not 1 <= a["conv_stride"][i] <= a["conv_kernel"][i] <= 16:
            raise ValueError(f"hubert.arch.conv_kernel[{i}] = {a['conv_kernel'][i]} / conv_stride[{i}] = {a['conv_stride'][i]}: need 1 <= stride <= kernel <= 16")
    if a["conv_kernel"][0] not in (3, 5, 10):
        raise ValueError(f"hubert.arch.conv_kernel[0] = {a['conv_kernel'][0]} is not supported (3, 5 or 10)")
    h, heads = int(a["hidden_size"]), int(a["num_attention_heads"])
    if h <= 0 or h % 32 or h > 2048:
        raise ValueError(f"hubert.arch.hidden_size = {h} must be a multiple of 32, at most 2048")
    if heads <= 0 or h % heads or h // heads not in HEAD_SIZES:
        raise ValueError(f"hubert.arch.num_attention_heads = {heads}: hidden_size / heads must be one of {HEAD_SIZES}")
    if a["intermediate_size"] <= 0 or a["intermediate_size"] % 32:
        raise ValueError(f"hubert.arch.intermediate_size = {a['intermediate_size']} must be a multiple of 32")
    if not 1 <= a["num_hidden_layers"] <= 48:
        raise ValueError(f"hubert.arch.num_hidden_layers = {a['num_hidden_layers']} is outside [1, 48]")
    g = int(a["num_conv_pos_embedding_groups"])
    if g <= 0 or h % g or h // g not in (16, 32, 48, 64):
        raise ValueError(f"hubert.arch.num_conv_pos_embedding_groups = {g}: hidden_size / groups must be 16, 32, 48 or 64")
    if not 1 <= a["num_conv_pos_embeddings"] <= 256:
        raise ValueError(f"hubert.arch.num_conv_pos_embeddings = {a['num_conv_pos_embeddings']} is outside [1, 256]")
    return a


def arch_from_model_config(cfg) -> dict:
    """``hubert.arch`` of a model config (optional; base values when absent); arch.hidden_size must equal hubert.hidden_dim."""
    from .config import hubert_dims

    hd = hubert_dims(cfg)[0]
    node = cfg.get("hubert") or {}
    given = dict(node.get("arch") or {})
    if "hidden_size" in given and int(given["hidden_size"]) != hd:
        raise ValueError(f"hubert.arch.hidden_size = {given['hidden_size']} does not equal hubert.hidden_dim = {hd}")
    a = arch(given)
    if a["hidden_size"] != hd:
        raise ValueError(f"hubert.arch.hidden_size = {a['hidden_size']} does not equal hubert.hidden_dim = {hd}")
    return a


def dims_struct(a: Mapping[str, Any]) -> SslDims:
    d = SslDims()
    d.hidden_size, d.num_hidden_layers, d.num_attention_heads = int(a["hidden_size"]), int(a["num_hidden_layers"]), int(a["num_attention_heads"])
    d.intermediate_size, d.num_feat_extract_layers = int(a["intermediate_size"]), len(a["conv_dim"])
    for i in range(len(a["conv_dim"])):
        d.conv_dim[i], d.conv_kernel[i], d.conv_stride[i] = int(a["conv_dim"][i]), int(a["conv_kernel"][i]), int(a["conv_stride"][i])
    d.num_conv_pos_embeddings, d.num_conv_pos_embedding_groups = int(a["num_conv_pos_embeddings"]), int(a["num_conv_pos_embedding_groups"])
    d.layer_norm_eps = float(a["layer_norm_eps"])
    return d


def min_samples(a: Optional[Mapping[str, Any]] = None) -> int:
    """Receptive field of the feature extractor: the shortest utterance with one frame (400 for HuBERT-base)."""
    a = a or ARCH_DEFAULTS
    n = 1
    for k, s in zip(reversed(a["conv_kernel"]), reversed(a["conv_stride"])):
        n = (n - 1) * s + k
    return n


def frames(samples: int, a: Optional[Mapping[str, Any]] = None) -> int:
    """Frames of the feature extractor, L -> floor((L - k) / s) + 1 per layer.  ValueError below the receptive field, where the reference
    raises too."""
    a = a or ARCH_DEFAULTS
    n = int(samples)
    for k, s in zip(a["conv_kernel"], a["conv_stride"]):
        if n < k:
            raise ValueError(f"an utterance of {int(samples)} samples is shorter than the feature extractor's receptive field ({min_samples(a)} samples)")
        n = (n - k) // s + 1
    return n


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source frame of every output frame of F.interpolate(mode="nearest", size=n_out): floor(j * float32(n_in / n_out)) in fp32, clamped."""
    scale = np.float32(n_in) / np.float32(n_out)
    j = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(j * scale).astype(np.int64), n_in - 1)


def fold_pos_conv_weight(g: np.ndarray, v: np.ndarray) -> np.ndarray:
    """weight_norm(dim=2) of the positional conv: w[:, :, t] = g[t] * v[:, :, t] / ||v[:, :, t]||, in double, rounded to fp32 once."""
    v64 = np.asarray(v, np.float64)
    norm = np.sqrt((v64 * v64).sum(axis=(0, 1), keepdims=True))
    return (v64 * (np.asarray(g, np.float64).reshape(1, 1, -1) / norm)).astype(np.float32)
