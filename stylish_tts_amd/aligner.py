"""Shapes and host-side rules of the text aligner (the reference's train/models/text_aligner.py: tdnn_blstm_ctc_model) and of the CTC forced
alignment behind it (train/dataprep/align_text.py: torch_align): the layer spec the engine runs, the dims struct of the C-ABI, the BatchNorm fold
(float64, what csrc/aligner.hip.h does at finalize) and the feasibility rule of an alignment.  No GPU here."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Sequence

import numpy as np

HIDDEN = 640
BN_EPS = 1e-5
MAX_TDNN, MAX_FFN, MAX_TOKENS = 4, 8, 510
# tdnn_blstm_ctc_model_base (text_aligner.py:33-45)
BASE_SPEC = (("tdnn", 5, 1, 1), ("tdnn", 3, 1, 1), ("tdnn", 3, 1, 1), ("ffn", 5))


class AlignerDims(C.Structure):
    """stts_aligner_dims (include/stylish_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "hidden", "classes", "n_tdnn", "ffn_layers")] + [("tdnn_kernel", C.c_int32 * 4)]


def dims(n_mels: int = 80, num_symbols: int = 178, hidden_dim: int = HIDDEN, tdnn_blstm_spec: Sequence = BASE_SPEC) -> Dict[str, Any]:
    """The constructor arguments of tdnn_blstm_ctc_model as the engine's dims; ValueError for a spec the engine (or the reference) has no form for:
    the engine runs 1-4 ("tdnn", k, 1, 1) layers with odd k <= 7 followed by exactly one ("ffn", n)."""
    spec = [tuple(s) if isinstance(s, (tuple, list)) else (s,) for s in tdnn_blstm_spec]
    kernels, ffn = [], None
    for i, s in enumerate(spec):
        kind = s[0] if s else None
        if kind == "blstm":
            raise ValueError("text aligner: tdnn_blstm_spec entry 'blstm' is not supported (the reference's Blstm_with_skip does not exist, so no checkpoint can have one)")
        if kind == "tdnn":
            if ffn is not None:
                raise ValueError("text aligner: a 'tdnn' layer after the 'ffn' is not supported (the engine runs tdnn layers, then one ffn)")
            if len(s) < 3:
                raise ValueError(f"text aligner: tdnn spec {s!r} must be ('tdnn', kernel_size, stride[, dilation])")
            k, stride, dil = int(s[1]), int(s[2]), int(s[3]) if len(s) >= 4 else 1
            if stride != 1 or dil != 1:
                raise ValueError(f"text aligner: tdnn stride = {stride}, dilation = {dil} is not supported (the engine runs stride 1, dilation 1)")
            if k % 2 != 1 or not 1 <= k <= 7:
                raise ValueError(f"text aligner: tdnn kernel_size = {k} is not supported (odd, at most 7)")
            kernels.append(k)
        elif kind == "ffn":
            if ffn is not None or i != len(spec) - 1:
                raise ValueError("text aligner: exactly one 'ffn' entry, the last one, is supported")
            if len(s) < 2 or not 1 <= int(s[1]) <= MAX_FFN:
                raise ValueError(f"text aligner: ffn spec {s!r} must be ('ffn', layers) with 1 to {MAX_FFN} layers")
            ffn = int(s[1])
        else:
            raise ValueError(f"text aligner: unknown tdnn_blstm_spec entry {s!r}")
    if not 1 <= len(kernels) <= MAX_TDNN or ffn is None:
        raise ValueError(f"text aligner: the spec needs 1 to {MAX_TDNN} 'tdnn' layers and one 'ffn' (got {len(kernels)} and {0 if ffn is None else 1})")
    if hidden_dim % 32 or not 32 <= hidden_dim <= 2048:
        raise ValueError(f"text aligner: hidden_dim = {hidden_dim} must be a multiple of 32, at most 2048")
    if not 1 <= int(num_symbols) <= 255:
        raise ValueError(f"text aligner: num_symbols = {num_symbols} outside [1, 255]")
    return dict(n_mels=int(n_mels), num_symbols=int(num_symbols), hidden=int(hidden_dim), classes=int(num_symbols) + 1, tdnn_kernel=kernels, ffn_layers=ffn)


def dims_struct(d) -> AlignerDims:
    k = list(d["tdnn_kernel"]) + [0] * (4 - len(d["tdnn_kernel"]))
    return AlignerDims(d["n_mels"], d["hidden"], d["classes"], len(d["tdnn_kernel"]), d["ffn_layers"], (C.c_int32 * 4)(*k))


def fold_batchnorm(running_mean, running_var):
    """BatchNorm1d(affine=False) in eval mode as y = x * scale + shift, formed in float64 and rounded once (csrc/aligner.hip.h, finalize_aligner)."""
    m, v = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    sc = 1.0 / np.sqrt(v + BN_EPS)
    return sc.astype(np.float32), (-m * sc).astype(np.float32)


def min_frames(tokens: Sequence[int]) -> int:
    """Frames a CTC path over ``tokens`` needs: one per token plus one blank between every adjacent equal pair."""
    t = [int(x) for x in tokens]
    return len(t) + sum(1 for a, b in zip(t, t[1:]) if a == b)


def check_alignable(frames: int, tokens: Sequence[int], what: str = "utterance") -> None:
    """ValueError where the reference's forced alignment has no path (or the engine no room for the states)."""
    P = len(tokens)
    if not 1 <= P <= MAX_TOKENS:
        raise ValueError(f"{what}: {P} tokens, the alignment takes 1 to {MAX_TOKENS}")
    need = min_frames(tokens)
    if frames < need:
        raise ValueError(f"{what}: {frames} frames cannot hold {P} tokens (one frame per token plus one per adjacent equal pair = {need})")
