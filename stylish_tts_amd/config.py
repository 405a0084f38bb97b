"""Model-shape contract: the same ``model.yml`` keys the reference validates.

The reference shapes its whole inference graph from ``ModelConfig``
(``/root/reference/src/stylish_tts/lib/config_loader.py:369-414``) loaded by
``load_model_config_yaml`` (``config_loader.py:442-455``) from
``train/config/model.yml``.  This module parses that YAML into plain
attribute-access records; only the keys the inference hot path reads are
required, every other key of the reference schema is carried through
untouched so a reference ``model.yml`` loads unchanged.
"""
from __future__ import annotations

import io
import json
from typing import Any, Mapping

import numpy as np
import yaml


class Record(dict):
    """dict with attribute access (nested)."""

    def __getattr__(self, k: str) -> Any:
        try:
            return self[k]
        except KeyError as e:  # pragma: no cover - error path
            raise AttributeError(k) from e

    def __setattr__(self, k: str, v: Any) -> None:
        self[k] = v


def _wrap(x: Any) -> Any:
    if isinstance(x, Mapping):
        return Record({k: _wrap(v) for k, v in x.items()})
    if isinstance(x, list):
        return [_wrap(v) for v in x]
    return x


# keys the hot path reads (subset of ModelConfig, config_loader.py:369-414)
_REQUIRED = {
    "": ["n_fft", "win_length", "hop_length", "style_dim", "inter_dim", "sample_rate"],
    "decoder": ["hidden_dim", "residual_dim"],
    "generator": ["input_dim", "hidden_dim", "conv_intermediate_dim", "io_conv_kernel_size"],
    "text_encoder": ["tokens", "hidden_dim", "filter_channels", "heads", "layers", "kernel_size"],
    "style_encoder": ["layers"],
    "duration_predictor": ["n_layer", "duration_classes", "max_duration"],
    "pitch_energy_predictor": ["inter_dim"],
}

# The default model.yml of the reference (train/config/model.yml), restated as
# data: only the hot-path keys.  Used when no YAML is given (bench, tests).
DEFAULT_MODEL = {
    "multispeaker": False,
    "n_mels": 80,
    "sample_rate": 24000,
    "n_fft": 2048,
    "win_length": 1200,
    "hop_length": 300,
    "style_dim": 64,
    "inter_dim": 128,
    "decoder": {"hidden_dim": 512, "residual_dim": 64},
    "generator": {
        "type": "freegan",
        "input_dim": 512,
        "hidden_dim": 512,
        "conv_intermediate_dim": 1536,
        "io_conv_kernel_size": 7,
        "conformer_layers": 5,
        "conv_layers": 5,
    },
    "text_encoder": {
        "tokens": 178,
        "hidden_dim": 128,
        "filter_channels": 512,
        "heads": 8,
        "layers": 8,
        "kernel_size": 3,
        "dropout": 0.2,
    },
    "style_encoder": {"layers": 2},
    "duration_predictor": {
        "n_layer": 4,
        "duration_classes": 16,
        "max_duration": 50,
        "dropout": 0.2,
        "last_dropout": 0.5,
    },
    "pitch_energy_predictor": {"inter_dim": 256, "dropout": 0.2},
    # feature extractors whose OUTPUT WIDTHS size the flow-matching mel decoder (model.yml:68-74; the extractors themselves are given tensors)
    # (hubert.sr and the optional hubert.arch - HubertConfig fields, base values when absent - shape the content encoder itself: hubert_ssl_config)
    "hubert": {"hidden_dim": 768, "sr": 16000},
    "mel_style_encoder": {"max_channels": 384, "skip_downsample": True},
    "speaker_embedder": {"hidden_dim": 10240},
    # text symbols (model.yml:81-85); index = position in pad + punctuation + letters + letters_ipa
    "symbol": {
        "pad": '$',
        "punctuation": ';:,.!?¡¿—…"()“” ',
        "letters": 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz',
        "letters_ipa": "ɑɐɒæɓʙβɔɕçɗɖðʤəɘɚɛɜɝɞɟʄɡɠɢʛɦɧħɥʜɨɪʝɭɬɫɮʟɱɯɰŋɳɲɴøɵɸθœɶʘɹɺɾɻʀʁɽʂʃʈʧʉʊʋⱱʌɣɤʍχʎʏʑʐʒʔʡʕʢǀǁᵊǃˈˌːˑʼʴʰʱʲʷˠˤ˞↓↑→↗↘'̩'ᵻ",
    },
}


def validate(cfg: Record) -> Record:
    for section, keys in _REQUIRED.items():
        node = cfg if section == "" else cfg.get(section)
        if node is None:
            raise ValueError(f"model config: missing section '{section}'")
        for k in keys:
            if k not in node:
                raise ValueError(f"model config: missing key '{section}.{k}'".replace("'.", "'"))
    g = cfg.generator
    if g.get("type", "freegan") != "freegan":
        # GeneratorConfig.type is Literal["freegan"] (config_loader.py:203); the
        # ringformer generator cannot be instantiated in the reference either.
        raise ValueError("only generator.type == 'freegan' is executable in the reference")
    if cfg.hop_length % 4 != 0:
        raise ValueError("hop_length must be divisible by 4 (vocoder runs at hop/4)")
    return cfg


def geometry(cfg) -> tuple:
    """The vocoder's STFT geometry of a model config: (n_fft, win_length, h, bins, specialised), h = hop_length / 4 the vocoder hop and
    specialised True for the model.yml default 2048 / 1200 / 300 (the engine's specialised kernels).  Raises ValueError naming the rule a
    geometry breaks; the engine's finalize applies the same rules (csrc/signal_geom.hip.h: signal_geometry)."""
    n_fft, win, hop, sr = int(cfg.n_fft), int(cfg.win_length), int(cfg.hop_length), cfg.sample_rate
    if n_fft <= 0 or n_fft & (n_fft - 1):
        raise ValueError(f"n_fft {n_fft} is not a power of two")
    if not 256 <= n_fft <= 4096:
        raise ValueError(f"n_fft {n_fft} is outside [256, 4096]")
    if not 1 <= win <= n_fft:
        raise ValueError(f"win_length {win} is outside [1, n_fft = {n_fft}]")
    if hop <= 0 or hop % 4:
        raise ValueError(f"hop_length {hop} is not a positive multiple of 4 (the vocoder runs at hop / 4)")
    if not sr > 0:
        raise ValueError(f"sample_rate {sr} is not positive")
    h, lo = hop // 4, (n_fft - win) // 2
    # NOLA over one period of the overlap-add envelope, torch.istft's threshold (the window in fp32, as the engine's table)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)).astype(np.float32).astype(np.float64)
    env = np.zeros(h)
    np.add.at(env, (lo + np.arange(win)) % h, w * w)
    if not env.min() > 1e-11:
        raise ValueError(f"NOLA: the overlap-add envelope of Hann({win})^2 at hop {h} reaches {env.min():.3g} (must exceed 1e-11)")
    return n_fft, win, h, n_fft // 2 + 1, (n_fft, win, hop) == (2048, 1200, 300)


def hubert_dims(cfg) -> tuple:
    """(hubert.hidden_dim, speaker_embedder.hidden_dim): the feature widths of the voice-conversion models (models/models.py:92-101,
    models/hubert_encoder.py:9-11).  Raises ValueError naming a missing or non-positive width."""
    out = []
    for section in ("hubert", "speaker_embedder"):
        node = cfg.get(section)
        v = node.get("hidden_dim") if node is not None else None
        if v is None:
            raise ValueError(f"model config: missing key '{section}.hidden_dim'")
        if isinstance(v, bool) or int(v) != v or int(v) <= 0:
            raise ValueError(f"{section}.hidden_dim {v} is not a positive integer")
        out.append(int(v))
    return tuple(out)


def hubert_ssl_config(cfg) -> tuple:
    """(hubert.sr, arch) of the HuBERT content encoder (model.yml:68-71): ``sr`` defaults to 16000, ``hubert.arch`` is an optional mapping of
    transformers HubertConfig fields over the HuBERT-base values (hubert_ssl.ARCH_DEFAULTS).  Raises ValueError naming the field for an
    unsupported graph, a non-positive rate, or an arch.hidden_size that is not hubert.hidden_dim."""
    from .hubert_ssl import DEFAULT_SR, arch_from_model_config

    a = arch_from_model_config(cfg)
    sr = (cfg.get("hubert") or {}).get("sr", DEFAULT_SR)
    if isinstance(sr, bool) or int(sr) != sr or int(sr) <= 0:
        raise ValueError(f"hubert.sr {sr} is not a positive integer")
    return int(sr), a


def check_width(what: str, got: int, key: str, expected: int) -> None:
    """ValueError naming the width when an input's feature width is not the configured one."""
    if int(got) != int(expected):
        raise ValueError(f"{what} has width {int(got)}; {key} is {int(expected)}")


def load_model_config(src: Any = None) -> Record:
    """Accepts None (reference default), a path, an open file, a YAML/JSON string or a dict."""
    if src is None:
        data = DEFAULT_MODEL
    elif isinstance(src, Mapping):
        data = src
    elif isinstance(src, (io.IOBase,)) or hasattr(src, "read"):
        data = yaml.safe_load(src)
    elif isinstance(src, str) and ("\n" in src or src.lstrip().startswith("{")):
        data = yaml.safe_load(src)
    else:
        with open(src, "r", encoding="utf-8") as f:
            data = yaml.safe_load(f)
    return validate(_wrap(data))


def to_json(cfg: Record) -> str:
    return json.dumps(cfg, sort_keys=True)
