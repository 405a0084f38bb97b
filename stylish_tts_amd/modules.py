"""Drop-in nn.Module shims: the reference's constructor arguments, forward() signatures and state_dict keys, with
every forward() executed by libstylish_hip.so.

Reference classes mirrored (paths relative to /root/reference/src/stylish_tts/train/):
  TextEncoder            models/text_encoder.py:397-462
  TextStyleEncoder       models/text_style_encoder.py:6-26
  DurationPredictor      models/duration_predictor.py:8-36
  DurationProcessor      utils.py:385-494
  PitchEnergyPredictor   models/pitch_energy_predictor.py:11-121
  Decoder                models/decoder.py:6-60
  Generator              models/generator.py:340-438
  SpeechPredictor        models/speech_predictor.py:13-129
  ExportModel            models/export_model.py:5-45
  HubertSpeechPredictor       models/speech_predictor.py:132-251
  HubertPitchEnergyPredictor  models/pitch_energy_predictor.py:124-191
  MelStyleEncoder             models/mel_style_encoder.py:120-151
  CfmPitchPredictor           models/cfm/cfm_pitch_predictor.py:12-51 (+ norm_f0_zscore / denorm_f0_zscore, train/stage_type.py:783-829)
  AdaptiveHubert              models/ssl.py:16-31
  RmvpePitchExtractor         dataprep/rmvpe/inference.py:12-65 (E2E0 of model.py:49-86; MelSpectrogram of spec.py:7-71)
  TextAligner                 models/text_aligner.py:16-127 (tdnn_blstm_ctc_model / CTCModel) + dataprep/align_text.py:159-210 (torch_align)
  LogMelSpectrogram           torchaudio MelSpectrogram + calculate_mel (stage_type.py:1023-1032), preprocess (dataprep/align_text.py:112-117),
                              log_norm / compute_log_mel_stats (utils.py:71-148)
  Resample                    torchaudio.transforms.Resample as models/ssl.py:21-24 and dataprep/rmvpe/inference.py:50-59 build it
  MultiSpectrogram            train/multi_spectrogram.py:25-81
  MultiResolutionSTFTLoss     train/losses.py:14-35 (forward values; fused from the audio behind one MultiSpectrogram.forward call's lists, else on the tensors)
  MagPhaseLoss                train/losses.py:38-154 (forward values; leaves pred.phase unmodified)
  PosteriorEncoder            models/flow.py:234-293 (+ FlowStatistics, utils.py:357-360)

Differences, all additive: forward() of the stochastic modules takes an optional ``noise`` dict with the three draws
the reference takes from the global torch generator (``prior_noise`` [B,128,4T], ``src_noise`` [B,1,300T],
``init_phase`` [1,1]); when omitted they are drawn with torch on the device.  Weights live in a flat store keyed by
the reference's state_dict names (both weight-norm flavours), so ``load_state_dict`` accepts reference checkpoints;
``posterior_encoder.*`` keys never enter a shim's own store: SpeechPredictor builds a PosteriorEncoder from a complete set (copy-synthesis,
``forward(audio_gt=...)``), every other case ignores them.  There is no CPU path: forward() needs the GPU library.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import params
from .config import DEFAULT_MODEL, Record, check_width, hubert_dims, load_model_config
from .runtime import HipModel, Segments

W_DECODER, W_FLOW, W_GENERATOR, W_SPEECH_TEXT, W_DURATION, W_PE_TEXT, W_PE_STYLE, W_PITCH_ENERGY = 1, 2, 4, 8, 16, 32, 64, 128
W_HUBERT, W_HUBERT_PE = 512, 1024  # hubert_speech_predictor.{phone_encoder, style_encoder}; hubert_pitch_energy_predictor.*
W_PE_MEL_STYLE, W_CFM_PITCH = 2048, 4096  # pe_mel_style_encoder.*; cfm_pitch_predictor.spk_emb.*
W_CFM_PITCH_NET = 8192  # cfm_pitch_predictor.{asr_emb, blocks, out_proj}
W_SSL = 16384  # hubert.model.* (AdaptiveHubert; finalized by stts_ssl_finalize)
W_RMVPE = 32768  # rmvpe.* (RmvpePitchExtractor; finalized by stts_rmvpe_finalize)
W_ALIGNER = 65536  # text_aligner.* (TextAligner; finalized by stts_aligner_finalize)
W_WAVLM = 131072  # wavlm.* (WavLM; finalized by stts_wavlm_finalize)
W_POSTERIOR = 262144  # speech_predictor.posterior_encoder.* (PosteriorEncoder; outside STTS_W_ALL)
W_FLOW_STATS = 524288  # speech_predictor.flow.* + prior_encoder.* packed again in fp32 for the flow statistics (outside STTS_W_ALL)

_ENGINES: Dict[int, HipModel] = {}


def get_engine(cfg=None, device: int = 0) -> HipModel:
    """One stts_ctx per device, shared by every shim (weights are namespaced by module name)."""
    if device not in _ENGINES or _ENGINES[device].ctx is None:
        _ENGINES[device] = HipModel(cfg if cfg is not None else load_model_config(), device)
    return _ENGINES[device]


class FlowStatistics(NamedTuple):
    """utils.py:357-360: a latent and the Gaussian it was drawn from, each [B, C, T]."""

    z: torch.Tensor
    mean: torch.Tensor
    logstd: torch.Tensor


class DecoderPrediction:
    """utils.py:363-382 (inference fields; copy-synthesis fills mel_stats, and with flow_stats=True the other three statistics)."""

    def __init__(self, *, audio, magnitude, phase):
        self.audio, self.magnitude, self.phase = audio, magnitude, phase
        self.text_stats = self.text2mel_stats = self.mel_stats = self.mel2text_stats = None


class HipModule(torch.nn.Module):
    """Flat parameter store with the reference's keys + lazy binding to the engine."""

    module_name = ""   # namespace inside the stts_ctx
    key_prefix = ""    # prefix of this module's keys inside that namespace (standalone sub-modules)
    components = 0     # STTS_W_* mask

    def __init__(self, spec, cfg, engine: Optional[HipModel] = None):
        super().__init__()
        self.cfg = cfg
        self._spec = spec
        self._store = OrderedDict((n, torch.zeros(s, dtype=torch.float32)) for n, s, _ in spec)
        self._engine = engine
        self._dirty = True
        self._device_index = 0

    # ---- nn.Module surface the reference's callers touch (models/export_model.py:19-28)
    def state_dict(self, *args, prefix: str = "", **kwargs):
        return OrderedDict((prefix + k, v) for k, v in self._store.items())

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        missing = [k for k in self._store if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._store and not k.startswith("posterior_encoder.")]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        for k in self._store:
            if k in state_dict:
                v = torch.as_tensor(state_dict[k]).detach().to("cpu", torch.float32)
                if tuple(v.shape) != tuple(self._store[k].shape):
                    raise RuntimeError(f"load_state_dict: shape mismatch for {k}: {tuple(v.shape)} vs {tuple(self._store[k].shape)}")
                self._store[k] = v.clone()
        self._dirty = True
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def parameters(self, recurse: bool = True):
        return iter(self._store.values())

    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True):
        return iter((prefix + k, v) for k, v in self._store.items())

    def to(self, *args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (str, torch.device)):
                d = torch.device(a)
                if d.type == "cuda":
                    self._device_index = d.index or 0
        return self

    def load_synthetic(self, seed: int = 0):
        """Name-keyed synthetic weights (params.synth_state_dict), as used by the golden fixtures."""
        sd = params.synth_state_dict(self._spec, seed, prefix=self.module_name + "." + self.key_prefix)
        self.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return self

    # ---- engine binding
    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self.cfg, self._device_index)
        self._bind()
        return self._engine

    def _bind(self):
        """Shims share one engine per device and several may map to the same component (two Decoder instances, a Decoder
        next to a SpeechPredictor, the reference's three TextEncoder instances): the engine remembers which shim packed
        each component last, and a shim whose weights are not the packed ones re-binds before it runs."""
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        bits = [1 << i for i in range(self.components.bit_length()) if self.components >> i & 1]
        if self._dirty or any(owners.get(b) is not self for b in bits):
            self._load_into(eng)
            eng.finalize(self.components)  # releases the previous packing of these components (stts_finalize_weights)
            for b in bits:
                owners[b] = self
            self._dirty = False


    def _load_into(self, eng: HipModel):
        eng.load_state_dict(self.module_name, self._store, prefix=self.key_prefix)


# ------------------------------------------------------------------------------------------------ helpers
def _f(x: torch.Tensor, dev) -> torch.Tensor:
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _pack_tokens(texts: torch.Tensor, lengths: torch.Tensor, dev):
    L = [int(v) for v in lengths.tolist()]
    toks = torch.cat([texts[b, : L[b]] for b in range(len(L))]).to(device=dev, dtype=torch.int64).contiguous()
    return toks, Segments(L, dev)


def _pack_rows(eng: HipModel, x_bcp: torch.Tensor, lengths) -> torch.Tensor:
    """[B,C,P] padded -> packed time-major [sum P, ld] (transpose on the GPU library, row selection is plumbing)."""
    B, C, P = x_bcp.shape
    tmaj = eng.to_time_major(_f(x_bcp, eng.device))  # [B*P, ld]
    idx = torch.cat([torch.arange(b * P, b * P + int(lengths[b]), device=eng.device) for b in range(B)])
    return tmaj.index_select(0, idx).contiguous()


def _unpack_rows(eng: HipModel, x: torch.Tensor, seg: Segments, C: int, P: int) -> torch.Tensor:
    """packed [sum P, ld] -> [B,C,P] zero padded."""
    B = seg.n
    padded = torch.zeros(B * P, x.shape[1], dtype=torch.float32, device=eng.device)
    idx = torch.cat([torch.arange(b * P, b * P + seg.lengths[b], device=eng.device) for b in range(B)])
    padded.index_copy_(0, idx, x)
    return eng.to_channel_major(padded, B, C, P)


def _durations_from_alignment(alignment: torch.Tensor, lengths, dev):
    """The reference passes the 0/1 matrix [B,P,T] (utils.py:476-489); the library takes integer durations."""
    d = alignment.sum(dim=2).round().to(torch.int32)
    L = [int(v) for v in lengths]
    dur = torch.cat([d[b, : L[b]] for b in range(len(L))]).to(dev).contiguous()
    T = [int(d[b, : L[b]].sum().item()) for b in range(len(L))]
    return dur, T


def draw_noise(B: int, T4: int, dev, flow_dim: int = 128, h: int = 75):
    """The reference's three draws (models/flow.py:314; models/generator.py:272,306) with torch's generator; h = hop_length / 4."""
    return dict(prior_noise=torch.randn(B, flow_dim, T4, device=dev), src_noise=torch.randn(B, 1, h * T4, device=dev),
                init_phase=torch.rand(1, 1, device=dev))


# ------------------------------------------------------------------------------------------------ modules
class TextEncoder(HipModule):
    module_name, components, _which = "pe_text_encoder", W_PE_TEXT, 2

    def __init__(self, *, inter_dim, config, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        c2 = Record(cfg)
        c2["text_encoder"] = Record(config)
        self.inter_dim = inter_dim
        super().__init__(params.text_encoder_spec("", c2, inter_dim), cfg, engine)

    def forward(self, x, x_lengths, spks=None):
        eng = self.engine
        toks, seg = _pack_tokens(x, x_lengths, eng.device)
        mu, xh = eng.text_encoder(self._which, seg, toks, return_hidden=True)
        P = x.shape[1]
        mask = (torch.arange(P, device=eng.device)[None, :] < x_lengths.to(eng.device)[:, None]).unsqueeze(1).float()
        return _unpack_rows(eng, mu, seg, self.inter_dim, P), _unpack_rows(eng, xh, seg, self.cfg.text_encoder.hidden_dim, P), mask


class TextStyleEncoder(HipModule):
    module_name, components, _which = "pe_text_style_encoder", W_PE_STYLE, 2

    def __init__(self, inter_dim, style_dim, config, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        c2 = Record(cfg)
        c2["style_encoder"] = Record(config)
        c2["style_dim"] = style_dim
        super().__init__(params.text_style_encoder_spec("", c2, inter_dim), cfg, engine)

    def forward(self, x, lengths):
        eng = self.engine
        L = [int(v) for v in lengths.tolist()]
        return eng.text_style(self._which, Segments(L, eng.device), _pack_rows(eng, x, L))


class DurationPredictor(HipModule):
    module_name, components = "duration_predictor", W_DURATION

    def __init__(self, style_dim, inter_dim, text_config, style_config, duration_config, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        super().__init__(params.duration_predictor_spec(cfg), cfg, engine)

    def forward(self, texts, text_lengths):
        eng = self.engine
        toks, seg = _pack_tokens(texts, text_lengths, eng.device)
        logits, _ = eng.duration(seg, toks)
        B, P = texts.shape
        # padded positions: prosody is masked to 0 there (prosody_encoder.py:80), so the reference returns the bias
        out = self._store["duration_proj.linear_layer.bias"].to(eng.device).expand(B, P, -1).clone()
        for b in range(B):
            out[b, : seg.lengths[b]] = logits[seg.host[b] : seg.host[b + 1]]
        return out


# the frames a duration class stands for, and the class of a duration of 0 .. 50 frames (utils.py:391-450)
_CLASS_TO_DUR = [1, 2, 3, 4, 5, 6, 7, 9, 12, 15, 18, 22, 27, 32, 38, 46]
_DUR_TO_CLASS = [0, 0, 1, 2, 3, 4, 5, 6] + [7] * 3 + [8] * 3 + [9] * 3 + [10] * 3 + [11] * 5 + [12] * 5 + [13] * 5 + [14] * 7 + [15] * 9


class DurationProcessor(torch.nn.Module):
    """utils.py:385-494: logits [P,16] -> 0/1 alignment [P,T]; dur_to_class / align_to_class: the host tables of the duration targets."""

    def __init__(self, class_count, max_dur):
        super().__init__()
        self.class_count, self.max_dur = class_count, max_dur
        # utils.py:391-450, host tables (kept out of state_dict: the shim's keys stay as they were)
        self.register_buffer("class_to_dur_table", torch.tensor(_CLASS_TO_DUR, dtype=torch.float32), persistent=False)
        self.register_buffer("dur_to_class_table", torch.tensor(_DUR_TO_CLASS, dtype=torch.float32), persistent=False)

    def dur_to_class(self, durs):
        """utils.py:459-461: durations clamped to [1, max_dur] -> their class (a float tensor, like the reference's table)."""
        durs = torch.as_tensor(durs).clamp(min=1, max=self.max_dur)
        return self.dur_to_class_table.to(durs.device)[durs.long()]

    def align_to_class(self, alignment):
        """utils.py:463-466: a 0/1 alignment [.., P, T] -> the duration class of every token."""
        return self.dur_to_class(torch.as_tensor(alignment).sum(dim=-1).clamp(min=1, max=50))

    def prediction_to_duration(self, pred, text_length=None):
        from . import _lib
        from .runtime import _ptr, _stream

        lib = _lib.load()
        p = pred.to(dtype=torch.float32).contiguous()
        if not p.is_cuda:
            p = p.cuda()
        dur = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
        _lib.check(lib.stts_duration_decode(_stream(), _ptr(p), p.shape[1], p.shape[0], _ptr(dur)))
        return dur

    def duration_to_alignment(self, duration):
        from . import _lib
        from .runtime import _ptr, _stream

        lib = _lib.load()
        d = duration.to(dtype=torch.int32).contiguous()
        if not d.is_cuda:
            d = d.cuda()
        T = int(d.sum().item())  # the same host round trip the reference has (test_onnx.py:65-66)
        out = torch.empty(d.shape[0], T, dtype=torch.float32, device=d.device)
        _lib.check(lib.stts_duration_to_alignment(_stream(), _ptr(d), d.shape[0], T, _ptr(out)))
        return out

    def forward(self, pred, text_length):
        return self.duration_to_alignment(self.prediction_to_duration(pred, text_length))


class PitchEnergyPredictor(HipModule):
    module_name, components = "pitch_energy_predictor", W_PITCH_ENERGY

    def __init__(self, style_dim, inter_dim, text_config, style_config, duration_config, pitch_energy_config, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        super().__init__(params.pitch_energy_predictor_spec(cfg), cfg, engine)

    def forward(self, text_encoding, text_lengths, alignment, style):
        eng = self.engine
        L = [int(v) for v in text_lengths.tolist()]
        dur, T = _durations_from_alignment(alignment, L, eng.device)
        sp, st = Segments(L, eng.device), Segments(T, eng.device)
        f0, en = eng.pitch_energy(sp, st, dur, _pack_rows(eng, text_encoding, L), _f(style, eng.device))
        Tm = alignment.shape[2]
        F0 = torch.zeros(len(L), Tm, device=eng.device)
        N = torch.zeros(len(L), Tm, device=eng.device)
        for b in range(len(L)):
            F0[b, : T[b]] = f0[st.host[b] : st.host[b + 1]]
            N[b, : T[b]] = en[st.host[b] : st.host[b + 1]]
        return F0, N


class Decoder(HipModule):
    module_name, key_prefix, components = "speech_predictor", "decoder.", W_DECODER

    def __init__(self, *, dim_in, style_dim, dim_out, hidden_dim, residual_dim, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        super().__init__(params.decoder_spec("", dim_in, style_dim, hidden_dim, residual_dim), cfg, engine)
        self.hidden_dim = hidden_dim

    def forward(self, asr, F0_curve, N, s):
        eng = self.engine
        B, _, T4 = asr.shape
        seg = Segments([T4] * B, eng.device)
        x = eng.decoder(seg, eng.to_time_major(_f(asr, eng.device)), _f(F0_curve, eng.device).reshape(-1), _f(N, eng.device).reshape(-1),
                        _f(s, eng.device))
        return eng.to_channel_major(x, B, self.hidden_dim, T4), F0_curve


class Generator(HipModule):
    module_name, key_prefix, components = "speech_predictor", "generator.", W_GENERATOR

    def __init__(self, *, style_dim, n_fft, win_length, hop_length, config, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        super().__init__(params.generator_spec("", cfg), cfg, engine)
        self.n_bins = n_fft // 2 + 1
        self.hop4 = hop_length // 4

    def forward(self, *, mel, style, pitch, energy=None, noise=None):
        eng = self.engine
        B, _, T4 = mel.shape
        seg = Segments([T4] * B, eng.device)
        nz = noise or draw_noise(B, T4, eng.device, h=self.hop4)
        spec, phase = eng.harmonic_stft(seg, _f(pitch, eng.device).reshape(-1), _f(torch.as_tensor(nz["src_noise"]), eng.device).reshape(-1),
                                        _f(torch.as_tensor(nz["init_phase"]), eng.device).reshape(-1), batch_scope=True)
        audio, la, ph = eng.vocoder(seg, eng.to_time_major(_f(mel, eng.device)), _f(style, eng.device), spec, phase, return_spec=True)
        eng.check_status()
        rep = lambda t: torch.cat([t, t[:, :, -1:]], dim=2)  # F.pad(..., mode="replicate") (generator.py:425-426)  # noqa: E731
        return DecoderPrediction(audio=audio.reshape(B, 1, self.hop4 * T4), magnitude=rep(eng.to_channel_major(la, B, self.n_bins, T4)),
                                 phase=rep(eng.to_channel_major(ph, B, self.n_bins, T4)))


class PosteriorEncoder(HipModule):
    """models/flow.py:234-293: recording -> (z, mean, logstd), z ~ q(z | audio).  The reference's constructor; SpeechPredictor builds it with
    out = hidden = decoder.hidden_dim // 4, kernel 3, dilation 1, 12 layers, hop_length // 4 and style_dim conditioning
    (models/speech_predictor.py:39-49).  The STFT is the engine's (the vocoder's geometry), so n_fft / hop_length / win_length must be the
    config's; dilation_rate must be 1 (the reference never builds another)."""

    module_name, key_prefix, components = "speech_predictor", "posterior_encoder.", W_POSTERIOR

    def __init__(self, out_channels, hidden_channels, kernel_size, dilation_rate, n_layers, n_fft, hop_length, win_length, gin_channels=0, cfg=None, engine=None):
        cfg = cfg or load_model_config()
        if dilation_rate != 1:
            raise ValueError(f"PosteriorEncoder: dilation_rate {dilation_rate} is not built (the reference uses 1)")
        if (n_fft, win_length, hop_length) != (cfg.n_fft, cfg.win_length, cfg.hop_length // 4):
            raise ValueError(f"PosteriorEncoder: STFT geometry {(n_fft, win_length, hop_length)} is not the engine's {(cfg.n_fft, cfg.win_length, cfg.hop_length // 4)}")
        if gin_channels not in (0, cfg.style_dim):
            raise ValueError(f"PosteriorEncoder: gin_channels {gin_channels} must be 0 or style_dim {cfg.style_dim}")
        if kernel_size % 2 != 1 or hidden_channels % 32 or out_channels % 4:
            raise ValueError("PosteriorEncoder: kernel_size must be odd, hidden_channels a multiple of 32, out_channels a multiple of 4")
        super().__init__(params.posterior_encoder_spec(cfg, "", hidden_channels, out_channels, kernel_size, n_layers, gin_channels), cfg, engine)
        self.out_channels, self.hidden_channels, self.gin_channels, self.hop = out_channels, hidden_channels, gin_channels, hop_length

    @classmethod
    def from_config(cls, cfg=None, engine=None):
        """As SpeechPredictor.__init__ builds it (models/speech_predictor.py:39-49)."""
        cfg = cfg or load_model_config()
        fh = cfg.decoder.hidden_dim // 4
        return cls(fh, fh, 3, 1, 12, cfg.n_fft, cfg.hop_length // 4, cfg.win_length, gin_channels=cfg.style_dim, cfg=cfg, engine=engine)

    def packed(self, seg: Segments, audio, style=None, noise=None, **kw):
        """Packed rows: audio [hop * rows] (seg at the vocoder-frame rate), style [n_utt, 64] or None, noise [rows, out] (drawn when omitted)
        -> HipModel.posterior's dict."""
        eng = self.engine
        if noise is None:
            noise = torch.randn(seg.rows, self.out_channels, device=eng.device)
        return eng.posterior(seg, audio=audio, style=style, noise=noise, **kw)

    def forward(self, x, g=None, noise=None):
        eng = self.engine
        x = _f(torch.as_tensor(x), eng.device)
        if x.dim() == 3:
            x = x[:, 0]
        B, S = x.shape
        if S % self.hop:
            raise ValueError(f"PosteriorEncoder: {S} samples are not a multiple of the hop {self.hop}")
        T4 = S // self.hop
        seg = Segments([T4] * B, eng.device)
        style = None if g is None else _f(torch.as_tensor(g), eng.device).reshape(B, -1)
        nz = None if noise is None else _f(torch.as_tensor(noise), eng.device).transpose(1, 2).reshape(B * T4, self.out_channels).contiguous()
        o = self.packed(seg, x.reshape(-1), style, nz)
        eng.check_status()
        return tuple(eng.to_channel_major(o[k], B, self.out_channels, T4) for k in ("z", "mean", "logstd"))


class SpeechPredictor(HipModule):
    module_name, components = "speech_predictor", W_DECODER | W_FLOW | W_GENERATOR | W_SPEECH_TEXT

    def __init__(self, model_config=None, engine=None):
        cfg = model_config if model_config is not None else load_model_config()
        super().__init__(params.speech_predictor_spec(cfg), cfg, engine)
        self.__dict__["_posterior"] = None  # (not a registered sub-module: state_dict() keeps the inference inventory)

    @property
    def has_posterior(self) -> bool:
        return self._posterior is not None

    @property
    def posterior(self) -> Optional[PosteriorEncoder]:
        return self._posterior

    def attach_posterior(self, module: Optional[PosteriorEncoder]):
        """Use `module` for forward(audio_gt=...) (None detaches).  Its weights stay its own: state_dict() here is unchanged."""
        if module is not None and not isinstance(module, PosteriorEncoder):
            raise TypeError("attach_posterior: a modules.PosteriorEncoder is expected")
        self.__dict__["_posterior"] = module
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        res = super().load_state_dict(state_dict, strict, assign)
        # a complete, correctly shaped posterior_encoder.* set builds the posterior; anything less is ignored as before
        want = params.posterior_encoder_spec(self.cfg)
        try:
            ok = all(n in state_dict and tuple(torch.as_tensor(state_dict[n]).shape) == tuple(sh) for n, sh, _ in want)
        except Exception:  # noqa: BLE001 - an entry that is no tensor: malformed, ignored
            ok = False
        if ok:
            pe = PosteriorEncoder.from_config(self.cfg, self._engine)
            pe.load_state_dict({n[len(pe.key_prefix):]: state_dict[n] for n, _, _ in want})
            self.attach_posterior(pe)
        return res

    def _bind(self):
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        bits = [1 << i for i in range(self.components.bit_length()) if self.components >> i & 1]
        rebinding = self._dirty or any(owners.get(b) is not self for b in bits)
        super()._bind()
        if rebinding:  # the flow statistics' packing is of the weights loaded before: packed again on their next use
            owners.pop(W_FLOW_STATS, None)

    def _bind_flow_stats(self, eng: HipModel):
        """W_FLOW_STATS is finalized lazily, on the first forward(flow_stats=True) after this shim's weights were (re)bound."""
        owners = eng.__dict__.setdefault("_owners", {})
        if owners.get(W_FLOW_STATS) is not self:
            eng.finalize(W_FLOW_STATS)
            owners[W_FLOW_STATS] = self

    def _resynthesize(self, texts, text_lengths, alignment, pitch, energy, audio_gt, noise, flow_stats=False):
        """forward(audio_gt=...): text encoder + style -> posterior(audio_gt | style) -> post_flow -> harmonic source + vocoder.  flow_stats: also
        decoder -> prior (text_stats) -> reverse flow (text2mel_stats), and the forward flow of the posterior's statistics (mel2text_stats)."""
        eng = self.engine
        pe = self._posterior
        if pe._engine is None:
            pe._engine = eng
        if pe._engine is not eng:
            raise RuntimeError("forward(audio_gt=...): the attached PosteriorEncoder is bound to another engine than this SpeechPredictor; build it with engine=<the "
                               "speech predictor's engine> (or with none)")
        pe.engine  # noqa: B018 - binds (packs) the posterior's weights
        # `energy` is read with flow_stats only: it feeds the decoder, which copy-synthesis alone does not run (the vocoder takes mel, style and pitch)
        toks, sp = _pack_tokens(texts, text_lengths, eng.device)
        dur, T = _durations_from_alignment(alignment, sp.lengths, eng.device)
        st = Segments(T, eng.device)
        st4 = st.scaled(4)
        B = sp.n
        h, nb, fh = self.cfg.hop_length // 4, self.cfg.n_fft // 2 + 1, self.cfg.decoder.hidden_dim // 4
        waves = list(audio_gt) if isinstance(audio_gt, (list, tuple)) else [w for w in torch.as_tensor(audio_gt)]
        waves = [_f(torch.as_tensor(w), eng.device).reshape(-1) for w in waves]
        if len(waves) != B:
            raise ValueError(f"audio_gt holds {len(waves)} recordings for {B} texts")
        for b in range(B):
            if waves[b].numel() < 4 * h * T[b]:
                raise ValueError(f"audio_gt[{b}] has {waves[b].numel()} samples, the alignment needs {4 * h * T[b]}")
        wave = torch.cat([waves[b][: 4 * h * T[b]] for b in range(B)]).contiguous()
        enc = eng.text_encoder(1, sp, toks)
        style = eng.text_style(1, sp, enc)
        pk = lambda t: torch.cat([_f(t, eng.device)[b, : T[b]] for b in range(B)])  # noqa: E731
        p4 = eng.upsample4(st, st4, pk(pitch))
        nz = noise or dict(draw_noise(B, 4 * max(T), eng.device, flow_dim=fh, h=h), posterior_noise=torch.randn(B, fh, 4 * max(T), device=eng.device))
        qn = _f(torch.as_tensor(nz["posterior_noise"]), eng.device)
        sn = _f(torch.as_tensor(nz["src_noise"]), eng.device)
        qn_tm = torch.cat([qn[b, :, : 4 * T[b]].t() for b in range(B)]).contiguous()
        sn_flat = torch.cat([sn[b, 0, : 4 * h * T[b]] for b in range(B)]).contiguous()
        ip = _f(torch.as_tensor(nz["init_phase"]), eng.device).reshape(-1)
        o = eng.posterior(st4, audio=wave, style=style, noise=qn_tm, mel=True)
        spec, phase = eng.harmonic_stft(st4, p4, sn_flat, ip, batch_scope=True)
        audio, la, ph = eng.vocoder(st4, o["mel"], style, spec, phase, return_spec=True)
        stats = dict(mel_stats=o)
        if flow_stats:
            if "prior_noise" not in nz:
                raise ValueError("forward(flow_stats=True): the noise dict needs prior_noise [B, 128, 4 T] (the prior's draw) next to posterior_noise")
            self._bind_flow_stats(eng)
            pn = _f(torch.as_tensor(nz["prior_noise"]), eng.device)
            pn_tm = torch.cat([pn[b, :, : 4 * T[b]].t() for b in range(B)]).contiguous()
            asr = eng.length_regulate(sp, st4, dur, 4, enc, self.cfg.inter_dim)
            x = eng.decoder(st4, asr, p4, eng.upsample4(st, st4, pk(energy)), style)
            text = eng.prior_stats(st4, x, pn_tm)
            stats.update(text_stats=text, text2mel_stats=eng.flow_stats(st4, text["z"], text["mean"], text["logstd"], style, reverse=True),
                         mel2text_stats=eng.flow_stats(st4, o["z"], o["mean"], o["logstd"], style, reverse=False))
        eng.check_status()
        if len(set(T)) == 1:
            T4 = 4 * T[0]
            rep = lambda t: torch.cat([t, t[:, :, -1:]], dim=2)  # noqa: E731
            pred = DecoderPrediction(audio=audio.reshape(B, 1, h * T4), magnitude=rep(eng.to_channel_major(la, B, nb, T4)),
                                     phase=rep(eng.to_channel_major(ph, B, nb, T4)))
            for name, d in stats.items():
                setattr(pred, name, FlowStatistics(*(eng.to_channel_major(d[k], B, fh, T4) for k in ("z", "mean", "logstd"))))
            return pred
        pred = DecoderPrediction(audio=[audio[h * st4.host[b] : h * st4.host[b + 1]] for b in range(B)], magnitude=None, phase=None)
        rows = lambda t, b: t[st4.host[b] : st4.host[b + 1]].t().unsqueeze(0).contiguous()  # noqa: E731
        for name, d in stats.items():
            setattr(pred, name, [FlowStatistics(*(rows(d[k], b) for k in ("z", "mean", "logstd"))) for b in range(B)])
        return pred

    def forward(self, texts, text_lengths, alignment, pitch, energy, audio_gt=None, noise=None, return_spectra=True, flow_stats=False):
        """audio_gt (copy-synthesis; [B, 300 T], [B, 1, 300 T] or a list of recordings for a ragged batch) needs a posterior (has_posterior): the
        vocoder then runs on post_flow(z_mel), z_mel ~ q(z | audio_gt, style); decoder and reverse flow are not run.  The prediction carries
        mel_stats = FlowStatistics(z, mean, logstd) (a list per utterance for a ragged batch); text_stats, text2mel_stats and mel2text_stats
        stay None.  The noise dict then holds posterior_noise [B, 128, 4 T] in place of prior_noise.
        flow_stats=True (with audio_gt): additionally the decoder, the prior with its three outputs (noise key prior_noise, next to
        posterior_noise), the reverse flow of the prior's statistics and the forward flow of the posterior's - all four FlowStatistics of the
        reference's training forward (speech_predictor.py:99-128), what NormalizingFlowLoss reads.  audio, magnitude, phase and mel_stats are
        the bits of the flow_stats=False call with the same noise."""
        if flow_stats and audio_gt is None:
            raise NotImplementedError("flow_stats=True needs audio_gt: the mel and mel2text statistics come from the posterior encoder of a recording")
        if audio_gt is not None:
            if not self.has_posterior:
                raise NotImplementedError("audio_gt needs the posterior encoder: load a state_dict that holds the complete posterior_encoder.* set, "
                                          "or attach_posterior(modules.PosteriorEncoder)")
            return self._resynthesize(texts, text_lengths, alignment, pitch, energy, audio_gt, noise, flow_stats)
        eng = self.engine
        toks, sp = _pack_tokens(texts, text_lengths, eng.device)
        dur, T = _durations_from_alignment(alignment, sp.lengths, eng.device)
        st = Segments(T, eng.device)
        st4 = st.scaled(4)
        B = sp.n
        enc = eng.text_encoder(1, sp, toks)
        style = eng.text_style(1, sp, enc)
        asr = eng.length_regulate(sp, st4, dur, 4, enc, self.cfg.inter_dim)
        pk = lambda t: torch.cat([_f(t, eng.device)[b, : T[b]] for b in range(B)])  # noqa: E731
        p4, e4 = eng.upsample4(st, st4, pk(pitch)), eng.upsample4(st, st4, pk(energy))
        equal = len(set(T)) == 1
        h, nb = self.cfg.hop_length // 4, self.cfg.n_fft // 2 + 1
        nz = noise or draw_noise(B, 4 * max(T), eng.device, h=h)
        pn = _f(torch.as_tensor(nz["prior_noise"]), eng.device)
        sn = _f(torch.as_tensor(nz["src_noise"]), eng.device)
        pn_tm = torch.cat([pn[b, :, : 4 * T[b]].t() for b in range(B)]).contiguous()
        sn_flat = torch.cat([sn[b, 0, : 4 * h * T[b]] for b in range(B)]).contiguous()
        ip = _f(torch.as_tensor(nz["init_phase"]), eng.device).reshape(-1)
        x = eng.decoder(st4, asr, p4, e4, style)
        mel = eng.prior_flow(st4, x, style, pn_tm)
        spec, phase = eng.harmonic_stft(st4, p4, sn_flat, ip, batch_scope=True)
        audio, la, ph = eng.vocoder(st4, mel, style, spec, phase, return_spec=True)
        eng.check_status()
        if equal:
            T4 = 4 * T[0]
            rep = lambda t: torch.cat([t, t[:, :, -1:]], dim=2)  # noqa: E731
            return DecoderPrediction(audio=audio.reshape(B, 1, h * T4), magnitude=rep(eng.to_channel_major(la, B, nb, T4)),
                                     phase=rep(eng.to_channel_major(ph, B, nb, T4)))
        return DecoderPrediction(audio=[audio[h * st4.host[b] : h * st4.host[b + 1]] for b in range(B)], magnitude=None, phase=None)


def _stat_rows(stats, dev):
    """FlowStatistics of [B, C, T] tensors, or a list of per-utterance ones ([1, C, T_b]) -> ({z, mean, logstd} packed time-major rows, lengths)."""
    items = stats if isinstance(stats, (list, tuple)) and not isinstance(stats, FlowStatistics) else [stats]
    lengths = [int(t.z.shape[2]) for t in items for _ in range(t.z.shape[0])]
    rows = {k: torch.cat([_f(getattr(t, k), dev).transpose(1, 2).reshape(-1, t.z.shape[1]) for t in items]).contiguous() for k in ("z", "mean", "logstd")}
    return rows, lengths


def flow_kl_sums(eng: HipModel, pred):
    """The sums behind NormalizingFlowLoss's two scores (train/losses.py:205-222) of a prediction that carries all four FlowStatistics
    -> (device double [2, B]: kl_text, kl_audio per utterance; lengths [B])."""
    text, L = _stat_rows(pred.text_stats, eng.device)
    t2m, _ = _stat_rows(pred.text2mel_stats, eng.device)
    mel, _ = _stat_rows(pred.mel_stats, eng.device)
    m2t, _ = _stat_rows(pred.mel2text_stats, eng.device)
    seg = Segments(L, eng.device)
    return torch.stack([eng.kl_sums(seg, 0, m2t["z"], m2t["logstd"], text["mean"], text["logstd"]),
                        eng.kl_sums(seg, 1, t2m["mean"], t2m["logstd"], mel["mean"], mel["logstd"])]), L


def flow_kl_score(sums, lengths):
    """host numbers [B] of one score -> (sum / rows: the reference's mask sums to B T, not B T C; every utterance's own value)."""
    tot = 0.0
    for v in sums:
        tot += v
    return tot / sum(lengths), [v / n for v, n in zip(sums, lengths)]


def has_flow_stats(pred) -> bool:
    return all(getattr(pred, k, None) is not None for k in ("text_stats", "text2mel_stats", "mel_stats", "mel2text_stats"))


class NormalizingFlowLoss(torch.nn.Module):
    """train/losses.py:205-222 as validation numbers: kl_text = kl_loss(z_mel2text, logstd_mel2text, mean_text, logstd_text) and kl_audio =
    kl_loss_normal(mean_text2mel, logstd_text2mel, mean_mel, logstd_mel) of a prediction from SpeechPredictor.forward(audio_gt=, flow_stats=True),
    summed in fp64 on the engine (stts_val_kl_sums).  No gradients."""

    def __init__(self, cfg=None, engine: Optional[HipModel] = None):
        super().__init__()
        self.cfg, self._engine = cfg, engine

    def scores(self, pred) -> dict:
        if not has_flow_stats(pred):
            raise ValueError("NormalizingFlowLoss: the prediction carries no flow statistics (SpeechPredictor.forward(audio_gt=..., flow_stats=True) fills them)")
        eng = self._engine if self._engine is not None else get_engine(self.cfg)
        sums, L = flow_kl_sums(eng, pred)
        host = sums.cpu().tolist()
        out = {}
        for name, row in zip(("kl_text", "kl_audio"), host):
            out[name], out[name + "_utt"] = flow_kl_score(row, L)
        return out

    def forward(self, pred, log):
        sc = self.scores(pred)
        log.add_loss("kl_text", torch.tensor(sc["kl_text"], dtype=torch.float64))
        log.add_loss("kl_audio", torch.tensor(sc["kl_audio"], dtype=torch.float64))


class STFT(torch.nn.Module):
    """models/stft.py:6-187: the conv-form STFT of the ONNX export, same constructor and transform() / inverse() signatures.
    Only the model.yml geometry is built (filter_length 2048, window 1200, hann, center, replicate); any hop."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window="hann", center=True, pad_mode="replicate", cfg=None, engine=None):
        super().__init__()
        if (filter_length, win_length, window, center, pad_mode) != (2048, 1200, "hann", True, "replicate"):
            raise NotImplementedError("the HIP conv-form STFT is built for filter_length 2048, win_length 1200, hann, center, replicate (model.yml)")
        self.filter_length, self.hop_length, self.win_length, self.n_fft = filter_length, hop_length, win_length, filter_length
        self.freq_bins = filter_length // 2 + 1
        self._engine = engine
        self._cfg = cfg

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine

    def transform(self, waveform: torch.Tensor):
        """waveform [B, T] -> magnitude, x, y [B, 1025, T // hop + 1] (stft.py:98-139), any T like the reference.
        A tail shorter than a hop: the reference pads by REPLICATION, so extending the waveform to the next multiple of the hop with copies of its
        last sample leaves every frame it produces unchanged and appends one frame, which is dropped."""
        eng, hop = self.engine, self.hop_length
        B, T = waveform.shape
        F = T // hop + 1
        wave = _f(waveform, eng.device)
        if T % hop:
            wave = torch.cat([wave, wave[:, -1:].expand(B, hop - T % hop)], dim=1)
        Fk = wave.shape[1] // hop + 1
        seg = Segments([Fk] * B, eng.device)
        mag, x, y = eng.conv_stft_transform(seg, wave.reshape(-1).contiguous(), hop)
        return tuple(eng.to_channel_major(v, B, self.freq_bins, Fk)[:, :, :F].contiguous() for v in (mag, x, y))

    def inverse(self, magnitude: torch.Tensor, x: torch.Tensor, y: torch.Tensor, length=None):
        """[B, 1025, F] x 3 -> waveform [B, 1, (F - 1) * hop] (stft.py:141-187)."""
        eng, hop = self.engine, self.hop_length
        B, _, F = magnitude.shape
        seg = Segments([F] * B, eng.device)
        tmaj = [eng.to_time_major(_f(v, eng.device), 1056) for v in (magnitude, x, y)]
        wave = eng.conv_stft_inverse(seg, *tmaj, hop).reshape(B, 1, (F - 1) * hop)
        return wave if length is None else wave[..., :length]


class LogMelSpectrogram(torch.nn.Module):
    """The reference's mel front end on the engine: ``torchaudio.transforms.MelSpectrogram(n_mels, n_fft, win_length, hop_length, sample_rate)`` at its
    defaults followed by ``(log(1e-5 + mel) - mean) / std`` - calculate_mel (train/stage_type.py:1023-1032) with frames="even", preprocess
    (train/dataprep/align_text.py:112-117) with frames="drop_last" - plus log_norm's energy curve and compute_log_mel_stats (train/utils.py:71-148).
    Audio in at ``sample_rate`` (``Resample`` converts another rate); ragged batches through ``lengths`` [B] samples, every utterance getting what it gets
    alone, bit for bit.  Only torchaudio's defaults are built: HTK scale, norm None, power 2, f_min 0, f_max sample_rate / 2."""

    def __init__(self, n_mels, n_fft, win_length, hop_length, sample_rate, mean=-4.0, std=4.0, frames="even", engine=None, cfg=None):
        from . import log_mel

        super().__init__()
        log_mel.check_geometry(n_fft, win_length, hop_length, n_mels, sample_rate)
        log_mel.frames(n_fft, hop_length, frames)  # ValueError for an unknown policy
        self.n_mels, self.n_fft, self.win_length, self.hop_length, self.sample_rate = int(n_mels), int(n_fft), int(win_length), int(hop_length), int(sample_rate)
        self.mean, self.std, self.frames = float(mean), float(std), frames
        self._engine = engine
        self._cfg = cfg

    @classmethod
    def from_config(cls, cfg, n_mels=None, **kw):
        """The front end of a model config: its n_fft / win_length / hop_length / sample_rate, ``cfg.n_mels`` mel bins unless given (the text
        aligner's is 80)."""
        return cls(cfg.n_mels if n_mels is None else n_mels, cfg.n_fft, cfg.win_length, cfg.hop_length, cfg.sample_rate, cfg=cfg, **kw)

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine

    def _geom(self):
        return self.n_fft, self.win_length, self.hop_length, self.n_mels, self.sample_rate

    def _lengths(self, wave, lengths):
        if wave.dim() != 2:
            raise ValueError(f"audio must be [B, samples], got shape {tuple(wave.shape)}")
        B, S = wave.shape
        L = [S] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != B or any(n > S for n in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {S} samples")
        return L

    def frame_counts(self, lengths, frames=None):
        """Frames of utterances of ``lengths`` samples (host arithmetic only); ValueError for a length the transform refuses."""
        from . import log_mel

        return log_mel.frame_counts(lengths, self.n_fft, self.hop_length, self.frames if frames is None else frames)

    def _run(self, wave, lengths, frames=None, mean=None, std=None, **kw):
        L = self._lengths(wave, lengths)
        self.frame_counts(L, frames)  # ValueError before any device work
        eng = self.engine
        wd = _f(wave, eng.device)
        flat = torch.cat([wd[b, : L[b]] for b in range(len(L))]).contiguous()
        return eng.log_mel(Segments(L, eng.device), flat, *self._geom(), mean=self.mean if mean is None else mean, std=self.std if std is None else std,
                           frames=self.frames if frames is None else frames, **kw)

    def packed(self, wave, lengths=None, **kw):
        """wave [B, samples] -> (normalised log-mel rows [sum frames, n_mels] packed time-major on the device, their Segments): what
        ``HipModel.mel_style`` / ``HipModel.text_aligner`` read.  Keywords: frames / mean / std override the constructor's; ld, out, energy, raw as
        ``HipModel.log_mel``.  The host reads nothing back."""
        return self._run(wave, lengths, **kw)

    def forward(self, wave, lengths=None):
        """wave [B, samples] -> (mel [B, n_mels, T_max], mel_length [B]), zero padded past each length (calculate_mel's return for a dense batch)."""
        rows, seg = self._run(wave, lengths)
        out = rows.new_zeros((seg.n, seg.max_len, self.n_mels))
        for b in range(seg.n):
            out[b, : seg.lengths[b]] = rows[seg.host[b] : seg.host[b + 1]]
        return out.transpose(1, 2).contiguous(), torch.tensor(seg.lengths, dtype=torch.long, device=rows.device)

    def energy(self, wave, lengths=None, packed: bool = False):
        """log_norm(mel, mean, std) of the normalised mel (train/utils.py:71-77) = sum_m (1e-5 + mel)^0.33: energy [B, T_max] zero padded, or with
        packed=True (rows [sum frames], Segments)."""
        _, seg, en = self._run(wave, lengths, mel=False, energy=True)
        if packed:
            return en, seg
        out = en.new_zeros((seg.n, seg.max_len))
        for b in range(seg.n):
            out[b, : seg.lengths[b]] = en[seg.host[b] : seg.host[b + 1]]
        return out

    def stats(self, waves, return_partials: bool = False):
        """compute_log_mel_stats (train/utils.py:80-148) over a list of 1-D recordings at ``sample_rate`` (or a dense [B, samples] batch):
        (mean, std, count) of log(1e-5 + mel) over every frame, reduced on the device in a fixed order."""
        from . import log_mel

        ws = [w for w in waves] if not (isinstance(waves, torch.Tensor) and waves.dim() == 1) else [waves]
        if not ws or any(w.dim() != 1 for w in ws):
            raise ValueError("stats takes a list of 1-D recordings or a [B, samples] batch")
        L = [int(w.numel()) for w in ws]
        log_mel.frame_counts(L, self.n_fft, self.hop_length, "all")
        eng = self.engine
        flat = torch.cat([_f(w, eng.device) for w in ws]).contiguous()
        return eng.log_mel_stats(Segments(L, eng.device), flat, *self._geom(), return_partials=return_partials)


# ------------------------------------------------------------------------------------------------ validation scores (csrc/val_scores.hip.h)
def _wave_batch(x, lengths=None):
    """[B, samples] / [B, 1, samples] / a list of 1-D recordings (+ lengths [B]) -> (list of 1-D tensors cut to their lengths, their lengths)."""
    if isinstance(x, (list, tuple)):
        ws = [torch.as_tensor(w).reshape(-1) for w in x]
    else:
        x = torch.as_tensor(x)
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError(f"audio must be [B, samples], [B, 1, samples] or a list of 1-D recordings, got shape {tuple(x.shape)}")
        ws = [x[b] for b in range(x.shape[0])]
    if lengths is not None:
        L = [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != len(ws) or any(n > w.numel() for n, w in zip(L, ws)):
            raise ValueError(f"lengths {L} do not fit {len(ws)} recordings of {[int(w.numel()) for w in ws]} samples")
        ws = [w[:n] for w, n in zip(ws, L)]
    return ws, [int(w.numel()) for w in ws]


def _pack_waves(eng: HipModel, ws):
    return torch.cat([_f(w, eng.device) for w in ws]).contiguous()


def mel_score(sums):
    """sums [R, B, 2] (HipModel.mel_sums, on the host) -> (mel, [mel_r], [mel_utt]): per resolution sum_u numerators / (sum_u denominators + 1e-6)
    - MultiResolutionSTFTLoss' number for an equal-length batch - and their mean; per utterance the same of its own sums.  Plain float64
    arithmetic in a fixed order."""
    R, B = len(sums), len(sums[0])
    mel_r = []
    for r in range(R):
        num = den = 0.0
        for u in range(B):
            num += float(sums[r][u][0])
            den += float(sums[r][u][1])
        mel_r.append(num / (den + 1e-6))
    mel_utt = []
    for u in range(B):
        s = 0.0
        for r in range(R):
            s += float(sums[r][u][0]) / (float(sums[r][u][1]) + 1e-6)
        mel_utt.append(s / R)
    return sum(mel_r) / R, mel_r, mel_utt


def magphase_score(sums, rows: int, n_bins: int):
    """sums [B, 4] (HipModel.magphase_sums, on the host), the batch's rows and bins -> (mag, phase, the three phase terms): the means over every
    (utterance, bin, frame) and, for "phase", the sum of the three."""
    tot = [0.0] * 4
    for u in range(len(sums)):
        for c in range(4):
            tot[c] += float(sums[u][c])
    count = float(rows) * float(n_bins)
    terms = [tot[1] / count, tot[2] / count, tot[3] / count]
    return tot[0] / count, (terms[0] + terms[1]) + terms[2], terms


class _SpectrogramList(list):
    """A list MultiSpectrogram.forward returned.  It remembers the audio it came from and its tensors as they were, so that MultiResolutionSTFTLoss
    can score an untouched pair of lists on the fused path (fp64 from the samples to the sums) instead of from these fp32 tensors."""

    source = None
    stamp = None

    def untouched(self) -> bool:
        return self.stamp is not None and self.stamp == [(id(t), t._version) for t in self]


class MultiSpectrogram(torch.nn.Module):
    """train/multi_spectrogram.py:25-81 on the engine, same constructor and forward: per resolution the log1p mel spectrogram, the masked phase and
    the magnitude of torch.stft (periodic Hann).  ``forward`` runs the resolutions given to the constructor (the reference's forward reads the
    module-level list, which is the constructor's default).  Only the Hann window is built; MelScale at torchaudio's defaults with 128 mels."""

    def __init__(self, resolutions=None, window=torch.hann_window, *, sample_rate, engine=None, cfg=None):
        from . import val_scores

        super().__init__()
        if window is not torch.hann_window:
            raise NotImplementedError("the HIP MultiSpectrogram is built for torch.hann_window")
        self.resolutions = [val_scores.as_tuple(r) for r in (val_scores.resolutions if resolutions is None else resolutions)]
        self.sample_rate, self.n_mels = int(sample_rate), val_scores.N_MELS
        for fft, hop, window_length in self.resolutions:
            val_scores.check_geometry(fft, window_length, hop, self.n_mels, self.sample_rate)
        self._engine = engine
        self._cfg = cfg

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine

    def calculate_single(self, audio, index, item=None):
        """audio [B, samples] -> (mag [B, 1, 128, F], phase [B, n_bins, F], fft_mag [B, 1, n_bins, F]) at resolution ``index``."""
        fft, hop, window_length = self.resolutions[index]
        ws, L = _wave_batch(audio)
        if len(set(L)) != 1:
            raise ValueError("MultiSpectrogram takes an equal-length batch [B, samples], as the reference does (HipModel.multi_spectrogram runs ragged ones)")
        eng = self.engine
        seg = Segments(L, eng.device)
        seg_m, mag, phase, fft_mag = eng.multi_spectrogram(seg, _pack_waves(eng, ws), fft, window_length, hop, self.n_mels, self.sample_rate, mag=True, phase=True,
                                                           fft_mag=True)
        B, F, nb = seg.n, seg_m.lengths[0], fft // 2 + 1
        return (eng.to_channel_major(mag, B, self.n_mels, F).unsqueeze(1), eng.to_channel_major(phase, B, nb, F),
                eng.to_channel_major(fft_mag, B, nb, F).unsqueeze(1))

    def forward(self, *, target, pred):
        out = [_SpectrogramList() for _ in range(6)]
        for index in range(len(self.resolutions)):
            t = self.calculate_single(target, index)
            p = self.calculate_single(pred, index)
            for dst, v in zip(out, (t[0], p[0], t[1], p[1], t[2], p[2])):
                dst.append(v)
        out[0].source = out[1].source = dict(target=target, pred=pred, resolutions=self.resolutions, sample_rate=self.sample_rate, n_mels=self.n_mels,
                                             engine=self.engine)
        for lst in out[:2]:
            lst.stamp = [(id(t), t._version) for t in lst]
        return tuple(out)


class MultiResolutionSTFTLoss(torch.nn.Module):
    """train/losses.py:14-35: mean over the resolutions of ||t - p||_1 / (||t||_1 + 1e-6), logged as "mel".  Two forms, and which one runs shows in
    ``last_path``:
      "fused"    ``target_list`` / ``pred_list`` are the two lists of ONE MultiSpectrogram.forward call, as it returned them (same tensors, none
                 edited in place since): the score is formed on the engine from the audio behind them (HipModel.mel_sums: fp64 from the samples to
                 the sums, what pipeline.validation_scores reports), not from their fp32 tensors;
      "tensors"  any other lists of tensors - sliced, copied, edited, built elsewhere: the reference's own arithmetic on the tensors given, summed in
                 float64 by torch on their device.  It differs from the fused number by the tensors' rounding to fp32 (a few 1e-8 of the score)."""

    def __init__(self, *, sample_rate):
        super().__init__()
        self.sample_rate = int(sample_rate)
        self.last_path = None

    def spectral_convergence_loss(self, target, pred):
        t, p = torch.as_tensor(target).double(), torch.as_tensor(pred).double()
        return (t - p).abs().sum() / (t.abs().sum() + 1e-6)

    def forward(self, *, target_list, pred_list, log):
        src = getattr(target_list, "source", None)
        if src is not None and getattr(pred_list, "source", None) is src and target_list.untouched() and pred_list.untouched():
            eng = src["engine"]
            tw, L = _wave_batch(src["target"])
            pw, Lp = _wave_batch(src["pred"])
            sums = eng.mel_sums(Segments(L, eng.device), _pack_waves(eng, tw), _pack_waves(eng, pw), src["resolutions"], src["n_mels"], src["sample_rate"],
                                seg_pred=Segments(Lp, eng.device))
            loss = torch.tensor(mel_score(sums.cpu().tolist())[0], dtype=torch.float64)
            self.last_path = "fused"
        else:
            if len(target_list) != len(pred_list) or len(target_list) == 0:
                raise ValueError(f"{len(target_list)} target spectrograms, {len(pred_list)} predictions")
            loss = sum(self.spectral_convergence_loss(t, p) for t, p in zip(target_list, pred_list)) / len(target_list)
            self.last_path = "tensors"
        log.add_loss("mel", loss)
        return loss


def _magphase_sums(eng: HipModel, gt_waves, L, logamp_rows, phase_rows, seg_rows, n_fft, win, hop):
    """MagPhaseLoss' sums [B, 4] (float64, on the device) from packed prediction rows; nothing is read back."""
    return eng.magphase_sums(Segments(L, eng.device), _pack_waves(eng, gt_waves), seg_rows, logamp_rows, phase_rows, logamp_rows.shape[1], n_fft, win, hop)


class MagPhaseLoss(torch.nn.Module):
    """train/losses.py:85-154 on the engine, same constructor and forward: ``pred`` has .magnitude (log-magnitude) and .phase [B, n_bins, F], ``gt``
    is the recording [B, samples] with F = samples // (hop_length // 4) + 1; logs "mag" and "phase".  Unlike the reference, which overwrites
    ``pred.phase`` with its masked copy, this leaves ``pred`` as it was."""

    def __init__(self, *, n_fft, hop_length, win_length, engine=None, cfg=None):
        from . import val_scores

        super().__init__()
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length) // 4, int(win_length)
        val_scores.check_geometry(self.n_fft, self.win_length, self.hop_length)
        self._engine = engine
        self._cfg = cfg

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine

    def sums(self, pred, gt):
        """(sums [B, 4] float64 on the device, the batch's rows): HipModel.magphase_sums of the prediction; nothing is read back."""
        from . import val_scores

        ws, L = _wave_batch(gt)
        mg, ph = torch.as_tensor(pred.magnitude), torch.as_tensor(pred.phase)
        nb = self.n_fft // 2 + 1
        if mg.dim() != 3 or mg.shape != ph.shape or mg.shape[0] != len(L) or mg.shape[1] != nb:
            raise ValueError(f"pred.magnitude / pred.phase must be [{len(L)}, {nb}, frames], got {tuple(mg.shape)} / {tuple(ph.shape)}")
        val_scores.frame_counts(L, self.n_fft, self.hop_length)
        val_scores.check_rows(L, [mg.shape[2]] * len(L), self.hop_length)
        eng = self.engine
        la, pr = eng.to_time_major(_f(mg, eng.device)), eng.to_time_major(_f(ph, eng.device))
        seg_rows = Segments([mg.shape[2]] * len(L), eng.device)
        return _magphase_sums(eng, ws, L, la, pr, seg_rows, self.n_fft, self.win_length, self.hop_length), seg_rows.rows

    def scores(self, pred, gt):
        """(mag, phase, [instantaneous, frequency, time]) as Python floats; one host read."""
        sums, rows = self.sums(pred, gt)
        return magphase_score(sums.cpu().tolist(), rows, self.n_fft // 2 + 1)

    def forward(self, pred, gt, log):
        mag, phase, _ = self.scores(pred, gt)
        log.add_loss("mag", torch.tensor(mag, dtype=torch.float64))
        log.add_loss("phase", torch.tensor(phase, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ alignment, duration and CFM scores
class _EngineUser(torch.nn.Module):
    def __init__(self, engine=None, cfg=None):
        super().__init__()
        self._engine, self._cfg = engine, cfg

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine


def duration_score(sums, lengths):
    """sums [B, 3] (HipModel.duration_sums, on the host), token counts [B] -> (duration_ce, duration, [ce_utt], [cdw_utt]): CDW_CCELoss' two values
    of every utterance, ce_u = -s0 / (s1 + 1e-9) and cdw_u = -100 s2 / P_u, and DurationLoss.forward's means over the utterances."""
    ce = [-float(s[0]) / (float(s[1]) + 1e-9) for s in sums]
    cdw = [-100.0 * float(s[2]) / float(n) for s, n in zip(sums, lengths)]
    return sum(ce) / len(ce), sum(cdw) / len(cdw), ce, cdw


class CDW_CCELoss(_EngineUser):
    """train/losses.py:429-459 on the engine: forward(pred [N, C], target [N]) -> (-ce.sum(), -100 cdw.sum()) of one utterance as fp32 tensors,
    from the fp64 sums of HipModel.duration_sums.  The distance weights are built for ``alpha`` = 2 (what DurationLoss constructs); another
    alpha raises.  ``weight=None`` raises ValueError in forward (the reference calls exit(1) there)."""

    def __init__(self, classes, *, alpha=1.0, weight=None, engine=None, cfg=None):
        super().__init__(engine, cfg)
        self.classes, self.alpha = int(classes), float(alpha)
        self.custom_weight = None if weight is None else torch.as_tensor(weight).detach().to(torch.float32).reshape(-1)
        if self.custom_weight is not None and self.custom_weight.numel() != self.classes:
            raise ValueError(f"{self.custom_weight.numel()} class weights for {self.classes} classes")

    def sums(self, pred, target, lengths=None):
        """pred [sum P, C] packed rows, target [sum P], lengths [B] (default: one utterance) -> [B, 3] float64 on the device; nothing is read back."""
        if self.custom_weight is None:
            raise ValueError("CDW_CCELoss needs class weights (weight=None is the branch in which the reference exits)")
        if self.alpha != 2.0:
            raise NotImplementedError(f"CDW_CCELoss: the engine builds the distance weights of alpha = 2, not {self.alpha}")
        pred = torch.as_tensor(pred)
        if pred.dim() != 2 or pred.shape[1] != self.classes:
            raise ValueError(f"pred must be [N, {self.classes}], got {tuple(pred.shape)}")
        eng = self.engine
        L = [pred.shape[0]] if lengths is None else [int(v) for v in lengths]
        return eng.duration_sums(Segments(L, eng.device), pred, torch.as_tensor(target).reshape(-1), self.custom_weight)

    def forward(self, pred, target):
        s = self.sums(pred, target)[0]
        n = torch.as_tensor(pred).shape[0]
        return (-s[0] / (s[1] + 1e-9)).to(torch.float32), (-100.0 * s[2] / n).to(torch.float32)


class DurationLoss(_EngineUser):
    """train/losses.py:462-476 on the engine: forward(pred [B, P, C] logits, gt [B, P] duration classes, text_length [B]) -> (loss_ce, loss_cdw),
    the means over the utterances of CDW_CCELoss(alpha = 2) on every utterance's own tokens; one launch for the batch."""

    def __init__(self, *, class_count, weight, engine=None, cfg=None):
        super().__init__(engine, cfg)
        self.loss = CDW_CCELoss(class_count, alpha=2, weight=weight, engine=engine, cfg=cfg)

    def sums(self, pred, gt, text_length):
        """(sums [B, 3] float64 on the device, the token counts); nothing is read back beyond text_length."""
        pred, gt = torch.as_tensor(pred), torch.as_tensor(gt)
        L = [int(v) for v in torch.as_tensor(text_length).tolist()]
        if pred.dim() != 3 or gt.dim() != 2 or pred.shape[0] != len(L) or gt.shape[0] != len(L) or any(n < 1 or n > pred.shape[1] or n > gt.shape[1] for n in L):
            raise ValueError(f"pred {tuple(pred.shape)} / gt {tuple(gt.shape)} do not fit text lengths {L}")
        self.loss._engine = self.loss._engine or self.engine
        rows = torch.cat([pred[b, : L[b]] for b in range(len(L))])
        tg = torch.cat([gt[b, : L[b]] for b in range(len(L))]).long()
        return self.loss.sums(rows, tg, L), L

    def scores(self, pred, gt, text_length):
        """dict(duration_ce, duration, duration_ce_utt, duration_utt) as Python numbers; one host read."""
        s, L = self.sums(pred, gt, text_length)
        ce, cdw, ce_u, cdw_u = duration_score(s.cpu().tolist(), L)
        return dict(duration_ce=ce, duration=cdw, duration_ce_utt=ce_u, duration_utt=cdw_u)

    def forward(self, pred, gt, text_length):
        s, L = self.sums(pred, gt, text_length)
        n = torch.tensor(L, dtype=torch.float64, device=s.device)
        ce, cdw = -s[:, 0] / (s[:, 1] + 1e-9), -100.0 * s[:, 2] / n
        return ce.mean().to(torch.float32), cdw.mean().to(torch.float32)


def align_loss_value(nll_utt, frame_lengths, token_lengths, loss=None):
    """CTCLossWithLabelPriors.forward's reduction on the host, from per-utterance float64 values: fp32 roundings of the values, then
    ``loss.reduction`` ("mean" without a loss: the mean of float32(nll_u) / P_u) and ``loss.reference_pairing``, in fp32 like the tensor form."""
    reduction = "mean" if loss is None else loss.reduction
    v = np.asarray(nll_utt, np.float64).astype(np.float32)
    if loss is not None and loss.reference_pairing:
        v = v[sorted(range(len(v)), key=lambda i: -int(frame_lengths[i]))]
    if reduction == "none":
        return [float(x) for x in v]
    if reduction == "sum":
        return float(torch.from_numpy(v).sum())
    return float((torch.from_numpy(v) / torch.tensor([float(n) for n in token_lengths], dtype=torch.float32)).mean())


class CTCLossWithLabelPriors(_EngineUser):
    """train/losses.py:508-639 on the engine: the CTC loss of log_probs [T, N, C] (already log-softmaxed) against padded targets [N, P], with the
    label priors of the "train" step accumulated and applied as the reference does.  Two stated deviations: (1) the likelihood is exact - k2
    prunes its lattice with output_beam = 10; (2) the reference hands k2 a batch sorted by frame count but the UNSORTED target_lengths, so its
    "mean" divides an utterance's likelihood by another utterance's token count unless the batch was sorted already (read from the code, k2 not
    run); here every utterance is paired with its own length, and ``reference_pairing=True`` reproduces the reference's pairing (stable
    descending sort by frame count) from the per-utterance values.  on_train_epoch_end() takes no accelerator: one process."""

    prior_threshold = -12.0

    def __init__(self, prior_scaling_factor=0.0, blank=0, reduction="mean", engine=None, cfg=None, reference_pairing=False):
        super().__init__(engine, cfg)
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        self.blank, self.reduction, self.reference_pairing = int(blank), reduction, bool(reference_pairing)
        self.log_priors = None      # [1, 1, C] float64 on the device, like the reference's shape
        self.log_priors_sum = None  # [1, C]
        self.num_samples = 0
        self.prior_scaling_factor = prior_scaling_factor

    def _pack(self, log_probs, targets, input_lengths, target_lengths):
        log_probs, targets = torch.as_tensor(log_probs), torch.as_tensor(targets)
        TL = [int(v) for v in torch.as_tensor(input_lengths).tolist()]
        PL = [int(v) for v in torch.as_tensor(target_lengths).tolist()]
        if log_probs.dim() != 3 or targets.dim() != 2 or not (log_probs.shape[1] == targets.shape[0] == len(TL) == len(PL)):
            raise ValueError(f"log_probs {tuple(log_probs.shape)} [T, N, C] and targets {tuple(targets.shape)} [N, P] do not fit {len(TL)} / {len(PL)} lengths")
        if any(n < 1 or n > log_probs.shape[0] for n in TL) or any(n < 1 or n > targets.shape[1] for n in PL):
            raise ValueError(f"input_lengths {TL} / target_lengths {PL} do not fit {log_probs.shape[0]} frames and {targets.shape[1]} tokens")
        eng = self.engine
        lp = _f(log_probs, eng.device)
        rows = torch.cat([lp[: TL[b], b] for b in range(len(TL))]).contiguous()
        tg = torch.cat([targets[b, : PL[b]] for b in range(len(PL))]).to(device=eng.device, dtype=torch.int32)
        return rows, tg, Segments(TL, eng.device), Segments(PL, eng.device)

    def nll(self, log_probs, targets, input_lengths, target_lengths, step_type="train"):
        """The per-utterance negative log-likelihoods [N] float64 on the device (+inf where no path exists).  step_type "train" accumulates the
        label priors of this batch and applies the current ones, as forward does."""
        rows, tg, seg_t, seg_p = self._pack(log_probs, targets, input_lengths, target_lengths)
        eng = self.engine
        priors = None
        if step_type == "train":
            batch = eng.ctc_prior_sums(seg_t, rows)[None]  # [1, C]
            self.num_samples += seg_t.rows
            self.log_priors_sum = batch if self.log_priors_sum is None else torch.logaddexp(self.log_priors_sum, batch)
            if self.log_priors is not None and self.prior_scaling_factor > 0:
                priors = self.log_priors
        return eng.ctc_nll(seg_t, rows, seg_p, tg, self.blank, log_priors=priors, prior_scale=float(self.prior_scaling_factor) if priors is not None else 0.0)

    def forward(self, log_probs, targets, input_lengths, target_lengths, step_type="train"):
        nll = self.nll(log_probs, targets, input_lengths, target_lengths, step_type).to(torch.float32)
        TL = [int(v) for v in torch.as_tensor(input_lengths).tolist()]
        P = torch.as_tensor(target_lengths).to(device=nll.device, dtype=torch.float32)
        if self.reference_pairing:  # the reference's order of the values: sorted by frame count, longest first, ties in batch order
            order = sorted(range(len(TL)), key=lambda i: -TL[i])
            nll = nll[torch.tensor(order, device=nll.device)]
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        return (nll / P).mean()

    def on_train_epoch_end(self, train=None):
        if self.log_priors_sum is not None:
            new = self.log_priors_sum[None] - math.log(self.num_samples + 1e-9)
            self.log_priors = torch.clamp(new, min=self.prior_threshold)
            self.log_priors_sum = None
            self.num_samples = 0


class Resample(torch.nn.Module):
    """``torchaudio.transforms.Resample`` on the engine, same constructor: windowed-sinc conversion from ``orig_freq`` to ``new_freq``
    ("sinc_interp_hann" or "sinc_interp_kaiser").  The target is torchaudio's float64 result: the coefficients stay fp64 on the device, so the fp32
    roundings torchaudio applies to them are not reproduced (resample.py, csrc/resample.hip.h).  Ragged batches through ``lengths``: every utterance
    gets what it gets alone, bit for bit.  Equal rates return the input's values."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = "sinc_interp_hann", lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, beta: Optional[float] = None, engine=None, cfg=None):
        from . import resample

        super().__init__()
        self.o, self.n, self.width, self.taps, _, _ = resample.check(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta = resampling_method, int(lowpass_filter_width), float(rolloff), beta
        self._engine = engine
        self._cfg = cfg

    @property
    def engine(self) -> HipModel:
        if self._engine is None:
            self._engine = get_engine(self._cfg, 0)
        return self._engine

    def out_lengths(self, lengths):
        """Output sample counts ceil(n * samples / o) of utterances of ``lengths`` samples (host arithmetic only)."""
        from . import resample

        return resample.out_lengths(lengths, self.orig_freq, self.new_freq)

    def _lengths(self, wave, lengths):
        if wave.dim() != 2:
            raise ValueError(f"audio must be [B, samples], got shape {tuple(wave.shape)}")
        B, S = wave.shape
        L = [S] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(L) != B or any(n > S for n in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {S} samples")
        self.out_lengths(L)  # ValueError for an utterance without a sample, before any device work
        return L

    def packed_rows(self, flat, seg: Segments):
        """Packed samples [sum samples] with their Segments -> (packed samples at new_freq, their Segments), on the device."""
        return self.engine.resample(seg, flat, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method, self.beta)

    def packed(self, waveform, lengths=None):
        """waveform [B, samples] -> (packed samples at new_freq [sum ceil(n samples / o)] on the device, their Segments).  The host reads nothing back."""
        L = self._lengths(waveform, lengths)
        eng = self.engine
        wd = _f(waveform, eng.device)
        flat = torch.cat([wd[b, : L[b]] for b in range(len(L))]).contiguous()
        return self.packed_rows(flat, Segments(L, eng.device))

    def forward(self, waveform, lengths=None):
        """waveform [..., time] -> [..., ceil(n time / o)], as torchaudio gives it; with ``lengths`` [...] every utterance is converted on its own
        and the samples past its output length are zero."""
        shape = tuple(waveform.shape)
        if len(shape) < 1:
            raise ValueError("audio must have a time axis")
        rows, seg = self.packed(waveform.reshape(-1, shape[-1]), lengths)
        if lengths is None:
            return rows.reshape(shape[:-1] + (seg.lengths[0],))
        from . import resample

        out = rows.new_zeros((seg.n, resample.out_length(shape[-1], self.orig_freq, self.new_freq)))
        for b in range(seg.n):
            out[b, : seg.lengths[b]] = rows[seg.host[b] : seg.host[b + 1]]
        return out.reshape(shape[:-1] + (out.shape[1],))


class ExportModel(torch.nn.Module):
    """models/export_model.py:5-45: the inference composition (B = 1 in the reference: '1 1 l -> l')."""

    def __init__(self, *, speech_predictor, duration_predictor=None, pitch_energy_predictor, pe_text_encoder, pe_text_style_encoder, device=None,
                 **kwargs):
        super().__init__()
        self.speech_predictor, self.pitch_energy_predictor = speech_predictor, pitch_energy_predictor
        self.pe_text_encoder, self.pe_text_style_encoder = pe_text_encoder, pe_text_style_encoder

    def forward(self, texts, text_lengths, alignment, noise=None):
        pe_text_encoding, _, _ = self.pe_text_encoder(texts, text_lengths)
        pe_text_style = self.pe_text_style_encoder(pe_text_encoding, text_lengths)
        pitch, energy = self.pitch_energy_predictor(pe_text_encoding, text_lengths, alignment, pe_text_style)
        prediction = self.speech_predictor(texts, text_lengths, alignment, pitch, energy, noise=noise)
        assert prediction.audio.shape[0] == 1, "ExportModel.forward returns a single waveform (export_model.py:44)"
        return prediction.audio.reshape(-1)


def _hubert_cfg(cfg, hubert_dim: int, spk_dim: int):
    c2 = Record(cfg)
    c2["hubert"] = Record(dict(cfg.get("hubert") or {}, hidden_dim=hubert_dim))
    c2["speaker_embedder"] = Record(dict(cfg.get("speaker_embedder") or {}, hidden_dim=spk_dim))
    hubert_dims(c2)
    return c2


def _pack_curve(x: torch.Tensor, L, dev) -> torch.Tensor:
    x = _f(torch.as_tensor(x), dev)
    return torch.cat([x[b, : L[b]] for b in range(len(L))]).contiguous()


def _unpack_curve(x: torch.Tensor, seg: Segments, P: int, equal: bool):
    if equal:
        return x.reshape(seg.n, P)
    return [x[seg.host[b] : seg.host[b + 1]] for b in range(seg.n)]


def _check_feats(cfg, phones: torch.Tensor, spk_emb: torch.Tensor, hubert_dim: int, spk_dim: int):
    if phones.dim() != 3:
        raise ValueError(f"HuBERT features must be [B, {hubert_dim}, T], got shape {tuple(phones.shape)}")
    check_width("HuBERT features", phones.shape[1], "hubert.hidden_dim", hubert_dim)
    if spk_emb.dim() != 2:
        raise ValueError(f"speaker embeddings must be [B, {spk_dim}], got shape {tuple(spk_emb.shape)}")
    check_width("speaker embedding", spk_emb.shape[1], "speaker_embedder.hidden_dim", spk_dim)
    if spk_emb.shape[0] != phones.shape[0]:
        raise ValueError(f"{spk_emb.shape[0]} speaker embeddings for {phones.shape[0]} utterances")


class HubertPitchEnergyPredictor(HipModule):
    """models/pitch_energy_predictor.py:124-191: HuBERT features [B, hubert_dim, T] + speaker embedding [B, spk_dim] -> F0, N [B, T]
    (ragged lengths: lists of [T_b]).  Statistics per utterance over its own frames (the reference at B = 1)."""

    module_name, components = "hubert_pitch_energy_predictor", W_HUBERT_PE

    def __init__(self, hubert_dim, spk_dim, style_dim, inter_dim, style_config, pitch_energy_config, cfg=None, engine=None):
        cfg = _hubert_cfg(cfg or load_model_config(), hubert_dim, spk_dim)
        if style_dim != cfg.style_dim or inter_dim != cfg.inter_dim:
            raise ValueError(f"style_dim / inter_dim ({style_dim}, {inter_dim}) must be the model config's ({cfg.style_dim}, {cfg.inter_dim})")
        super().__init__(params.hubert_pitch_energy_predictor_spec(cfg), cfg, engine)
        self.hubert_dim, self.spk_dim = int(hubert_dim), int(spk_dim)

    def forward(self, phones, phone_lengths, spk_emb):
        _check_feats(self.cfg, phones, spk_emb, self.hubert_dim, self.spk_dim)
        eng = self.engine
        L = [int(v) for v in torch.as_tensor(phone_lengths).tolist()]
        seg = Segments(L, eng.device)
        _, pe_style = eng.speaker_style(_f(spk_emb, eng.device), style=False)
        f0, en = eng.hubert_pitch_energy(seg, _pack_rows(eng, phones, L), pe_style)
        equal = len(set(L)) == 1 and L[0] == phones.shape[2]
        return _unpack_curve(f0, seg, L[0], equal), _unpack_curve(en, seg, L[0], equal)


class HubertSpeechPredictor(HipModule):
    """models/speech_predictor.py:132-251 (inference: audio_gt=None).  The phone_encoder and style_encoder are this module's own
    component (W_HUBERT); its decoder, prior_encoder, flow, post_flow and generator run on the engine's frame path, whose weights are
    re-bound from this module whenever another shim (SpeechPredictor, Decoder, Generator) packed them last."""

    module_name, components = "hubert_speech_predictor", W_DECODER | W_FLOW | W_GENERATOR | W_HUBERT
    _OWN = ("phone_encoder.", "style_encoder.")

    def __init__(self, model_config=None, engine=None):
        cfg = model_config if model_config is not None else load_model_config()
        self.hubert_dim, self.spk_dim = hubert_dims(cfg)
        super().__init__(params.hubert_speech_predictor_spec(cfg), cfg, engine)

    def _load_into(self, eng: HipModel):
        own = OrderedDict((k, v) for k, v in self._store.items() if k.startswith(self._OWN))
        frame = OrderedDict((k, v) for k, v in self._store.items() if not k.startswith(self._OWN))
        eng.load_state_dict(self.module_name, own)
        eng.load_state_dict("speech_predictor", frame)  # the names the frame path is packed from (include/stylish_hip.h, STTS_W_DECODER..)

    def forward(self, phones, phone_lengths, spk_emb, pitch, energy, audio_gt=None, noise=None):
        if audio_gt is not None:
            raise NotImplementedError("audio_gt (posterior encoder, training only: speech_predictor.py:225-232) is outside the inference hot path")
        _check_feats(self.cfg, phones, spk_emb, self.hubert_dim, self.spk_dim)
        eng = self.engine
        L = [int(v) for v in torch.as_tensor(phone_lengths).tolist()]
        B = len(L)
        st = Segments(L, eng.device)
        st4 = st.scaled(4)
        asr = eng.hubert_encoder(st, _pack_rows(eng, phones, L))
        style, _ = eng.speaker_style(_f(spk_emb, eng.device), pe_style=False)
        p4, e4 = eng.upsample4(st, st4, _pack_curve(pitch, L, eng.device)), eng.upsample4(st, st4, _pack_curve(energy, L, eng.device))
        h, nb = self.cfg.hop_length // 4, self.cfg.n_fft // 2 + 1
        nz = noise or draw_noise(B, 4 * max(L), eng.device, flow_dim=self.cfg.decoder.hidden_dim // 4, h=h)
        pn = _f(torch.as_tensor(nz["prior_noise"]), eng.device)
        sn = _f(torch.as_tensor(nz["src_noise"]), eng.device)
        pn_tm = torch.cat([pn[b, :, : 4 * L[b]].t() for b in range(B)]).contiguous()
        sn_flat = torch.cat([sn[b, 0, : 4 * h * L[b]] for b in range(B)]).contiguous()
        ip = _f(torch.as_tensor(nz["init_phase"]), eng.device).reshape(-1)
        x = eng.decoder(st4, asr, p4, e4, style)
        mel = eng.prior_flow(st4, x, style, pn_tm)
        spec, phase = eng.harmonic_stft(st4, p4, sn_flat, ip, batch_scope=True)
        audio, la, ph = eng.vocoder(st4, mel, style, spec, phase, return_spec=True)
        eng.check_status()
        if len(set(L)) == 1 and L[0] == phones.shape[2]:
            T4 = 4 * L[0]
            rep = lambda t: torch.cat([t, t[:, :, -1:]], dim=2)  # noqa: E731
            return DecoderPrediction(audio=audio.reshape(B, 1, h * T4), magnitude=rep(eng.to_channel_major(la, B, nb, T4)),
                                     phase=rep(eng.to_channel_major(ph, B, nb, T4)))
        return DecoderPrediction(audio=[audio[h * st4.host[b] : h * st4.host[b + 1]] for b in range(B)], magnitude=None, phase=None)


def mel_style_levels(n_mels: int, skip_downsamples: bool):
    """(number of "half" downsamplings, the shortest mel the encoder takes).  The reference needs n_mels to halve exactly at every level
    (an odd F gives mismatched shortcut / residual shapes) and 5 x 5 positions left for shared.6 (models/mel_style_encoder.py:139)."""
    n_down = 3 if skip_downsamples else 4
    if n_mels % (1 << n_down) or (n_mels >> n_down) < 5:
        raise ValueError(f"MelStyleEncoder: n_mels = {n_mels} must be a multiple of {1 << n_down} and at least {5 << n_down}")
    t_min = 1
    while True:
        t = t_min
        for _ in range(n_down):
            t = (t + 1) // 2
        if t >= 5:
            return n_down, t_min
        t_min += 1


def mel_style_tap_shapes(dim_in: int, max_conv_dim: int, skip_downsamples: bool, lengths):
    """[(rows, ld, cout, F, per-utterance T)] of the four ResBlk taps of stts_mel_style_forward_taps (channels-last, ld = cout padded to 16)."""
    out, c, F, T = [], dim_in, dim_in, [int(x) for x in lengths]
    for i in range(4):
        co = min(2 * c, max_conv_dim)
        if not (i == 3 and skip_downsamples):
            F, T = F // 2, [(t + 1) // 2 for t in T]
        out.append((F * sum(T), (co + 15) // 16 * 16, co, F, T))
        c = co
    return out


class MelStyleEncoder(HipModule):
    """models/mel_style_encoder.py:120-151: x [B, 1, n_mels, T] -> style [B, style_dim].  ``lengths`` (optional, [B] mel frames) runs a
    ragged batch: each utterance gets what the reference gives it alone; without it the batch is dense and equals the reference on it.
    The engine slot is ``component``: "pe_mel_style_encoder" (models/models.py:57-62) or "cfm_pitch_predictor.spk_emb"
    (models/cfm/cfm_pitch_predictor.py:25-27); the dims come from the weights."""

    _SLOTS = {"pe_mel_style_encoder": ("pe_mel_style_encoder", "", W_PE_MEL_STYLE),
              "cfm_pitch_predictor.spk_emb": ("cfm_pitch_predictor", "spk_emb.", W_CFM_PITCH)}

    def __init__(self, dim_in=48, style_dim=48, max_conv_dim=384, skip_downsamples=False, cfg=None, engine=None, component="pe_mel_style_encoder"):
        if component not in self._SLOTS:
            raise ValueError(f"component must be one of {sorted(self._SLOTS)}")
        self.module_name, self.key_prefix, self.components = self._SLOTS[component]
        self.dim_in, self.style_dim, self.max_conv_dim, self.skip_downsamples = int(dim_in), int(style_dim), int(max_conv_dim), bool(skip_downsamples)
        self.n_down, self.min_frames = mel_style_levels(self.dim_in, self.skip_downsamples)
        super().__init__(params.mel_style_encoder_spec(self.dim_in, self.style_dim, self.max_conv_dim, self.skip_downsamples), cfg or load_model_config(), engine)

    def _load_into(self, eng: HipModel):
        eng.load_state_dict(self.module_name, self._store, prefix=self.key_prefix)

    def _lengths(self, x, lengths):
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.dim_in:
            raise ValueError(f"MelStyleEncoder input must be [B, 1, {self.dim_in}, T], got shape {tuple(x.shape)}")
        B, T = x.shape[0], x.shape[3]
        L = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != B or any(t < 1 or t > T for t in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {T} frames")
        return L

    def forward(self, x, lengths=None):
        return self.run(x, lengths)[0]

    def from_audio(self, wave, lengths, mel_stats, front: Optional["LogMelSpectrogram"] = None):
        """wave [B, samples] at the model's sample rate (lengths [B] samples, or None) -> style [B, style_dim]: the ``dim_in``-mel front end of the
        model config (LogMelSpectrogram.from_config, frames="even"; ``front`` to give another) normalised by mel_stats = (mean, std), its packed
        rows handed to the encoder as they are.  Equals forward() on LogMelSpectrogram.forward's output, bit for bit; no host read in between."""
        if front is None:
            front = LogMelSpectrogram.from_config(self.cfg, self.dim_in, mean=mel_stats[0], std=mel_stats[1])
        if front.n_mels != self.dim_in:
            raise ValueError(f"the front end has {front.n_mels} mel bins, the encoder takes {self.dim_in}")
        eng = self.engine
        front._engine = eng
        rows, seg = front.packed(wave, lengths, mean=mel_stats[0], std=mel_stats[1])
        return eng.mel_style(self.components, seg, rows, self.style_dim)

    def run(self, x, lengths=None, taps: bool = False):
        """(style, taps or None); taps = the four ResBlk outputs as lists of per-utterance [cout, F, T] tensors."""
        L = self._lengths(x, lengths)
        eng = self.engine
        seg = Segments(L, eng.device)
        xd = _f(x, eng.device)[:, 0]  # [B, F, T]
        mel = torch.cat([xd[b, :, : L[b]].t() for b in range(len(L))]).contiguous()  # packed time-major rows [sum T, n_mels]
        if not taps:
            return eng.mel_style(self.components, seg, mel, self.style_dim), None
        shapes = mel_style_tap_shapes(self.dim_in, self.max_conv_dim, self.skip_downsamples, L)
        style, flat = eng.mel_style(self.components, seg, mel, self.style_dim, tap_floats=sum(r * ld for r, ld, *_ in shapes))
        out, o = [], 0
        for rows, ld, co, F, T in shapes:
            blk = flat[o : o + rows * ld].view(rows, ld)[:, :co]
            o += rows * ld
            per, r0 = [], 0
            for t in T:
                per.append(blk[r0 : r0 + t * F].reshape(t, F, co).permute(2, 1, 0))
                r0 += t * F
            out.append(per)
        return style, out


def norm_f0_zscore(f0, uv, log_f0_mean, log_f0_std):
    """train/stage_type.py:783-798 for numpy arrays and torch tensors: (log2(f0 + 1e-8) - mean) / std, 0 where uv > 0."""
    is_torch = isinstance(f0, torch.Tensor)
    log_f0 = torch.log2(f0 + 1e-8) if is_torch else np.log2(f0 + 1e-8)
    normed = (log_f0 - log_f0_mean) / log_f0_std
    if uv is not None:
        normed[uv > 0] = 0
    return normed


def denorm_f0_zscore(normed_f0, uv, log_f0_mean, log_f0_std, min_hz=50, max_hz=1200):
    """train/stage_type.py:801-829 for numpy arrays and torch tensors: clamp(2^(x * std + mean), min_hz, max_hz), 0 where uv > 0.
    log_f0_mean / log_f0_std are the training set's log2 F0 statistics (train/train_context.py:209-214), not part of a checkpoint."""
    f0 = 2 ** (normed_f0 * log_f0_std + log_f0_mean)
    f0 = f0.clamp(min=min_hz, max=max_hz) if isinstance(f0, torch.Tensor) else np.clip(f0, a_min=min_hz, a_max=max_hz)
    if uv is not None:
        f0[uv > 0] = 0
    return f0


class CfmPitchPredictor(HipModule):
    """models/cfm/cfm_pitch_predictor.py:12-51: forward(asr [B, asr_dim, T], mel [B, n_mels, Tm]) -> normed F0 [B, 1, T].  The speaker
    branch (spk_emb, a MelStyleEncoder) is engine component STTS_W_CFM_PITCH, the frame-rate network STTS_W_CFM_PITCH_NET; both load from
    the reference's full state dict (in_proj is kept and ignored, as forward ignores it).  ``asr_lengths`` / ``mel_lengths`` (optional,
    [B]) run a ragged batch: each utterance gets what the reference gives it alone, frames past asr_lengths[b] are 0; without them
    the batch is dense and equals the reference on it."""

    module_name = "cfm_pitch_predictor"
    components = W_CFM_PITCH | W_CFM_PITCH_NET
    hidden = 256

    def __init__(self, asr_dim=768, n_mels=80, cfg=None, engine=None):
        self.asr_dim, self.n_mels = int(asr_dim), int(n_mels)
        self.min_mel_frames = mel_style_levels(self.n_mels, True)[1]
        super().__init__(params.cfm_pitch_predictor_spec(self.asr_dim, self.n_mels), cfg or load_model_config(), engine)

    def _load_into(self, eng: HipModel):
        eng.load_state_dict(self.module_name, self._store)

    def _lengths(self, asr, mel, asr_lengths, mel_lengths):
        if asr.dim() != 3 or asr.shape[1] != self.asr_dim:
            raise ValueError(f"CfmPitchPredictor asr must be [B, {self.asr_dim}, T], got shape {tuple(asr.shape)}")
        if mel.dim() != 3 or mel.shape[1] != self.n_mels or mel.shape[0] != asr.shape[0]:
            raise ValueError(f"CfmPitchPredictor mel must be [{asr.shape[0]}, {self.n_mels}, Tm], got shape {tuple(mel.shape)}")
        B, T, Tm = asr.shape[0], asr.shape[2], mel.shape[2]
        La = [T] * B if asr_lengths is None else [int(v) for v in torch.as_tensor(asr_lengths).tolist()]
        Lm = [Tm] * B if mel_lengths is None else [int(v) for v in torch.as_tensor(mel_lengths).tolist()]
        if len(La) != B or any(t < 1 or t > T for t in La):
            raise ValueError(f"asr_lengths {La} do not fit a batch of {B} x {T} frames")
        if len(Lm) != B or any(t < 1 or t > Tm for t in Lm):
            raise ValueError(f"mel_lengths {Lm} do not fit a batch of {B} x {Tm} frames")
        return La, Lm  # (mels below min_mel_frames are the engine's to reject, as for MelStyleEncoder)

    def forward(self, asr, mel, asr_lengths=None, mel_lengths=None):
        return self.run(asr, mel, asr_lengths, mel_lengths)[0]

    def speaker_style(self, mel, mel_rows_lengths):
        """spk_emb(mel) [B, 256] from packed inputs: (mel [B, n_mels, Tm], lengths)."""
        eng = self.engine
        sm = Segments(mel_rows_lengths, eng.device)
        md = _f(mel, eng.device)
        rows = torch.cat([md[b, :, : mel_rows_lengths[b]].t() for b in range(len(mel_rows_lengths))]).contiguous()
        return eng.mel_style(W_CFM_PITCH, sm, rows, self.hidden)

    def run(self, asr, mel, asr_lengths=None, mel_lengths=None, f0_log2_stats=None, uv=None, taps: bool = False):
        """(normed [B, 1, T], hz [B, 1, T] or None, taps or None).  f0_log2_stats = (log2 mean, log2 std) also gives
        denorm_f0_zscore(normed, uv, mean, std) from the same launch (uv [B, T] or [B, 1, T], > 0 = unvoiced); taps = the asr_emb
        output and the four block outputs as lists of per-utterance [256, T_b] tensors."""
        La, Lm = self._lengths(asr, mel, asr_lengths, mel_lengths)
        eng = self.engine
        dev = eng.device
        B, T = asr.shape[0], asr.shape[2]
        spk = self.speaker_style(mel, Lm)
        sa = Segments(La, dev)
        rows = _pack_rows(eng, asr, La)
        uv_rows = None
        if uv is not None:
            u = torch.as_tensor(uv).to(dev, torch.float32).reshape(B, T)
            uv_rows = torch.cat([u[b, : La[b]] for b in range(B)]).contiguous()
        res = eng.cfm_pitch(sa, rows, spk, f0_log2_stats=f0_log2_stats, uv=uv_rows, taps=taps)
        res = res if isinstance(res, tuple) else (res,)

        def dense(x):
            out = torch.zeros(B, 1, T, dtype=torch.float32, device=dev)
            for b in range(B):
                out[b, 0, : La[b]] = x[sa.host[b] : sa.host[b + 1]]
            return out

        normed = dense(res[0])
        hz = dense(res[1]) if f0_log2_stats is not None else None
        tp = None
        if taps:
            t = res[-1]
            tp = [[t[k, sa.host[b] : sa.host[b + 1]].t() for b in range(B)] for k in range(5)]
        return normed, hz, tp


class AdaptiveHubert(HipModule):
    """train/models/ssl.py:16-31: wave [B, samples] at ``hubert_sr`` -> HuBERT features [B, hidden, time_dim] (last_hidden_state resampled to
    time_dim frames by F.interpolate's nearest rule).  ``hubert_path``: a LOCAL directory with config.json and model.safetensors (or
    pytorch_model.bin); nothing is ever downloaded.  Without it ``config`` (HubertConfig fields, hubert_ssl.arch) shapes the network and
    load_state_dict takes the reference's keys (``model.*``; masked_spec_embed and final_proj.* are stored and unused).
    ``lengths`` (optional, [B] samples) runs a ragged batch: each utterance gets what the reference gives it alone (the reference's own
    padded batch lets GroupNorm, the positional conv and the attention see the padding); without it the batch is dense and equals the
    reference on it.  The reference resamples model_sr -> hubert_sr first; this shim takes audio that already is at hubert_sr unless
    ``sample_rate`` names another rate (``sample_rate=self.model_sr``: the reference's own forward), which is converted on the engine."""

    module_name = "hubert"
    components = W_SSL

    def __init__(self, hubert_path=None, model_sr: int = 24000, hubert_sr: int = 16000, config=None, cfg=None, engine=None):
        from . import hubert_ssl

        sd = None
        if hubert_path is not None:
            import json
            import os

            with open(os.path.join(hubert_path, "config.json"), "r", encoding="utf-8") as f:
                config = json.load(f)
            st = os.path.join(hubert_path, "model.safetensors")
            if os.path.exists(st):
                from safetensors.torch import load_file

                sd = load_file(st)
            else:
                sd = torch.load(os.path.join(hubert_path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        self.arch = hubert_ssl.arch(config)
        self.model_sr, self.sr = int(model_sr), int(hubert_sr)
        self.hidden = self.arch["hidden_size"]
        super().__init__(params.hubert_ssl_spec(self.arch), cfg or load_model_config(), engine)
        if sd is not None:
            self.load_state_dict({(k if k.startswith("model.") else "model." + k): v for k, v in sd.items()}, strict=False)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # older checkpoints spell the positional conv's weight norm weight_g / weight_v
        q = "model.encoder.pos_conv_embed.conv."
        sd = dict(state_dict)
        if q + "weight_g" in sd:
            sd[q + "parametrizations.weight.original0"] = sd.pop(q + "weight_g")
            sd[q + "parametrizations.weight.original1"] = sd.pop(q + "weight_v")
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _bind(self):
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        if self._dirty or owners.get(W_SSL) is not self:
            self._load_into(eng)
            eng.ssl_finalize(self.arch)
            owners[W_SSL] = self
            self._dirty = False

    def frames(self, samples: int) -> int:
        from . import hubert_ssl

        return hubert_ssl.frames(samples, self.arch)

    def _lengths(self, wave, lengths, sample_rate=None):
        """Sample counts at the rate of ``wave`` and at hubert_sr (the same list without a resampling)."""
        if wave.dim() != 2:
            raise ValueError(f"AdaptiveHubert input must be [B, samples], got shape {tuple(wave.shape)}")
        B, S = wave.shape
        L = [S] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != B or any(n < 1 or n > S for n in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {S} samples")
        Lr = L
        if sample_rate is not None and int(sample_rate) != self.sr:
            from . import resample

            resample.check(sample_rate, self.sr)
            Lr = resample.out_lengths(L, sample_rate, self.sr)
        for n in Lr:
            self.frames(n)  # ValueError below the receptive field, where the reference raises
        return L, Lr

    def packed(self, wave, time_dims, lengths=None, taps: bool = False, sample_rate: Optional[int] = None):
        """Packed rows [sum time_dims, ld] (the ``feats`` of the engine's HuBERT stages) for per-utterance ``time_dims``.  sample_rate: the rate of
        ``wave`` where it is not hubert_sr - ``Resample(sample_rate, hubert_sr)`` at torchaudio's defaults runs first, on the device, and the
        receptive-field check applies to the resampled length."""
        L, Lr = self._lengths(wave, lengths, sample_rate)
        T = [int(t) for t in time_dims]
        if len(T) != len(L) or min(T) < 1:
            raise ValueError(f"time_dim {T} must be one positive frame count per utterance")
        eng = self.engine
        wd = _f(wave, eng.device)
        flat = torch.cat([wd[b, : L[b]] for b in range(len(L))]).contiguous()
        seg = Segments(L, eng.device)
        if Lr is not L:
            flat, seg = eng.resample(seg, flat, int(sample_rate), self.sr)
        return eng.hubert_ssl(seg, flat, Segments(T, eng.device), taps=taps)

    def forward(self, wave, time_dim, lengths=None, sample_rate: Optional[int] = None):
        """sample_rate=None: ``wave`` is at hubert_sr.  sample_rate=self.model_sr is the reference's own forward (resample, then the network)."""
        B, T = wave.shape[0], int(time_dim)
        rows = self.packed(wave, [T] * B, lengths, sample_rate=sample_rate)
        return rows[:, : self.hidden].reshape(B, T, self.hidden).permute(0, 2, 1).contiguous()


class WavLM(HipModule):
    """transformers' WavLMModel in eval mode on the engine (csrc/wavlm.hip.h): ``config`` holds WavLMConfig fields (wavlm.arch; the base model when
    None), load_state_dict takes ``WavLMModel.state_dict()`` keys (masked_spec_embed is stored and unused).  ``model_path``: a LOCAL directory with
    config.json and model.safetensors (or pytorch_model.bin); nothing is ever downloaded and no pretrained weights ship with the engine.
    Audio is mono at 16 kHz.  ``lengths`` runs a ragged batch in which every utterance gets what it gets alone, bit for bit (the reference's
    padded batch would let GroupNorm, the positional conv and the attention see the padding).  Forward values only: no gradients."""

    module_name = "wavlm"
    components = W_WAVLM
    sr = 16000

    def __init__(self, config=None, engine=None, cfg=None, model_path=None):
        from . import wavlm

        sd = None
        if model_path is not None:
            import json
            import os

            with open(os.path.join(model_path, "config.json"), "r", encoding="utf-8") as f:
                config = json.load(f)
            st = os.path.join(model_path, "model.safetensors")
            if os.path.exists(st):
                from safetensors.torch import load_file

                sd = load_file(st)
            else:
                sd = torch.load(os.path.join(model_path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        self.arch = wavlm.arch(config)
        self.hidden = self.arch["hidden_size"]
        self.n_states = self.arch["num_hidden_layers"] + 1
        super().__init__(params.wavlm_spec(self.arch), cfg or load_model_config(), engine)
        if sd is not None:
            self.load_state_dict({(k[len("wavlm."):] if k.startswith("wavlm.") else k): v for k, v in sd.items()}, strict=False)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # older checkpoints spell the positional conv's weight norm weight_g / weight_v
        q = "encoder.pos_conv_embed.conv."
        sd = dict(state_dict)
        if q + "weight_g" in sd:
            sd[q + "parametrizations.weight.original0"] = sd.pop(q + "weight_g")
            sd[q + "parametrizations.weight.original1"] = sd.pop(q + "weight_v")
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _bind(self):
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        if self._dirty or owners.get(W_WAVLM) is not self:
            self._load_into(eng)
            eng.wavlm_finalize(self.arch)
            owners[W_WAVLM] = self
            self._dirty = False

    def frames(self, samples: int) -> int:
        from . import wavlm

        return wavlm.frames(samples, self.arch)

    def _pack(self, wave, lengths):
        """(packed samples on the device, their Segments) of wave [B, samples] or a list of 1-D waveforms."""
        eng = self.engine
        if isinstance(wave, (list, tuple)):
            ws = [_f(torch.as_tensor(w).reshape(-1), eng.device) for w in wave]
            L = [int(w.numel()) for w in ws] if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
            if len(L) != len(ws) or any(n < 1 or n > w.numel() for n, w in zip(L, ws)):
                raise ValueError(f"lengths {L} do not fit the {len(ws)} waveforms given")
            flat = torch.cat([w[:n] for w, n in zip(ws, L)]).contiguous()
        else:
            w = torch.as_tensor(wave)
            if w.dim() == 3 and w.shape[1] == 1:
                w = w[:, 0]
            if w.dim() != 2:
                raise ValueError(f"WavLM input must be [B, samples] or [B, 1, samples], got shape {tuple(w.shape)}")
            B, S = w.shape
            L = [S] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
            if len(L) != B or any(n < 1 or n > S for n in L):
                raise ValueError(f"lengths {L} do not fit a batch of {B} x {S} samples")
            wd = _f(w, eng.device)
            flat = wd.reshape(-1) if lengths is None else torch.cat([wd[b, : L[b]] for b in range(B)]).contiguous()
        return flat, Segments(L, eng.device)

    def hidden_states(self, wave, lengths=None, gate: bool = False):
        """wave [B, samples] (or [B, 1, samples], or a list) at 16 kHz -> a tuple of num_hidden_layers + 1 packed tensors [sum frames, hidden]:
        transformers' ``hidden_states`` (state 0 is the encoder LayerNorm's output), utterance after utterance."""
        flat, seg = self._pack(wave, lengths)
        for n in seg.lengths:
            self.frames(n)  # ValueError below the receptive field, where the reference raises
        res = self.engine.wavlm_states(seg, flat, gate=gate)
        states = res[0] if gate else res
        tup = tuple(states[k] for k in range(states.shape[0]))
        return (tup, res[1]) if gate else tup

    def forward(self, wave, lengths=None):
        """last_hidden_state as [B, frames, hidden] for a dense batch."""
        last = self.hidden_states(wave, lengths)[-1]
        B = len(wave) if isinstance(wave, (list, tuple)) else torch.as_tensor(wave).shape[0]
        if last.shape[0] % B or lengths is not None:
            raise ValueError("forward() returns a dense [B, frames, hidden]: use hidden_states() for a ragged batch")
        return last.reshape(B, -1, self.hidden)


class WavLMLoss(torch.nn.Module):
    """train/losses.py:408-426 on the engine, same constructor shape: ``model`` is a modules.WavLM (or a LOCAL checkpoint directory; nothing is
    downloaded), ``forward(wav, y_rec)`` resamples both from ``model_sr`` to ``slm_sr`` (Resample at torchaudio's defaults: Hann, width 6), runs
    both through WavLM and returns the mean absolute difference over all hidden states as a 0-d float64 tensor - what the stages log as "slm".
    Inputs: [B, L], [B, 1, L], or lists of 1-D waveforms; ``lengths`` [B] for ragged batches, where every utterance is its own run and the mean is
    over real frames only (the reference would run the padding through the network).  The value is
    sum of all sums / (states * total frames * hidden); forward value only, no gradients.  The two waveforms of a pair run as utterances u and
    u + B of one call; no hidden state leaves the device, and ``sums`` does not read anything back."""

    def __init__(self, model, model_sr, slm_sr: int = 16000, engine=None):
        super().__init__()
        self.wavlm = model if isinstance(model, WavLM) else WavLM(model_path=model, engine=engine)
        if int(slm_sr) != self.wavlm.sr:
            raise ValueError(f"WavLM takes audio at {self.wavlm.sr} Hz, got slm_sr = {slm_sr}")
        self.model_sr, self.slm_sr = int(model_sr), int(slm_sr)
        self.resample = None if self.model_sr == self.slm_sr else Resample(self.model_sr, self.slm_sr, engine=self.wavlm._engine, cfg=self.wavlm.cfg)

    def sums(self, wav, y_rec, lengths=None):
        """(sums [B, states] float64, frames [B] int32) on the device; nothing is read back."""
        m = self.wavlm
        a, sa = m._pack(wav, lengths)
        b, sb = m._pack(y_rec, lengths)
        if sa.lengths != sb.lengths:
            raise ValueError(f"the recordings have {sa.lengths} samples, the synthesised waveforms {sb.lengths}: a pair must have one length")
        eng = m.engine
        if self.resample is not None:
            self.resample._engine = eng
            a, sa = self.resample.packed_rows(a, sa)
            b, sb = self.resample.packed_rows(b, sb)
        for n in sa.lengths:
            m.frames(n)  # ValueError below the receptive field
        return eng.wavlm_l1(Segments(sa.lengths + sb.lengths, eng.device), torch.cat([a, b]))

    def scores(self, wav, y_rec, lengths=None):
        """(slm, [per-utterance slm]) as Python floats; one host read."""
        from . import wavlm

        sums, fr = self.sums(wav, y_rec, lengths)
        both = torch.cat([sums, fr.to(torch.float64)[:, None]], dim=1).cpu().tolist()
        return wavlm.score([r[:-1] for r in both], [int(r[-1]) for r in both], self.wavlm.hidden)

    def forward(self, wav, y_rec, lengths=None):
        return torch.tensor(self.scores(wav, y_rec, lengths)[0], dtype=torch.float64)


class RmvpePitchExtractor(HipModule):
    """The reference's RMVPE pitch extractor (train/dataprep/rmvpe/inference.py:12-65) on the engine: ``E2E0`` in eval mode, ``mel2hidden``'s
    per-utterance reflect padding to a multiple of 32 frames, ``to_local_average_f0`` and the log-mel front end.  ``config``: E2E0's constructor
    arguments (rmvpe.dims: n_blocks, inter_layers, en_out_channels; anything else the reference's extractor fixes raises ValueError).
    load_state_dict takes E2E0's keys (``num_batches_tracked`` accepted and ignored).  ``mel_basis`` [128, 513] is a buffer the caller may set
    (the reference takes it from its audio library); the default is rmvpe.default_mel_basis().  ``lengths`` / ``sample_lengths`` run ragged
    batches in which every utterance gets what it gets alone.  Outputs past an utterance's length are 0."""

    module_name = "rmvpe"
    components = W_RMVPE
    sr = 16000

    def __init__(self, config=None, engine=None, cfg=None):
        from . import rmvpe

        self.dims = rmvpe.dims(config)
        super().__init__(params.rmvpe_spec(self.dims), cfg or load_model_config(), engine)
        self._basis_dev = None
        self.mel_basis = torch.from_numpy(rmvpe.default_mel_basis())
        self.thred = 0.03  # the voicing threshold of calls that do not name one (VoiceConverter.convert_audio)

    @property
    def mel_basis(self) -> torch.Tensor:
        return self._mel_basis

    @mel_basis.setter
    def mel_basis(self, value):
        from . import rmvpe

        b = torch.as_tensor(value).detach().to("cpu", torch.float32).contiguous()
        self._band = torch.from_numpy(rmvpe.basis_band(b.numpy()))  # ValueError for another shape
        self._mel_basis = b
        self._basis_dev = None

    @classmethod
    def from_safetensors(cls, path, config=None, engine=None):
        """The reference's checkpoint format: one .safetensors file of E2E0's state_dict."""
        from safetensors import safe_open

        sd = {}
        with safe_open(path, framework="pt", device="cpu") as f:
            for k in f.keys():
                sd[k] = f.get_tensor(k)
        m = cls(config, engine)
        m.load_state_dict(sd)
        return m

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = dict(state_dict)
        for k in self._store:  # a BatchNorm's step counter plays no part in eval mode: absent or present, any value
            if k.endswith(".num_batches_tracked"):
                sd[k] = torch.zeros(())
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _load_into(self, eng: HipModel):
        eng.load_state_dict(self.module_name, {k: v for k, v in self._store.items() if not k.endswith(".num_batches_tracked")})

    def _bind(self):
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        if self._dirty or owners.get(W_RMVPE) is not self:
            self._load_into(eng)
            eng.rmvpe_finalize(self.dims)
            owners[W_RMVPE] = self
            self._dirty = False

    # ---- shapes
    def _mel_lengths(self, mel, lengths):
        from . import rmvpe

        if mel.dim() != 3 or mel.shape[1] != rmvpe.N_MELS:
            raise ValueError(f"RMVPE input must be a log-mel [B, {rmvpe.N_MELS}, T], got shape {tuple(mel.shape)}")
        B, T = mel.shape[0], mel.shape[2]
        L = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != B or any(n > T for n in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {T} frames")
        for n in L:
            rmvpe.padded_frames(n)  # ValueError below 17 frames, where the reference's reflect padding raises
        return L

    def _frames(self, frames, B):
        if frames is None:
            return None
        Fr = [int(frames)] * B if isinstance(frames, int) else [int(v) for v in torch.as_tensor(frames).tolist()]
        if len(Fr) != B or min(Fr) < 1:
            raise ValueError(f"frames {Fr} must be one positive frame count per utterance")
        return Fr

    @staticmethod
    def _unpack(rows, seg: Segments):
        """packed [rows, ...] -> [B, max length, ...], zeros past every utterance's length"""
        out = rows.new_zeros((seg.n, seg.max_len) + tuple(rows.shape[1:]))
        for b in range(seg.n):
            out[b, : seg.lengths[b]] = rows[seg.host[b] : seg.host[b + 1]]
        return out

    def _pack_mel(self, mel, L):
        md = _f(mel, self.engine.device)
        return torch.cat([md[b, :, : L[b]].t() for b in range(len(L))]).contiguous()

    # ---- the reference's methods
    def mel2hidden(self, mel, lengths=None):
        """mel [B, 128, T] -> salience [B, T, 360]."""
        L = self._mel_lengths(mel, lengths)
        eng = self.engine
        seg = Segments(L, eng.device)
        h, _ = eng.rmvpe(seg, self._pack_mel(mel, L), f0=False)
        return self._unpack(h, seg)

    DECODERS = ("argmax", "viterbi")

    @classmethod
    def _decoder(cls, decoder: str, use_viterbi: bool = False) -> bool:
        """True for decoder="viterbi".  The reference's own flag, use_viterbi=True, stays refused: it promises librosa's decoder, whose floating point
        is not pinned here; the engine's exact Viterbi decode of the same objective is asked for by its own name, decoder="viterbi"."""
        if use_viterbi:
            raise NotImplementedError('use_viterbi=True (the reference\'s librosa decoder, bit parity unpinned) is not built; decoder="viterbi" is the '
                                      "engine's exact Viterbi decode of the same objective")
        if decoder not in cls.DECODERS:
            raise ValueError(f"decoder must be one of {cls.DECODERS}, got {decoder!r}")
        return decoder == "viterbi"

    def decode(self, hidden, thred: float = 0.03, use_viterbi: bool = False, decoder: str = "argmax", lengths=None, return_path: bool = False):
        """salience [B, T, 360] (or [T, 360]) -> f0 [B, T] in Hz, 0 on unvoiced frames.  decoder="viterbi": the objective of the reference's
        to_viterbi_f0 solved exactly - the local average around the best path through the 360 classes (HipModel.rmvpe_viterbi), every utterance on its
        own ``lengths`` frames (default: all T), zeros past them; return_path=True also returns the path [B, T] int32.  use_viterbi=True raises
        NotImplementedError as before (_decoder)."""
        viterbi = self._decoder(decoder, use_viterbi)
        if hidden.dim() not in (2, 3) or hidden.shape[-1] != 360 or hidden.shape[-2] < 1:
            raise ValueError(f"salience must be [B, T, 360], got shape {tuple(hidden.shape)}")
        if not viterbi:
            if lengths is not None or return_path:
                raise ValueError('lengths and return_path belong to decoder="viterbi"')
            eng = self.engine
            h = _f(hidden, eng.device)
            return eng.rmvpe_decode(h.reshape(-1, 360), thred).reshape(h.shape[:-1])
        B, T = (1, hidden.shape[0]) if hidden.dim() == 2 else hidden.shape[:2]
        L = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        if len(L) != B or any(n < 1 or n > T for n in L):
            raise ValueError(f"lengths {L} do not fit a batch of {B} x {T} frames (at least one frame each)")
        eng = self.engine
        h = _f(hidden, eng.device).reshape(B, T, 360)
        seg = Segments(L, eng.device)
        rows = h.reshape(-1, 360) if all(n == T for n in L) else torch.cat([h[b, : L[b]] for b in range(B)])
        f0, path = eng.rmvpe_viterbi(seg, rows, thred, path=True)
        f0, path = self._unpack(f0, seg), self._unpack(path, seg)
        if hidden.dim() == 2:
            f0, path = f0[0], path[0]
        return (f0, path) if return_path else f0

    def _viterbi_f0(self, seg: Segments, mel_rows, thred):
        """The network's salience and the Viterbi decode at its 100 frames / s."""
        eng = self.engine
        h, _ = eng.rmvpe(seg, mel_rows, thred, f0=False)
        return eng.rmvpe_viterbi(seg, h, thred)

    def packed(self, mel, lengths=None, frames=None, thred: float = 0.03, return_segments: bool = False, decoder: str = "argmax"):
        """Packed f0 rows [sum frames] on the device (100 frames / s, or resampled to ``frames`` per utterance), as the engine's stages take curves.
        decoder="viterbi": the Viterbi decode of the salience (before any resampling)."""
        use_viterbi = self._decoder(decoder)
        L = self._mel_lengths(mel, lengths)
        Fr = self._frames(frames, len(L))
        eng = self.engine
        seg = Segments(L, eng.device)
        if use_viterbi:
            f0 = self._viterbi_f0(seg, self._pack_mel(mel, L), thred)
        else:
            _, f0 = eng.rmvpe(seg, self._pack_mel(mel, L), thred, hidden=False)
        if Fr is not None:
            seg_o = Segments(Fr, eng.device)
            f0, seg = eng.rmvpe_resample(seg, f0, seg_o), seg_o
        return (f0, seg) if return_segments else f0

    def forward(self, mel, lengths=None, frames=None, thred: float = 0.03, decoder: str = "argmax"):
        """mel [B, 128, T] -> f0 [B, T] (or [B, max frames] after the linear resampling to ``frames``)."""
        f0, seg = self.packed(mel, lengths, frames, thred, return_segments=True, decoder=decoder)
        return self._unpack(f0, seg)

    RESAMPLE_WIDTH = 128  # the lowpass_filter_width of the reference's resampler (inference.py:55-57)

    def _wave_lengths(self, wave, sample_lengths, sample_rate, resample: bool = False):
        """Sample counts at the rate of ``wave`` and at 16 kHz (the same list without a resampling); the length checks apply to the latter."""
        from . import rmvpe

        if int(sample_rate) != self.sr and not resample:
            raise ValueError(f"RMVPE takes audio at {self.sr} Hz, got {sample_rate} (pass resample=True to convert it on the engine, as the reference does)")
        if wave.dim() != 2:
            raise ValueError(f"RMVPE audio must be [B, samples], got shape {tuple(wave.shape)}")
        B, S = wave.shape
        L = [S] * B if sample_lengths is None else [int(v) for v in torch.as_tensor(sample_lengths).tolist()]
        if len(L) != B or any(n > S for n in L):
            raise ValueError(f"sample_lengths {L} do not fit a batch of {B} x {S} samples")
        Lr = L
        if int(sample_rate) != self.sr:
            from . import resample as rs

            rs.check(sample_rate, self.sr, self.RESAMPLE_WIDTH)
            Lr = rs.out_lengths(L, sample_rate, self.sr)
        for n in Lr:
            rmvpe.mel_frames(n)  # ValueError at 512 samples or fewer
        return L, Lr

    def mel_packed(self, wave, sample_lengths=None, sample_rate: int = 16000, linear: bool = False, resample: bool = False):
        """wave [B, samples] at 16 kHz -> packed log-mel rows [sum frames, 128] and their Segments (frames = samples // 160 + 1).  resample=True:
        ``wave`` is at ``sample_rate`` and the reference's Resample(sample_rate, 16000, lowpass_filter_width=128) runs first, on the device."""
        L, Lr = self._wave_lengths(wave, sample_lengths, sample_rate, resample)
        eng = self.engine
        if self._basis_dev is None or self._basis_dev[0].device != eng.device:
            self._basis_dev = (self._mel_basis.to(eng.device), self._band.to(eng.device))
        wd = _f(wave, eng.device)
        flat = torch.cat([wd[b, : L[b]] for b in range(len(L))]).contiguous()
        seg = Segments(L, eng.device)
        if Lr is not L:
            flat, seg = eng.resample(seg, flat, int(sample_rate), self.sr, self.RESAMPLE_WIDTH)
        return eng.rmvpe_mel(seg, flat, self._basis_dev[0], self._basis_dev[1], linear=linear)

    def mel(self, wave, sample_lengths=None, sample_rate: int = 16000, resample: bool = False):
        """wave [B, samples] -> log-mel [B, 128, max frames] (MelSpectrogram.forward, keyshift 0, speed 1, center=True)."""
        rows, seg = self.mel_packed(wave, sample_lengths, sample_rate, resample=resample)
        return self._unpack(rows, seg).transpose(1, 2).contiguous()

    def packed_from_audio(self, wave, sample_lengths=None, frames=None, thred: Optional[float] = None, sample_rate: int = 16000, return_segments: bool = False,
                          resample: bool = False, decoder: str = "argmax"):
        """Packed f0 rows [sum frames] on the device from audio [B, samples] at 16 kHz (resample=True: at ``sample_rate``, converted on the engine
        first); thred None: ``self.thred``.  decoder="viterbi": the Viterbi decode of the salience (before any resampling to ``frames``)."""
        from . import rmvpe

        use_viterbi = self._decoder(decoder)

        thred = self.thred if thred is None else thred

        for n in self._wave_lengths(wave, sample_lengths, sample_rate, resample)[1]:
            rmvpe.padded_frames(rmvpe.mel_frames(n))  # ValueError below 17 frames
        rows, seg = self.mel_packed(wave, sample_lengths, sample_rate, resample=resample)
        Fr = self._frames(frames, seg.n)
        eng = self.engine
        if use_viterbi:
            f0 = self._viterbi_f0(seg, rows, thred)
        else:
            _, f0 = eng.rmvpe(seg, rows, thred, hidden=False)
        if Fr is not None:
            seg_o = Segments(Fr, eng.device)
            f0, seg = eng.rmvpe_resample(seg, f0, seg_o), seg_o
        return (f0, seg) if return_segments else f0

    def infer_from_audio(self, wave16k, sample_lengths=None, frames=None, thred: float = 0.03, sample_rate: int = 16000, use_viterbi: bool = False,
                         resample: bool = False, decoder: str = "argmax"):
        """wave [B, samples] at 16 kHz -> f0 [B, T] (T = samples // 160 + 1, or ``frames`` after the linear resampling).  resample=True with another
        ``sample_rate`` is the reference's infer_from_audio: its width-128 resampler to 16 kHz runs first.  decoder="viterbi": the Viterbi decode;
        use_viterbi=True raises NotImplementedError as before (_decoder)."""
        self._decoder(decoder, use_viterbi)
        f0, seg = self.packed_from_audio(wave16k, sample_lengths, frames, thred, sample_rate, return_segments=True, resample=resample, decoder=decoder)
        return self._unpack(f0, seg)


class TextAligner(HipModule):
    """The reference's text aligner (train/models/text_aligner.py: ``tdnn_blstm_ctc_model``, ``CTCModel.forward`` in eval mode) and the forced
    alignment of train/dataprep/align_text.py (``torch_align``) on the engine.  Constructor: ``tdnn_blstm_ctc_model``'s arguments, with
    ``tdnn_blstm_ctc_model_base``'s spec as the default (``drop_out`` is the identity in eval mode); a spec the engine has no form for - a
    'blstm' entry, which the reference cannot build either - raises ValueError.  load_state_dict takes CTCModel's keys (``num_batches_tracked``
    accepted and ignored).  Always fp32.  Ragged batches: every utterance gets what it gets alone, bit for bit."""

    module_name = "text_aligner"
    components = W_ALIGNER

    def __init__(self, n_mels: int = 80, num_symbols: int = 178, hidden_dim: int = 640, drop_out: float = 0.1, tdnn_blstm_spec=None, engine=None, cfg=None):
        from . import aligner

        self.dims = aligner.dims(n_mels, num_symbols, hidden_dim, aligner.BASE_SPEC if tdnn_blstm_spec is None else tdnn_blstm_spec)
        self.n_mels, self.num_symbols, self.blank = self.dims["n_mels"], self.dims["num_symbols"], self.dims["num_symbols"]
        super().__init__(params.text_aligner_spec(self.dims), cfg or load_model_config(), engine)

    @classmethod
    def from_safetensors(cls, path, n_mels: int = 80, num_symbols: int = 178, engine=None):
        """The reference's alignment model file (dataset.alignment_model_path): one .safetensors file of CTCModel's state_dict."""
        from safetensors import safe_open

        sd = {}
        with safe_open(path, framework="pt", device="cpu") as f:
            for k in f.keys():
                sd[k] = f.get_tensor(k)
        m = cls(n_mels, num_symbols, engine=engine)
        m.load_state_dict(sd)
        return m

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = dict(state_dict)
        for k in self._store:  # a BatchNorm's step counter plays no part in eval mode: absent or present, any value
            if k.endswith(".num_batches_tracked"):
                sd[k] = torch.zeros(())
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _load_into(self, eng: HipModel):
        eng.load_state_dict(self.module_name, {k: v for k, v in self._store.items() if not k.endswith(".num_batches_tracked")})

    def _bind(self):
        eng = self._engine
        owners = eng.__dict__.setdefault("_owners", {})
        if self._dirty or owners.get(W_ALIGNER) is not self:
            self._load_into(eng)
            eng.aligner_finalize(self.dims)
            owners[W_ALIGNER] = self
            self._dirty = False

    def _lengths(self, sources, source_lengths):
        if sources.dim() != 3 or sources.shape[2] != self.n_mels:
            raise ValueError(f"aligner input must be [B, T, {self.n_mels}], got shape {tuple(sources.shape)}")
        B, T = sources.shape[0], sources.shape[1]
        L = [T] * B if source_lengths is None else [int(v) for v in torch.as_tensor(source_lengths).tolist()]
        if len(L) != B or any(n > T or n < 1 for n in L):
            raise ValueError(f"source_lengths {L} do not fit a batch of {B} x {T} frames")
        return L

    def packed(self, sources, source_lengths=None, taps: bool = False):
        """sources [B, T, n_mels] -> (packed log-prob rows [sum T, classes] on the device, their Segments[, taps])."""
        L = self._lengths(sources, source_lengths)
        eng = self.engine
        seg = Segments(L, eng.device)
        xd = _f(sources, eng.device)
        rows = torch.cat([xd[b, : L[b]] for b in range(len(L))]).contiguous()
        out = eng.text_aligner(seg, rows, taps=taps)
        return (out[0], seg, out[1]) if taps else (out, seg)

    def forward(self, sources, source_lengths):
        """CTCModel.forward: (ctc_log_prob [T, B, V + 1], None).  Rows past an utterance's length are 0 (the reference computes values from masked
        frames there that nothing reads)."""
        lp, seg = self.packed(sources, source_lengths)
        T = sources.shape[1]
        out = lp.new_zeros((T, seg.n, lp.shape[1]))
        for b in range(seg.n):
            out[: seg.lengths[b], b] = lp[seg.host[b] : seg.host[b + 1]]
        return out, None

    def _check_texts(self, L, texts, text_lengths):
        from . import aligner

        texts = torch.as_tensor(texts)
        PL = [int(v) for v in torch.as_tensor(text_lengths).tolist()]
        if texts.dim() != 2 or len(PL) != len(L) or any(n > texts.shape[1] for n in PL):
            raise ValueError(f"texts of shape {tuple(texts.shape)} with text_lengths {PL} do not fit {len(L)} utterances")
        toks = [[int(v) for v in texts[b, : PL[b]].tolist()] for b in range(len(L))]
        for b, tk in enumerate(toks):
            aligner.check_alignable(L[b], tk, f"utterance {b}")
            if any(not 0 <= v < self.num_symbols for v in tk):
                raise ValueError(f"utterance {b}: token ids must lie in [0, {self.num_symbols})")
        return toks, PL

    def _align_rows(self, lp, seg, toks, PL):
        eng = self.engine
        seg_p = Segments(PL, eng.device)
        tg = torch.tensor([v for tk in toks for v in tk], dtype=torch.int32, device=eng.device)
        r = eng.ctc_align(seg, lp, seg_p, tg, self.blank)
        stack = torch.stack([r["durations"].to(torch.float32), r["left"], r["right"]])
        return ([stack[:, seg_p.host[b] : seg_p.host[b + 1]] for b in range(seg.n)], [r["scores"][seg.host[b] : seg.host[b + 1]] for b in range(seg.n)])

    def align(self, mels, mel_lengths, texts, text_lengths):
        """calculate_alignments' core for a ragged batch (align_text.py:138-152): mels [B, T, n_mels] normalised log-mel, texts [B, P] token ids ->
        (list of [3, P] float tensors (pred_dur, left, right), list of per-frame path log-probs ``scores`` [T]), all on the device.  One
        deviation from torch_align: blank frames in front of the first token count to token 0 (the reference's loop trips its assert there).
        ValueError where no alignment exists: fewer frames than tokens plus adjacent equal pairs."""
        L = self._lengths(mels, mel_lengths)
        toks, PL = self._check_texts(L, texts, text_lengths)
        lp, seg = self.packed(mels, L)
        return self._align_rows(lp, seg, toks, PL)

    def align_audio(self, wave, sample_lengths, texts, text_lengths, mel_stats=(-4.0, 4.0), front: Optional["LogMelSpectrogram"] = None):
        """align() from recordings: wave [B, samples] at the model's sample rate (sample_lengths [B], or None) through preprocess's front end
        (align_text.py:112-117: the ``n_mels``-mel transform of the model config, the last frame dropped, normalised by mel_stats = (mean, std);
        ``front`` to give another LogMelSpectrogram), its packed rows handed to the aligner as they are.  Equals align() on that mel, bit for bit;
        the frame counts follow from the sample counts on the host."""
        if front is None:
            front = LogMelSpectrogram.from_config(self.cfg, self.n_mels, mean=mel_stats[0], std=mel_stats[1], frames="drop_last")
        if front.n_mels != self.n_mels:
            raise ValueError(f"the front end has {front.n_mels} mel bins, the aligner takes {self.n_mels}")
        Ls = front._lengths(wave, sample_lengths)
        L = front.frame_counts(Ls, "drop_last")
        toks, PL = self._check_texts(L, texts, text_lengths)
        eng = self.engine
        front._engine = eng
        rows, seg = front.packed(wave, Ls, frames="drop_last", mean=mel_stats[0], std=mel_stats[1])
        return self._align_rows(eng.text_aligner(seg, rows), seg, toks, PL)

    def _score_rows(self, lp, seg, toks, PL, loss):
        """One ctc_align, one ctc_nll, one confidence launch on the log-prob rows, one host read."""
        eng = self.engine
        seg_p = Segments(PL, eng.device)
        tg = torch.tensor([v for tk in toks for v in tk], dtype=torch.int32, device=eng.device)
        r = eng.ctc_align(seg, lp, seg_p, tg, self.blank)
        if loss is not None and loss.blank != self.blank:
            raise ValueError(f"the loss has blank {loss.blank}, the aligner {self.blank}")
        nll = eng.ctc_nll(seg, lp, seg_p, tg, self.blank)  # step_type "eval": no label priors
        conf = eng.ctc_confidence_sums(seg, r["scores"])
        host = torch.cat([nll, conf]).cpu().tolist()  # the one host read
        B = seg.n
        nll_utt, conf_sum = host[:B], host[B:]
        return dict(align_loss=align_loss_value(nll_utt, seg.lengths, PL, loss), nll_utt=nll_utt, confidence=sum(conf_sum) / float(seg.rows),
                    confidence_utt=[conf_sum[b] / float(seg.lengths[b]) for b in range(B)])

    def alignment_scores(self, mels, mel_lengths, texts, text_lengths, loss: Optional["CTCLossWithLabelPriors"] = None):
        """What validate_alignment logs about a batch (train/stage_type.py:79-111) and align_text's per-file score (align_text.py:155): mels
        [B, T, n_mels] normalised log-mel, texts [B, P] -> dict of Python numbers:
          align_loss      the loss' "eval" value: ``loss.reduction`` and pairing over the fp32 per-utterance values (default: "mean", every
                          utterance with its own token count)
          nll_utt         every utterance's CTC negative log-likelihood (float64, exact over all paths)
          confidence      the total of exp(scores) over the total number of frames, scores the Viterbi path's log-probs
          confidence_utt  every utterance's mean of exp(scores): the number a dataset is filtered by
        One aligner forward, one ctc_align, one ctc_nll, one confidence launch, one host read."""
        L = self._lengths(mels, mel_lengths)
        toks, PL = self._check_texts(L, texts, text_lengths)
        lp, seg = self.packed(mels, L)
        return self._score_rows(lp, seg, toks, PL, loss)

    def alignment_scores_audio(self, wave, sample_lengths, texts, text_lengths, loss: Optional["CTCLossWithLabelPriors"] = None, mel_stats=(-4.0, 4.0),
                               front: Optional["LogMelSpectrogram"] = None):
        """alignment_scores() from recordings, through the front end of align_audio."""
        if front is None:
            front = LogMelSpectrogram.from_config(self.cfg, self.n_mels, mean=mel_stats[0], std=mel_stats[1], frames="drop_last")
        if front.n_mels != self.n_mels:
            raise ValueError(f"the front end has {front.n_mels} mel bins, the aligner takes {self.n_mels}")
        Ls = front._lengths(wave, sample_lengths)
        L = front.frame_counts(Ls, "drop_last")
        toks, PL = self._check_texts(L, texts, text_lengths)
        eng = self.engine
        front._engine = eng
        rows, seg = front.packed(wave, Ls, frames="drop_last", mean=mel_stats[0], std=mel_stats[1])
        return self._score_rows(eng.text_aligner(seg, rows), seg, toks, PL, loss)


def build_inference_modules(cfg=None, engine=None, synthetic_seed: Optional[int] = None, hubert: bool = False, mel_style: bool = False,
                            cfm_pitch: bool = False, ssl: bool = False, aligner: bool = False):
    """The five modules of the inference composition (models/models.py:32-63, :79-101), optionally with synthetic weights.
    hubert=True adds the voice-conversion pair hubert_speech_predictor / hubert_pitch_energy_predictor (models/models.py:92-101);
    mel_style=True adds pe_mel_style_encoder (models/models.py:57-62); cfm_pitch=True adds cfm_pitch_predictor (models/models.py:72-75);
    ssl=True adds hubert, the AdaptiveHubert content encoder shaped by hubert.arch / hubert.sr (train/models/ssl.py:16-31);
    aligner=True adds text_aligner, tdnn_blstm_ctc_model_base(n_mels, text_encoder.tokens) (models/models.py:28-30)."""
    cfg = cfg or load_model_config()
    m = dict(
        speech_predictor=SpeechPredictor(cfg, engine=engine),
        duration_predictor=DurationPredictor(cfg.style_dim, cfg.inter_dim, cfg.text_encoder, cfg.style_encoder, cfg.duration_predictor, cfg=cfg,
                                             engine=engine),
        pitch_energy_predictor=PitchEnergyPredictor(cfg.style_dim, cfg.pitch_energy_predictor.inter_dim, cfg.text_encoder, cfg.style_encoder,
                                                    cfg.duration_predictor, cfg.pitch_energy_predictor, cfg=cfg, engine=engine),
        pe_text_encoder=TextEncoder(inter_dim=cfg.pitch_energy_predictor.inter_dim, config=cfg.text_encoder, cfg=cfg, engine=engine),
        pe_text_style_encoder=TextStyleEncoder(cfg.pitch_energy_predictor.inter_dim, cfg.style_dim, cfg.style_encoder, cfg=cfg, engine=engine),
    )
    if hubert:
        hd, sd = hubert_dims(cfg)
        m["hubert_speech_predictor"] = HubertSpeechPredictor(cfg, engine=engine)
        m["hubert_pitch_energy_predictor"] = HubertPitchEnergyPredictor(hd, sd, cfg.style_dim, cfg.inter_dim, cfg.style_encoder, cfg.pitch_energy_predictor,
                                                                        cfg=cfg, engine=engine)
    if mel_style:
        ms = Record(cfg.get("mel_style_encoder") or DEFAULT_MODEL["mel_style_encoder"])  # model.yml section, config.DEFAULT_MODEL when absent
        m["pe_mel_style_encoder"] = MelStyleEncoder(cfg.n_mels, cfg.style_dim, ms.max_channels, ms.skip_downsample, cfg=cfg, engine=engine)
    if cfm_pitch:
        m["cfm_pitch_predictor"] = CfmPitchPredictor(hubert_dims(cfg)[0], cfg.n_mels, cfg=cfg, engine=engine)
    if ssl:
        from .config import hubert_ssl_config

        sr, a = hubert_ssl_config(cfg)
        m["hubert"] = AdaptiveHubert(None, cfg.sample_rate, sr, config=a, cfg=cfg, engine=engine)
    if aligner:
        m["text_aligner"] = TextAligner(cfg.n_mels, cfg.text_encoder.tokens, engine=engine, cfg=cfg)
    if synthetic_seed is not None:
        for mod in m.values():
            mod.load_synthetic(synthetic_seed)
    return m
