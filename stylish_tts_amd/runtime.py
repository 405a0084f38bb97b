"""Host-side handle on the HIP library: context, weights, and the stage calls on torch device tensors.

PyTorch is plumbing here (device memory, streams); all arithmetic runs in libstylish_hip.so.
Tensors at this level are TIME-MAJOR packed rows (see include/stylish_hip.h); the nn.Module shims in
``modules.py`` convert from/to the reference's ``[B, C, T]`` layout at the module boundary.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import geometry, load_model_config

N_BINS_LD = 1056  # 1025 bins padded to a multiple of 32 floats (spectrum rows of an fp32 engine; HipModel.har_ld is the engine's own stride)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Segments:
    """Utterance row offsets (host int32 array + device copy).

    capacity=True (``Segments.capacity``): the host array holds UPPER BOUNDS - cumulative capacities that size every buffer and
    grid - and the device tensor the real offsets, written on the device by ``HipModel.frame_offsets`` (include/stylish_hip.h,
    STTS_SEG_CAPACITY): no host read of the predicted durations is needed before the frame-rate stages."""

    def __init__(self, lengths: Sequence[int], device, dev: Optional[torch.Tensor] = None, capacity: bool = False):
        lengths = [int(x) for x in lengths]
        self.lengths = lengths
        self.host = np.zeros(len(lengths) + 1, np.int32)
        self.host[1:] = np.cumsum(lengths)
        self.dev = dev if dev is not None else torch.from_numpy(self.host).to(device)
        self.n = len(lengths)
        self.rows = int(self.host[-1])
        self.max_len = max(lengths)
        self.is_capacity = capacity

    @classmethod
    def capacity(cls, caps: Sequence[int], device) -> "Segments":
        """Capacity layout: `caps` rows per utterance at most; the device offsets are uninitialised until frame_offsets fills them."""
        return cls(caps, device, dev=torch.empty(len(caps) + 1, dtype=torch.int32, device=device), capacity=True)

    @property
    def flags(self) -> int:
        return 1 if self.is_capacity else 0  # STTS_SEG_CAPACITY

    @property
    def host_ptr(self):
        return self.host.ctypes.data_as(C.c_void_p)

    def scaled(self, k: int, dev: Optional[torch.Tensor] = None) -> "Segments":
        if self.is_capacity:
            assert dev is not None, "a scaled capacity layout needs its own device offsets"
            return Segments([x * k for x in self.lengths], self.dev.device, dev=dev, capacity=True)
        return Segments([x * k for x in self.lengths], self.dev.device)


class CapacityOverflow(RuntimeError):
    """An utterance's predicted frame count exceeded the capacity its buffers were sized for (stts_frame_offsets)."""


class HipModel:
    """Owns a stts_ctx.  weights: {module name: {state_dict key: array}} for the five inference modules."""

    PRECISIONS = {"f32": 0, "bf16": 1, "f16": 2, "f32_native": 3}

    def __init__(self, cfg=None, device: int = 0, precision: str = "f32"):
        """precision: operand precision of the contractions ("f32" = the reference's arithmetic, fp32 products formed from exact
        three-term bf16 splits on the bf16 matrix cores; "f32_native" = the same on the f32 matrix cores; "bf16" / "f16" round
        the matrix-core operands, fp32 accumulate; include/stylish_hip.h:stts_set_precision)."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}")
        if not torch.cuda.is_available():
            raise RuntimeError("HipModel needs a GPU (MI355X); there is no CPU fallback in the product path")
        self.lib = _lib.load()
        self.cfg = cfg if cfg is not None else load_model_config()
        # STFT geometry (ValueError naming the broken rule before any device work): h = vocoder hop (samples per row of the frame path),
        # n_bins = n_fft / 2 + 1, ld_lp = the row stride of logamp / phase outputs (N_BINS_LD at the default geometry)
        self.n_fft, self.win_length, self.hop4, self.n_bins, _ = geometry(self.cfg)
        self.ld_lp = (self.n_bins + 31) // 32 * 32
        self.device = torch.device("cuda", device)
        self._dims = _lib.dims_from_config(self.cfg)
        h = C.c_void_p()
        _lib.check(self.lib.stts_ctx_create(C.byref(self._dims), device, C.byref(h)))
        self.ctx = h
        self.precision = precision
        _lib.check(self.lib.stts_set_precision(self.ctx, self.PRECISIONS[precision]))
        # row stride of the harmonic spectra = the prior convs' packed input width, asked from the library (1025 bins padded to 32 in fp32, 64 in the 16-bit modes)
        self.har_ld = int(self.lib.stts_har_ld(self.ctx))
        # grow-only workspaces (_grow), one per launch stream (stages issued on different streams may run concurrently): the frame path's, the
        # phoneme-rate stages' (shared with the HuBERT stages: same stream discipline), MelStyleEncoder's, CfmPitchPredictor's, AdaptiveHubert's
        self._ws: Dict[int, torch.Tensor] = {}
        self._pws: Dict[int, torch.Tensor] = {}
        self._mws: Dict[int, torch.Tensor] = {}
        self._cpws: Dict[int, torch.Tensor] = {}
        self._sslws: Dict[int, torch.Tensor] = {}
        self._rvws: Dict[int, torch.Tensor] = {}
        self._rvvws: Dict[int, torch.Tensor] = {}
        self._rv_lt = None  # the Viterbi decode's transition table on this device
        self._alws: Dict[int, torch.Tensor] = {}
        self._ctcws: Dict[int, torch.Tensor] = {}
        self._ws_lock = threading.Lock()

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.stts_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights: Mapping[str, Mapping[str, "np.ndarray | torch.Tensor"]], which: int = 7):
        for mod, sd in weights.items():
            self.load_state_dict(mod, sd)
        self.finalize(which)

    def load_state_dict(self, module: str, sd: Mapping[str, "np.ndarray | torch.Tensor"], prefix: str = ""):
        for k, v in sd.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            a = np.ascontiguousarray(v, dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            name = (module + "." if module else "") + prefix + k
            _lib.check(self.lib.stts_load_weight(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), shape, max(a.ndim, 1)))

    def finalize(self, which: int = 7):
        _lib.check(self.lib.stts_finalize_weights(self.ctx, which))

    def check_status(self):
        _lib.check(self.lib.stts_check_status(self.ctx, _stream()))

    def frame_offsets(self, seg_p: Segments, dur: torch.Tensor, caps: Sequence[int]):
        """Device-side DurationProcessor bookkeeping: -> (mel-rate Segments, vocoder-rate Segments, need) as CAPACITY layouts whose
        device offsets are the real ones (cumulative predicted frames).  `caps`: mel frames each utterance may have at most.
        need [n_utt] int32 (device): the frames each utterance asked for; need[u] > caps[u] = overflow: the utterance was truncated
        to its capacity (every stage stays in bounds) and the call must be repeated with larger capacities (CapacityOverflow is
        what Synthesizer raises internally when it reads `need` with the audio)."""
        st = Segments.capacity(caps, self.device)
        off4 = torch.empty(seg_p.n + 1, dtype=torch.int32, device=self.device)
        need = torch.empty(seg_p.n, dtype=torch.int32, device=self.device)
        cap_dev = torch.from_numpy(st.host).to(self.device, non_blocking=True)
        _lib.check(self.lib.stts_frame_offsets(self.ctx, _stream(), seg_p.n, _ptr(seg_p.dev), _ptr(dur), _ptr(cap_dev), _ptr(st.dev), _ptr(off4), _ptr(need)))
        return st, st.scaled(4, dev=off4), need

    # ------------------------------------------------------------------ workspace
    def _grow(self, pool: Dict[int, torch.Tensor], need: int) -> torch.Tensor:
        """The current stream's workspace of `pool`, reallocated when it is smaller than `need` bytes."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        with self._ws_lock:
            ws = pool.get(key)
            if ws is None or ws.numel() < need:
                ws = pool[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def workspace(self, seg: Segments) -> torch.Tensor:
        return self._grow(self._ws, int(self.lib.stts_frame_workspace_bytes(self.ctx, seg.rows, seg.n, seg.max_len)))

    def _f32(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ stages (time-major tensors)
    def decoder(self, seg: Segments, asr, pitch, energy, style):
        dh = self.cfg.decoder.hidden_dim
        x = self._f32(seg.rows, dh)
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_decoder_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(asr), asr.shape[1], _ptr(pitch),
                                                 _ptr(energy), _ptr(style), _ptr(x), dh, _ptr(ws), ws.numel()))
        return x

    def prior_flow(self, seg: Segments, x, style, prior_noise, return_z=False):
        dh = self.cfg.decoder.hidden_dim
        mel = self._f32(seg.rows, dh)
        zp = self._f32(seg.rows, dh // 4) if return_z else None
        zf = self._f32(seg.rows, dh // 4) if return_z else None
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_prior_flow_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], _ptr(style),
                                                    _ptr(prior_noise), _ptr(mel), dh, _ptr(zp), _ptr(zf), _ptr(ws), ws.numel()))
        return (mel, zp, zf) if return_z else mel

    def harmonic_stft(self, seg: Segments, pitch, src_noise, init_phase, batch_scope=True, return_signal=False):
        spec = self._f32(seg.rows, self.har_ld)
        phase = self._f32(seg.rows, self.har_ld)
        sig = self._f32(seg.rows * self.hop4) if return_signal else None
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_harmonic_stft(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(pitch), _ptr(src_noise),
                                               _ptr(init_phase), int(batch_scope), _ptr(sig), _ptr(spec), _ptr(phase), self.har_ld, _ptr(ws),
                                               ws.numel()))
        return (spec, phase, sig) if return_signal else (spec, phase)

    def vocoder(self, seg: Segments, mel, style, har_spec, har_phase, return_spec=False):
        audio = self._f32(seg.rows * self.hop4)
        la = self._f32(seg.rows, self.ld_lp) if return_spec else None
        ph = self._f32(seg.rows, self.ld_lp) if return_spec else None
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_vocoder_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(mel), mel.shape[1], _ptr(style),
                                                 _ptr(har_spec), _ptr(har_phase), har_spec.shape[1], _ptr(audio), _ptr(la), _ptr(ph), self.ld_lp,
                                                 _ptr(ws), ws.numel()))
        return (audio, la, ph) if return_spec else audio

    def frame_path(self, seg: Segments, asr, pitch, energy, style, prior_noise, src_noise, init_phase, batch_scope=True, out=None):
        audio = out if out is not None else self._f32(seg.rows * self.hop4)
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_frame_path(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(asr), asr.shape[1], _ptr(pitch),
                                            _ptr(energy), _ptr(style), _ptr(prior_noise), _ptr(src_noise), _ptr(init_phase), int(batch_scope),
                                            _ptr(audio), _ptr(ws), ws.numel(), seg.flags))
        return audio

    def posterior(self, seg: Segments, audio=None, spectra=None, style=None, noise=None, taps=False, mel=False, stats=True):
        """PosteriorEncoder.forward on packed rows (stts_posterior_forward; needs W_POSTERIOR, and W_FLOW for mel=True).  audio [hop4 * rows]
        packed, or spectra = (har_spec, har_phase) as [rows, >= n_bins] rows (copied into zero-padded [rows, har_ld] buffers).  style
        [n_utt, 64] or None (the reference's g=None); noise [rows, 128].  -> dict: z, mean, logstd [rows, 128] (stats=False: z only),
        har_spec / har_phase [rows, har_ld] (what the call read or wrote), mel [rows, hidden_dim] = post_flow(z) when mel=True, and with
        taps=True x0 (cat[pre_spec, pre_phase]) and wn (the WaveNet's output)."""
        if (audio is None) == (spectra is None):
            raise ValueError("posterior: give exactly one of audio and spectra")
        if noise is None:
            raise ValueError("posterior: noise [rows, 128] is required")
        fh, dh = self.cfg.decoder.hidden_dim // 4, self.cfg.decoder.hidden_dim
        if audio is not None:
            spec, phase = self._f32(seg.rows, self.har_ld), self._f32(seg.rows, self.har_ld)
        else:
            spec, phase = (torch.zeros(seg.rows, self.har_ld, dtype=torch.float32, device=self.device) for _ in range(2))
            for dst, src in zip((spec, phase), spectra):
                dst[:, : self.n_bins] = src[:, : self.n_bins]
        o = dict(z=self._f32(seg.rows, fh), har_spec=spec, har_phase=phase)
        if stats:
            o.update(mean=self._f32(seg.rows, fh), logstd=self._f32(seg.rows, fh))
        if mel:
            o["mel"] = self._f32(seg.rows, dh)
        if taps:
            o.update(x0=self._f32(seg.rows, fh), wn=self._f32(seg.rows, fh))
        ws = self._grow(self._ws, int(self.lib.stts_posterior_workspace_bytes(self.ctx, seg.rows, seg.n, seg.max_len)))
        _lib.check(self.lib.stts_posterior_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(audio), _ptr(spec), _ptr(phase), self.har_ld,
                                                   _ptr(style), _ptr(noise), _ptr(o["z"]), _ptr(o.get("mean")), _ptr(o.get("logstd")), _ptr(o.get("mel")), dh,
                                                   _ptr(o.get("x0")), _ptr(o.get("wn")), _ptr(ws), ws.numel(), seg.flags))
        return o

    # ------------------------------------------------------------------ flow statistics (needs W_FLOW_STATS)
    def flow_stats_workspace_bytes(self, seg: Segments) -> int:
        """What stts_flow_stats_forward carves for this batch (0 before W_FLOW_STATS is finalized)."""
        return int(self.lib.stts_flow_stats_workspace_bytes(self.ctx, seg.rows, seg.n, seg.max_len))

    def flow_stats(self, seg: Segments, z, mean, logstd, style, reverse: bool):
        """ResidualCouplingBlock.forward with the three streams (stts_flow_stats_forward): z, mean, logstd [rows, 128], style [n_utt, 64]
        -> dict z, mean, logstd [rows, 128] (new buffers).  reverse=False is the forward direction (mel -> text), True the reverse one."""
        o = {k: self._f32(seg.rows, z.shape[1]) for k in ("z", "mean", "logstd")}
        ws = self._grow(self._ws, self.flow_stats_workspace_bytes(seg))
        _lib.check(self.lib.stts_flow_stats_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), int(bool(reverse)), _ptr(z), _ptr(mean), _ptr(logstd),
                                                    _ptr(style), _ptr(o["z"]), _ptr(o["mean"]), _ptr(o["logstd"]), _ptr(ws), ws.numel(), seg.flags))
        return o

    def prior_stats(self, seg: Segments, x, noise):
        """PriorEncoder.forward with all three outputs (stts_prior_stats_forward): x [rows, ld >= 512] (the decoder's output), noise [rows, 128]
        -> dict z = mean + noise exp(logstd), mean, logstd [rows, 128]."""
        fh = self.cfg.decoder.hidden_dim // 4
        o = {k: self._f32(seg.rows, fh) for k in ("z", "mean", "logstd")}
        _lib.check(self.lib.stts_prior_stats_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], _ptr(noise), _ptr(o["z"]),
                                                     _ptr(o["mean"]), _ptr(o["logstd"]), None, 0, seg.flags))
        return o

    def kl_sums(self, seg: Segments, kind: int, a, b, c, d):
        """Per-utterance fp64 sums of the KL term over rows and channels (stts_val_kl_sums) -> device double [n_utt].  kind 0 = kl_loss(z_p=a,
        logs_q=b, m_p=c, logs_p=d), 1 = kl_loss_normal(m_q=a, ...); the reference's score is sums.sum() / rows."""
        sums = torch.empty(seg.n, dtype=torch.float64, device=self.device)
        ws = torch.empty(seg.rows + 32, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_val_kl_sums(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), kind, _ptr(a), _ptr(b), _ptr(c), _ptr(d), a.shape[1], a.shape[1],
                                             _ptr(sums), _ptr(ws), ws.numel() * 8))
        return sums

    def op_flow_stats_layer(self, seg: Segments, layer: int, z, mean, logstd, style, reverse: bool, form: int = 0, pad_rows: int = 0):
        """Coupling layer `layer` of the flow statistics alone (test surface) -> (z', mean', logstd', h0): h0 = the next coupling layer's pre(z') where
        the form produces it (a fused form with a next layer; NaN otherwise).  form: 0 = plain contractions, 16 | 32 | 64 = wn_stats_kernel on that
        block height.  pad_rows: canary rows (NaN) behind the outputs."""
        outs = [torch.full((seg.rows + pad_rows, z.shape[1]), float("nan"), dtype=torch.float32, device=self.device) for _ in range(4)]
        ws = torch.empty(self.flow_stats_workspace_bytes(seg), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.stts_op_flow_stats_layer(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), layer, int(bool(reverse)), form, _ptr(z), _ptr(mean),
                                                     _ptr(logstd), _ptr(style), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(ws), ws.numel()))
        return tuple(outs)

    # ------------------------------------------------------------------ layout bridge + single ops
    def op_posterior_layer(self, seg: Segments, layer: int, h, out, cond, form: int = 0, out_acc: Optional[bool] = None, pad_rows: int = 0):
        """WaveNet layer `layer` of the finalized posterior encoder alone (test surface): h, out [rows, 128], cond [n_utt, ld] -> (h', out').
        form: 0 = plain contractions, 16 | 32 | 64 = wn_post_kernel on that block height.  pad_rows: canary rows (NaN) behind the outputs."""
        H = h.shape[1]
        h_out = torch.full((seg.rows + pad_rows, H), float("nan"), dtype=torch.float32, device=self.device)
        o_out = torch.full((seg.rows + pad_rows, H), float("nan"), dtype=torch.float32, device=self.device)
        ws = self._f32(seg.rows * H + 64)
        acc = layer > 0 if out_acc is None else out_acc
        _lib.check(self.lib.stts_op_posterior_layer(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), layer, form, int(acc), _ptr(h), _ptr(out),
                                                    _ptr(cond), cond.shape[1], _ptr(h_out), _ptr(o_out), _ptr(ws), ws.numel() * 4))
        return h_out, o_out


    def to_time_major(self, x_bct: torch.Tensor, ld: Optional[int] = None) -> torch.Tensor:
        B, Cc, T = x_bct.shape
        ld = ld or ((Cc + 31) // 32 * 32)
        y = self._f32(B * T, ld)
        _lib.check(self.lib.stts_to_time_major(_stream(), _ptr(x_bct.contiguous()), B, Cc, T, _ptr(y), ld))
        return y

    def to_channel_major(self, x: torch.Tensor, B: int, Cc: int, T: int) -> torch.Tensor:
        y = self._f32(B, Cc, T)
        _lib.check(self.lib.stts_to_channel_major(_stream(), _ptr(x), x.shape[1], B, Cc, T, _ptr(y)))
        return y

    def op_conv1d(self, seg: Segments, x, cin, w: np.ndarray, bias: Optional[np.ndarray], dil=1, act=0, force_tile=0, precision: Optional[str] = None):
        cout, _, k = w.shape
        ldy = (cout + 31) // 32 * 32
        y = torch.zeros(seg.rows, ldy, dtype=torch.float32, device=self.device)
        w = np.ascontiguousarray(w, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        _lib.check(self.lib.stts_op_conv1d(_stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], cin, w.ctypes.data_as(C.c_void_p),
                                           None if b is None else b.ctypes.data_as(C.c_void_p), cout, k, dil, act, _ptr(y), ldy, force_tile,
                                           self.PRECISIONS[precision or self.precision]))
        return y

    def op_conv1d_x3(self, seg: Segments, x, cin, w: np.ndarray, bias: Optional[np.ndarray], dil=1, x2=None, cin2=0, aff: Optional[np.ndarray] = None,
                     xaff_mode=0, slope=1.0, presplit=False, force_tile=0, precision: Optional[str] = None):
        """stts_op_conv1d_x3: the fp32 contraction with a second input segment x2 (w [cout, cin + cin2, k]), an input affine of x
        (aff [n_utt, 2, ldx] scale / shift rows, xaff_mode 1 or 2) or pre-split activation planes."""
        cout, _, k = w.shape
        ldy = (cout + 31) // 32 * 32
        y = torch.zeros(seg.rows, ldy, dtype=torch.float32, device=self.device)
        w = np.ascontiguousarray(w, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        a = None if aff is None else np.ascontiguousarray(aff, np.float32)
        _lib.check(self.lib.stts_op_conv1d_x3(_stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], cin,
                                              None if x2 is None else _ptr(x2), 0 if x2 is None else x2.shape[1], cin2, w.ctypes.data_as(C.c_void_p),
                                              None if b is None else b.ctypes.data_as(C.c_void_p), cout, k, dil,
                                              None if a is None else a.ctypes.data_as(C.c_void_p), xaff_mode, slope, int(presplit), _ptr(y), ldy,
                                              force_tile, self.PRECISIONS[precision or self.precision]))
        return y

    def op_conv1d_epi(self, seg: Segments, segments, bias: Optional[np.ndarray], precision: str, force_tile: int, act=0, alpha=1.0, r=None, rcol0=0,
                      y=None, ycol0=0, y16=None, ycol16=0, sumsq=None, stat=None, tune=0):
        """stts_op_conv1d_epi: the 16-bit store contraction with its whole epilogue, written INTO the caller's tensors (nothing is allocated or cleared
        here, so a test can pre-fill them with a sentinel).  segments: one or two (x [rows, ldx] fp32, cin, w [cout, cin, k], dil); r / y fp32
        [rows, ld], y16 int16 [rows, ld] (the mode's bit patterns), sumsq fp32 [n_utt, ss_stride, ld_ss], stat fp32 [n_utt, nchunk, 2, ld_stat].
        A capacity `seg` (host = cumulative capacities, dev = real offsets) sets the capacity flag."""
        a = _lib.ConvEpiArgs()
        keep = []
        a.seg_off_host, a.seg_off_dev = seg.host_ptr, _ptr(seg.dev)
        a.n_utt, a.capacity, a.nseg = seg.n, int(seg.is_capacity), len(segments)
        a.cout = int(segments[0][2].shape[0])
        for i, (x, cin, w, dil) in enumerate(segments):
            assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2 and w.shape[0] == a.cout and w.shape[1] == cin
            w = np.ascontiguousarray(w, np.float32)
            keep.append(w)
            s = a.seg[i]
            s.x, s.w_host, s.x_elems = _ptr(x), w.ctypes.data_as(C.c_void_p), x.numel()
            s.ldx, s.cin, s.k, s.dil = x.shape[1], cin, w.shape[2], dil
        if bias is not None:
            b = np.ascontiguousarray(bias, np.float32)
            assert b.shape == (a.cout,)
            keep.append(b)
            a.bias_host = b.ctypes.data_as(C.c_void_p)
        a.act, a.alpha, a.force_tile, a.tune, a.precision = act, alpha, force_tile, tune, self.PRECISIONS[precision]
        for t, dt in ((r, torch.float32), (y, torch.float32), (y16, torch.int16), (sumsq, torch.float32), (stat, torch.float32)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.is_cuda)
        if r is not None:
            a.r, a.r_elems, a.ldr, a.rcol0 = _ptr(r), r.numel(), r.shape[1], rcol0
        if y is not None:
            a.y, a.y_elems, a.ldy, a.ycol0 = _ptr(y), y.numel(), y.shape[1], ycol0
        if y16 is not None:
            a.y16, a.y16_elems, a.ldy16, a.ycol16 = _ptr(y16), y16.numel(), y16.shape[1], ycol16
        if sumsq is not None:
            assert sumsq.dim() == 3 and sumsq.shape[0] == seg.n
            a.sumsq, a.sumsq_elems, a.ss_stride, a.ld_ss = _ptr(sumsq), sumsq.numel(), sumsq.shape[1], sumsq.shape[2]
        if stat is not None:
            assert stat.dim() == 4 and stat.shape[0] == seg.n and stat.shape[2] == 2
            a.stat, a.stat_elems, a.stat_nchunk, a.ld_stat = _ptr(stat), stat.numel(), stat.shape[1], stat.shape[3]
        _lib.check(self.lib.stts_op_conv1d_epi(_stream(), C.byref(a)))

    # ------------------------------------------------------------------ the kernels between the contractions (test surface)
    @staticmethod
    def _fill_args(a, seg: Optional[Segments], fields: dict, keep: list):
        """Fill an args struct of include/stylish_hip.h by field name: a CUDA tensor sets the pointer and, where the struct has one, `<name>_elems`;
        a numpy array (the *_host fields) is passed as contiguous fp32; everything else is assigned as it is.  Nothing is allocated or cleared."""
        if seg is not None:
            a.seg_off_host, a.seg_off_dev, a.n_utt = seg.host_ptr, _ptr(seg.dev), seg.n
        names = {n for n, _ in a._fields_}
        for k, v in fields.items():
            if v is None:
                continue
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.is_contiguous(), k
                setattr(a, k, _ptr(v))
                if k + "_elems" in names:
                    setattr(a, k + "_elems", v.numel())
            elif isinstance(v, np.ndarray):
                v = np.ascontiguousarray(v, np.float32)
                keep.append(v)
                setattr(a, k, v.ctypes.data_as(C.c_void_p))
            else:
                setattr(a, k, v)
        return a

    def op_adain(self, seg: Segments, **fields):
        """stts_op_adain (fields of stts_adain_args by name): chunk statistics -> merge -> apply of AdaIN, into the caller's tensors."""
        keep = []
        a = self._fill_args(_lib.AdainArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_adain(_stream(), C.byref(a)))

    def op_wino_stat(self, seg: Segments, **fields):
        """stts_op_wino_stat (fields of stts_wino_stat_args): the Winograd-form conv with the statistics its output transform leaves."""
        keep = []
        a = self._fill_args(_lib.WinoStatArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_wino_stat(_stream(), C.byref(a)))

    def op_row_layernorm(self, seg: Optional[Segments], outs, **fields):
        """stts_op_row_layernorm (fields of stts_row_layernorm_args; outs: one or two dicts of stts_ln_out fields)."""
        keep = []
        a = self._fill_args(_lib.RowLayerNormArgs(), seg, fields, keep)
        a.nout = len(outs)
        for i, o in enumerate(outs):
            self._fill_args(a.out[i], None, o, keep)
        _lib.check(self.lib.stts_op_row_layernorm(_stream(), C.byref(a)))

    def op_dwconv(self, seg: Segments, **fields):
        """stts_op_dwconv (fields of stts_dwconv_args): depthwise conv, alone or with the adaptive LayerNorm (fused / two launches)."""
        keep = []
        a = self._fill_args(_lib.DwconvArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_dwconv(_stream(), C.byref(a)))

    def op_grn(self, seg: Segments, **fields):
        """stts_op_grn (fields of stts_grn_args): GRN factor from a slot table, then the input-affine table or the scaled weight copies."""
        keep = []
        a = self._fill_args(_lib.GrnArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_grn(_stream(), C.byref(a)))

    def op_conv2d(self, seg_in: Segments, seg_out: Segments, dt, df, **fields):
        """stts_op_conv2d (fields of stts_conv2d_args): the 2-D implicit-GEMM convolution, one launch; seg_in / seg_out: the offsets of the input level and of
        the base grid (used >> sh), dt / df: the taps."""
        assert seg_in.n == seg_out.n and len(dt) == len(df) <= 25
        keep = []
        a = self._fill_args(_lib.Conv2dArgs(), None, fields, keep)
        a.off_in_host, a.off_in_dev, a.off_out_host, a.off_out_dev, a.n_utt = seg_in.host_ptr, _ptr(seg_in.dev), seg_out.host_ptr, _ptr(seg_out.dev), seg_in.n
        a.ntap = len(dt)
        for i, (t, f) in enumerate(zip(dt, df)):
            a.dt[i], a.df[i] = int(t), int(f)
        _lib.check(self.lib.stts_op_conv2d(_stream(), C.byref(a)))

    # ------------------------------------------------------------------ the flow-matching estimator's row kernels (test surface)
    def op_cfm_elem(self, seg: Optional[Segments], **fields):
        """stts_op_cfm_elem (fields of stts_cfm_elem_args): kind 0 Mish in place, 1 SwiGLU, 2 the gated residual (the only one with offsets)."""
        keep = []
        a = self._fill_args(_lib.CfmElemArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_cfm_elem(_stream(), C.byref(a)))

    def op_rms_adaln(self, seg: Segments, **fields):
        """stts_op_rms_adaln (fields of stts_rms_adaln_args): RMSNorm + AdaLN, optionally fused with the previous branch's gated residual."""
        keep = []
        a = self._fill_args(_lib.RmsAdalnArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_rms_adaln(_stream(), C.byref(a)))

    def op_rope(self, seg: Segments, **fields):
        """stts_op_rope (fields of stts_rope_args): kind 0 the estimator's axial RoPE, 1 the encoders' sequence RoPE, in place."""
        keep = []
        a = self._fill_args(_lib.RopeArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_rope(_stream(), C.byref(a)))

    def op_cfm_small(self, **fields):
        """stts_op_cfm_small (fields of stts_cfm_small_args): kind 0 the per-utterance Linear, 1 its LayerNorm, 2 the timestep embedding."""
        keep = []
        a = self._fill_args(_lib.CfmSmallArgs(), None, fields, keep)
        _lib.check(self.lib.stts_op_cfm_small(_stream(), C.byref(a)))

    def op_cfm_source(self, seg: Segments, curves: Segments, **fields):
        """stts_op_cfm_source (fields of stts_cfm_source_args): the sine source; seg: frames, curves: the points of F0 / N per utterance."""
        assert seg.n == curves.n
        keep = []
        a = self._fill_args(_lib.CfmSourceArgs(), seg, fields, keep)
        a.curve_off_host, a.curve_off_dev = curves.host_ptr, _ptr(curves.dev)
        _lib.check(self.lib.stts_op_cfm_source(_stream(), C.byref(a)))

    # ------------------------------------------------------------------ the small kernels between the stages (test surface)
    def op_glue(self, seg: Optional[Segments], tok: Optional[Segments] = None, wf=None, wn=None, **fields):
        """stts_op_glue (fields of stts_glue_args): kind 0 decoder front (wf / wn: the 3-tap filters), 1 run_style, 2 embed, 3 mean_rows, 4 broadcast_style,
        5 row_utt, 6 frame_token_map + local_token (seg: frames, tok: tokens)."""
        keep = []
        a = self._fill_args(_lib.GlueArgs(), seg, fields, keep)
        if tok is not None:
            a.tok_off_host, a.tok_off_dev = tok.host_ptr, _ptr(tok.dev)
        for i in range(3):
            if wf is not None:
                a.wf[i] = float(wf[i])
            if wn is not None:
                a.wn[i] = float(wn[i])
        _lib.check(self.lib.stts_op_glue(_stream(), C.byref(a)))

    def op_chan_conv(self, seg: Segments, **fields):
        """stts_op_chan_conv (fields of stts_chan_conv_args): the one-channel conv (F0 / N heads, the vocoder's Nyquist bin), one or two sets per launch."""
        keep = []
        a = self._fill_args(_lib.ChanConvArgs(), seg, fields, keep)
        _lib.check(self.lib.stts_op_chan_conv(_stream(), C.byref(a)))

    def op_adain_block(self, prefix: str, seg: Segments, x, cin, cout, style):
        y = self._f32(seg.rows, cout)
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_op_adain_block(self.ctx, _stream(), prefix.encode(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], cin,
                                                cout, _ptr(style), _ptr(y), cout, _ptr(ws), ws.numel()))
        return y

    BLOCK_PLAN_FIELDS = ("conv1", "conv2", "rows16", "norm1", "norm2", "next_norm1", "take_pending", "defer_conv2", "shortcut", "cast_x16", "y16", "affine_serial",
                         "bridge_w", "force_tile", "pending")
    CHAIN_PLAN_FIELDS = ("wino", "sc_out", "rows16", "wino_stats", "stats", "bridge_w", "side")

    def op_adain_chain(self, seg: Segments, x, style, blocks, *, fold_rows=-1, fold16_rows=-1, rows16=-1, sc_side_min_rows=-1, affine_serial=False,
                       no_wino_conv2sc=False, no_stat_fuse=False, no_wino_stats=False, bridge=0, wino=False, stats=False, xs16=False, side=False, defer=False,
                       force_tile=0):
        """stts_op_adain_chain: one AdaptiveDecoderBlock or two chained ones under the caller's plan thresholds (-1: the engine's own) and offers.
        blocks: one or two dicts {prefix, cin, cout, y [rows, ldy] fp32, y16 (optional) [rows, ldy16] int16}, written INTO the caller's tensors (of a pair,
        blocks[0]["y"] already holds the constant columns).  Returns (chain plan, [block plans]) as dicts of integers (csrc/adain_block.hip.h)."""
        a = _lib.AdainChainArgs()
        ws = self.workspace(seg)
        plan = (C.c_int32 * (8 + 16 * len(blocks)))()
        assert x.dtype == torch.float32 and x.is_contiguous() and style.dtype == torch.float32 and style.is_contiguous()
        a.seg_off_host, a.seg_off_dev, a.n_utt, a.nblocks = seg.host_ptr, _ptr(seg.dev), seg.n, len(blocks)
        a.x, a.x_elems, a.ldx, a.style, a.style_elems = _ptr(x), x.numel(), x.shape[1], _ptr(style), style.numel()
        a.ws, a.ws_bytes, a.plan_out = _ptr(ws), ws.numel(), C.cast(plan, C.c_void_p)
        a.fold_rows, a.fold16_rows, a.rows16, a.sc_side_min_rows = fold_rows, fold16_rows, rows16, sc_side_min_rows
        a.affine_serial, a.no_wino_conv2sc, a.no_stat_fuse, a.no_wino_stats, a.bridge = int(affine_serial), int(no_wino_conv2sc), int(no_stat_fuse), int(no_wino_stats), bridge
        a.offer_wino, a.offer_stats, a.offer_rows16, a.offer_side, a.defer, a.force_tile = int(wino), int(stats), int(xs16), int(side), int(defer), force_tile
        for i, b in enumerate(blocks):
            y, y16 = b["y"], b.get("y16")
            assert y.dtype == torch.float32 and y.is_contiguous() and y.is_cuda and (y16 is None or (y16.dtype == torch.int16 and y16.is_contiguous() and y16.is_cuda))
            o = a.blocks[i]
            o.prefix, o.cin, o.cout = b["prefix"].encode(), b["cin"], b["cout"]
            o.y, o.y_elems, o.ldy = _ptr(y), y.numel(), y.shape[1]
            if y16 is not None:
                o.y16, o.y16_elems, o.ldy16 = _ptr(y16), y16.numel(), y16.shape[1]
        rc = self.lib.stts_op_adain_chain(self.ctx, _stream(), C.byref(a))
        v = list(plan)
        self.last_chain_plan = (dict(zip(self.CHAIN_PLAN_FIELDS, v[:8])), [dict(zip(self.BLOCK_PLAN_FIELDS, v[8 + 16 * i : 24 + 16 * i])) for i in range(len(blocks))])
        _lib.check(rc)
        return self.last_chain_plan

    def op_attention(self, seg_q: Segments, seg_k: Segments, q, k, v, heads: int, kc: int, band_centre=None, window: int = 0, kernel: int = 0):
        """Packed multi-head attention (test surface): q [q rows, heads * kc], k / v [k rows, heads * kc] -> [q rows, heads * kc]."""
        o = self._f32(seg_q.rows, heads * kc)
        _lib.check(self.lib.stts_op_attention(_stream(), seg_q.n, seg_q.host_ptr, _ptr(seg_q.dev), seg_k.host_ptr, _ptr(seg_k.dev), _ptr(q), _ptr(k), _ptr(v),
                                              _ptr(o), heads, kc, None if band_centre is None else _ptr(band_centre), window, kernel))
        return o

    def op_mrf_block(self, prefix: str, seg: Segments, x, channels, kernel, style):
        y = self._f32(seg.rows, channels)
        ws = self.workspace(seg)
        _lib.check(self.lib.stts_op_mrf_block(self.ctx, _stream(), prefix.encode(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], channels,
                                              kernel, _ptr(style), _ptr(y), channels, _ptr(ws), ws.numel()))
        return y

    # ------------------------------------------------------------------ vocoder STFT kernels at any geometry (test surface)
    def op_stft_geom(self, seg: Segments, sig: torch.Tensor, n_fft: int, win: int, h: int, generic: bool = True):
        """sig: packed samples, h per row -> spec, phase [rows, round_up(n_fft/2 + 1, 32)] (stts_op_stft_geom)."""
        ld = (n_fft // 2 + 1 + 31) // 32 * 32
        spec, phase = self._f32(seg.rows, ld), self._f32(seg.rows, ld)
        _lib.check(self.lib.stts_op_stft_geom(_stream(), seg.n, seg.host_ptr, _ptr(seg.dev), n_fft, win, h, _ptr(sig), _ptr(spec), _ptr(phase), ld,
                                              int(generic)))
        return spec, phase

    def op_istft_geom(self, seg: Segments, logamp: torch.Tensor, phase: torch.Tensor, n_fft: int, win: int, h: int, generic: bool = True):
        """logamp, phase [rows, ld] -> audio [rows * h] (stts_op_istft_geom: tanh of the iSTFT with the replicated last frame)."""
        audio = self._f32(seg.rows * h)
        _lib.check(self.lib.stts_op_istft_geom(_stream(), seg.n, seg.host_ptr, _ptr(seg.dev), n_fft, win, h, _ptr(logamp), _ptr(phase), logamp.shape[1],
                                               _ptr(audio), int(generic)))
        return audio

    # ------------------------------------------------------------------ conv-form STFT of the ONNX export (models/stft.py)
    def conv_stft_transform(self, seg_frames: Segments, wave: torch.Tensor, hop: int):
        """wave: packed samples, utterance u has (frames_u - 1) * hop of them -> mag, x, y [frames, 1056] time-major."""
        mag, x, y = (self._f32(seg_frames.rows, N_BINS_LD) for _ in range(3))
        _lib.check(self.lib.stts_conv_stft_transform(self.ctx, _stream(), seg_frames.n, seg_frames.host_ptr, _ptr(seg_frames.dev), _ptr(wave), hop,
                                                     _ptr(mag), _ptr(x), _ptr(y), N_BINS_LD))
        return mag, x, y

    def conv_stft_inverse(self, seg_frames: Segments, mag, x, y, hop: int):
        out = self._f32((seg_frames.rows - seg_frames.n) * hop)
        ws = self._f32(seg_frames.rows * 1200)
        _lib.check(self.lib.stts_conv_stft_inverse(self.ctx, _stream(), seg_frames.n, seg_frames.host_ptr, _ptr(seg_frames.dev), _ptr(mag), _ptr(x), _ptr(y),
                                                   mag.shape[1], hop, _ptr(out), _ptr(ws), ws.numel() * 4))
        return out

    # ------------------------------------------------------------------ phoneme-rate stages (packed tokens)
    def _ph_ws(self, seg_p: Segments, seg_t: Optional[Segments] = None) -> torch.Tensor:
        rows_t, max_t = (seg_t.rows, seg_t.max_len) if seg_t is not None else (0, 0)
        return self._grow(self._pws, int(self.lib.stts_phoneme_workspace_bytes(self.ctx, seg_p.rows, rows_t, seg_p.n, seg_p.max_len, max_t)))

    def text_encoder(self, which: int, seg: Segments, tokens: torch.Tensor, return_hidden=False):
        """tokens int64 [n_tok] (packed) -> mu [n_tok, inter] (+ last hidden [n_tok, 128])."""
        inter = self.cfg.pitch_energy_predictor.inter_dim if which == 2 else self.cfg.inter_dim
        mu = self._f32(seg.rows, inter)
        xh = self._f32(seg.rows, self.cfg.text_encoder.hidden_dim) if return_hidden else None
        ws = self._ph_ws(seg)
        _lib.check(self.lib.stts_text_encoder_forward(self.ctx, _stream(), which, seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(tokens), _ptr(mu), inter,
                                                      _ptr(xh), _ptr(ws), ws.numel()))
        return (mu, xh) if return_hidden else mu

    def text_style(self, which: int, seg: Segments, x: torch.Tensor):
        style = self._f32(seg.n, self.cfg.style_dim)
        ws = self._ph_ws(seg)
        _lib.check(self.lib.stts_text_style_forward(self.ctx, _stream(), which, seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), x.shape[1], _ptr(style),
                                                    _ptr(ws), ws.numel()))
        return style

    def duration(self, seg: Segments, tokens: torch.Tensor, taps=False):
        """-> logits [n_tok,16], dur int32 [n_tok] (+ dict of taps)."""
        logits = self._f32(seg.rows, 16)
        dur = torch.empty(seg.rows, dtype=torch.int32, device=self.device)
        t = None
        if taps:
            t = dict(text_mu=self._f32(seg.rows, self.cfg.inter_dim), style=self._f32(seg.n, self.cfg.style_dim),
                     prosody=self._f32(seg.rows, self.cfg.inter_dim + self.cfg.style_dim))
        ws = self._ph_ws(seg)
        _lib.check(self.lib.stts_duration_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(tokens), _ptr(logits), _ptr(dur),
                                                  _ptr(t["text_mu"]) if t else None, _ptr(t["style"]) if t else None,
                                                  _ptr(t["prosody"]) if t else None, _ptr(ws), ws.numel()))
        return (logits, dur, t) if taps else (logits, dur)

    def pitch_energy(self, seg_p: Segments, seg_t: Segments, dur: torch.Tensor, pe_enc: torch.Tensor, pe_style: torch.Tensor, taps=False):
        """dur int32 [n_tok]; -> f0, energy [n_frames] at the mel-frame rate."""
        f0 = self._f32(seg_t.rows)
        en = self._f32(seg_t.rows)
        C = self.cfg.pitch_energy_predictor.inter_dim + self.cfg.style_dim
        t = dict(prosody=self._f32(seg_p.rows, C), cross=self._f32(seg_t.rows, C)) if taps else None
        ws = self._ph_ws(seg_p, seg_t)
        _lib.check(self.lib.stts_pitch_energy_forward(self.ctx, _stream(), seg_p.n, seg_p.host_ptr, _ptr(seg_p.dev), seg_t.host_ptr, _ptr(seg_t.dev),
                                                      _ptr(dur), _ptr(pe_enc), pe_enc.shape[1], _ptr(pe_style), _ptr(f0), _ptr(en),
                                                      _ptr(t["prosody"]) if t else None, _ptr(t["cross"]) if t else None, _ptr(ws), ws.numel(), seg_t.flags))
        return (f0, en, t) if taps else (f0, en)

    def length_regulate(self, seg_p: Segments, seg_f: Segments, dur: torch.Tensor, rep: int, enc: torch.Tensor, C: int):
        """enc [n_tok, ld] -> [n_frames, C] rows gathered by the duration alignment at rate rep (1 or 4)."""
        out = self._f32(seg_f.rows, C)
        idx = torch.empty(seg_f.rows, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.stts_length_regulate(self.ctx, _stream(), seg_p.n, _ptr(dur), _ptr(seg_p.dev), _ptr(seg_f.dev), seg_f.rows, rep, _ptr(enc),
                                                 enc.shape[1], C, _ptr(out), C, _ptr(idx)))
        return out

    def upsample4(self, seg_t: Segments, seg_t4: Segments, x: torch.Tensor):
        y = self._f32(seg_t4.rows)
        _lib.check(self.lib.stts_upsample4(self.ctx, _stream(), seg_t.n, seg_t.host_ptr, _ptr(seg_t.dev), _ptr(seg_t4.dev), _ptr(x), _ptr(y)))
        return y

    # ------------------------------------------------------------------ HuBERT voice conversion (packed feature frames)
    def _hb_ws(self, rows_T: int, n_utt: int, max_len: int) -> torch.Tensor:
        return self._grow(self._pws, int(self.lib.stts_hubert_workspace_bytes(self.ctx, rows_T, n_utt, max_len)))

    def speaker_style(self, spk_emb: torch.Tensor, style: bool = True, pe_style: bool = True):
        """spk_emb [n_utt, ld >= speaker_embedder.hidden_dim] -> (style, pe_style) [n_utt, style_dim] each (None where not asked)."""
        n = spk_emb.shape[0]
        s = self._f32(n, self.cfg.style_dim) if style else None
        p = self._f32(n, self.cfg.style_dim) if pe_style else None
        ws = self._hb_ws(0, n, 1)
        _lib.check(self.lib.stts_speaker_style(self.ctx, _stream(), n, _ptr(spk_emb), spk_emb.shape[1], _ptr(s), _ptr(p), _ptr(ws), ws.numel()))
        return s, p

    def hubert_encoder(self, seg: Segments, feats: torch.Tensor) -> torch.Tensor:
        """feats [rows_T, ld] packed feature frames -> asr [4 rows_T, inter_dim] (decoder input at the vocoder-frame rate)."""
        asr = self._f32(4 * seg.rows, self.cfg.inter_dim)
        ws = self._hb_ws(seg.rows, seg.n, seg.max_len)
        _lib.check(self.lib.stts_hubert_encoder_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(feats), feats.shape[1], _ptr(asr),
                                                        asr.shape[1], _ptr(ws), ws.numel()))
        return asr

    def hubert_pitch_energy(self, seg: Segments, feats: torch.Tensor, pe_style: torch.Tensor, taps: bool = False):
        """feats [rows_T, ld], pe_style [n_utt, style_dim] -> f0, energy [rows_T] (+ prosody tap [rows_T, inter_dim + style_dim])."""
        f0, en = self._f32(seg.rows), self._f32(seg.rows)
        pros = self._f32(seg.rows, self.cfg.inter_dim + self.cfg.style_dim) if taps else None
        ws = self._hb_ws(seg.rows, seg.n, seg.max_len)
        _lib.check(self.lib.stts_hubert_pitch_energy_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(feats), feats.shape[1],
                                                             _ptr(pe_style), _ptr(f0), _ptr(en), _ptr(pros), _ptr(ws), ws.numel()))
        return (f0, en, pros) if taps else (f0, en)

    # ------------------------------------------------------------------ MelStyleEncoder (packed mel frames)
    def mel_style(self, which: int, seg: Segments, mel: torch.Tensor, style_dim: int, tap_floats: int = 0):
        """mel [rows_T, ld >= n_mels] packed time-major -> style [n_utt, style_dim] of the encoder `which` (STTS_W_PE_MEL_STYLE /
        STTS_W_CFM_PITCH); tap_floats > 0 also returns the four ResBlk outputs, flat (include/stylish_hip.h, stts_mel_style_forward_taps)."""
        need = int(self.lib.stts_mel_style_workspace_bytes(self.ctx, which, seg.rows, seg.n))
        if need == 0:
            _lib.check(1)  # the weights of `which` are not finalized: the library's message
        ws = self._grow(self._mws, need)
        out = self._f32(seg.n, style_dim)
        args = (self.ctx, _stream(), which, seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(mel), mel.shape[1], _ptr(out))
        if tap_floats:
            taps = self._f32(tap_floats)
            _lib.check(self.lib.stts_mel_style_forward_taps(*args, _ptr(taps), _ptr(ws), ws.numel()))
            return out, taps
        _lib.check(self.lib.stts_mel_style_forward(*args, _ptr(ws), ws.numel()))
        return out

    # ------------------------------------------------------------------ CfmPitchPredictor, frame-rate network (packed pitch frames)
    def cfm_pitch(self, seg: Segments, asr_rows: torch.Tensor, spk_style: torch.Tensor, f0_log2_stats=None, uv: Optional[torch.Tensor] = None,
                  taps: bool = False):
        """asr_rows [rows_T, ld >= asr_dim] packed time-major, spk_style [n_utt, 256] (mel_style(W_CFM_PITCH)) -> normed F0 [rows_T];
        with f0_log2_stats = (log2 mean, log2 std) also F0 in Hz [rows_T] (denorm_f0_zscore; uv [rows_T] > 0 -> 0), returned as
        (normed, hz); taps=True appends [5, rows_T, 256] (asr_emb output, then each ConvNeXt block's).  include/stylish_hip.h,
        stts_cfm_pitch_forward."""
        need = int(self.lib.stts_cfm_pitch_workspace_bytes(self.ctx, seg.rows, seg.n))
        if need == 0:
            _lib.check(1)  # the weights are not finalized: the library's message
        ws = self._grow(self._cpws, need)
        normed = self._f32(seg.rows)
        hz = self._f32(seg.rows) if f0_log2_stats is not None else None
        mean, std = (float(f0_log2_stats[0]), float(f0_log2_stats[1])) if f0_log2_stats is not None else (0.0, 1.0)
        if uv is not None:
            uv = uv.to(self.device, torch.float32).contiguous()
        spk = spk_style.to(self.device, torch.float32).contiguous()
        args = (self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(asr_rows), asr_rows.shape[1], _ptr(spk), _ptr(normed),
                _ptr(hz), mean, std, _ptr(uv))
        out = [normed] + ([hz] if hz is not None else [])
        if taps:
            t = self._f32(5, seg.rows, 256)
            _lib.check(self.lib.stts_cfm_pitch_forward_taps(*args, _ptr(t), _ptr(ws), ws.numel()))
            out.append(t)
        else:
            _lib.check(self.lib.stts_cfm_pitch_forward(*args, _ptr(ws), ws.numel()))
        return out[0] if len(out) == 1 else tuple(out)

    # ------------------------------------------------------------------ AdaptiveHubert, the HuBERT content encoder (packed waveforms)
    def ssl_finalize(self, arch) -> None:
        """Pack the weights loaded under "hubert." for the HubertConfig fields ``arch`` (hubert_ssl.arch); include/stylish_hip.h, stts_ssl_finalize."""
        from . import hubert_ssl

        self._ssl_arch = dict(arch)
        self._ssl_dims = hubert_ssl.dims_struct(arch)
        _lib.check(self.lib.stts_ssl_finalize(self.ctx, C.byref(self._ssl_dims)))

    def hubert_ssl(self, seg_s: Segments, wave: torch.Tensor, seg_t: Segments, ld: Optional[int] = None, taps: bool = False):
        """wave [sum samples] packed mono audio at hubert.sr (utterance offsets seg_s), seg_t: the time_dim of every utterance ->
        feats [sum time_dim, ld] packed time-major rows (ld: hidden_size padded to 32 unless given; pad columns zero), the ``feats`` of
        hubert_encoder / hubert_pitch_energy / cfm_pitch.  taps=True also returns a dict of intermediate rows (include/stylish_hip.h,
        stts_ssl_forward_taps; "frames": the per-utterance frame counts).  Nothing is read back by the host."""
        from . import hubert_ssl

        if getattr(self, "_ssl_dims", None) is None:
            _lib.check(self.lib.stts_ssl_forward(self.ctx, _stream(), 0, None, None, None, None, None, None, 0, None, 0))  # not finalized: the library's message
        a = self._ssl_arch
        H = a["hidden_size"]
        ld = (H + 31) // 32 * 32 if ld is None else int(ld)
        if seg_s.n != seg_t.n:
            raise ValueError(f"{seg_s.n} utterances of audio but {seg_t.n} time_dim entries")
        need = int(self.lib.stts_ssl_workspace_bytes(self.ctx, seg_s.n, seg_s.host_ptr))
        if need == 0:
            # too short an utterance (or bad offsets): let the entry point name it, it fails before any launch
            need = 256
        ws = self._grow(self._sslws, need)
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg_s.rows:
            raise ValueError(f"packed waveform of {wave.numel()} samples, the offsets describe {seg_s.rows}")
        feats = self._f32(seg_t.rows, ld)
        args = (self.ctx, _stream(), seg_s.n, seg_s.host_ptr, _ptr(seg_s.dev), _ptr(wave), seg_t.host_ptr, _ptr(seg_t.dev), _ptr(feats), ld)
        if not taps:
            _lib.check(self.lib.stts_ssl_forward(*args, _ptr(ws), ws.numel()))
            return feats
        fr = [hubert_ssl.frames(n, a) if n >= hubert_ssl.min_samples(a) else 0 for n in seg_s.lengths]
        F, rows0 = sum(fr), int(self.lib.stts_ssl_tap_rows(C.byref(self._ssl_dims), seg_s.n, seg_s.host_ptr))
        t = dict(conv0=self._f32(max(rows0, 1), a["conv_dim"][0]), conv0_off=torch.zeros(seg_s.n + 1, dtype=torch.int32, device=self.device),
                 conv_last=self._f32(max(F, 1), a["conv_dim"][-1]), proj=self._f32(max(F, 1), H), pos=self._f32(max(F, 1), H),
                 layers=self._f32(a["num_hidden_layers"], max(F, 1), H), hidden=self._f32(max(F, 1), H))
        _lib.check(self.lib.stts_ssl_forward_taps(*args, _ptr(t["conv0"]), _ptr(t["conv0_off"]), _ptr(t["conv_last"]), _ptr(t["proj"]), _ptr(t["pos"]),
                                                  _ptr(t["layers"]), _ptr(t["hidden"]), _ptr(ws), ws.numel()))
        t["frames"] = fr
        return feats, t

    # ------------------------------------------------------------------ WavLM and its perceptual distance (packed waveforms at 16 kHz)
    def wavlm_finalize(self, arch) -> None:
        """Pack the weights loaded under "wavlm." for the WavLMConfig fields ``arch`` (wavlm.arch); include/stylish_hip.h, stts_wavlm_finalize."""
        from . import wavlm

        self._wavlm_arch = dict(arch)
        self._wavlm_dims = wavlm.dims_struct(arch)
        _lib.check(self.lib.stts_wavlm_finalize(self.ctx, C.byref(self._wavlm_dims)))

    def _wavlm_ws(self, seg_s: Segments, wave: torch.Tensor, pairs: int):
        if getattr(self, "_wavlm_dims", None) is None:
            _lib.check(self.lib.stts_wavlm_forward_states(self.ctx, _stream(), 0, None, None, None, None, None, None, 0))  # not finalized: the library's message
        # 0: too short an utterance, an unequal pair or bad offsets - the entry point names it, it fails before any launch
        need = int(self.lib.stts_wavlm_workspace_bytes(self.ctx, seg_s.n, seg_s.host_ptr, pairs)) or 256
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg_s.rows:
            raise ValueError(f"packed waveform of {wave.numel()} samples, the offsets describe {seg_s.rows}")
        return self._grow(self._sslws, need), wave

    def wavlm_states(self, seg_s: Segments, wave: torch.Tensor, gate: bool = False):
        """wave [sum samples] packed mono audio at 16 kHz -> states [layers + 1, sum frames, hidden]: transformers' hidden_states, packed rows.
        gate=True also returns layer 0's gate [sum frames, heads] (a test tap).  Nothing is read back by the host."""
        from . import hubert_ssl

        ws, wave = self._wavlm_ws(seg_s, wave, 0)
        a = self._wavlm_arch
        F = sum(hubert_ssl.frames(n, a) if n >= hubert_ssl.min_samples(a) else 0 for n in seg_s.lengths)
        states = self._f32(a["num_hidden_layers"] + 1, max(F, 1), a["hidden_size"])
        g0 = self._f32(max(F, 1), a["num_attention_heads"]) if gate else None
        _lib.check(self.lib.stts_wavlm_forward_states(self.ctx, _stream(), seg_s.n, seg_s.host_ptr, _ptr(seg_s.dev), _ptr(wave), _ptr(states),
                                                      _ptr(g0) if gate else None, _ptr(ws), ws.numel()))
        return (states, g0) if gate else states

    def wavlm_l1(self, seg_s: Segments, wave: torch.Tensor):
        """2 B packed waveforms, utterances u and u + B of equal length -> (sums [B, layers + 1] float64, frames [B] int32), both on the device:
        the sums of |difference| of every hidden state over the pair's frames and channels (stts_wavlm_l1_sums).  Nothing is read back."""
        if seg_s.n % 2:
            raise ValueError(f"{seg_s.n} utterances do not form pairs")
        B = seg_s.n // 2
        ws, wave = self._wavlm_ws(seg_s, wave, B)
        sums = torch.empty(max(B, 1), self._wavlm_arch["num_hidden_layers"] + 1, dtype=torch.float64, device=self.device)
        fr = torch.empty(max(B, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.stts_wavlm_l1_sums(self.ctx, _stream(), B, seg_s.host_ptr, _ptr(seg_s.dev), _ptr(wave), _ptr(sums), _ptr(fr), _ptr(ws), ws.numel()))
        return sums, fr

    def wavlm_bucket_table(self, max_d: int) -> "np.ndarray":
        """The bucket of rel_attn_embed the attention reads at every distance -max_d .. max_d (int32 [2 max_d + 1]); stts_wavlm_bucket_table."""
        out = np.zeros(2 * int(max_d) + 1, np.int32)
        _lib.check(self.lib.stts_wavlm_bucket_table(self.ctx, int(max_d), out.ctypes.data_as(C.c_void_p)))
        return out

    # ------------------------------------------------------------------ RMVPE pitch extractor (packed log-mel frames at 100 frames / s)
    def rmvpe_finalize(self, dims) -> None:
        """Pack the weights loaded under "rmvpe." for E2E0's constructor arguments ``dims`` (rmvpe.dims); include/stylish_hip.h, stts_rmvpe_finalize."""
        from . import rmvpe

        self._rv_dims_d = dict(dims)
        self._rv_dims = rmvpe.dims_struct(dims)
        _lib.check(self.lib.stts_rmvpe_finalize(self.ctx, C.byref(self._rv_dims)))

    def rmvpe(self, seg: Segments, mel_rows: torch.Tensor, thred: float = 0.03, hidden: bool = True, f0: bool = True, taps: bool = False):
        """mel_rows [rows_T, ld >= 128] packed time-major log-mel frames (utterance offsets seg, at least 17 frames each) -> (hidden [rows_T, 360]
        or None, f0 [rows_T] in Hz or None); taps=True appends the flat tap buffer (include/stylish_hip.h, stts_rmvpe_forward_taps).  Nothing is
        read back by the host."""
        if getattr(self, "_rv_dims", None) is None:
            _lib.check(self.lib.stts_rmvpe_forward(self.ctx, _stream(), 0, None, None, None, 0, 0.0, None, None, None, 0))  # not finalized: the library's message
        if mel_rows.dim() != 2 or mel_rows.shape[0] != seg.rows:
            raise ValueError(f"packed mel of shape {tuple(mel_rows.shape)}, the offsets describe {seg.rows} frames")
        need = int(self.lib.stts_rmvpe_workspace_bytes(self.ctx, seg.n, seg.host_ptr)) or 256  # 0: too short an utterance - the entry point names it
        ws = self._grow(self._rvws, need)
        mel_rows = mel_rows.to(self.device, torch.float32).contiguous()
        h = self._f32(seg.rows, 360) if hidden else None
        f = self._f32(seg.rows) if f0 else None
        args = (self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(mel_rows), mel_rows.shape[1], float(thred), _ptr(h), _ptr(f))
        if not taps:
            _lib.check(self.lib.stts_rmvpe_forward(*args, _ptr(ws), ws.numel()))
            return h, f
        t = self._f32(max(1, int(self.lib.stts_rmvpe_tap_floats(C.byref(self._rv_dims), seg.n, seg.host_ptr))))
        _lib.check(self.lib.stts_rmvpe_forward_taps(*args, _ptr(t), _ptr(ws), ws.numel()))
        return h, f, t

    def rmvpe_mel(self, seg_s: Segments, wave: torch.Tensor, basis: torch.Tensor, band: torch.Tensor, linear: bool = False):
        """wave [sum samples] packed mono audio at 16 kHz -> (log-mel rows [sum frames, 128], their Segments); linear=True also returns the mel
        before the clamp and the log.  basis [128, 513] float32 and band [128, 2] int32 on the device (include/stylish_hip.h, stts_rmvpe_mel)."""
        from . import rmvpe

        seg_m = Segments([rmvpe.mel_frames(n) for n in seg_s.lengths], self.device)
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg_s.rows:
            raise ValueError(f"packed waveform of {wave.numel()} samples, the offsets describe {seg_s.rows}")
        out = self._f32(seg_m.rows, 128)
        lin = self._f32(seg_m.rows, 128) if linear else None
        _lib.check(self.lib.stts_rmvpe_mel(self.ctx, _stream(), seg_s.n, seg_s.host_ptr, _ptr(seg_s.dev), seg_m.host_ptr, _ptr(seg_m.dev), _ptr(wave), _ptr(basis),
                                           _ptr(band), _ptr(out), 128, _ptr(lin)))
        return (out, seg_m, lin) if linear else (out, seg_m)

    def rmvpe_decode(self, salience: torch.Tensor, thred: float = 0.03, center: Optional[torch.Tensor] = None) -> torch.Tensor:
        """salience [rows, 360] -> f0 [rows] in Hz (to_local_average_f0; include/stylish_hip.h, stts_rmvpe_decode).  ``center`` [rows] int: the local
        average around these bins, not around every row's argmax (stts_rmvpe_decode_at)."""
        s = salience.to(self.device, torch.float32).contiguous()
        if s.dim() != 2 or s.shape[1] != 360 or s.shape[0] < 1:
            raise ValueError(f"salience must be [rows, 360], got shape {tuple(s.shape)}")
        out = self._f32(s.shape[0])
        if center is None:
            _lib.check(self.lib.stts_rmvpe_decode(self.ctx, _stream(), s.shape[0], _ptr(s), 360, float(thred), _ptr(out)))
            return out
        c = center.to(self.device, torch.int32).contiguous()
        if c.dim() != 1 or c.numel() != s.shape[0]:
            raise ValueError(f"{c.numel()} centres for {s.shape[0]} rows")
        _lib.check(self.lib.stts_rmvpe_decode_at(self.ctx, _stream(), s.shape[0], _ptr(s), 360, _ptr(c), float(thred), _ptr(out)))
        return out

    def rmvpe_viterbi(self, seg: Segments, salience: torch.Tensor, thred: float = 0.03, path: bool = False, logp: bool = False):
        """to_viterbi_f0 on the device (include/stylish_hip.h, stts_rmvpe_viterbi): salience [rows, 360] packed rows with frame offsets seg (at least one
        frame each) -> f0 [rows] in Hz around the best path through the 360 classes; path=True / logp=True append the path [rows] int32 and its score
        [B] float64.  Nothing is read back by the host."""
        from . import rmvpe

        s = salience.to(self.device, torch.float32).contiguous()
        if s.dim() != 2 or s.shape[1] != 360 or s.shape[0] != seg.rows:
            raise ValueError(f"salience of shape {tuple(s.shape)}, the offsets describe {seg.rows} rows of 360 classes")
        band, lt_out, eps = rmvpe.viterbi_tables()
        if self._rv_lt is None:
            self._rv_lt = torch.from_numpy(band.copy()).to(self.device)
        need = int(self.lib.stts_rmvpe_viterbi_workspace_bytes(seg.n, seg.host_ptr)) or 256  # 0: an empty utterance - the entry point names it
        ws = self._grow(self._rvvws, need)
        f0 = self._f32(seg.rows)
        p = torch.empty(seg.rows, dtype=torch.int32, device=self.device) if path else None
        lp = torch.empty(seg.n, dtype=torch.float64, device=self.device) if logp else None
        _lib.check(self.lib.stts_rmvpe_viterbi(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(s), 360, _ptr(self._rv_lt), lt_out, eps, float(thred),
                                               _ptr(p), _ptr(lp), _ptr(f0), _ptr(ws), ws.numel()))
        out = (f0,) + ((p,) if path else ()) + ((lp,) if logp else ())
        return out[0] if len(out) == 1 else out

    def rmvpe_resample(self, seg_in: Segments, f0: torch.Tensor, seg_out: Segments) -> torch.Tensor:
        """Packed curves at seg_in's frames -> packed curves at seg_out's frames, linear with align_corners=True, on the device."""
        if seg_in.n != seg_out.n or f0.numel() != seg_in.rows:
            raise ValueError(f"{f0.numel()} values for {seg_in.rows} frames in {seg_in.n} utterances, {seg_out.n} output utterances")
        out = self._f32(seg_out.rows)
        _lib.check(self.lib.stts_rmvpe_resample(self.ctx, _stream(), seg_in.n, _ptr(seg_in.dev), seg_out.host_ptr, _ptr(seg_out.dev), _ptr(f0.contiguous()), _ptr(out)))
        return out

    # ------------------------------------------------------------------ log-mel front end (packed waveforms at the model's sample rate)
    def _log_mel_args(self, seg_s: Segments, wave: torch.Tensor, n_fft, win_length, hop_length, n_mels, sample_rate, frames):
        from . import log_mel

        log_mel.check_geometry(n_fft, win_length, hop_length, n_mels, sample_rate)
        seg_m = Segments(log_mel.frame_counts(seg_s.lengths, int(n_fft), int(hop_length), frames), self.device)
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg_s.rows:
            raise ValueError(f"packed waveform of {wave.numel()} samples, the offsets describe {seg_s.rows}")
        args = (self.ctx, _stream(), seg_s.n, seg_s.host_ptr, _ptr(seg_s.dev), seg_m.host_ptr, _ptr(seg_m.dev), _ptr(wave), int(n_fft), int(win_length),
                int(hop_length), int(n_mels), int(sample_rate))
        return seg_m, wave, args

    def log_mel(self, seg_s: Segments, wave: torch.Tensor, n_fft: int, win_length: int, hop_length: int, n_mels: int, sample_rate: int, mean: float = -4.0,
                std: float = 4.0, frames: str = "even", ld: Optional[int] = None, mel: bool = True, energy: bool = False, raw: bool = False,
                out: Optional[torch.Tensor] = None):
        """wave [sum samples] packed mono audio at sample_rate (utterance offsets seg_s) -> (mel rows [sum frames, ld >= n_mels] or None, their Segments
        [, energy [sum frames]][, raw log-mel rows]): (log(1e-5 + MelSpectrogram(wave)) - mean) / std as the packed time-major rows mel_style /
        text_aligner read, in one launch (include/stylish_hip.h, stts_log_mel_forward).  frames: "even" (calculate_mel), "drop_last" (preprocess) or "all"
        (log_mel.frames).  out: rows to write into (columns >= n_mels keep their values).  ValueError for a geometry or a length the transform
        refuses.  Nothing is read back by the host."""
        seg_m, wave, args = self._log_mel_args(seg_s, wave, n_fft, win_length, hop_length, n_mels, sample_rate, frames)
        if not (mel or energy or raw):
            raise ValueError("log_mel: no output asked for")
        ld = int(n_mels) if ld is None else int(ld)
        if out is not None:
            if out.dtype != torch.float32 or out.device != self.device or out.dim() != 2 or out.shape[0] != seg_m.rows or not out.is_contiguous():
                raise ValueError(f"out must be contiguous float32 [{seg_m.rows}, ld] on {self.device}, got {tuple(out.shape)}")
            ld, mel = out.shape[1], True
        if ld < int(n_mels):
            raise ValueError(f"ld {ld} < n_mels {n_mels}")
        rows = out if out is not None else (self._f32(seg_m.rows, ld) if mel else None)
        en = self._f32(seg_m.rows) if energy else None
        rw = self._f32(seg_m.rows, ld) if raw else None
        _lib.check(self.lib.stts_log_mel_forward(*args, float(mean), float(std), _ptr(rows), ld, _ptr(en), _ptr(rw)))
        return (rows, seg_m) + ((en,) if energy else ()) + ((rw,) if raw else ())

    def log_mel_stats(self, seg_s: Segments, wave: torch.Tensor, n_fft: int, win_length: int, hop_length: int, n_mels: int, sample_rate: int,
                      return_partials: bool = False):
        """compute_log_mel_stats (train/utils.py:80-148) of the packed recordings on the device, over all samples // hop + 1 frames of each:
        (mean, std, count) as Python numbers (the one host read; include/stylish_hip.h, stts_log_mel_stats); return_partials=True appends the
        per-frame sums [sum frames, 2] (float64, on the device) and their Segments."""
        seg_m, wave, args = self._log_mel_args(seg_s, wave, n_fft, win_length, hop_length, n_mels, sample_rate, "all")
        part = torch.empty(seg_m.rows, 2, dtype=torch.float64, device=self.device)
        stats = torch.empty(3, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_log_mel_stats(*args, _ptr(part), _ptr(stats)))
        m, s, n = stats.cpu().tolist()
        return (m, s, int(n)) + ((part, seg_m) if return_partials else ())

    # ------------------------------------------------------------------ validation scores (packed waveforms; csrc/val_scores.hip.h)
    def _packed_wave(self, seg: Segments, wave: torch.Tensor, what: str = "waveform") -> torch.Tensor:
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg.rows:
            raise ValueError(f"packed {what} of {wave.numel()} samples, the offsets describe {seg.rows}")
        return wave

    def multi_spectrogram(self, seg: Segments, wave: torch.Tensor, n_fft: int, win: int, hop: int, n_mels: int = 128, sample_rate: Optional[int] = None,
                          mag: bool = True, phase: bool = False, fft_mag: bool = False, ld_mag: Optional[int] = None, ld_bins: Optional[int] = None,
                          out: Optional[Dict[str, torch.Tensor]] = None):
        """MultiSpectrogram.calculate_single (train/multi_spectrogram.py:40-55) of the packed recordings as time-major rows over all samples // hop + 1
        frames of each: -> (their Segments, mag [rows, ld_mag >= n_mels] = log1p of the mel of |X|, phase [rows, ld_bins >= n_fft / 2 + 1] =
        (|X| > 1e-3) * angle(X), fft_mag [rows, ld_bins] = |X|), None for what was not asked.  out: {"mag" | "phase" | "fft_mag": rows to write into}
        (columns beyond the width keep their values).  fp64 arithmetic, one rounding (include/stylish_hip.h, stts_multi_spectrogram_forward).
        ValueError for a geometry or a length the transform refuses.  Nothing is read back by the host."""
        from . import val_scores

        sr = int(self.cfg.sample_rate if sample_rate is None else sample_rate)
        val_scores.check_geometry(n_fft, win, hop, n_mels, sr)
        seg_m = Segments(val_scores.frame_counts(seg.lengths, int(n_fft), int(hop)), self.device)
        wave = self._packed_wave(seg, wave)
        out = dict(out or {})
        if not (mag or phase or fft_mag or out):
            raise ValueError("multi_spectrogram: no output asked for")
        bins = int(n_fft) // 2 + 1
        ld_mag = int(n_mels) if ld_mag is None else int(ld_mag)
        ld_bins = bins if ld_bins is None else int(ld_bins)
        for k, t in out.items():
            if k not in ("mag", "phase", "fft_mag"):
                raise ValueError(f"out has no {k!r}")
            if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[0] != seg_m.rows or not t.is_contiguous():
                raise ValueError(f"out[{k!r}] must be contiguous float32 [{seg_m.rows}, ld] on {self.device}, got {tuple(t.shape)}")
        if "mag" in out:
            ld_mag = out["mag"].shape[1]
        if "phase" in out or "fft_mag" in out:
            ld_bins = out.get("phase", out.get("fft_mag")).shape[1]
            if any(out[k].shape[1] != ld_bins for k in ("phase", "fft_mag") if k in out):
                raise ValueError("out['phase'] and out['fft_mag'] must share one row stride")
        if ld_mag < int(n_mels) or ld_bins < bins:
            raise ValueError(f"ld_mag {ld_mag} < n_mels {n_mels} or ld_bins {ld_bins} < {bins} bins")
        mg = out["mag"] if "mag" in out else (self._f32(seg_m.rows, ld_mag) if mag else None)
        ph = out["phase"] if "phase" in out else (self._f32(seg_m.rows, ld_bins) if phase else None)
        fm = out["fft_mag"] if "fft_mag" in out else (self._f32(seg_m.rows, ld_bins) if fft_mag else None)
        _lib.check(self.lib.stts_multi_spectrogram_forward(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), seg_m.host_ptr, _ptr(seg_m.dev), _ptr(wave),
                                                           int(n_fft), int(win), int(hop), int(n_mels), sr, _ptr(mg), ld_mag, _ptr(fm), _ptr(ph), ld_bins))
        return seg_m, mg, ph, fm

    def mel_sums(self, seg: Segments, target: torch.Tensor, pred: torch.Tensor, resolutions=None, n_mels: int = 128, sample_rate: Optional[int] = None,
                 seg_pred: Optional[Segments] = None, return_partials: bool = False):
        """The sums of MultiResolutionSTFTLoss (train/losses.py:14-35) over the packed pairs (target, pred), one fused launch per resolution and no
        spectrogram written: -> [R, B, 2] float64 on the device, [r, u] = (sum |t - p|, sum |t|) of utterance u's log1p mel spectrogram at resolution r
        (include/stylish_hip.h, stts_val_mel_sums).  resolutions: Resolution-like objects or (fft, hop, window) tuples, default the reference's three.
        seg_pred: the prediction's own offsets when they were built apart; ValueError naming an utterance whose sample counts differ.
        return_partials=True appends the list of per-frame partials [rows_r, 2] and of their Segments."""
        from . import val_scores

        sr = int(self.cfg.sample_rate if sample_rate is None else sample_rate)
        res = [val_scores.as_tuple(r) for r in (val_scores.resolutions if resolutions is None else resolutions)]
        seg_pred = seg if seg_pred is None else seg_pred
        val_scores.check_pair(seg.lengths, seg_pred.lengths)
        target, pred = self._packed_wave(seg, target, "target"), self._packed_wave(seg_pred, pred, "prediction")
        sums = torch.empty(len(res), seg.n, 2, dtype=torch.float64, device=self.device)
        parts, segs = [], []
        for i, (fft, hop, window) in enumerate(res):
            val_scores.check_geometry(fft, window, hop, n_mels, sr)
            sz = val_scores.sizes(seg.lengths, fft, hop)
            seg_m = Segments(val_scores.frame_counts(seg.lengths, fft, hop), self.device)
            part = torch.empty(sz["mel_partials"], dtype=torch.float64, device=self.device)
            _lib.check(self.lib.stts_val_mel_sums(self.ctx, _stream(), seg.n, seg.host_ptr, seg_pred.host_ptr, _ptr(seg.dev), seg_m.host_ptr, _ptr(seg_m.dev),
                                                  _ptr(target), _ptr(pred), fft, window, hop, int(n_mels), sr, _ptr(part), _ptr(sums[i])))
            parts.append(part.view(-1, 2))
            segs.append(seg_m)
        return (sums, parts, segs) if return_partials else sums

    def magphase_sums(self, seg_samples: Segments, gt: torch.Tensor, seg_rows: Segments, logamp_rows: torch.Tensor, phase_rows: torch.Tensor, ld: int,
                      n_fft: int, win: int, hop: int) -> torch.Tensor:
        """The sums of MagPhaseLoss.forward (train/losses.py:85-154) over the packed recordings gt and the prediction's log-magnitude / phase as
        time-major rows [rows, ld >= n_fft / 2 + 1] (what vocoder(return_spec=True) returns, plus the reference's repeated last frame): hop is the
        transform's (the reference's hop_length // 4).  -> [B, 4] float64 on the device: the L1 sum of "mag" and the three weighted anti-wrapping
        sums of "phase" (include/stylish_hip.h, stts_val_magphase_sums).  phase_rows is not modified.  ValueError naming an utterance whose row
        count is not samples // hop + 1."""
        from . import val_scores

        val_scores.check_geometry(n_fft, win, hop)
        val_scores.frame_counts(seg_samples.lengths, int(n_fft), int(hop))
        val_scores.check_rows(seg_samples.lengths, seg_rows.lengths, hop)
        gt = self._packed_wave(seg_samples, gt, "recording")
        ld = int(ld)
        for name, t in (("logamp_rows", logamp_rows), ("phase_rows", phase_rows)):
            if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or tuple(t.shape) != (seg_rows.rows, ld) or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous float32 [{seg_rows.rows}, {ld}] on {self.device}, got {tuple(t.shape)}")
        if ld < int(n_fft) // 2 + 1:
            raise ValueError(f"ld {ld} < {int(n_fft) // 2 + 1} bins")
        sz = val_scores.sizes(seg_samples.lengths, n_fft, hop)
        scratch = torch.empty(sz["magphase_scratch"], dtype=torch.float64, device=self.device)
        part = torch.empty(sz["magphase_partials"], dtype=torch.float64, device=self.device)
        sums = torch.empty(seg_samples.n, 4, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_val_magphase_sums(self.ctx, _stream(), seg_samples.n, seg_samples.host_ptr, _ptr(seg_samples.dev), seg_rows.host_ptr,
                                                   _ptr(seg_rows.dev), _ptr(gt), _ptr(logamp_rows), _ptr(phase_rows), ld, int(n_fft), int(win), int(hop),
                                                   _ptr(scratch), _ptr(part), _ptr(sums)))
        return sums

    def smooth_l1_sums(self, seg: Segments, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """[B] float64 on the device: each utterance's sum of smooth_l1(a - b), beta 1, over the packed fp32 vectors a and b (utterance offsets seg),
        added in a fixed order (include/stylish_hip.h, stts_val_smooth_l1_sums).  The reference's mean is sums.sum() / seg.rows."""
        a, b = self._packed_wave(seg, a, "vector a"), self._packed_wave(seg, b, "vector b")
        if min(seg.lengths) < 1:
            raise ValueError(f"utterance {seg.lengths.index(min(seg.lengths))} has no values")
        sums = torch.empty(seg.n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_val_smooth_l1_sums(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(a), _ptr(b), _ptr(sums)))
        return sums

    # ------------------------------------------------------------------ windowed-sinc resampler (packed waveforms at any rate)
    def resample(self, seg_in: Segments, wave: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                 resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None):
        """wave [sum samples] packed mono audio at orig_freq (utterance offsets seg_in) -> (wave_out [sum ceil(n samples / o)] at new_freq, seg_out):
        torchaudio.transforms.Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta) of every utterance on its own, with
        the float64 result as the target (fp64 coefficients, products and sums, one rounding; include/stylish_hip.h, stts_resample_forward).  Equal
        rates return a copy of the input.  ValueError outside the limits of resample.check.  Nothing is read back by the host."""
        from . import resample

        _, _, _, _, method, b = resample.check(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        seg_out = Segments(resample.out_lengths(seg_in.lengths, orig_freq, new_freq), self.device)
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() != 1 or wave.numel() != seg_in.rows:
            raise ValueError(f"packed waveform of {wave.numel()} samples, the offsets describe {seg_in.rows}")
        out = self._f32(seg_out.rows)
        _lib.check(self.lib.stts_resample_forward(self.ctx, _stream(), int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), method, b,
                                                  seg_in.n, seg_in.host_ptr, _ptr(seg_in.dev), seg_out.host_ptr, _ptr(seg_out.dev), _ptr(wave), _ptr(out)))
        return out, seg_out

    # ------------------------------------------------------------------ text aligner + CTC forced alignment (packed normalised log-mel rows)
    def aligner_finalize(self, dims) -> None:
        """Pack the weights loaded under "text_aligner." for the dims of aligner.dims(); include/stylish_hip.h, stts_aligner_finalize."""
        from . import aligner

        self._al_dims_d = dict(dims)
        self._al_dims = aligner.dims_struct(dims)
        _lib.check(self.lib.stts_aligner_finalize(self.ctx, C.byref(self._al_dims)))

    def text_aligner(self, seg: Segments, mel_rows: torch.Tensor, taps: bool = False):
        """mel_rows [rows_T, ld >= n_mels] packed time-major normalised log-mel (utterance offsets seg) -> log_probs [rows_T, classes]; taps=True
        also returns a dict of the intermediate rows (include/stylish_hip.h, stts_aligner_forward_taps).  Nothing is read back by the host."""
        if getattr(self, "_al_dims", None) is None:
            _lib.check(self.lib.stts_aligner_forward(self.ctx, _stream(), 0, None, None, None, 0, None, 0, None, 0))  # not finalized: the library's message
        if mel_rows.dim() != 2 or mel_rows.shape[0] != seg.rows:
            raise ValueError(f"packed mel of shape {tuple(mel_rows.shape)}, the offsets describe {seg.rows} frames")
        d = self._al_dims_d
        need = int(self.lib.stts_aligner_workspace_bytes(self.ctx, seg.n, seg.host_ptr)) or 256  # 0: bad offsets - the entry point names them
        ws = self._grow(self._alws, need)
        mel_rows = mel_rows.to(self.device, torch.float32).contiguous()
        V, H = d["classes"], d["hidden"]
        lp = self._f32(seg.rows, V)
        args = (self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(mel_rows), mel_rows.shape[1], _ptr(lp), V)
        if not taps:
            _lib.check(self.lib.stts_aligner_forward(*args, _ptr(ws), ws.numel()))
            return lp
        t = self._f32(max(1, int(self.lib.stts_aligner_tap_floats(C.byref(self._al_dims), seg.n, seg.host_ptr))))
        _lib.check(self.lib.stts_aligner_forward_taps(*args, _ptr(t), _ptr(ws), ws.numel()))
        R, n = seg.rows, len(d["tdnn_kernel"])
        out = {f"tdnn{i}": t[i * R * H : (i + 1) * R * H].view(R, H) for i in range(n)}
        out["ffn"] = t[n * R * H : (n + 1) * R * H].view(R, H)
        out["logits"] = t[(n + 1) * R * H : (n + 1) * R * H + R * V].view(R, V)
        return lp, out

    def ctc_align(self, seg_t: Segments, log_probs: torch.Tensor, seg_p: Segments, targets: torch.Tensor, blank: int, path: Optional[torch.Tensor] = None):
        """CTC forced alignment and torch_align's post-processing on the device (include/stylish_hip.h, stts_ctc_align): log_probs [sum T, ld] with
        frame offsets seg_t, targets [sum P] with token offsets seg_p -> dict(path [sum T] int32, scores [sum T], durations [sum P] int32,
        left [sum P], right [sum P]).  ``path`` given: only the post-processing runs on it.  Nothing is read back by the host."""
        if seg_t.n != seg_p.n:
            raise ValueError(f"{seg_t.n} utterances of frames but {seg_p.n} of tokens")
        lp = log_probs.to(self.device, torch.float32).contiguous()
        if lp.dim() != 2 or lp.shape[0] != seg_t.rows:
            raise ValueError(f"log-probs of shape {tuple(lp.shape)}, the offsets describe {seg_t.rows} frames")
        tg = targets.to(self.device, torch.int32).contiguous()
        if tg.dim() != 1 or tg.numel() != seg_p.rows:
            raise ValueError(f"{tg.numel()} targets, the offsets describe {seg_p.rows}")
        given = path is not None
        if given:
            p = path.to(self.device, torch.int32).contiguous().clone()
            if p.dim() != 1 or p.numel() != seg_t.rows:
                raise ValueError(f"a path of {p.numel()} labels for {seg_t.rows} frames")
            ws = None
        else:
            p = torch.empty(seg_t.rows, dtype=torch.int32, device=self.device)
            need = int(self.lib.stts_ctc_align_workspace_bytes(seg_t.n, seg_t.host_ptr, seg_p.host_ptr)) or 256  # 0: bad offsets - the entry point names them
            ws = self._grow(self._ctcws, need)
        out = dict(path=p, scores=self._f32(seg_t.rows), durations=torch.empty(seg_p.rows, dtype=torch.int32, device=self.device), left=self._f32(seg_p.rows),
                   right=self._f32(seg_p.rows))
        _lib.check(self.lib.stts_ctc_align(_stream(), seg_t.n, seg_t.host_ptr, _ptr(seg_t.dev), seg_p.host_ptr, _ptr(seg_p.dev), _ptr(lp), lp.shape[1], lp.shape[1],
                                           int(blank), _ptr(tg), 1 if given else 0, _ptr(p), _ptr(out["scores"]), _ptr(out["durations"]), _ptr(out["left"]),
                                           _ptr(out["right"]), _ptr(ws), 0 if ws is None else ws.numel()))
        return out

    def _log_prob_rows(self, seg_t: Segments, log_probs: torch.Tensor, classes: Optional[int]):
        lp = log_probs.to(self.device, torch.float32).contiguous()
        if lp.dim() != 2 or lp.shape[0] != seg_t.rows:
            raise ValueError(f"log-probs of shape {tuple(lp.shape)}, the offsets describe {seg_t.rows} frames")
        V = lp.shape[1] if classes is None else int(classes)
        if not 1 <= V <= lp.shape[1]:
            raise ValueError(f"{V} classes in rows of {lp.shape[1]}")
        return lp, V

    def ctc_nll(self, seg_t: Segments, log_probs: torch.Tensor, seg_p: Segments, targets: torch.Tensor, blank: int, log_priors: Optional[torch.Tensor] = None,
                prior_scale: float = 0.0, classes: Optional[int] = None) -> torch.Tensor:
        """[B] float64 on the device: every utterance's CTC negative log-likelihood, the exact sum over all paths in fp64 (include/stylish_hip.h,
        stts_ctc_nll); +inf where no path exists.  log_probs [sum T, ld] with frame offsets seg_t (``classes`` <= ld columns count, default all),
        targets [sum P] with token offsets seg_p.  ``log_priors`` [classes]: every emission is log_probs - prior_scale * log_priors.  Nothing is
        read back by the host."""
        if seg_t.n != seg_p.n:
            raise ValueError(f"{seg_t.n} utterances of frames but {seg_p.n} of tokens")
        lp, V = self._log_prob_rows(seg_t, log_probs, classes)
        tg = targets.to(self.device, torch.int32).contiguous()
        if tg.dim() != 1 or tg.numel() != seg_p.rows:
            raise ValueError(f"{tg.numel()} targets, the offsets describe {seg_p.rows}")
        pr = None
        if log_priors is not None:
            pr = log_priors.to(self.device, torch.float64).reshape(-1).contiguous()
            if pr.numel() != V:
                raise ValueError(f"{pr.numel()} label priors for {V} classes")
        nll = torch.empty(seg_t.n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_ctc_nll(_stream(), seg_t.n, seg_t.host_ptr, _ptr(seg_t.dev), seg_p.host_ptr, _ptr(seg_p.dev), _ptr(lp), lp.shape[1], V, int(blank),
                                         _ptr(tg), _ptr(pr), float(prior_scale), _ptr(nll)))
        return nll

    def ctc_confidence_sums(self, seg_t: Segments, scores: torch.Tensor) -> torch.Tensor:
        """[B] float64 on the device: each utterance's sum of exp(scores[t]) over the path log-probs of ctc_align (include/stylish_hip.h,
        stts_ctc_confidence_sums), added in a fixed order.  Nothing is read back by the host."""
        sc = self._packed_wave(seg_t, scores, "scores")
        sums = torch.empty(seg_t.n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_ctc_confidence_sums(_stream(), seg_t.n, seg_t.host_ptr, _ptr(seg_t.dev), _ptr(sc), _ptr(sums)))
        return sums

    def ctc_prior_sums(self, seg_t: Segments, log_probs: torch.Tensor, classes: Optional[int] = None) -> torch.Tensor:
        """[classes] float64 on the device: logsumexp of every class over all frames of the batch (include/stylish_hip.h, stts_ctc_prior_sums):
        chunk partials merged in chunk order.  Nothing is read back by the host."""
        lp, V = self._log_prob_rows(seg_t, log_probs, classes)
        need = int(self.lib.stts_ctc_prior_sums_workspace_bytes(seg_t.n, seg_t.host_ptr, V)) or 256  # 0: bad offsets - the entry point names them
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        out = torch.empty(V, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_ctc_prior_sums(_stream(), seg_t.n, seg_t.host_ptr, _ptr(seg_t.dev), _ptr(lp), lp.shape[1], V, _ptr(out), _ptr(ws), ws.numel() * 8))
        return out

    def duration_sums(self, seg_p: Segments, logits: torch.Tensor, targets: torch.Tensor, weight: torch.Tensor, classes: Optional[int] = None) -> torch.Tensor:
        """[B, 3] float64 on the device: the sums of DurationLoss / CDW_CCELoss over packed token rows logits [sum P, ld] (``classes`` <= min(ld, 64)
        columns count, default all), targets [sum P] classes, weight [classes] (include/stylish_hip.h, stts_val_duration_sums).  Nothing is read
        back by the host."""
        lg = logits.to(self.device, torch.float32).contiguous()
        if lg.dim() != 2 or lg.shape[0] != seg_p.rows:
            raise ValueError(f"logits of shape {tuple(lg.shape)}, the offsets describe {seg_p.rows} tokens")
        V = lg.shape[1] if classes is None else int(classes)
        if not 2 <= V <= min(64, lg.shape[1]):
            raise ValueError(f"{V} classes in rows of {lg.shape[1]}: 2 to 64 are built")
        tg = targets.to(self.device, torch.int32).contiguous()
        if tg.dim() != 1 or tg.numel() != seg_p.rows:
            raise ValueError(f"{tg.numel()} targets, the offsets describe {seg_p.rows}")
        w = weight.to(self.device, torch.float32).reshape(-1).contiguous()
        if w.numel() != V:
            raise ValueError(f"{w.numel()} class weights for {V} classes")
        if min(seg_p.lengths) < 1:
            raise ValueError(f"utterance {seg_p.lengths.index(min(seg_p.lengths))} has no tokens")
        sums = torch.empty(seg_p.n, 3, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_val_duration_sums(self.ctx, _stream(), seg_p.n, seg_p.host_ptr, _ptr(seg_p.dev), _ptr(lg), lg.shape[1], V, _ptr(tg), _ptr(w),
                                                   _ptr(sums)))
        return sums

    def diff_sums(self, seg: Segments, a: torch.Tensor, b: torch.Tensor, kind: str) -> torch.Tensor:
        """[B] float64 on the device: each utterance's sum of |a - b| (kind "l1") or (a - b)^2 (kind "l2") over the packed fp32 vectors a and b,
        added in a fixed order (include/stylish_hip.h, stts_val_diff_sums).  The reference's l1_loss / mse_loss is sums.sum() / seg.rows."""
        if kind not in ("l1", "l2"):
            raise ValueError(f"kind must be 'l1' or 'l2', got {kind!r}")
        a, b = self._packed_wave(seg, a, "vector a"), self._packed_wave(seg, b, "vector b")
        if min(seg.lengths) < 1:
            raise ValueError(f"utterance {seg.lengths.index(min(seg.lengths))} has no values")
        sums = torch.empty(seg.n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stts_val_diff_sums(self.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(a), _ptr(b), 1 if kind == "l2" else 0, _ptr(sums)))
        return sums
