"""tokens → waveforms: the whole inference chain on packed, ragged batches.

The reference has no packaged inferencer (README roadmap): its callers loop per utterance over
DurationPredictor → DurationProcessor → ExportModel (``train/test_onnx.py:48-79``, ``train/stage_type.py:483-523``).
This is that composition for a list of utterances of any lengths in ONE pass: every stage runs on the packed
sequences (per-utterance semantics, no padding).

The reference reads the predicted durations on the host between its two models (``test_onnx.py:65-66``) because the
alignment matrix must be sized.  Here nothing is read back in the middle: the frame-rate stages run on CAPACITY SEGMENTS
(include/stylish_hip.h, STTS_SEG_CAPACITY) - every buffer and grid is sized by an upper bound of each utterance's frame
count, the real offsets are computed on the device from the durations (``stts_frame_offsets``) and the waveforms come out
packed by the real lengths, which the host reads ONCE, with the audio.  The upper bound is frames-per-token x tokens: it
is ``frames_per_token`` (default 8; the reference's table allows 46 per token, real speech averages 5-6) - a FIXED function of
the token counts by default, so the same text gets the same buffers, launch plans and bits in every call - and a call whose
prediction does not fit (the frame counts read with the audio exceed a capacity; the truncated segments kept every kernel in
bounds) is repeated with exactly the capacities it asked for.  ``adapt=True`` lets the ratio follow the model's predictions
in steps of 2 frames per token (fewer repeated calls for slow voices; capacities - and through the launch plans the last bits
of the waveform - can then change between two calls of the same text while the ratio is still settling).
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .runtime import CapacityOverflow, HipModel, Segments
from .text import TextCleaner, frame_tokens, to_int16, write_wav


class Synthesizer:
    """engine: a HipModel with all components finalized (load_weights(..., which=255))."""

    MAX_FRAMES_PER_TOKEN = 46  # the largest entry of the reference's duration table (train/utils.py:391-393)

    def __init__(self, engine: HipModel, frames_per_token: float = 8.0, adapt: bool = False):
        """frames_per_token: capacity (mel frames per token) the frame-rate buffers are sized by.  adapt=False (default): the same
        capacities for the same token counts in every call, hence the same launch plans and bit-identical results from call to call;
        adapt=True: the ratio follows what the model predicts, quantised to steps of 2 frames per token."""
        self.eng = engine
        self.cfg = engine.cfg
        self._ratio = float(frames_per_token)
        self._adapt = adapt
        self.capacity_retries = 0  # calls repeated because a prediction did not fit its capacity
        self.text_cleaner = TextCleaner(self.cfg.symbol) if "symbol" in self.cfg else None
        self._lane = self._new_lane()
        self._lanes: List[dict] = []  # extra lanes of map(): one per concurrent call

    def _new_lane(self, own_stream: bool = False) -> dict:
        # the three text encoders only share the tokens: two of them (with their style encoders) run on side streams
        # next to the duration predictor and the host read of the frame counts, each issued from its own host thread: a
        # text encoder is ~120 launches (~0.5 ms of host time), so one thread cannot feed three streams (the C calls
        # release the GIL)
        dev = self.eng.device
        return dict(side=[torch.cuda.Stream(device=dev) for _ in range(2)], pool=ThreadPoolExecutor(max_workers=2, thread_name_prefix="stts-side"),
                    main=torch.cuda.Stream(device=dev) if own_stream else None)

    def map(self, batches: Sequence[Sequence[Sequence[int]]], workers: int = 2, noise: Optional[Sequence[Optional[Dict[str, torch.Tensor]]]] = None):
        """Several batches, `workers` of them in flight: each call runs on its own stream from its own host thread, so one
        batch's phoneme-rate stages (hundreds of small launches, the host read of its frame counts) overlap another's frame
        path.  Results in input order; per batch the arithmetic is that of __call__."""
        if workers <= 1 or len(batches) <= 1:
            return [self(b, noise=None if noise is None else noise[i]) for i, b in enumerate(batches)]
        while len(self._lanes) < workers:
            self._lanes.append(self._new_lane(own_stream=True))
        caller = torch.cuda.current_stream(self.eng.device)
        fork = torch.cuda.Event()
        fork.record(caller)

        def run(i):
            lane = self._lanes[i % workers]
            torch.cuda.set_device(self.eng.device)
            with torch.cuda.stream(lane["main"]):
                lane["main"].wait_event(fork)
                out = self._run(batches[i], None if noise is None else noise[i], False, lane)
                for w in out:
                    w.record_stream(caller)
            return out

        if not hasattr(self, "_map_pool") or self._map_pool._max_workers < workers:
            self._map_pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="stts-lane")
        # a lane serves its batches in order (its stream and workspace are its own), different lanes run concurrently
        futs = [self._map_pool.submit(lambda k=k: [run(i) for i in range(k, len(batches), workers)]) for k in range(workers)]
        per_lane = [f.result() for f in futs]
        for lane in self._lanes[:workers]:
            caller.wait_stream(lane["main"])
        return [per_lane[i % workers][i // workers] for i in range(len(batches))]

    def infer(self, texts: Sequence[str], noise: Optional[Dict[str, torch.Tensor]] = None, out_prefix: Optional[str] = None, combine: bool = False):
        """Phoneme strings → int16 waveforms, all utterances in one pass (the loop body of ``train/test_onnx.py:48-90``).

        With ``out_prefix`` the samples are also written as ``<prefix>_<i>.wav`` (or ``<prefix>_combined.wav``).
        """
        if self.text_cleaner is None:
            raise ValueError("model config has no 'symbol' section")
        waves = self([frame_tokens(self.text_cleaner(t)) for t in texts], noise=noise)
        samples = [to_int16(w) for w in waves]
        if out_prefix is not None:
            if combine:
                write_wav(f"{out_prefix}_combined.wav", np.concatenate(samples, axis=-1), self.cfg.sample_rate)
            else:
                for i, smp in enumerate(samples):
                    write_wav(f"{out_prefix}_{i}.wav", smp, self.cfg.sample_rate)
        return samples

    def __call__(self, token_lists: Sequence[Sequence[int]], noise: Optional[Dict[str, torch.Tensor]] = None, return_details: bool = False):
        return self._run(token_lists, noise, return_details, self._lane)

    @torch.no_grad()
    def resynthesize(self, token_lists: Sequence[Sequence[int]], recordings, alignments_or_durations, pitch, noise: Optional[Dict[str, torch.Tensor]] = None):
        """Copy-synthesis (the reference's SpeechPredictor.forward with audio_gt, models/speech_predictor.py:104-118): the recording's posterior latent
        z ~ q(z | recording, style) through post_flow and the vocoder; the text gives the style only, so the result tells how good the vocoder half of a
        checkpoint is.  recordings: 1-D waveforms at the model's sample rate, at least hop_length samples per mel frame of the alignment;
        alignments_or_durations: per utterance the integer durations [tokens] or the 0/1 alignment matrix [tokens, frames]; pitch: per utterance
        the F0 curve [frames] (mel-frame rate, as validate_acoustic takes it from the data set).  The energy curve of the reference's call feeds the
        decoder only, which this path does not run, so none is taken.  noise: packed draws posterior_noise [rows, 128], src_noise [rows * hop / 4],
        init_phase [1] (rows = 4 x the mel frames).  Needs W_POSTERIOR finalized next to the speech predictor.  -> waveforms, one per utterance."""
        eng, dev = self.eng, self.eng.device
        L = [len(t) for t in token_lists]
        if not (len(recordings) == len(alignments_or_durations) == len(pitch) == len(L)):
            raise ValueError("resynthesize: token_lists, recordings, alignments_or_durations and pitch must have one entry per utterance")
        durs = []
        for b, a in enumerate(alignments_or_durations):
            a = torch.as_tensor(a)
            d = a.sum(dim=1).round() if a.dim() == 2 else a
            if d.numel() != L[b]:
                raise ValueError(f"utterance {b}: {d.numel()} durations for {L[b]} tokens")
            durs.append([int(v) for v in d.tolist()])
        T = [sum(d) for d in durs]
        st = Segments(T, dev)
        st4 = st.scaled(4)
        R, h = st4.rows, eng.hop4
        if int(eng.lib.stts_posterior_workspace_bytes(eng.ctx, R, st4.n, st4.max_len)) == 0:
            raise RuntimeError("resynthesize needs the posterior encoder: load speech_predictor.posterior_encoder.* and finalize W_POSTERIOR")
        waves = [torch.as_tensor(w).to(device=dev, dtype=torch.float32).reshape(-1) for w in recordings]
        for b, w in enumerate(waves):
            if w.numel() < 4 * h * T[b]:
                raise ValueError(f"recording {b} has {w.numel()} samples, its alignment needs {4 * h * T[b]}")
        wave = torch.cat([w[: 4 * h * T[b]] for b, w in enumerate(waves)]).contiguous()
        f0 = torch.cat([torch.as_tensor(p).to(device=dev, dtype=torch.float32).reshape(-1)[: T[b]] for b, p in enumerate(pitch)]).contiguous()
        if f0.numel() != st.rows:
            raise ValueError("resynthesize: a pitch curve is shorter than its alignment")
        toks = torch.tensor([int(v) for t in token_lists for v in t], dtype=torch.int64, device=dev)
        sp = Segments(L, dev)
        style = eng.text_style(1, sp, eng.text_encoder(1, sp, toks))
        p4 = eng.upsample4(st, st4, f0)
        if noise is None:
            noise = dict(posterior_noise=torch.randn(R, self.cfg.decoder.hidden_dim // 4, device=dev), src_noise=torch.randn(R * h, device=dev),
                         init_phase=torch.rand(1, device=dev))
        o = eng.posterior(st4, audio=wave, style=style, noise=noise["posterior_noise"], mel=True, stats=False)
        spec, phase = eng.harmonic_stft(st4, p4, noise["src_noise"], noise["init_phase"], batch_scope=False)
        audio = eng.vocoder(st4, o["mel"], style, spec, phase)
        eng.check_status()
        return [audio[h * int(st4.host[b]) : h * int(st4.host[b + 1])] for b in range(len(L))]

    host_syncs_per_call = 0  # reads of device data by the host between the duration predictor and the frame path

    def stage_times(self, token_lists, noise=None) -> Dict[str, float]:
        """One call with events between the stages on the caller's stream: milliseconds of the phoneme-rate part (everything up to
        the frame path's inputs: three text encoders, styles, durations, pitch / energy, length regulator) and of the frame path."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        lane = dict(self._lane, events=ev)  # the events travel with this call only (concurrent map() lanes record nothing into them)
        self._run(token_lists, noise, False, lane)
        torch.cuda.synchronize(self.eng.device)
        return dict(phoneme_ms=ev[0].elapsed_time(ev[1]), frame_ms=ev[1].elapsed_time(ev[2]))

    def _capacities(self, L: Sequence[int]) -> List[int]:
        r = min(self._ratio, float(self.MAX_FRAMES_PER_TOKEN))
        return [min(self.MAX_FRAMES_PER_TOKEN * n, int(np.ceil(r * n)) + 8) for n in L]

    @torch.no_grad()
    def _run(self, token_lists, noise, return_details, lane):
        L = [len(t) for t in token_lists]
        caps = self._capacities(L)
        while True:
            try:
                return self._run_once(token_lists, L, caps, noise, return_details, lane)
            except CapacityOverflow as e:  # rare: the model predicted more frames than this call's buffers hold - repeat it with what it asked for
                self.capacity_retries += 1
                caps = [max(int(n), c) for n, c in zip(e.need, caps)]

    def _run_once(self, token_lists, L, caps, noise, return_details, lane):
        eng, dev = self.eng, self.eng.device
        toks = torch.tensor([int(v) for t in token_lists for v in t], dtype=torch.int64, device=dev)
        sp = Segments(L, dev)
        main = torch.cuda.current_stream(dev)
        ev = lane.get("events")
        if ev:
            ev[0].record(main)
        ready = torch.cuda.Event()
        ready.record(main)
        # 2a/3a. the pitch/energy and speech text + style encoders: phoneme-rate, independent of the durations
        def encode(which, stream):
            torch.cuda.set_device(dev)
            with torch.cuda.stream(stream):
                stream.wait_event(ready)
                e = eng.text_encoder(which, sp, toks)
                y = eng.text_style(which, sp, e)
                for t in (e, y):
                    t.record_stream(main)  # consumed on the caller's stream below
            return e, y

        jobs = [lane["pool"].submit(encode, 2, lane["side"][0]), lane["pool"].submit(encode, 1, lane["side"][1])]
        # 1. durations (DurationPredictor + DurationProcessor.prediction_to_duration), then the frame offsets ON THE DEVICE:
        #    st / st4 are capacity layouts (host = upper bounds, device = the real cumulative frame counts)
        _, dur = eng.duration(sp, toks)
        st, st4, need = eng.frame_offsets(sp, dur, caps)
        (pe_enc, pe_style), (enc, style) = jobs[0].result(), jobs[1].result()
        main.wait_stream(lane["side"][0])
        main.wait_stream(lane["side"][1])
        # 2b. pitch / energy (PitchEnergyPredictor on the pe encoders' outputs)
        f0, en = eng.pitch_energy(sp, st, dur, pe_enc, pe_style)
        # 3b. speech predictor front (length regulator, x4 upsampling)
        asr = eng.length_regulate(sp, st4, dur, 4, enc, self.cfg.inter_dim)
        p4, e4 = eng.upsample4(st, st4, f0), eng.upsample4(st, st4, en)
        # 4. frame path.  Explicit noise is indexed by the REAL packed rows (as the outputs are): only its first rows are read.
        R = st4.rows
        if noise is None:
            noise = dict(prior_noise=torch.randn(R, 128, device=dev), src_noise=torch.randn(R * eng.hop4, device=dev),
                         init_phase=torch.rand(1, device=dev))
        if ev:
            ev[1].record(main)
        audio = eng.frame_path(st4, asr, p4, e4, style, noise["prior_noise"], noise["src_noise"], noise["init_phase"], batch_scope=False)
        if ev:
            ev[2].record(main)
        # the one host read of the call: the frame counts, together with the audio (the .cpu() waits for the stream)
        T = [int(v) for v in need.cpu().tolist()]
        if any(t > c for t, c in zip(T, caps)):  # truncated utterances: this call's output is invalid, and so is whatever the truncated
            # data left in the error word - it is read (which clears it) and dropped, then the call is repeated with what it asked for
            try:
                eng.check_status()
            except RuntimeError:
                pass
            e = CapacityOverflow(f"predicted frames {T} exceed the capacities {list(caps)}")
            e.need = T
            raise e
        eng.check_status()  # only a call whose capacities fitted reports the device-side status
        # adapt: capacity of the next calls = 1.25 x the largest frames-per-token ratio seen so far, rounded UP to a multiple of 2 (monotone
        # and coarse: it settles after the first calls, and equal inputs then get equal capacities, launch plans and results)
        if self._adapt:
            want = 1.25 * max(t / max(n, 1) for t, n in zip(T, L))
            self._ratio = min(float(self.MAX_FRAMES_PER_TOKEN), max(self._ratio, 2.0 * float(np.ceil(want / 2.0))))
        off = np.concatenate([[0], np.cumsum(T)]) * (4 * eng.hop4)  # hop_length samples per mel frame
        waves = [audio[int(off[i]) : int(off[i + 1])] for i in range(len(L))]
        if return_details:
            Tm = int(sum(T))
            return waves, dict(durations=dur, frames=T, pitch=f0[:Tm], energy=en[:Tm], style=style, capacities=list(caps))
        return waves


class VoiceConverter:
    """The reference's voice-conversion path (the hubert_acoustic models, train/stage_type.py:907-1015) on one engine: HuBERT features of
    the source speech + a wespeaker embedding of the target speaker -> waveforms.  HubertPitchEnergyPredictor predicts F0 / energy from
    the features and the target embedding (unless the caller gives them), then HubertSpeechPredictor renders the features with that
    prosody in the target's style.

    The engine must hold the weights of both models: hubert_speech_predictor.{phone_encoder, style_encoder} and
    hubert_pitch_energy_predictor.* finalized as STTS_W_HUBERT | STTS_W_HUBERT_PE, and the hubert_speech_predictor's decoder .. generator
    as the frame path (``modules.HubertSpeechPredictor`` binds them; pass the shims as ``modules`` to have them re-bound before each call).
    One packed ragged batch per call; the frame counts are known up front, so nothing is read back by the host before the audio."""

    host_syncs_per_call = 0  # reads of device data by the host between the pitch predictor and the frame path

    def __init__(self, engine: HipModel, modules: Sequence[torch.nn.Module] = ()):
        from .config import hubert_dims

        self.eng = engine
        self.cfg = engine.cfg
        self.hubert_dim, self.spk_dim = hubert_dims(self.cfg)
        self._modules = list(modules)

    @torch.no_grad()
    def convert(self, features, lengths, spk_emb, pitch=None, energy=None, noise: Optional[Dict[str, torch.Tensor]] = None,
                return_details: bool = False, ref_mel=None, ref_mel_lengths=None, f0_log2_stats=None, uv=None, _packed_feats=None, _packed_pitch=None,
                _packed_uv=None, ref_wave=None, ref_wave_lengths=None, mel_stats=(-4.0, 4.0), energy_wave=None, energy_wave_lengths=None):
        """features [B, hubert_dim, T] (mel-frame rate, zero padded past lengths[b]), spk_emb [B, spk_dim]; optional pitch / energy
        [B, T] replace the predicted curves; noise: the packed draws of ``Synthesizer`` (prior_noise [4 sum T, 128], src_noise
        [4 sum T * hop / 4], init_phase [1]).  -> list of B float waveforms (hop_length samples per frame).
        ref_mel [B, n_mels, Tm] (normalised mel of the target speaker, ref_mel_lengths [B] optional): F0 comes from the CFM pitch predictor
        (cfm_pitch_predictor: STTS_W_CFM_PITCH | STTS_W_CFM_PITCH_NET on this engine) on the same features, denormed on the device with
        f0_log2_stats = (log2 mean, log2 std) of the training set, 0 where uv [B, T] > 0; energy is HubertPitchEnergyPredictor's unless
        given.
        ref_wave [B, samples] (the target speaker's recording at the model's sample rate, ref_wave_lengths [B] optional) in place of ref_mel: its
        normalised log-mel (modules.LogMelSpectrogram.from_config, mel_stats = (mean, std) of the training set) is computed on the engine and its
        packed rows go to the speaker encoder as they are.  energy_wave [B, samples] (the SOURCE at the model's sample rate) in place of energy:
        the curve is LogMelSpectrogram.energy of it (log_norm, train/utils.py:71-77); its frame counts must equal ``lengths``."""
        from .config import check_width
        from .modules import LogMelSpectrogram, _pack_curve, _pack_rows, _f

        eng, dev = self.eng, self.eng.device
        for m in self._modules:
            _ = m.engine  # re-bind if another shim packed these components last
        L = [int(v) for v in torch.as_tensor(lengths).tolist()]
        check_width("speaker embedding", spk_emb.shape[-1], "speaker_embedder.hidden_dim", self.spk_dim)
        if _packed_feats is None:
            if features.dim() != 3:
                raise ValueError(f"HuBERT features must be [B, {self.hubert_dim}, T], got shape {tuple(features.shape)}")
            check_width("HuBERT features", features.shape[1], "hubert.hidden_dim", self.hubert_dim)
            if len(L) != features.shape[0] or spk_emb.shape[0] != len(L) or min(L) <= 0 or max(L) > features.shape[2]:
                raise ValueError(f"lengths {L} do not describe features of shape {tuple(features.shape)} / {spk_emb.shape[0]} speaker embeddings")
        elif spk_emb.shape[0] != len(L) or min(L) <= 0 or _packed_feats.shape[0] != sum(L):
            raise ValueError(f"lengths {L} do not describe {_packed_feats.shape[0]} packed feature rows / {spk_emb.shape[0]} speaker embeddings")
        if ref_mel is not None and ref_wave is not None:
            raise ValueError("give ref_mel or ref_wave (its mel is computed on the engine), not both")
        if energy is not None and energy_wave is not None:
            raise ValueError("give energy or energy_wave (its energy curve is computed on the engine), not both")
        front = None
        if ref_wave is not None or energy_wave is not None:
            front = LogMelSpectrogram.from_config(self.cfg, mean=mel_stats[0], std=mel_stats[1], engine=eng)
        if energy_wave is not None:
            Le = front.frame_counts(front._lengths(energy_wave, energy_wave_lengths))
            if Le != L:
                raise ValueError(f"energy_wave gives {Le} mel frames, lengths are {L}")
        has_energy = energy is not None or energy_wave is not None
        cfm = ref_mel is not None or ref_wave is not None
        if cfm:
            if pitch is not None:
                raise ValueError("give ref_mel (F0 from the CFM pitch predictor) or pitch, not both")
            if f0_log2_stats is None:
                raise ValueError("ref_mel needs f0_log2_stats = (log2 F0 mean, log2 F0 std) of the training set")
            if ref_wave is not None:
                if ref_wave.dim() != 2 or ref_wave.shape[0] != len(L):
                    raise ValueError(f"ref_wave must be [{len(L)}, samples], got shape {tuple(ref_wave.shape)}")
                front.frame_counts(front._lengths(ref_wave, ref_wave_lengths))  # ValueError for a recording the transform refuses
            elif ref_mel.dim() != 3 or ref_mel.shape[0] != len(L):
                raise ValueError(f"ref_mel must be [{len(L)}, n_mels, Tm], got shape {tuple(ref_mel.shape)}")
            if ref_mel is not None:
                Lm = [ref_mel.shape[2]] * len(L) if ref_mel_lengths is None else [int(v) for v in torch.as_tensor(ref_mel_lengths).tolist()]
                if len(Lm) != len(L) or min(Lm) < 1 or max(Lm) > ref_mel.shape[2]:
                    raise ValueError(f"ref_mel_lengths {Lm} do not fit ref_mel of shape {tuple(ref_mel.shape)}")
        elif _packed_pitch is None and (pitch is None) != (not has_energy):
            raise ValueError("give both pitch and energy, or neither")
        st = Segments(L, dev)
        st4 = st.scaled(4)
        feats = _pack_rows(eng, features, L) if _packed_feats is None else _packed_feats
        style, pe_style = eng.speaker_style(_f(spk_emb, dev), pe_style=not has_energy)
        en_given = None
        if energy_wave is not None:
            en_given = front.energy(energy_wave, energy_wave_lengths, packed=True)[0]
        elif energy is not None:
            en_given = _pack_curve(energy, L, dev)
        if cfm:
            from .modules import W_CFM_PITCH

            if ref_wave is not None:
                mel_rows, seg_m = front.packed(ref_wave, ref_wave_lengths)
            else:
                md = _f(ref_mel, dev)
                mel_rows, seg_m = torch.cat([md[b, :, : Lm[b]].t() for b in range(len(L))]).contiguous(), Segments(Lm, dev)
            spk = eng.mel_style(W_CFM_PITCH, seg_m, mel_rows, 256)
            uv_rows = _pack_curve(uv, L, dev) if uv is not None else _packed_uv
            _, f0 = eng.cfm_pitch(st, feats, spk, f0_log2_stats=f0_log2_stats, uv=uv_rows)
            en = eng.hubert_pitch_energy(st, feats, pe_style)[1] if en_given is None else en_given
        elif _packed_pitch is not None:  # convert_audio's extracted curve (packed rows); energy predicted unless given
            f0 = _packed_pitch
            en = eng.hubert_pitch_energy(st, feats, pe_style)[1] if en_given is None else en_given
        elif pitch is None:
            f0, en = eng.hubert_pitch_energy(st, feats, pe_style)
        else:
            f0, en = _pack_curve(pitch, L, dev), en_given
        asr = eng.hubert_encoder(st, feats)
        p4, e4 = eng.upsample4(st, st4, f0), eng.upsample4(st, st4, en)
        R = st4.rows
        if noise is None:
            noise = dict(prior_noise=torch.randn(R, self.cfg.decoder.hidden_dim // 4, device=dev), src_noise=torch.randn(R * eng.hop4, device=dev),
                         init_phase=torch.rand(1, device=dev))
        audio = eng.frame_path(st4, asr, p4, e4, style, noise["prior_noise"], noise["src_noise"], noise["init_phase"], batch_scope=False)
        eng.check_status()
        waves = [audio[eng.hop4 * st4.host[b] : eng.hop4 * st4.host[b + 1]] for b in range(len(L))]
        if return_details:
            return waves, dict(pitch=f0, energy=en, style=style, pe_style=pe_style, asr=asr)
        return waves

    @torch.no_grad()
    def convert_audio(self, wave, sample_lengths, frames, spk_emb, ssl=None, pitch_extractor=None, sample_rate=None, decoder: str = "argmax", **kw):
        """Voice conversion from audio: wave [B, samples] at hubert.sr (zero padded past sample_lengths[b]), frames [B] = the mel-frame count
        of every utterance (the reference's time_dim; an argument, so the host reads nothing back) -> HuBERT features on the engine
        (``ssl``: the modules.AdaptiveHubert bound to this engine, or the one among this converter's modules) written as the packed rows
        convert() consumes, then convert() with the same keywords (pitch, energy, noise, ref_mel, ref_wave, energy_wave, ...).
        pitch_extractor (a modules.RmvpePitchExtractor; the audio must be at its 16 kHz): the source's own F0 is extracted on the engine and
        resampled to ``frames``.  Without ref_mel it becomes the pitch (energy from HubertPitchEnergyPredictor unless given); with ref_mel it
        gives the voicing flags uv = (f0 == 0), formed on the device, unless uv is given.  The host reads nothing back.  decoder="viterbi": that F0
        is the extractor's Viterbi decode (the objective of to_viterbi_f0: no one-frame octave jumps), found at its 100 frames / s before the resampling.
        sample_rate: the rate of ``wave`` where it is not hubert.sr.  The content encoder then gets torchaudio's default (width-6) resampling of it
        and the pitch extractor the reference's width-128 one, each from the original recording, on the engine.  At the model's sample rate the
        same ``wave`` may also be passed as ref_wave / energy_wave: one recording in, at one rate."""
        from .modules import AdaptiveHubert

        if ssl is None:
            ssl = next((m for m in self._modules if isinstance(m, AdaptiveHubert)), None)
        if ssl is None:
            raise ValueError("convert_audio needs an AdaptiveHubert: pass ssl= or list it among the converter's modules")
        if ssl.hidden != self.hubert_dim:
            raise ValueError(f"the content encoder has width {ssl.hidden}; hubert.hidden_dim is {self.hubert_dim}")
        T = [int(v) for v in torch.as_tensor(frames).tolist()]
        ssl._engine = ssl._engine or self.eng
        if sample_rate is not None and (int(sample_rate) != sample_rate or int(sample_rate) < 1):
            raise ValueError(f"sample_rate {sample_rate} must be a positive integer")
        if pitch_extractor is not None:
            if kw.get("pitch") is not None:
                raise ValueError("give pitch_extractor (F0 from the source audio) or pitch, not both")
            if sample_rate is None and pitch_extractor.sr != ssl.sr:
                raise ValueError(f"the pitch extractor takes audio at {pitch_extractor.sr} Hz, the content encoder at {ssl.sr} Hz")
        feats = ssl.packed(wave, T, sample_lengths) if sample_rate is None else ssl.packed(wave, T, sample_lengths, sample_rate=int(sample_rate))
        if pitch_extractor is not None:
            pitch_extractor._engine = pitch_extractor._engine or self.eng
            vk = {} if decoder == "argmax" else dict(decoder=decoder)  # the default call stays what it was
            if sample_rate is None:
                f0 = pitch_extractor.packed_from_audio(wave, sample_lengths, T, **vk)
            else:
                f0 = pitch_extractor.packed_from_audio(wave, sample_lengths, T, sample_rate=int(sample_rate), resample=True, **vk)
            if kw.get("ref_mel") is not None or kw.get("ref_wave") is not None:
                if kw.get("uv") is None:
                    kw["_packed_uv"] = (f0 == 0).to(torch.float32)
            else:
                kw["_packed_pitch"] = f0
        return self.convert(None, T, spk_emb, _packed_feats=feats, **kw)

    def convert_int16(self, features, lengths, spk_emb, pitch=None, energy=None, noise=None, out_prefix: Optional[str] = None):
        """convert() as int16 samples; with ``out_prefix`` also written as ``<prefix>_<i>.wav`` (like ``Synthesizer.infer``)."""
        samples = [to_int16(w) for w in self.convert(features, lengths, spk_emb, pitch, energy, noise)]
        if out_prefix is not None:
            for i, smp in enumerate(samples):
                write_wav(f"{out_prefix}_{i}.wav", smp, self.cfg.sample_rate)
        return samples


def _curve_pair(pair, what):
    """(predicted, recorded) curves [B, T] / lists of 1-D curves -> (list of 1-D predicted, list of 1-D recorded, their lengths)."""
    from .modules import _wave_batch

    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise ValueError(f"{what} must be a pair (predicted, recorded)")
    (a, La), (b, Lb) = _wave_batch(pair[0]), _wave_batch(pair[1])
    if La != Lb:
        raise ValueError(f"{what}: the predicted curves have {La} values, the recorded ones {Lb}")
    return a, b, La


def _value_pair(pair, what):
    """(predicted, target) tensors [B, ...] or lists of tensors of any shape -> (list of 1-D predicted, list of 1-D target, their sizes)."""
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise ValueError(f"{what} must be a pair (predicted, target)")
    out = []
    for x in pair:
        if isinstance(x, (list, tuple)):
            out.append([torch.as_tensor(v).reshape(-1) for v in x])
        else:
            x = torch.as_tensor(x)
            out.append([x.reshape(-1)] if x.dim() < 2 else [x[b].reshape(-1) for b in range(x.shape[0])])
    La, Lb = [int(v.numel()) for v in out[0]], [int(v.numel()) for v in out[1]]
    if La != Lb or not La or min(La) < 1:
        raise ValueError(f"{what}: the predictions have {La} values, the targets {Lb}")
    return out[0], out[1], La


@torch.no_grad()
def duration_scores(engine: HipModel, logits, alignment_or_durations, text_lengths, weight) -> dict:
    """What validate_duration logs (train/stage_type.py:514-520): logits [B, P, C] of the duration predictor, the batch's 0/1 alignment [B, P, T] or
    its durations [B, P] in frames, text_lengths [B], weight [C] the class weights of DurationLoss -> dict(duration_ce, duration,
    duration_ce_utt, duration_utt) of Python numbers: DurationLoss.forward's two values and every utterance's own, from the fp64 sums of one
    launch, read from the device once."""
    from .modules import DurationLoss, DurationProcessor

    logits, x = torch.as_tensor(logits), torch.as_tensor(alignment_or_durations)
    if logits.dim() != 3 or x.dim() not in (2, 3) or x.shape[:2] != logits.shape[:2]:
        raise ValueError(f"logits {tuple(logits.shape)} [B, P, C] do not fit an alignment [B, P, T] / durations [B, P] of shape {tuple(x.shape)}")
    proc = DurationProcessor(logits.shape[2], 50)
    classes = proc.align_to_class(x.cpu()) if x.dim() == 3 else proc.dur_to_class(x.cpu())
    return DurationLoss(class_count=logits.shape[2], weight=weight, engine=engine).scores(logits, classes, text_lengths)


@torch.no_grad()
def validation_scores(engine: HipModel, audio, audio_gt, lengths=None, prediction=None, pitch=None, energy=None, slm=None, mel_l2=None, normed_pitch_l2=None,
                      linear_pitch=None) -> dict:
    """What the reference's validate_* functions log about a batch (train/stage_type.py), on the engine's fused kernels (nothing is materialised):
    audio / audio_gt: the synthesised waveforms and the recordings, [B, samples], [B, 1, samples] or lists of 1-D tensors (``lengths`` [B] cuts a
    padded batch).  -> dict of Python numbers, read from the device once:
      mel        MultiResolutionSTFTLoss over MultiSpectrogram: per resolution sum of the numerators / (sum of the denominators + 1e-6) over the
                 batch - the reference's number for an equal-length batch - averaged; mel_r the per-resolution values, mel_utt every
                 utterance's own score (what a ragged batch can report)
      mag, phase MagPhaseLoss at the engine's model.yml geometry, with ``prediction``: a DecoderPrediction (magnitude / phase [B, n_bins, F]) or the
                 time-major rows (logamp_rows, phase_rows[, Segments]) of ``HipModel.vocoder(return_spec=True)``, whose last row of every utterance is
                 repeated like the reference's replicate padding; phase_terms the three means "phase" adds up
      pitch, energy  smooth_l1_loss (beta 1, mean) of the pairs (predicted, recorded) given as ``pitch`` / ``energy``
      kl_text, kl_audio  when ``prediction`` carries all four FlowStatistics (SpeechPredictor.forward(audio_gt=, flow_stats=True)): the two scores of
                 NormalizingFlowLoss (the values of ``modules.NormalizingFlowLoss.scores``); kl_text_utt / kl_audio_utt every utterance's own value
      slm        with ``slm``: a modules.WavLMLoss - the mean absolute difference of WavLM's hidden states of the recordings and the synthesised
                 waveforms (the value of ``slm(audio_gt, audio)``, bit for bit); slm_utt every utterance's own value
      mel_l2, normed_pitch_l2, linear_pitch  with the pair (predicted, target) given under that name (tensors [B, ...] or lists of tensors): what
                 validate_cfm_mel / validate_cfm_pitch log, F.mse_loss (the two *_l2) and F.l1_loss (linear_pitch) over the batch, from fp64 sums;
                 <name>_utt every utterance's own mean
    ValueError naming the utterance whose lengths do not agree, or the geometry rule a length breaks."""
    from .modules import MagPhaseLoss, _magphase_sums, _pack_waves, _wave_batch, flow_kl_score, flow_kl_sums, has_flow_stats, magphase_score, mel_score

    eng = engine
    pw, Lp = _wave_batch(audio, lengths)
    gw, Lg = _wave_batch(audio_gt, lengths)
    seg_g, seg_p = Segments(Lg, eng.device), Segments(Lp, eng.device)
    parts = [eng.mel_sums(seg_g, _pack_waves(eng, gw), _pack_waves(eng, pw), sample_rate=eng.cfg.sample_rate, seg_pred=seg_p)]  # [R, B, 2]
    R, B = parts[0].shape[0], seg_g.n
    mp_rows = None
    if prediction is not None:
        n_fft, win, hop = eng.n_fft, eng.win_length, eng.hop4
        if hasattr(prediction, "magnitude"):
            mp, mp_rows = MagPhaseLoss(n_fft=n_fft, hop_length=4 * hop, win_length=win, engine=eng).sums(prediction, gw)
        else:
            la, ph = prediction[0], prediction[1]
            rows = [n // hop for n in Lg]
            seg_v = prediction[2] if len(prediction) > 2 else Segments(rows, eng.device)
            if seg_v.lengths != rows or la.shape[0] != seg_v.rows or ph.shape != la.shape:
                raise ValueError(f"the vocoder rows describe {seg_v.lengths} frames; the recordings' {Lg} samples at hop {hop} make {rows}")
            idx = torch.cat([torch.cat([torch.arange(seg_v.host[b], seg_v.host[b + 1]), torch.tensor([seg_v.host[b + 1] - 1])]) for b in range(seg_v.n)])
            idx = idx.to(eng.device)
            seg_r = Segments([r + 1 for r in rows], eng.device)
            mp = _magphase_sums(eng, gw, Lg, la.index_select(0, idx).contiguous(), ph.index_select(0, idx).contiguous(), seg_r, n_fft, win, hop)
            mp_rows = seg_r.rows
        parts.append(mp)  # [B, 4]
    curves = []
    for name, pair in (("pitch", pitch), ("energy", energy)):
        if pair is not None:
            a, b, L = _curve_pair(pair, name)
            parts.append(eng.smooth_l1_sums(Segments(L, eng.device), _pack_waves(eng, a), _pack_waves(eng, b)))  # [len(L)]
            curves.append((name, len(L), sum(L)))
    kl_len = None
    if prediction is not None and has_flow_stats(prediction):
        kl, kl_len = flow_kl_sums(eng, prediction)  # [2, B]
        parts.append(kl)
    if slm is not None:
        slm.wavlm._engine = slm.wavlm._engine or eng
        s_sums, s_fr = slm.sums(gw, pw)  # [B, states] float64, [B] int32
        parts += [s_sums, s_fr.to(torch.float64)]
    diffs = []
    for name, pair, kind in (("mel_l2", mel_l2, "l2"), ("normed_pitch_l2", normed_pitch_l2, "l2"), ("linear_pitch", linear_pitch, "l1")):
        if pair is not None:
            a, b, L = _value_pair(pair, name)
            diffs.append((name, L, eng.diff_sums(Segments(L, eng.device), _pack_waves(eng, a), _pack_waves(eng, b), kind)))  # [len(L)]
    parts += [d[2] for d in diffs]  # behind everything else: the offsets of the other parts stay where they were
    host = torch.cat([p.reshape(-1) for p in parts]).cpu().tolist()  # the one host read
    at = 2 * R * B
    mel, mel_r, mel_utt = mel_score([[host[2 * (r * B + u) : 2 * (r * B + u) + 2] for u in range(B)] for r in range(R)])
    out = dict(mel=mel, mel_r=mel_r, mel_utt=mel_utt)
    if mp_rows is not None:
        mag, phase, terms = magphase_score([host[at + 4 * u : at + 4 * u + 4] for u in range(B)], mp_rows, eng.n_bins)
        out.update(mag=mag, phase=phase, phase_terms=terms)
        at += 4 * B
    for name, n_utt, n in curves:
        tot = 0.0
        for v in host[at : at + n_utt]:
            tot += v
        out[name] = tot / n
        at += n_utt
    if kl_len is not None:
        nk = len(kl_len)
        for j, name in enumerate(("kl_text", "kl_audio")):
            out[name], out[name + "_utt"] = flow_kl_score(host[at + j * nk : at + (j + 1) * nk], kl_len)
        at += 2 * nk
    if slm is not None:
        from . import wavlm

        ns = slm.wavlm.n_states
        fr = [int(v) for v in host[at + ns * B : at + ns * B + B]]
        out["slm"], out["slm_utt"] = wavlm.score([host[at + ns * u : at + ns * u + ns] for u in range(B)], fr, slm.wavlm.hidden)
    at = len(host) - sum(len(L) for _, L, _ in diffs)
    for name, L, _ in diffs:
        tot = 0.0
        for v in host[at : at + len(L)]:
            tot += v
        out[name], out[name + "_utt"] = tot / sum(L), [v / n for v, n in zip(host[at : at + len(L)], L)]
        at += len(L)
    return out
