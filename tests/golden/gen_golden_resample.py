#!/usr/bin/env python3
"""Golden vectors of the windowed-sinc resampler and of the two reference front ends that begin with it, generated on the CPU in fp32 and in
float64.  torchaudio is not installed where the fixtures are made: ``torchaudio.transforms.Resample`` is the one piece restated here, from its
published source (functional._get_sinc_resample_kernel / _apply_sinc_resample_kernel: the kernel built in float64 with the phase offset p / n in
the default dtype and rounded to fp32 when ``dtype`` is None, F.pad + F.conv1d at stride o, the output cut to ceil(n length / o)), and installed
as the ``torchaudio.transforms.Resample`` stub before the reference runs:
  AdaptiveHubert (train/models/ssl.py:16-31) at model_sr 24000 / hubert_sr 16000 on the narrow architecture of gen_golden_ssl.py:
      ``m.resample(wave)`` and ``m(wave, time_dim)``
  RMVPE.infer_from_audio (train/dataprep/rmvpe/inference.py:44-65) at sample_rate 24000 with the narrow network and the stubs of
      gen_golden_rmvpe.py (its own ``Resample(24000, 16000, lowpass_filter_width=128)``)
The fp32 run is the reference as it runs; the float64 run is the same code with float64 weights, a ``dtype=torch.float64`` resampler and float64
audio.  Whether the restatement equals an installed torchaudio to the last bit cannot be checked here; the float64 outputs do not
depend on torchaudio's fp32 roundings.  Runs only where the reference exists; never from tests.

    python tests/golden/gen_golden_resample.py

resample_cases.npz   for every case of tests/resample64.py CASES
  <case>_lengths, <case>_wave        the recordings' sample counts and their samples, one after the other (fp32; resample64.signal)
  <case>_out32 / _out64              Resample(...)(wave) of each recording on its own, one after the other, fp32 form and dtype=float64
  <case>_err                         (max-abs, rms) of the fp32 run against the float64 run
resample_ssl.npz     wave [1, 12000] at 24 kHz (gen_golden_ssl.wave("r24k", 1, 12000)), time_dim 40
  wave, res32 / res64 / res_err      m.resample(wave) [1, 8000]
  out32 / out64 / out_err            m(wave, 40) [1, 128, 40]
resample_rmvpe.npz   audio [12000] at 24 kHz (0.33 x resample64.signal("rmvpe", 12000, 24000), rounded to fp32)
  audio, res32 / res64 / res_err     the width-128 resampler's output [1, 8000]
  hidden32 / hidden64 / hidden_err   mel2hidden's salience [1, 51, 360]
  f032 / f064 / f0_err               infer_from_audio's f0 [51] in Hz (0 unvoiced; err: max relative error on the voiced frames, rms of it)
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
os.environ.setdefault("HF_HUB_OFFLINE", "1")

import gen_golden_ssl as GS  # noqa: E402  (the stubs of gen_golden.py, transformers, the reference's AdaptiveHubert)
import gen_golden_rmvpe as GR  # noqa: E402  (librosa's stub, the reference's RMVPE)
from gen_golden import save  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import resample64 as R64  # noqa: E402
from stylish_tts_amd import rmvpe as R  # noqa: E402
from stylish_tts.train.dataprep.rmvpe import inference as rmvpe_inference  # noqa: E402


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta, dtype=None)."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None, *, dtype=None):
        super().__init__()
        self.orig_freq, self.new_freq, self.gcd = orig_freq, new_freq, math.gcd(int(orig_freq), int(new_freq))
        if self.orig_freq != self.new_freq:
            kernel, self.width = self._kernel(int(orig_freq) // self.gcd, int(new_freq) // self.gcd, lowpass_filter_width, rolloff, resampling_method, beta, dtype)
            self.register_buffer("kernel", kernel, persistent=False)

    @staticmethod
    def _kernel(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, dtype):
        if lowpass_filter_width <= 0:
            raise ValueError("Low pass filter width should be positive.")
        base_freq = min(orig_freq, new_freq) * rolloff
        width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
        idx_dtype = dtype if dtype is not None else torch.float64
        idx = torch.arange(-width, width + orig_freq, dtype=idx_dtype)[None, None] / orig_freq
        t = torch.arange(0, -new_freq, -1, dtype=dtype)[:, None, None] / new_freq + idx  # dtype None: p / n in fp32, the sum in float64
        t *= base_freq
        t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
        if resampling_method == "sinc_interp_hann":
            window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        else:
            if beta is None:
                beta = 14.769656459379492
            beta_tensor = torch.tensor(float(beta), dtype=torch.float64)  # float64: the target is the published definition, not a rounded beta
            window = torch.i0(beta_tensor * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(beta_tensor)
        t *= math.pi
        scale = base_freq / orig_freq
        kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
        kernels *= window * scale
        if dtype is None:
            kernels = kernels.to(dtype=torch.float32)
        return kernels, width

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        o, n = int(self.orig_freq) // self.gcd, int(self.new_freq) // self.gcd
        waveform = waveform.to(self.kernel.dtype)  # the float64 run feeds float64 audio whatever the caller's cast
        shape = waveform.size()
        waveform = waveform.view(-1, shape[-1])
        num_wavs, length = waveform.shape
        waveform = F.pad(waveform, (self.width, self.width + o))
        resampled = F.conv1d(waveform[:, None], self.kernel, stride=o)
        resampled = resampled.transpose(1, 2).reshape(num_wavs, -1)
        target_length = int(torch.ceil(torch.as_tensor(n * length / o)).long())
        resampled = resampled[..., :target_length]
        return resampled.view(shape[:-1] + resampled.shape[-1:])


sys.modules["torchaudio.transforms"].Resample = Resample
sys.modules["torchaudio"].transforms.Resample = Resample
rmvpe_inference.Resample = Resample  # inference.py binds the name at import

CASE_LENGTHS = lambda o: [1, 5, 7 * o - 1, 7 * o, 7 * o + 1]  # noqa: E731  (+ about 0.05 s)


def _err(a32, b64):
    e = np.asarray(a32, np.float64) - b64
    return np.array([np.abs(e).max(), np.sqrt((e * e).mean())])


def case_waves(case):
    orig, new = R64.CASES[case][:2]
    o, _ = R64.reduced(orig, new)
    L = CASE_LENGTHS(o) + [int(round(0.05 * orig))]
    return [R64.signal(f"golden.{case}.{i}", n, orig) for i, n in enumerate(L)]


def cases():
    out = {}
    for case, (orig, new, lpw, rolloff, method, beta) in R64.CASES.items():
        waves = case_waves(case)
        r32 = Resample(orig, new, method, lpw, rolloff, beta)
        r64 = Resample(orig, new, method, lpw, rolloff, beta, dtype=torch.float64)
        o32 = np.concatenate([r32(torch.from_numpy(w)).numpy() for w in waves])
        o64 = np.concatenate([r64(torch.from_numpy(w).double()).numpy() for w in waves])
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and o32.shape == o64.shape
        assert o64.size == sum(R64.out_length(w.size, orig, new) for w in waves)
        mine = np.concatenate([R64.resample(w, orig, new, lpw, rolloff, method, beta) for w in waves])
        d = np.abs(mine - o64).max() / np.abs(o64).max()
        assert d < 1e-12, (case, d)  # tests/resample64.py is the float64 run restated
        out[case + "_lengths"], out[case + "_wave"] = np.array([w.size for w in waves], np.int64), np.concatenate(waves)
        out[case + "_out32"], out[case + "_out64"], out[case + "_err"] = o32, o64, _err(o32, o64)
        print(f"    {case:>12s} {o64.size:6d} outputs in [{o64.min():8.4f}, {o64.max():8.4f}]  fp32 vs f64: max {out[case + '_err'][0]:.2e} rms {out[case + '_err'][1]:.2e}"
              f"  resample64 vs f64: {d:.1e}")
    save("resample_cases", **out)


def ssl():
    res, outs = {}, {}
    w = GS.wave("r24k", 1, 12000)
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m, _ = GS.build(GS.NARROW, dt)
        m.resample = sys.modules["torchaudio"].transforms.Resample(24000, 16000, dtype=None if dt == torch.float32 else dt)  # AdaptiveHubert.__init__'s line
        x = torch.from_numpy(w).to(dt)
        with torch.no_grad():
            res[tag], outs[tag] = m.resample(x).numpy(), m(x, 40).numpy()
        assert res[tag].shape == (1, 8000) and outs[tag].shape == (1, 128, 40) and res[tag].dtype == outs[tag].dtype == (np.float32 if tag == "32" else np.float64)
    mine = R64.resample(w[0], 24000, 16000)
    assert np.abs(mine - res["64"][0]).max() < 1e-12 * np.abs(res["64"]).max()
    out = dict(wave=w, res32=res["32"], res64=res["64"], res_err=_err(res["32"], res["64"]), out32=outs["32"], out64=outs["64"], out_err=_err(outs["32"], outs["64"]))
    sd = float(outs["64"].std())
    assert 1e-2 < sd < 1e2, sd
    print(f"    ssl: resample fp32 vs f64 max {out['res_err'][0]:.2e} rms {out['res_err'][1]:.2e}; features std {sd:.3f} fp32 vs f64 max {out['out_err'][0]:.2e} rms {out['out_err'][1]:.2e}")
    save("resample_ssl", **out)


def rmvpe():
    audio = (0.33 * R64.signal("rmvpe", 12000, 24000).astype(np.float64)).astype(np.float32)
    got = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        net, _ = GR.build(GR.NARROW, dt)
        ex = GR.RMVPE.__new__(GR.RMVPE)
        ex.model, ex.resample_kernel = net, {}
        ex.mel_extractor = GR.MelSpectrogram(R.N_MELS, R.SAMPLE_RATE, R.N_FFT, R.HOP, None, R.MEL_FMIN, R.MEL_FMAX).to(dt)
        ex.mel_extractor.hann_window["0_cpu"] = torch.hann_window(R.N_FFT, dtype=dt)
        if dt == torch.float64:  # the reference builds Resample(sample_rate, 16000, lowpass_filter_width=128) itself; its float64 twin is seeded under the same key
            ex.resample_kernel["24000"] = Resample(24000, 16000, lowpass_filter_width=128, dtype=dt)
        seen = {}
        m2h = ex.mel2hidden
        ex.mel2hidden = lambda mel: seen.setdefault("hidden", m2h(mel))
        f0 = ex.infer_from_audio(audio, sample_rate=24000, device="cpu")
        rk = ex.resample_kernel["24000"]
        assert isinstance(rk, Resample) and rk.kernel.dtype == dt and rk.kernel.shape == (2, 1, 391)
        got[tag] = dict(res=rk(torch.from_numpy(audio)[None]).numpy(), hidden=seen["hidden"].numpy(), f0=np.asarray(f0))
        assert got[tag]["res"].shape == (1, 8000) and got[tag]["hidden"].shape == (1, 51, 360) and got[tag]["f0"].shape == (51,), got[tag]["f0"].shape
        assert got[tag]["hidden"].dtype == (np.float32 if tag == "32" else np.float64)
    mine = R64.resample(audio, 24000, 16000, 128)
    assert np.abs(mine - got["64"]["res"][0]).max() < 1e-12 * np.abs(got["64"]["res"]).max()
    out = dict(audio=audio)
    for k in ("res", "hidden"):
        out[k + "32"], out[k + "64"], out[k + "_err"] = got["32"][k], got["64"][k], _err(got["32"][k], got["64"][k])
    f32, f64 = got["32"]["f0"].astype(np.float64), got["64"]["f0"].astype(np.float64)
    v = f64 > 0
    peak = got["64"]["hidden"][0].max(axis=1)
    assert v.any() and ((f32 > 0) == v).all() and (np.abs(peak - 0.03) > 1e-3).all(), "a frame sits on the voicing threshold"
    rel = np.abs(f32[v] / f64[v] - 1)
    out["f032"], out["f064"], out["f0_err"] = got["32"]["f0"].astype(np.float32), f64, np.array([rel.max(), np.sqrt((rel * rel).mean())])
    print(f"    rmvpe: resample fp32 vs f64 max {out['res_err'][0]:.2e}; salience max {out['hidden_err'][0]:.2e} rms {out['hidden_err'][1]:.2e}; "
          f"{int(v.sum())} voiced of {v.size}, f0 max rel {rel.max():.2e}")
    save("resample_rmvpe", **out)


def main():
    cases()
    ssl()
    rmvpe()


if __name__ == "__main__":
    main()
