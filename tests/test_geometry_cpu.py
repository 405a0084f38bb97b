"""STFT geometries other than the model.yml default (n_fft / win_length / hop_length), without a GPU: the rules of
stylish_tts_amd.config.geometry, the generator's parameter shapes, and the geom_* fixtures (tests/golden/gen_golden_geometry.py)
checked against a numpy composition of the oracle's parametric signal helpers, which the GPU tests lean on."""
import copy

import numpy as np
import pytest
import yaml

from conftest import load_golden
from oracle import stylish_oracle as O
from stylish_tts_amd import params, synth
from stylish_tts_amd.config import geometry, load_model_config

F32 = np.float32
GEOMS = ["geom_1024", "geom_512", "geom_4096"]


def geom_cfg(name):
    """The model config a geom_* fixture was generated with (its recorded overrides on the default model.yml) + the fixture."""
    g = load_golden(name)
    over = yaml.safe_load(bytes(g["config_overrides"]).decode())
    base = copy.deepcopy(dict(load_model_config()))
    base.update(over)
    return load_model_config(base), g


def cfg_with(**kv):
    base = copy.deepcopy(dict(load_model_config()))
    base.update(kv)
    return load_model_config(base)


@pytest.mark.parametrize("n_fft,win,hop", [(2048, 1200, 300), (1024, 1024, 256), (512, 400, 100), (4096, 2400, 600), (256, 256, 64),
                                           (256, 255, 4), (2048, 1000, 300), (4096, 4096, 1024), (1024, 777, 200)])
def test_supported_geometries(n_fft, win, hop):
    n, w, h, bins, spec = geometry(cfg_with(n_fft=n_fft, win_length=win, hop_length=hop))
    assert (n, w, h, bins) == (n_fft, win, hop // 4, n_fft // 2 + 1)
    assert spec == ((n_fft, win, hop) == (2048, 1200, 300))


@pytest.mark.parametrize("kv,rule", [
    (dict(n_fft=1000, win_length=800), "not a power of two"),
    (dict(n_fft=3072, win_length=1200), "not a power of two"),
    (dict(n_fft=8192), "outside [256, 4096]"),
    (dict(n_fft=128, win_length=128, hop_length=32), "outside [256, 4096]"),
    (dict(n_fft=1024, win_length=1200), "win_length 1200 is outside"),
    (dict(win_length=0), "win_length 0 is outside"),
    (dict(hop_length=302), "multiple of 4"),
    (dict(win_length=16, hop_length=400), "NOLA"),  # a 16-sample window cannot cover a hop of 100
    (dict(win_length=1, hop_length=4), "NOLA"),  # periodic Hann(1) = [0]
    (dict(sample_rate=0), "sample_rate"),
])
def test_refused_geometries_name_the_rule(kv, rule):
    base = copy.deepcopy(dict(load_model_config()))
    base.update(kv)
    cfg = load_model_config(base) if kv.get("hop_length", 4) % 4 == 0 else None
    if cfg is None:  # config.validate already refuses hop % 4 (its own message); geometry states the rule too
        from stylish_tts_amd.config import Record
        cfg = Record(base)
    with pytest.raises(ValueError, match=rule.replace("[", r"\[").replace("]", r"\]")):
        geometry(cfg)


@pytest.mark.parametrize("n_fft", [256, 1024, 4096])
def test_generator_spec_follows_n_fft(n_fft):
    cfg = cfg_with(n_fft=n_fft, win_length=n_fft // 2, hop_length=n_fft // 4)
    spec = {k: s for k, s, _ in params.generator_spec("", cfg)}
    bins, h = n_fft // 2 + 1, cfg.generator.hidden_dim
    assert spec["amp_output_conv.weight"][0] == bins and spec["phase_output_conv.weight"][0] == bins
    assert spec["amp_output_conv.bias"] == (bins,)
    assert spec["amp_prior_conv.weight"] == (h // 2, bins, 7) and spec["phase_prior_conv.weight"] == (h // 2, bins, 7)


def generator_geom(mel, style, pitch, src_noise, init_phase, w, n_fft, win, h, branch_hint):
    """oracle.generator_forward (models/generator.py:402-438) with the geometry as arguments: the oracle's parametric helpers
    generate_pcph(hop=h), stft_transform / istft(n_fft, h, win) composed with its conv / ConvNeXt / AdaLN blocks."""
    p = "generator."
    prior = O.generate_pcph(pitch[:, None, :], src_noise, init_phase, hop=h)[:, 0, :]
    har_spec, hx, hy = O.stft_transform(prior, n_fft, h, win)
    har_phase = np.arctan2(hy, hx).astype(F32)
    har_spec, har_phase = har_spec[:, :, :-1], har_phase[:, :, :-1]
    har_phase, bad = O.align_branch(har_phase, branch_hint, har_spec, return_bad=True)
    la_prior = O.conv1d(har_spec, w[p + "amp_prior_conv.weight"], w[p + "amp_prior_conv.bias"], padding=3)
    ph_prior = O.conv1d(har_phase, w[p + "phase_prior_conv.weight"], w[p + "phase_prior_conv.bias"], padding=3)
    x = O.conv1d(np.concatenate([mel, la_prior, ph_prior], axis=1), w[p + "projector.weight"], w[p + "projector.bias"])
    for i, k in enumerate((31, 15, 7, 3)):
        x = O.convnext_block(x, style, w, p + f"convnext.{i}.", k)
    xt = x.transpose(0, 2, 1)
    kk = w[p + "amp_output_conv.weight"].shape[2]
    la = O.adaptive_layer_norm(xt, style, w, p + "amp_final_layer_norm").transpose(0, 2, 1)
    la = O.conv1d(np.concatenate([la, la_prior], axis=1), w[p + "amp_output_conv.weight"], w[p + "amp_output_conv.bias"], padding=(kk - 1) // 2)
    ph = O.adaptive_layer_norm(xt, style, w, p + "phase_final_layer_norm").transpose(0, 2, 1)
    ph = O.conv1d(np.concatenate([ph, ph_prior], axis=1), w[p + "phase_output_conv.weight"], w[p + "phase_output_conv.bias"], padding=(kk - 1) // 2)
    la = np.concatenate([la, la[:, :, -1:]], axis=2)  # F.pad replicate (generator.py:425-426)
    ph = np.concatenate([ph, ph[:, :, -1:]], axis=2)
    audio = np.tanh(O.istft(np.exp(la), np.cos(ph), np.sin(ph), n_fft, h, win))[:, None, :].astype(F32)
    return audio, la, ph, bad


@pytest.mark.parametrize("name", GEOMS)
def test_fixture_against_oracle_composition(name):
    """The reference's waveform at this geometry, from the fixture's own mel, reproduced by the oracle helpers within fp32 tolerance
    (the atan2 cut bins adopted from the reference's tape): validates the fixture and the composition the GPU tests use."""
    cfg, g = geom_cfg(name)
    n_fft, win, h, bins, specialised = geometry(cfg)
    assert not specialised
    w = params.synth_state_dict(params.module_spec("speech_predictor", cfg), 0, prefix="speech_predictor.")
    T4 = g["mel"].shape[2]
    pitch = synth.pitch_curve("g" + name + ".pitch", 1, T4)
    style = (synth.normal("g" + name + ".style", (1, 64)) * 0.7).astype(F32)
    nz = synth.path_noise(name, 1, T4, hop4=h)
    assert g["audio"].shape == (1, 1, T4 * h)
    audio, la, ph, bad = generator_geom(g["mel"], style, pitch, nz["src_noise"], nz["init_phase"], w, n_fft, win, h,
                                        (g["cut_idx"].astype(np.int64), g["cut_phase"].astype(F32)))
    assert bad == 0
    assert la.shape == (1, bins, T4 + 1)
    kb = g["keep_bins"]
    scale = np.abs(g["logamp_bins"]).max()
    assert np.abs(la[:, kb] - g["logamp_bins"]).max() <= 2e-4 * scale, "logamp at the kept bins"
    assert np.abs(ph[:, kb] - g["phase_bins"]).max() <= 2e-4 * max(np.abs(g["phase_bins"]).max(), 1.0), "phase at the kept bins"
    err = np.abs(audio.astype(np.float64) - g["audio"]).max()
    assert err <= 1e-3, f"{name}: waveform max-abs err {err:.3e}"
