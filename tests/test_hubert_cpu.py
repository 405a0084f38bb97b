"""Host-only checks of the voice-conversion models: parameter inventories against the reference's key lists, config rules,
checkpoint round trips and the fixtures' consistency (tests/golden/gen_golden_hubert.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

from stylish_tts_amd import checkpoint, params
from stylish_tts_amd.config import check_width, hubert_dims, load_model_config

MODS = ("hubert_speech_predictor", "hubert_pitch_energy_predictor")


def test_spec_keys_equal_reference_state_dicts():
    cfg = load_model_config()
    for mod, fixture, key in (("hubert_speech_predictor", "hubert_sp_short", "sp_keys"), ("hubert_pitch_energy_predictor", "hubert_pe", "pe_keys")):
        ref = [str(k) for k in load_golden(fixture)[key]]
        spec = params.module_spec(mod, cfg)
        assert [n for n, _, _ in spec] == ref, mod
    shapes = params.spec_shapes(params.module_spec("hubert_speech_predictor", cfg))
    assert shapes["phone_encoder.phone_emb.weight"] == (128, 768, 1)
    assert shapes["style_encoder.0.weight"] == (256, 10240) and shapes["style_encoder.6.weight"] == (64, 128)
    pe = params.spec_shapes(params.module_spec("hubert_pitch_energy_predictor", cfg))
    assert pe["phone_quant.weight"] == (128, 768, 1) and pe["style_encoder.weight"] == (64, 10240) and pe["F0_proj.weight"] == (1, 192, 1)
    # the frame-path part of the HuBERT speech predictor is SpeechPredictor's, key for key and shape for shape
    sp = params.spec_shapes(params.module_spec("speech_predictor", cfg))
    frame = {k: v for k, v in shapes.items() if not k.startswith(("phone_encoder.", "style_encoder."))}
    assert frame and all(sp[k] == v for k, v in frame.items())
    # the text-to-speech composition's module list is unchanged
    assert "hubert_speech_predictor" not in params.MODULE_SPECS and checkpoint.INFERENCE_MODULES == (
        "speech_predictor", "duration_predictor", "pitch_energy_predictor", "pe_text_encoder", "pe_text_style_encoder")


def test_config_rules():
    cfg = load_model_config()
    assert hubert_dims(cfg) == (768, 10240)
    for bad in (0, -3, 2.5, None):
        raw = dict(load_model_config())
        raw["hubert"] = {"hidden_dim": bad} if bad is not None else {}
        with pytest.raises(ValueError, match="hubert.hidden_dim"):
            hubert_dims(load_model_config(raw))
    raw = dict(load_model_config())
    raw["speaker_embedder"] = {"hidden_dim": 0}
    with pytest.raises(ValueError, match="speaker_embedder.hidden_dim"):
        hubert_dims(load_model_config(raw))
    check_width("HuBERT features", 768, "hubert.hidden_dim", 768)
    with pytest.raises(ValueError, match="width 512; hubert.hidden_dim is 768"):
        check_width("HuBERT features", 512, "hubert.hidden_dim", 768)
    # a config with other widths gives specs of those widths
    raw = dict(load_model_config())
    raw["hubert"], raw["speaker_embedder"] = {"hidden_dim": 1024}, {"hidden_dim": 256}
    c2 = load_model_config(raw)
    s = params.spec_shapes(params.module_spec("hubert_pitch_energy_predictor", c2))
    assert s["phone_quant.weight"] == (128, 1024, 1) and s["style_encoder.weight"] == (64, 256)


def _synth(cfg):
    return {m: {k: torch.from_numpy(v) for k, v in params.synth_state_dict(params.module_spec(m, cfg), 0, prefix=m + ".").items()} for m in MODS}


def test_packed_round_trip_into_shims(tmp_path):
    from stylish_tts_amd import modules

    cfg = load_model_config()
    sds = _synth(cfg)
    path = os.path.join(tmp_path, "hubert.safetensors")
    pytest.importorskip("safetensors")
    checkpoint.save_packed(path, sds)
    back = checkpoint.load_packed(path)
    m = modules.build_inference_modules(cfg, hubert=True)
    checkpoint.load_into({k: m[k] for k in MODS}, back)
    for mod in MODS:
        got = m[mod].state_dict()
        assert list(got) == list(sds[mod])
        for k, v in sds[mod].items():
            assert torch.equal(got[k], v), (mod, k)
    # training-only posterior encoder keys are ignored, as SpeechPredictor's are
    sd = dict(sds["hubert_speech_predictor"], **{"posterior_encoder.pre.weight": torch.zeros(1)})
    m["hubert_speech_predictor"].load_state_dict(sd)


def test_accelerate_checkpoint_finds_both_modules(tmp_path):
    cfg = load_model_config()
    sds = _synth(cfg)
    for mod in MODS:
        i = checkpoint.MODEL_ORDER.index(mod)
        torch.save({"module." + k: v for k, v in sds[mod].items()}, os.path.join(tmp_path, f"pytorch_model_{i}.bin"))
    assert checkpoint.MODEL_ORDER.index("hubert_speech_predictor") == 12 and checkpoint.MODEL_ORDER.index("hubert_pitch_energy_predictor") == 13
    got = checkpoint.load_accelerate_checkpoint(str(tmp_path), modules=MODS)
    for mod in MODS:
        assert list(got[mod]) == list(sds[mod]) and all(torch.equal(got[mod][k], sds[mod][k]) for k in sds[mod])
    with pytest.raises(FileNotFoundError):
        checkpoint.load_accelerate_checkpoint(str(tmp_path))  # the default five are not there


def test_fixtures_are_self_consistent():
    pe = load_golden("hubert_pe")
    for T in (60, 272):
        assert pe[f"F0_{T}"].shape == (1, T) and pe[f"N_{T}"].shape == (1, T) and pe[f"style_{T}"].shape == (1, 64)
        kr = pe[f"keep_rows_{T}"]
        assert kr.max() == T - 1 and pe[f"prosody_rows_{T}"].shape == (len(kr), 192)
    for name, T in (("hubert_sp_short", 60), ("hubert_sp_long", 272)):
        g = load_golden(name)
        assert int(g["T"]) == T and g["audio"].shape == (1, 1, 4 * T * 75) and g["style"].shape == (1, 64)
        assert g["keep_rows"].max() == 4 * T - 1 and g["enc_rows"].shape == (len(g["keep_rows"]), 128)
        assert len(g["cut_idx"]) == len(g["cut_phase"])
        assert np.abs(g["audio"]).max() < 1.0  # tanh output
    assert load_golden("hubert_sp_long")["keep_rows"].max() >= 1024  # the long fixture reaches past 1024 positions
    cv = load_golden("hubert_convert")
    assert cv["F0"].shape == (1, int(cv["T"])) and cv["F0"].max() > 20.0 and cv["audio"].shape == (1, 1, 4 * int(cv["T"]) * 75)
    for n in ("hubert_pe", "hubert_sp_short", "hubert_sp_long", "hubert_convert"):
        g = load_golden(n)
        assert str(g["torch_version"])
        for k in g.files:
            if g[k].dtype.kind == "f":
                assert np.isfinite(g[k]).all(), (n, k)
