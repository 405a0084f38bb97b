"""CfmPitchPredictor without a GPU: the state-dict inventory against the reference's key list, the module spec from the model config,
norm_f0_zscore / denorm_f0_zscore against the reference (tests/golden/cfm_pitch.npz), the shim's shape and length checks, and the
checkpoint reader feeding the shim."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from stylish_tts_amd import checkpoint, modules, params
from stylish_tts_amd.config import load_model_config

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cfm_pitch.npz")


def test_spec_keys_equal_reference():
    ref = list(np.load(GOLD)["keys"])
    keys = [k for k, _, _ in params.cfm_pitch_predictor_spec(768, 80)]
    assert keys == ref
    assert "in_proj.weight" in keys and "spk_emb.shared.6.weight_orig" in keys


def test_spk_emb_part_is_the_mel_style_encoder_spec():
    spec = params.cfm_pitch_predictor_spec(768, 80)
    spk = [(k[len("spk_emb."):], s) for k, s, _ in spec if k.startswith("spk_emb.")]
    assert spk == [(k, s) for k, s, _ in params.mel_style_encoder_spec(80, 256, 1024, True)]


def test_module_spec_follows_hubert_dim_and_n_mels():
    cfg = load_model_config()
    shapes = params.spec_shapes(params.module_spec("cfm_pitch_predictor", cfg))
    assert shapes["asr_emb.0.weight"] == (1024, cfg.hubert.hidden_dim, 1)
    assert shapes["spk_emb.shared.0.weight_orig"] == (cfg.n_mels, 1, 3, 3)
    cfg2 = load_model_config()
    cfg2.hubert.hidden_dim = 1024
    assert params.spec_shapes(params.module_spec("cfm_pitch_predictor", cfg2))["asr_emb.0.weight"] == (1024, 1024, 1)
    m = modules.build_inference_modules(cfg, cfm_pitch=True)["cfm_pitch_predictor"]
    assert (m.asr_dim, m.n_mels) == (cfg.hubert.hidden_dim, cfg.n_mels)


@pytest.mark.parametrize("lib", ["torch", "numpy"])
def test_denorm_f0_zscore_equals_reference(lib):
    g = np.load(GOLD)
    mean, std = (float(v) for v in g["f0_log2_stats"])
    x = np.concatenate([np.linspace(-12, 12, 97), np.linspace(-1.5, 1.5, 63)]).astype(np.float32)  # the generator's inputs
    uv = g["denorm_uv"]
    if lib == "torch":
        m, s = torch.tensor(mean), torch.tensor(std)
        hz = modules.denorm_f0_zscore(torch.from_numpy(x), None, m, s).numpy()
        hz_uv = modules.denorm_f0_zscore(torch.from_numpy(x), torch.from_numpy(uv), m, s).numpy()
        np.testing.assert_array_equal(hz, g["denorm_hz"])
        np.testing.assert_array_equal(hz_uv, g["denorm_hz_uv"])
    else:
        hz = modules.denorm_f0_zscore(x, None, np.float32(mean), np.float32(std))
        hz_uv = modules.denorm_f0_zscore(x, uv, np.float32(mean), np.float32(std))
        np.testing.assert_allclose(hz, g["denorm_hz"], rtol=2e-6, atol=0)
        np.testing.assert_allclose(hz_uv, g["denorm_hz_uv"], rtol=2e-6, atol=0)
    assert hz.min() == 50 and hz.max() == 1200  # both clamp ends are covered
    assert (hz_uv[uv > 0] == 0).all() and (hz_uv[uv == 0] > 0).all()


@pytest.mark.parametrize("lib", ["torch", "numpy"])
def test_norm_f0_zscore_equals_reference(lib):
    g = np.load(GOLD)
    mean, std = (float(v) for v in g["f0_log2_stats"])
    f0 = g["norm_f0"]
    if lib == "torch":
        got = modules.norm_f0_zscore(torch.from_numpy(f0), torch.from_numpy(f0) == 0, torch.tensor(mean), torch.tensor(std)).numpy()
        np.testing.assert_array_equal(got, g["norm_normed"])
    else:
        got = modules.norm_f0_zscore(f0, f0 == 0, np.float32(mean), np.float32(std))
        np.testing.assert_allclose(got, g["norm_normed"], rtol=1e-5, atol=1e-6)


def test_shim_rejects_bad_shapes_and_lengths():
    m = modules.CfmPitchPredictor(768, 80)
    asr, mel = torch.zeros(2, 768, 50), torch.zeros(2, 80, 40)
    assert m._lengths(asr, mel, None, None) == ([50, 50], [40, 40])
    assert m._lengths(asr, mel, [3, 50], [33, 40]) == ([3, 50], [33, 40])
    for bad in [(torch.zeros(2, 512, 50), mel, None, None),   # asr width
                (torch.zeros(768, 50), mel, None, None),       # asr rank
                (asr, torch.zeros(2, 64, 40), None, None),     # n_mels
                (asr, torch.zeros(3, 80, 40), None, None),     # batch mismatch
                (asr, mel, [50, 51], None),                    # asr length beyond the batch
                (asr, mel, [0, 50], None),                     # empty utterance
                (asr, mel, [50], None),                        # wrong count
                (asr, mel, None, [40, 41])]:                   # mel length beyond the batch
        with pytest.raises(ValueError):
            m._lengths(*bad)


def test_accelerate_checkpoint_feeds_the_shim(tmp_path):
    accelerate = pytest.importorskip("accelerate")  # noqa: F841
    from accelerate.checkpointing import save_accelerator_state

    sd = {k: torch.from_numpy(v) for k, v in params.synth_state_dict(params.cfm_pitch_predictor_spec(768, 80), 6).items()}
    states = [sd if name == "cfm_pitch_predictor" else {"unused.weight": torch.zeros(2)} for name in checkpoint.MODEL_ORDER]
    save_accelerator_state(str(tmp_path), states, [], [], [], 0, 0, safe_serialization=False)
    assert os.path.basename(checkpoint.checkpoint_files(str(tmp_path), ["cfm_pitch_predictor"])["cfm_pitch_predictor"]) == "pytorch_model_11.bin"
    got = checkpoint.load_accelerate_checkpoint(str(tmp_path), modules=("cfm_pitch_predictor",))
    m = modules.build_inference_modules(load_model_config(), cfm_pitch=True)["cfm_pitch_predictor"]
    m.load_state_dict(got["cfm_pitch_predictor"])  # strict: in_proj and spk_emb included
    for k in sd:
        assert torch.equal(m.state_dict()[k], sd[k]), k
