"""MelStyleEncoder without a GPU: spectral-norm folding, the state-dict inventory against the reference's key lists, the n_mels / length
rules against what the reference rejects (tests/golden/mel_style_misc.npz), and the checkpoint reader on the new components."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from stylish_tts_amd import checkpoint, modules, params
from stylish_tts_amd.config import load_model_config

GOLD = os.path.join(os.path.dirname(__file__), "golden", "mel_style_misc.npz")
CONFIGS = {"pe": (80, 64, 384, True), "cfm": (80, 256, 1024, True)}


@pytest.mark.parametrize("iters", [64, 1])
@pytest.mark.parametrize("shape", [(160, 80, 3, 3), (80, 1, 3, 3), (384, 384, 5, 5)])
def test_spectral_fold_equals_torch_eval_weight(shape, iters):
    w = params.synth_tensor("sn.w", shape, "w")
    u, v = params.spectral_uv(w, "sn", iters=iters)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(shape[1], shape[0], shape[2], bias=False).double())
    with torch.no_grad():
        conv.weight_orig.copy_(torch.from_numpy(w))
        conv.weight_u.copy_(torch.from_numpy(u))
        conv.weight_v.copy_(torch.from_numpy(v))
    conv.eval()
    conv(torch.zeros(1, shape[1], 5, 5, dtype=torch.float64))  # eval: no power iteration, the weight from the stored u, v
    ref = conv.weight.detach().numpy()
    got = params.fold_spectral_norm(w, u, v)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)
    if iters == 1:  # not converged: sigma differs from the true largest singular value, and the fold must use the stored vectors
        assert abs(np.linalg.norm(got.reshape(shape[0], -1), 2) - 1.0) > 1e-6


def test_synthetic_uv_are_converged():
    w = params.synth_tensor("sn.w", (320, 160, 3, 3), "w")
    u, v = params.spectral_uv(w, "sn")
    # 64 float64 steps: sigma within 1 % of the largest singular value (the folded weight has spectral norm ~1)
    np.testing.assert_allclose(np.linalg.norm(params.fold_spectral_norm(w, u, v).reshape(320, -1), 2), 1.0, rtol=1e-2)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_spec_keys_equal_reference(cfg):
    ref = list(np.load(GOLD)[f"keys_{cfg}"])
    assert [k for k, _, _ in params.mel_style_encoder_spec(*CONFIGS[cfg])] == ref


def test_pe_module_spec_is_model_yml_configuration():
    spec = params.module_spec("pe_mel_style_encoder", load_model_config())
    assert [k for k, _, _ in spec] == list(np.load(GOLD)["keys_pe"])


def test_n_mels_rule_matches_reference():
    g = np.load(GOLD)
    rejected = set(int(x) for x in g["rejected_n_mels"])
    for n in g["n_mels_tried"]:
        n = int(n)
        if n in rejected:
            with pytest.raises(ValueError):
                modules.mel_style_levels(n, True)
        else:
            modules.mel_style_levels(n, True)


def test_min_frames_matches_reference():
    rej = np.load(GOLD)["rejected_lengths"]
    _, t_min = modules.mel_style_levels(80, True)
    assert t_min == 33 and int(rej.max()) == t_min - 1 and list(rej) == list(range(int(rej.min()), t_min))


def test_shim_rejects_lengths_that_do_not_fit_the_batch():
    """Lengths beyond the padded batch are the shim's to reject; mels below the minimum (33 frames) are the engine's (RuntimeError,
    tests/test_hip_mel_style.py), so that the C entry is the one place that checks them."""
    enc = modules.MelStyleEncoder(80, 64, 384, True)
    with pytest.raises(ValueError):
        enc._lengths(torch.zeros(2, 1, 80, 40), [40, 41])
    with pytest.raises(ValueError):
        enc._lengths(torch.zeros(2, 1, 80, 40), [40])
    assert enc._lengths(torch.zeros(2, 1, 80, 40), None) == [40, 40]
    assert enc.min_frames == 33


def test_tap_shapes_follow_the_reference_levels():
    shapes = modules.mel_style_tap_shapes(80, 384, True, [33, 240])
    assert [(s[2], s[3], s[4]) for s in shapes] == [(160, 40, [17, 120]), (320, 20, [9, 60]), (384, 10, [5, 30]), (384, 10, [5, 30])]


def test_accelerate_checkpoint_feeds_the_shim(tmp_path):
    accelerate = pytest.importorskip("accelerate")  # noqa: F841
    from accelerate.checkpointing import save_accelerator_state

    cfg = load_model_config()
    sd = {k: torch.from_numpy(v) for k, v in params.synth_state_dict(params.module_spec("pe_mel_style_encoder", cfg), 4).items()}
    spk = {("spk_emb." + k): torch.from_numpy(v) for k, v in params.synth_state_dict(params.mel_style_encoder_spec(*CONFIGS["cfm"]), 5).items()}
    states = []
    for name in checkpoint.MODEL_ORDER:
        states.append(sd if name == "pe_mel_style_encoder" else spk if name == "cfm_pitch_predictor" else {"unused.weight": torch.zeros(2)})
    save_accelerator_state(str(tmp_path), states, [], [], [], 0, 0, safe_serialization=False)
    got = checkpoint.load_accelerate_checkpoint(str(tmp_path), modules=("pe_mel_style_encoder", "cfm_pitch_predictor"))
    pe = modules.build_inference_modules(cfg, mel_style=True)["pe_mel_style_encoder"]
    pe.load_state_dict(got["pe_mel_style_encoder"])
    for k in sd:
        assert torch.equal(pe.state_dict()[k], sd[k])
    enc = modules.MelStyleEncoder(*CONFIGS["cfm"], component="cfm_pitch_predictor.spk_emb")
    enc.load_state_dict({k[len("spk_emb."):]: v for k, v in got["cfm_pitch_predictor"].items() if k.startswith("spk_emb.")})
    assert torch.equal(enc.state_dict()["shared.6.weight_orig"], spk["spk_emb.shared.6.weight_orig"])
