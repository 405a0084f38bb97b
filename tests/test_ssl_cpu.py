"""CPU side of the HuBERT content encoder (AdaptiveHubert): the parameter inventory, frame counts, the nearest index rule and the
weight-norm fold against the reference's recorded values (tests/golden/ssl_misc.npz), config handling, and the library's entry points."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def misc():
    return np.load(os.path.join(GOLD, "ssl_misc.npz"))


def test_spec_equals_the_reference_key_list_in_both_weight_norm_spellings(misc):
    from stylish_tts_amd import params

    keys, shapes = json.loads(str(misc["keys"])), json.loads(str(misc["shapes"]))
    spec = params.hubert_ssl_spec()
    assert [n for n, _, _ in spec] == keys
    assert [list(s) for _, s, _ in spec] == shapes
    assert len(keys) == 213 and "model.final_proj.weight" in keys and "model.masked_spec_embed" in keys
    q = "model.encoder.pos_conv_embed.conv."
    legacy = params.hubert_ssl_spec(weight_norm="legacy")
    want = [k.replace(q + "parametrizations.weight.original0", q + "weight_g").replace(q + "parametrizations.weight.original1", q + "weight_v") for k in keys]
    assert [n for n, _, _ in legacy] == want and [list(s) for _, s, _ in legacy] == shapes
    assert params.spec_shapes(spec)[q + "parametrizations.weight.original0"] == (1, 1, 128)
    with pytest.raises(ValueError):
        params.hubert_ssl_spec(weight_norm="other")


def test_frames_match_the_reference_and_reject_short_audio(misc):
    from stylish_tts_amd import hubert_ssl

    for n, f in zip(misc["frames_samples"], misc["frames"]):
        assert hubert_ssl.frames(int(n)) == int(f), n
    assert (hubert_ssl.frames(400), hubert_ssl.frames(719), hubert_ssl.frames(720), hubert_ssl.frames(16000), hubert_ssl.frames(48000)) == (1, 1, 2, 49, 149)
    assert hubert_ssl.min_samples() == 400
    for n in (0, 1, 399):
        with pytest.raises(ValueError, match="receptive field"):
            hubert_ssl.frames(n)


def test_nearest_index_rule(misc):
    from stylish_tts_amd import hubert_ssl

    for n_in, n_out in ((149, 240), (499, 800), (49, 7)):
        assert np.array_equal(hubert_ssl.nearest_index(n_in, n_out), misc[f"nearest_{n_in}_{n_out}"]), (n_in, n_out)


def test_weight_norm_fold_in_double(misc):
    from stylish_tts_amd import hubert_ssl, params

    sd = params.synth_state_dict([e for e in params.hubert_ssl_spec() if "pos_conv_embed" in e[0]], 0, prefix="hubert.")
    q = "model.encoder.pos_conv_embed.conv.parametrizations.weight.original"
    w = hubert_ssl.fold_pos_conv_weight(sd[q + "0"], sd[q + "1"])
    assert w.dtype == np.float32 and w.shape == (768, 48, 128)
    got, want = w.ravel()[misc["fold_idx"]].astype(np.float64), misc["fold"]
    assert np.abs(got - want).max() <= 2.0**-24 * np.abs(want).max()  # one fp32 rounding of the float64 fold
    # one norm per tap over the [768, 48] slice
    assert np.allclose(np.sqrt((w.astype(np.float64) ** 2).sum(axis=(0, 1))), sd[q + "0"].ravel(), rtol=1e-6)


@pytest.mark.parametrize("field,value", [("feat_extract_norm", "layer"), ("do_stable_layer_norm", True), ("conv_bias", True), ("hidden_act", "relu"),
                                         ("feat_extract_activation", "relu"), ("num_attention_heads", 7), ("num_conv_pos_embedding_groups", 5),
                                         ("intermediate_size", 100), ("num_hidden_layers", 0)])
def test_unsupported_fields_raise_naming_the_field(field, value):
    from stylish_tts_amd import hubert_ssl

    with pytest.raises(ValueError, match=field):
        hubert_ssl.arch({field: value})
    with pytest.raises(ValueError, match="conv_dim"):
        hubert_ssl.arch({"conv_dim": [512, 500, 512, 512, 512, 512, 512]})
    with pytest.raises(ValueError, match="conv_kernel"):
        hubert_ssl.arch({"conv_kernel": [10, 3, 3]})


def test_config_defaults_and_arch_section():
    from stylish_tts_amd import hubert_ssl
    from stylish_tts_amd.config import DEFAULT_MODEL, hubert_dims, hubert_ssl_config, load_model_config

    cfg = load_model_config()
    sr, a = hubert_ssl_config(cfg)
    assert sr == 16000 and a == hubert_ssl.arch() and a["hidden_size"] == hubert_dims(cfg)[0] == 768
    # a config without the new keys loads as before and gets the base values
    raw = copy.deepcopy(DEFAULT_MODEL)
    raw["hubert"] = {"hidden_dim": 768}
    old = load_model_config(raw)
    assert old.hubert == {"hidden_dim": 768} and hubert_ssl_config(old) == (16000, a)
    assert {k: v for k, v in cfg.items() if k != "hubert"} == {k: v for k, v in old.items() if k != "hubert"}
    raw["hubert"] = {"hidden_dim": 128, "sr": 8000, "arch": {"hidden_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2, "intermediate_size": 256,
                                                             "conv_dim": [64] * 7, "num_conv_pos_embedding_groups": 4}}
    sr, n = hubert_ssl_config(load_model_config(raw))
    assert sr == 8000 and n["hidden_size"] == 128 and n["conv_dim"] == (64,) * 7 and n["conv_kernel"] == (10, 3, 3, 3, 3, 2, 2)
    raw["hubert"]["arch"]["hidden_size"] = 256
    with pytest.raises(ValueError, match="hidden_size"):
        hubert_ssl_config(load_model_config(raw))
    raw["hubert"] = {"hidden_dim": 128}  # base arch, another width
    with pytest.raises(ValueError, match="hidden_size"):
        hubert_ssl_config(load_model_config(raw))
    raw["hubert"] = {"hidden_dim": 768, "sr": 0}
    with pytest.raises(ValueError, match="hubert.sr"):
        hubert_ssl_config(load_model_config(raw))
    raw["hubert"] = {}
    with pytest.raises(ValueError, match="hubert.hidden_dim"):
        hubert_ssl_config(load_model_config(raw))


def test_library_entry_points_and_frame_count():
    import ctypes as C

    from stylish_tts_amd import _lib, hubert_ssl

    lib = _lib.load()
    for name in ("stts_ssl_finalize", "stts_ssl_frames", "stts_ssl_workspace_bytes", "stts_ssl_forward", "stts_ssl_forward_taps", "stts_ssl_tap_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    d = hubert_ssl.dims_struct(hubert_ssl.arch())
    for n in (399, 400, 719, 720, 16000, 48000, 160000):
        want = hubert_ssl.frames(n) if n >= 400 else 0
        assert lib.stts_ssl_frames(C.byref(d), n) == want, n
    # conv0 tap rows: every utterance starts at a multiple of the later strides' product (64) and holds its 5-strided frames
    off = (C.c_int32 * 3)(0, 48000, 48720)
    rows = lib.stts_ssl_tap_rows(C.byref(d), 2, off)
    assert rows % 64 == 0 and rows >= (48000 - 10) // 5 + 1 + (720 - 10) // 5 + 1
    short = (C.c_int32 * 2)(0, 399)
    assert lib.stts_ssl_tap_rows(C.byref(d), 1, short) == 0


def test_module_shim_without_a_gpu(tmp_path):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules

    small = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, conv_dim=[32] * 7, num_conv_pos_embedding_groups=4,
                 num_conv_pos_embeddings=16)
    m = modules.AdaptiveHubert(config=small).load_synthetic(0)
    sd = m.state_dict()
    assert "model.final_proj.bias" in sd and sd["model.encoder.pos_conv_embed.conv.parametrizations.weight.original0"].shape == (1, 1, 16)
    # a local checkpoint directory: config.json + safetensors, HubertModel keys without the "model." prefix; no download
    st = pytest.importorskip("safetensors.torch")
    d = tmp_path / "ckpt"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(small, model_type="hubert")))
    st.save_file({k[len("model."):]: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    m2 = modules.AdaptiveHubert(str(d), 24000, 16000)
    assert m2.arch == m.arch and all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(ValueError, match="receptive field"):
        m2(torch.zeros(1, 399), 3)
    with pytest.raises(ValueError, match="feat_extract_norm"):
        modules.AdaptiveHubert(config={"feat_extract_norm": "layer"})
