"""The posterior encoder's surface that needs no GPU: the weight inventory against the reference's key list, the float64 restatement against the
float64 fixtures, the library's new entries, the SpeechPredictor shim with a posterior, and the mutants of tests/posterior64.py - each moves a tap past
the bar of tests/test_hip_posterior.py at that test's shapes, so the GPU tests would catch it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import posterior64 as P64  # noqa: E402

from stylish_tts_amd import modules, params  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
TAPS = ("x0", "wn", "mean", "logstd", "z")


def fixture(name):
    """posterior_narrow / posterior_3s (their parts joined), posterior_misc (g=None) or posterior_g1024 (the second geometry, kept inside posterior_misc.npz)."""
    if name == "posterior_g1024":
        return {k[len("g1024_"):]: v for k, v in np.load(os.path.join(GOLD, "posterior_misc.npz")).items() if k.startswith("g1024_")}
    g = {k: v for k, v in np.load(os.path.join(GOLD, name + ".npz")).items() if not k.startswith("g1024_")}
    for part in ("_spec", "_phase", "_spectra", "_stats"):
        if os.path.exists(os.path.join(GOLD, name + part + ".npz")):
            g.update(np.load(os.path.join(GOLD, name + part + ".npz")))
    return g


@pytest.fixture(scope="module")
def narrow():
    return fixture("posterior_narrow")


@pytest.fixture(scope="module")
def w64(cfg):
    return P64.Weights(params.synth_state_dict(params.posterior_encoder_spec(cfg, ""), 0, prefix="speech_predictor.posterior_encoder."))


def test_spec_is_the_reference_inventory(cfg, narrow):
    spec = params.posterior_encoder_spec(cfg, "")
    assert [n for n, _, _ in spec] == [str(k) for k in narrow["keys"]]
    sh = params.spec_shapes(spec)
    assert sh["pre_spec.weight"] == (64, cfg.n_fft // 2 + 1, 1) and sh["pre_phase.weight"] == sh["pre_spec.weight"]
    assert sh["enc.cond_layer.weight_v"] == (2 * 128 * 12, 64)
    assert all(sh[f"enc.in_layers.{i}.weight_v"] == (256, 128, 3) for i in range(12))
    assert all(sh[f"enc.res_skip_layers.{i}.weight_v"] == ((256 if i < 11 else 128), 128) for i in range(12))
    assert sh["proj_mean.weight"] == (128, 128) and sh["proj_logstd.weight"] == (128, 128)
    assert [n for n, _, _ in params.posterior_encoder_spec(cfg)] == ["posterior_encoder." + n for n, _, _ in spec]
    no_g = [str(k) for k in fixture("posterior_misc")["keys"]]
    assert [n for n, _, _ in params.posterior_encoder_spec(cfg, "", gin_channels=0)] == no_g and not any("cond_layer" in k for k in no_g)
    # the speech predictor's own inventory does not grow
    assert not any(n.startswith("posterior_encoder.") for n, _, _ in params.speech_predictor_spec(cfg))


@pytest.mark.parametrize("name", ("posterior_narrow", "posterior_misc", "posterior_g1024", "posterior_3s"))
def test_posterior64_reproduces_the_float64_taps(cfg, name):
    from stylish_tts_amd.config import load_model_config

    g = fixture(name)
    gin = cfg.style_dim if "style" in g else 0
    base = dict(cfg)
    base.update(n_fft=int(g["geom"][0]), win_length=int(g["geom"][1]), hop_length=int(g["geom"][2]))
    cfg = load_model_config(base)
    assert g["har_spec"].shape[1] == cfg.n_fft // 2 + 1
    W = P64.Weights(params.synth_state_dict(params.posterior_encoder_spec(cfg, "", gin_channels=gin), 0, prefix="speech_predictor.posterior_encoder."))
    n = g["har_spec"].shape[0]  # (posterior_3s: the spectra of the first 64 rows, whose rows 0 .. 51 see nothing else through 12 layers of k = 3)
    rows = slice(0, n if n == g["x0"].shape[0] else n - 12)
    g = dict(g, noise=g["noise"][:n], off=np.minimum(g["off"], n))
    o = P64.forward(W, g["har_spec"], g["har_phase"], g.get("style"), g["noise"], g["off"])
    for k in TAPS:
        assert P64.err(o[k][rows], g[k][rows])[0] <= 1e-12 * np.abs(g[k]).max(), k
    if n != g["x0"].shape[0]:
        return
    # a single layer is the stage's layer
    cond = P64.cond_rows(W, g["style"].astype(np.float64)) if gin else np.zeros((len(g["off"]) - 1, 2 * 128 * 12))
    h, out = o["x0"], np.zeros_like(o["x0"])
    for i in range(W.n_layers):
        h, out = P64.layer(W, i, h, out, cond, g["off"])
    assert P64.err(out, g["wn"])[0] <= 1e-12 * np.abs(g["wn"]).max()


def test_library_declares_and_exports_the_entries():
    from stylish_tts_amd import _lib

    lib = _lib.load()
    for name in ("stts_posterior_forward", "stts_posterior_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "stts_op_posterior_layer" in _lib.TEST_SIGNATURES and hasattr(lib, "stts_op_posterior_layer")
    assert len(_lib.SIGNATURES["stts_posterior_forward"][1]) == 21
    assert lib.stts_posterior_workspace_bytes(None, 16, 1, 16) == 0
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "stylish_hip.h")).read()
    assert "STTS_W_POSTERIOR = 262144" in hdr and "STTS_W_ALL = 255" in hdr
    assert modules.W_POSTERIOR == 262144


def test_speech_predictor_with_a_posterior(cfg):
    sp = modules.SpeechPredictor(cfg)
    before = [(k, tuple(v.shape)) for k, v in sp.state_dict().items()]
    assert not sp.has_posterior
    pe = modules.PosteriorEncoder.from_config(cfg).load_synthetic(0)
    sp.attach_posterior(pe)
    assert sp.has_posterior and [(k, tuple(v.shape)) for k, v in sp.state_dict().items()] == before
    assert sum(v.numel() for v in sp.state_dict().values()) == 42808288
    assert list(pe.state_dict().keys()) == [n for n, _, _ in params.posterior_encoder_spec(cfg, "")]
    with pytest.raises(TypeError):
        sp.attach_posterior(torch.nn.Linear(2, 2))
    # a complete set in a checkpoint builds it, with those weights
    sp2 = modules.SpeechPredictor(cfg)
    sd = dict(sp2.state_dict())
    sd.update({"posterior_encoder." + k: v for k, v in pe.state_dict().items()})
    sp2.load_state_dict(sd)
    assert sp2.has_posterior and [(k, tuple(v.shape)) for k, v in sp2.state_dict().items()] == before
    assert all(torch.equal(v, pe.state_dict()[k]) for k, v in sp2.posterior.state_dict().items())
    # the reference's constructor refuses what the engine does not build
    with pytest.raises(ValueError, match="dilation_rate"):
        modules.PosteriorEncoder(128, 128, 3, 2, 12, cfg.n_fft, cfg.hop_length // 4, cfg.win_length, gin_channels=64, cfg=cfg)
    with pytest.raises(ValueError, match="geometry"):
        modules.PosteriorEncoder(128, 128, 3, 1, 12, 1024, 75, 1024, gin_channels=64, cfg=cfg)


def test_incomplete_or_malformed_posterior_keys_are_ignored(cfg):
    pe = modules.PosteriorEncoder.from_config(cfg).load_synthetic(0)
    full = {"posterior_encoder." + k: v for k, v in pe.state_dict().items()}
    for spoil in ("missing", "shape", "stray", "junk"):
        sp = modules.SpeechPredictor(cfg)
        sd = dict(sp.state_dict())
        extra = dict(full)
        if spoil == "missing":
            del extra["posterior_encoder.enc.res_skip_layers.11.weight_v"]
        elif spoil == "shape":
            extra["posterior_encoder.proj_mean.weight"] = torch.zeros(128, 64)
        elif spoil == "stray":
            extra = {"posterior_encoder.pre_spec.weight": torch.zeros(3)}
        else:
            extra["posterior_encoder.pre_spec.bias"] = "not a tensor"
        sd.update(extra)
        sp.load_state_dict(sd)
        assert not sp.has_posterior, spoil
    with pytest.raises(NotImplementedError):
        modules.SpeechPredictor(cfg)(None, None, None, None, None, audio_gt=torch.zeros(1, 300))


@pytest.mark.parametrize("mutant", P64.MUTANTS)
def test_every_mutant_moves_a_tap_past_the_gpu_bar(cfg, narrow, w64, mutant):
    g = narrow
    if mutant == "last_frame_kept":
        o = P64.forward_last_frame_kept(w64, g["har_spec"].astype(np.float64), g["har_phase"].astype(np.float64), g["audio"],
                                        (cfg.n_fft, cfg.win_length, cfg.hop_length // 4), g["style"], g["noise"].astype(np.float64), g["off"])
    else:
        o = P64.forward(w64, g["har_spec"], g["har_phase"], g["style"], g["noise"], g["off"], mutant=mutant)
    worst = max(max(P64.err(o[k], g[k])[j] / g["err_" + k][j] for j in range(2)) for k in TAPS)
    assert worst > BAR, f"{mutant}: worst ratio {worst:.3g} stays inside the bar"
