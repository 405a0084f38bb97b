"""CPU side of the RMVPE pitch extractor: the parameter inventory against the reference's recorded key list, the BatchNorm fold and the
sub-pixel repacking against the float64 module's recorded values (tests/golden/rmvpe_misc.npz), the bench tool's plain-torch restatement
against the ``hidden`` fixtures, the shim's errors, the library's entry points, and VoiceConverter.convert_audio without the new keyword."""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
NARROW = dict(n_blocks=1, inter_layers=1, en_out_channels=8)


@pytest.fixture(scope="module")
def misc():
    return np.load(os.path.join(GOLD, "rmvpe_misc.npz"))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("rmvpe_bench", os.path.join(ROOT, "tools", "rmvpe_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synth_sd(dims=None):
    from stylish_tts_amd import params, rmvpe

    return params.synth_state_dict(params.rmvpe_spec(rmvpe.dims(dims)), 0, prefix="rmvpe.")


def test_spec_equals_the_reference_key_list(misc):
    from stylish_tts_amd import params

    keys, shapes = json.loads(str(misc["keys"])), json.loads(str(misc["shapes"]))
    spec = params.rmvpe_spec()
    assert [n for n, _, _ in spec] == keys
    assert [list(s) for _, s, _ in spec] == shapes
    assert len(keys) == 741 and "unet.encoder.bn.num_batches_tracked" in keys and "fc.0.gru.weight_hh_l0_reverse" in keys
    assert params.count_params(spec) == sum(int(np.prod(s)) for s in shapes)
    narrow = params.spec_shapes(params.rmvpe_spec(NARROW))
    assert narrow["unet.decoder.layers.0.conv1.0.weight"] == (256, 128, 3, 3) and narrow["unet.decoder.layers.4.conv2.0.shortcut.weight"] == (8, 16, 1, 1)
    assert "unet.encoder.layers.0.conv.1.conv.0.weight" not in narrow  # n_blocks = 1


@pytest.mark.parametrize("field,value", [("en_de_layers", 4), ("kernel_size", (1, 2)), ("n_gru", 0), ("n_gru", 2), ("n_mels", 80), ("n_blocks", 0), ("inter_layers", 9),
                                         ("en_out_channels", 128)])
def test_unsupported_arguments_raise_naming_the_argument(field, value):
    from stylish_tts_amd import modules, rmvpe

    with pytest.raises(ValueError, match=field):
        rmvpe.dims({field: value})
    with pytest.raises(ValueError, match=field):
        modules.RmvpePitchExtractor(config={field: value})
    with pytest.raises(ValueError, match="timbre"):
        rmvpe.dims({"timbre": 1})


def test_load_state_dict_rejects_missing_and_misshaped_keys_and_ignores_the_step_counters():
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules

    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_sd(NARROW).items()}
    m = modules.RmvpePitchExtractor(config=NARROW)
    m.load_state_dict(sd)
    counters = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(counters) == 28
    without = {k: v for k, v in sd.items() if k not in counters}
    m.load_state_dict(without)  # absent
    m.load_state_dict({**sd, counters[0]: torch.tensor(12345)})  # any value
    assert all(torch.equal(m.state_dict()[k], v) for k, v in without.items())
    with pytest.raises(RuntimeError, match="missing"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "cnn.bias"})
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict({**sd, "tf.layers.0.conv.0.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="shape mismatch for fc.1.weight"):
        m.load_state_dict({**sd, "fc.1.weight": torch.zeros(360, 256)})


def test_batchnorm_fold_and_subpixel_repacking_in_double(misc):
    from stylish_tts_amd import rmvpe

    sd = synth_sd()
    p = "unet.encoder.layers.2.conv.0.conv."
    w, b = rmvpe.fold_conv_bn(sd[p + "0.weight"], sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "1.running_mean"], sd[p + "1.running_var"])
    assert w.dtype == np.float64 and w.shape == (64, 32, 3, 3)
    assert np.abs(w.ravel()[misc["fold_w_idx"]] - misc["fold_w"]).max() <= 1e-14 * np.abs(misc["fold_w"]).max()
    assert np.abs(b - misc["fold_b"]).max() <= 1e-14
    # the four sub-pixel convolutions reproduce ConvTranspose2d + BatchNorm of the float64 module on the generator's input
    from stylish_tts_amd import synth

    q = "unet.decoder.layers.4.conv1."
    scale = sd[q + "1.weight"].astype(np.float64) / np.sqrt(sd[q + "1.running_var"].astype(np.float64) + 1e-5)
    shift = sd[q + "1.bias"].astype(np.float64) - sd[q + "1.running_mean"].astype(np.float64) * scale
    x = synth.normal("rmvpe.up_input", (1, 32, 5, 6)).astype(np.float64)
    sub = rmvpe.subpixel_weights(sd[q + "0.weight"], scale)
    assert sorted(len(o) for o, _ in sub.values()) == [1, 2, 2, 4]
    xp = np.pad(x[0], ((0, 0), (0, 1), (0, 1)))  # x[n] = 0
    out = np.zeros((16, 10, 12))
    for (pt, pf), (offs, ws) in sub.items():
        for (dt, df), wt in zip(offs, ws):
            out[:, pt::2, pf::2] += np.einsum("io,itf->otf", wt, xp[:, dt : dt + 5, df : df + 6])
    out += shift[:, None, None]
    assert misc["up_out"].shape == (1, 16, 10, 12)
    assert np.abs(out - misc["up_out"][0]).max() <= 1e-12


def test_padding_frame_and_interpolation_rules(misc):
    from stylish_tts_amd import rmvpe, synth

    assert [rmvpe.padded_frames(n) for n in (17, 32, 33, 64, 100)] == [32, 32, 64, 64, 128]
    for n in (0, 15, 16):
        with pytest.raises(ValueError, match="17"):
            rmvpe.padded_frames(n)
    assert [rmvpe.mel_frames(n) for n in (513, 1600, 16000)] == [4, 11, 101]
    with pytest.raises(ValueError, match="512"):
        rmvpe.mel_frames(512)
    for n_in, n_out in ((100, 80), (17, 13)):
        x = synth.pitch_curve(f"rmvpe.curve.{n_in}", 1, n_in)[0].astype(np.float64)
        i0, i1, lam = rmvpe.interp_linear_index(n_in, n_out)
        assert np.abs((1 - lam) * x[i0] + lam * x[i1] - misc[f"interp_{n_in}_{n_out}"]).max() <= 1e-10


def test_default_mel_basis_and_its_bands():
    from stylish_tts_amd import rmvpe

    b = rmvpe.default_mel_basis()
    assert b.shape == (128, 513) and b.dtype == np.float32 and (b >= 0).all()
    band = rmvpe.basis_band(b)
    hz = np.arange(513) * 16000 / 1024
    peak = hz[b.argmax(1)]
    assert (np.diff(band[:, 0]) >= 0).all() and (band[:, 1] > band[:, 0]).all() and band[0, 0] >= 1 and band[-1, 1] <= 513
    assert 30 <= peak[0] < 80 and 7700 < peak[-1] <= 8000 and (np.diff(peak) >= 0).all()
    for m in range(128):
        assert not b[m, : band[m, 0]].any() and not b[m, band[m, 1] :].any()
    # Slaney's area normalisation: a filter's integral over frequency is 1 where it spans enough bins to be sampled well
    area = (b.astype(np.float64) * (16000 / 1024)).sum(1)
    assert np.abs(area[64:] - 1).max() < 0.05
    with pytest.raises(ValueError, match="mel_basis"):
        rmvpe.basis_band(np.zeros((80, 513)))


@pytest.mark.parametrize("case,run,dims,T", [("narrow", "n33", NARROW, 33), ("narrow", "n100", NARROW, 100), ("full_a", "f17", None, 17)])
def test_torch_restatement_reproduces_the_hidden_fixture(bench, case, run, dims, T):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import rmvpe, synth

    g = np.load(os.path.join(GOLD, f"rmvpe_{case}.npz"))
    sd, d = synth_sd(dims), rmvpe.dims(dims)
    mel = torch.from_numpy((synth.normal("rmvpe.mel." + run, (1, 128, T)) * 2.0 - 5.0).astype(np.float32))
    idx, f32, f64 = g[f"{run}_hidden_idx"].astype(np.int64), g[f"{run}_hidden_f32"].astype(np.float64), g[f"{run}_hidden_f64"]
    with torch.no_grad():
        h32 = bench.mel2hidden(bench.to_dtype(sd, torch.float32), d, mel)
        h64 = bench.mel2hidden(bench.to_dtype(sd, torch.float64), d, mel.double())
    assert tuple(h32.shape) == (1, T, 360)
    ref = np.abs(f32 - f64).max()
    assert np.abs(h32.double().numpy().ravel()[idx] - f64).max() <= 4 * ref
    assert np.abs(h64.numpy().ravel()[idx] - f64).max() <= 1e-12


def test_torch_restatement_of_the_decode_and_the_log_mel(bench, misc):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import rmvpe, synth

    sal = torch.from_numpy(misc["decode_sal"])
    for k, th in enumerate(misc["decode_thred"]):
        got = bench.decode(sal.double(), float(th)).numpy()
        assert np.array_equal(got > 0, misc[f"decode_f64_{k}"] > 0)
        assert np.abs(got - misc[f"decode_f64_{k}"]).max() <= 1e-9
    basis = torch.from_numpy(rmvpe.default_mel_basis())
    x = torch.from_numpy((synth.normal("rmvpe.audio.1600", (1, 1600)) * 0.1).astype(np.float32)).double()
    assert np.abs(bench.log_mel(x, basis)[0].numpy() - misc["mel_1600_log64"]).max() <= 1e-9
    assert abs(bench.conv_flops_per_frame(rmvpe.dims()) * 1e-6 - 69.4) < 0.05


def test_shim_errors_without_a_gpu(tmp_path):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules

    m = modules.RmvpePitchExtractor(config=NARROW).load_synthetic(0)
    with pytest.raises(NotImplementedError):
        m.decode(torch.zeros(1, 20, 360), use_viterbi=True)
    with pytest.raises(NotImplementedError):
        m.infer_from_audio(torch.zeros(1, 16000), use_viterbi=True)
    for bad in (torch.zeros(1, 80, 40), torch.zeros(128, 40), torch.zeros(1, 128, 16)):
        with pytest.raises(ValueError):
            m.mel2hidden(bad)
    with pytest.raises(ValueError, match="lengths"):
        m(torch.zeros(2, 128, 40), lengths=[40, 41])
    with pytest.raises(ValueError, match="16000"):
        m.infer_from_audio(torch.zeros(1, 24000), sample_rate=24000)
    with pytest.raises(ValueError, match="512"):
        m.infer_from_audio(torch.zeros(1, 512))
    with pytest.raises(ValueError, match="17"):
        m.infer_from_audio(torch.zeros(1, 160 * 15))
    with pytest.raises(ValueError, match="mel_basis"):
        m.mel_basis = torch.zeros(128, 512)
    m.mel_basis = m.mel_basis * 2  # the buffer may be set
    assert float(m.mel_basis.max()) > 0 and m._band.shape == (128, 2)
    # the reference's checkpoint format
    st = pytest.importorskip("safetensors.torch")
    sd = m.state_dict()
    st.save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "rmvpe.safetensors"))
    m2 = modules.RmvpePitchExtractor.from_safetensors(str(tmp_path / "rmvpe.safetensors"), config=NARROW)
    assert list(m2.state_dict()) == list(sd) and all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items() if not k.endswith("num_batches_tracked"))
    with pytest.raises(RuntimeError):
        modules.RmvpePitchExtractor.from_safetensors(str(tmp_path / "rmvpe.safetensors"))  # full-size shapes


def test_library_entry_points_and_tap_sizes():
    import ctypes as C

    from stylish_tts_amd import _lib, rmvpe

    lib = _lib.load()
    for name in ("stts_rmvpe_finalize", "stts_rmvpe_workspace_bytes", "stts_rmvpe_forward", "stts_rmvpe_forward_taps", "stts_rmvpe_tap_floats", "stts_rmvpe_mel",
                 "stts_rmvpe_decode", "stts_rmvpe_resample"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    d = rmvpe.dims_struct(rmvpe.dims())
    off = (C.c_int32 * 3)(0, 17, 117)  # 32 + 128 padded frames
    Tp = 160
    want = sum((Tp >> (l + 1)) * (64 >> l) * (16 << l) for l in range(5)) + (Tp >> 5) * 4 * 512 + sum((Tp >> (4 - i)) * (8 << i) * (16 << (4 - i)) for i in range(5))
    assert lib.stts_rmvpe_tap_floats(C.byref(d), 2, off) == want + Tp * 128 * 4 + Tp * 512
    short = (C.c_int32 * 2)(0, 16)
    assert lib.stts_rmvpe_tap_floats(C.byref(d), 1, short) == 0
    bad = rmvpe.dims_struct(dict(rmvpe.dims(), n_gru=2))
    assert lib.stts_rmvpe_tap_floats(C.byref(bad), 2, off) == 0


def test_convert_audio_without_the_keyword_is_unchanged():
    torch = pytest.importorskip("torch")
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter

    sig = inspect.signature(VoiceConverter.convert_audio)
    assert sig.parameters["pitch_extractor"].default is None and list(sig.parameters)[:6] == ["self", "wave", "sample_lengths", "frames", "spk_emb", "ssl"]

    class Engine:
        cfg = load_model_config()

    class Ssl:
        hidden, sr, _engine = 768, 16000, None

        def packed(self, wave, T, lengths):
            return ("feats", tuple(T), tuple(lengths))

    class Px:
        sr, _engine = 16000, None

        def packed_from_audio(self, wave, lengths, T):
            return torch.tensor([0.0, 110.0, 0.0])

    vc, seen = VoiceConverter(Engine()), []
    vc.convert = lambda *a, **k: seen.append((a, k)) or "waves"
    w, spk = torch.zeros(1, 800), torch.zeros(1, 4)
    assert vc.convert_audio(w, [800], [3], spk, ssl=Ssl(), noise=None) == "waves"
    a, k = seen.pop()
    assert a == (None, [3], spk) and k == dict(_packed_feats=("feats", (3,), (800,)), noise=None)
    vc.convert_audio(w, [800], [3], spk, ssl=Ssl(), pitch_extractor=Px())
    a, k = seen.pop()
    assert sorted(k) == ["_packed_feats", "_packed_pitch"] and k["_packed_pitch"].tolist() == [0.0, 110.0, 0.0]
    vc.convert_audio(w, [800], [3], spk, ssl=Ssl(), pitch_extractor=Px(), ref_mel=torch.zeros(1, 80, 5))
    a, k = seen.pop()
    assert "_packed_pitch" not in k and k["_packed_uv"].tolist() == [1.0, 0.0, 1.0]
    with pytest.raises(ValueError, match="not both"):
        vc.convert_audio(w, [800], [3], spk, ssl=Ssl(), pitch_extractor=Px(), pitch=torch.zeros(1, 3))
    # convert() itself keeps its rule for the caller's curves
    src = inspect.getsource(VoiceConverter.convert)
    assert "give both pitch and energy, or neither" in src
