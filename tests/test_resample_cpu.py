"""No GPU: the host side of the windowed-sinc resampler - tests/resample64.py against the float64 arrays of the fixtures
(tests/golden/gen_golden_resample.py), the library's geometry / output-length entries and stylish_tts_amd/resample.py against hand values, the
interface limits with their numbers, and the shims' ValueError paths that need no device."""
import ctypes as C
import types

import numpy as np
import pytest

import resample64 as R64
from conftest import load_golden

# orig, new, lowpass_filter_width -> o, n, width, taps (by hand: width = ceil(lpw * o / (min(o, n) * 0.99)), taps = 2 width + o)
HAND = [
    ((24000, 16000, 6), (3, 2, 10, 23)),
    ((24000, 16000, 128), (3, 2, 194, 391)),
    ((44100, 16000, 6), (441, 160, 17, 475)),
    ((16000, 24000, 6), (2, 3, 7, 16)),
    ((48000, 16000, 6), (3, 1, 19, 41)),
]


@pytest.mark.parametrize("case", sorted(R64.CASES))
def test_resample64_reproduces_the_float64_run(case):
    g = load_golden("resample_cases")
    orig, new, lpw, rolloff, method, beta = R64.CASES[case]
    L = list(g[case + "_lengths"])
    o, _ = R64.reduced(orig, new)
    assert L[:5] == [1, 5, 7 * o - 1, 7 * o, 7 * o + 1] and g[case + "_wave"].dtype == np.float32 and g[case + "_wave"].size == sum(L)
    waves = np.split(g[case + "_wave"], np.cumsum(L)[:-1])
    mine = np.concatenate([R64.resample(w, orig, new, lpw, rolloff, method, beta) for w in waves])
    ref = g[case + "_out64"]
    assert ref.dtype == np.float64 and mine.shape == ref.shape == (sum(R64.out_length(n, orig, new) for n in L),)
    assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()
    e = g[case + "_out32"].astype(np.float64) - ref
    assert g[case + "_out32"].dtype == np.float32 and np.allclose(g[case + "_err"], [np.abs(e).max(), np.sqrt((e * e).mean())], rtol=1e-12) and g[case + "_err"][0] > 0


def test_resample64_reproduces_the_reference_front_ends_float64_resampling():
    g = load_golden("resample_ssl")
    assert g["wave"].shape == (1, 12000) and g["res64"].shape == (1, 8000) and g["out64"].shape == (1, 128, 40)
    assert np.abs(R64.resample(g["wave"][0], 24000, 16000) - g["res64"][0]).max() <= 1e-12 * np.abs(g["res64"]).max()
    g = load_golden("resample_rmvpe")
    assert g["audio"].shape == (12000,) and g["res64"].shape == (1, 8000) and g["hidden64"].shape == (1, 51, 360) and g["f064"].shape == (51,)
    assert np.abs(R64.resample(g["audio"], 24000, 16000, 128) - g["res64"][0]).max() <= 1e-12 * np.abs(g["res64"]).max()
    for k in ("res", "hidden"):
        e = g[k + "32"].astype(np.float64) - g[k + "64"]
        assert np.allclose(g[k + "_err"], [np.abs(e).max(), np.sqrt((e * e).mean())], rtol=1e-12) and g[k + "_err"][0] > 0


def test_equal_rates_and_the_cases_that_take_the_kernels_other_paths():
    from stylish_tts_amd import resample

    # equal rates reduce to 1 / 1 in the library as in the oracle, which copies
    assert resample.geometry(16000, 16000, 6)[:2] == resample.reduced(48000, 48000) == (1, 1) and resample.out_length(100, 16000, 16000) == 100
    x = R64.signal("copy", 100, 16000)
    assert (R64.resample(x, 16000, 16000) == x.astype(np.float64)).all() and (R64.resample(x, 48000, 48000, 128) == x).all()
    # the filter's DC gain is 1 up to the window's leakage: a constant stays a constant away from the edges
    y = R64.resample(np.ones(600), 24000, 16000)
    assert np.abs(y[20:-20] - 1.0).max() < 2e-3
    # the GPU cases hold one table of more than one 512-tap staging pass and one of more than one 256-phase block
    # (csrc/resample.hip.h: kResampleChunk, kResampleThreads)
    assert resample.geometry(*R64.CASES["r441_160_w128"][:4]) == (441, 160, 357, 1155)
    assert resample.geometry(*R64.CASES["r160_441"][:4]) == (160, 441, 7, 174)


@pytest.mark.parametrize("args,want", HAND)
def test_geometry_against_hand_values(args, want):
    from stylish_tts_amd import _lib, resample

    orig, new, lpw = args
    assert resample.geometry(orig, new, lpw) == want  # the library's host code
    assert resample.reduced(orig, new) + resample.width(orig, new, lpw) == want
    assert resample.check(orig, new, lpw)[:4] == want and R64.geometry(orig, new, lpw) == want
    lib = _lib.load()
    o, n = want[:2]
    for k in (1, 50):
        for ln in {o * k, o * k + 1, o * k + o - 1}:  # len mod o = 0, 1, o - 1
            m = -(-n * ln // o)
            assert lib.stts_resample_out_length(ln, orig, new) == resample.out_length(ln, orig, new) == R64.out_length(ln, orig, new) == m
    assert lib.stts_resample_out_length(3 * o, orig, new) == 3 * n
    t = resample.tile(orig, new)  # whole input steps of n outputs each, at most 4 per thread of a 256-thread block
    assert t % n == 0 and n <= t <= 4 * max(256, n)


def test_out_length_by_hand():
    from stylish_tts_amd import _lib, resample

    lib = _lib.load()
    # 24 -> 16 kHz: 3 -> 2.  6 samples -> 4, 7 -> ceil(14 / 3) = 5, 8 -> ceil(16 / 3) = 6
    assert [resample.out_length(s, 24000, 16000) for s in (1, 6, 7, 8)] == [1, 4, 5, 6]
    # 44.1 -> 16 kHz: 441 -> 160.  441 -> 160, 442 -> ceil(70720 / 441) = 161, 881 -> ceil(140960 / 441) = 320
    assert [resample.out_length(s, 44100, 16000) for s in (441, 442, 881)] == [160, 161, 320]
    assert [lib.stts_resample_out_length(s, 16000, 24000) for s in (1, 2, 3)] == [2, 3, 5]
    assert lib.stts_resample_out_length(-1, 3, 2) == -1 and lib.stts_resample_out_length(5, 0, 2) == -1
    assert resample.out_lengths([6, 7], 24000, 16000) == [4, 5]
    with pytest.raises(ValueError, match="utterance 1 has 0 samples"):
        resample.out_lengths([6, 0], 24000, 16000)


def test_every_limit_names_its_number():
    from stylish_tts_amd import _lib, resample

    lib = _lib.load()

    def status(*a):
        rc = lib.stts_resample_geometry(*a, None, None, None, None)
        return rc, lib.stts_last_error().decode()

    for args, py_words, c_words in [
        ((1025, 1, 6, 0.99), "reduces to 1025", "= 1025 is above 1024"),
        ((2, 2051, 6, 0.99), "reduces to 2051", "= 2051 is above 1024"),
        ((1023, 1024, 256, 0.99), "1024 phases x 1541 taps = 1577984", "1024 phases x 1541 taps = 1577984"),
        ((3, 2, 0, 0.99), "lowpass_filter_width 0 is outside [1, 256]", "lowpass_filter_width 0 is outside [1, 256]"),
        ((3, 2, 257, 0.99), "lowpass_filter_width 257", "lowpass_filter_width 257"),
        ((3, 2, 6, 0.0), "rolloff 0.0 is outside (0, 1]", "rolloff 0 is outside (0, 1]"),
        ((3, 2, 6, 1.01), "rolloff 1.01", "rolloff 1.01"),
        ((0, 2, 6, 0.99), "orig_freq 0", "orig_freq 0"),
    ]:
        with pytest.raises(ValueError) as ei:
            resample.check(*args)
        assert py_words in str(ei.value), (args, str(ei.value))
        rc, msg = status(*args)
        assert rc != 0 and c_words in msg, (args, msg)
    # a tiny rolloff makes the table too large, not an overflow
    rc, msg = status(1024, 1, 256, 1e-9)
    assert rc != 0 and "taps" in msg
    assert status(2048, 2, 6, 0.99)[0] == 0  # the limits apply after the gcd reduction
    with pytest.raises(ValueError, match="resampling_method must be one of"):
        resample.check(3, 2, 6, 0.99, "sinc_interpolation")
    for beta in (-1.0, 513.0, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            resample.check(3, 2, 6, 0.99, "sinc_interp_kaiser", beta)
    assert resample.check(3, 2, 6, 0.99, "sinc_interp_kaiser")[4:] == (1, resample.KAISER_BETA)


def test_forward_refuses_bad_offsets_before_any_device_work():
    """The offset checks of stts_resample_forward run on the host arrays, ahead of the first HIP call: a status with the numbers, no GPU needed."""
    from stylish_tts_amd import _lib

    lib = _lib.load()
    ctx = p = None  # no context and no device pointers: the interface conditions come first, and a call that met them all ends at "null argument"

    def run(lens_in, lens_out, orig=24000, new=16000, lpw=6, rolloff=0.99, method=0, beta=0.0):
        a = np.concatenate([[0], np.cumsum(lens_in)]).astype(np.int32)
        b = np.concatenate([[0], np.cumsum(lens_out)]).astype(np.int32)
        rc = lib.stts_resample_forward(ctx, None, orig, new, lpw, rolloff, method, beta, len(lens_in), a.ctypes.data_as(C.c_void_p), p, b.ctypes.data_as(C.c_void_p), p, p, p)
        return rc, lib.stts_last_error().decode()

    rc, msg = run([6, 0], [4, 0])
    assert rc != 0 and "utterance 1 has 0 samples" in msg
    rc, msg = run([6, 7], [4, 4])
    assert rc != 0 and "utterance 1: 4 output samples for 7 input samples at 3 -> 2, the formula gives 5" in msg
    rc, msg = run([6], [4], method=2)
    assert rc != 0 and "method 2" in msg
    rc, msg = run([6], [4], method=1, beta=-3.0)
    assert rc != 0 and "beta -3" in msg
    rc, msg = run([6], [4], lpw=300)
    assert rc != 0 and "lowpass_filter_width 300" in msg
    rc, msg = run([6, 7], [4, 5])
    assert rc != 0 and "null argument" in msg


def test_the_shims_refuse_on_the_host(cfg):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules

    for bad, words in [(dict(orig_freq=1025, new_freq=1), "1025"), (dict(lowpass_filter_width=0), "lowpass_filter_width 0"), (dict(rolloff=1.5), "rolloff 1.5"),
                       (dict(resampling_method="kaiser_best"), "resampling_method"), (dict(resampling_method="sinc_interp_kaiser", beta=-1.0), "beta -1.0")]:
        with pytest.raises(ValueError, match=words):
            modules.Resample(**{**dict(orig_freq=24000, new_freq=16000), **bad})
    rs = modules.Resample(24000, 16000)
    assert (rs.o, rs.n, rs.width, rs.taps) == (3, 2, 10, 23) and rs.out_lengths([6, 7]) == [4, 5]
    for fn in (rs.forward, rs.packed):  # refused before an engine is asked for
        with pytest.raises(ValueError, match="do not fit"):
            fn(torch.zeros(2, 30), [30, 31])
        with pytest.raises(ValueError, match="utterance 1 has 0 samples"):
            fn(torch.zeros(2, 30), [30, 0])
    with pytest.raises(ValueError, match=r"\[B, samples\]"):
        rs.packed(torch.zeros(30))

    # AdaptiveHubert: the receptive field (400 samples at 16 kHz) is measured on the RESAMPLED length: 599 samples at 24 kHz give 400, 598 give 399
    hub = modules.AdaptiveHubert(config=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7,
                                             num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=4))
    assert hub._lengths(torch.zeros(1, 599), None, 24000) == ([599], [400]) and hub._lengths(torch.zeros(1, 400), None, None) == ([400], [400])
    assert hub._lengths(torch.zeros(1, 400), None, 16000) == ([400], [400])
    with pytest.raises(ValueError):
        hub.forward(torch.zeros(1, 598), 3, sample_rate=24000)
    with pytest.raises(ValueError):
        hub.packed(torch.zeros(1, 399), [3])
    with pytest.raises(ValueError, match="reduces to 16001"):
        hub.forward(torch.zeros(1, 4000), 3, sample_rate=16001)

    # RmvpePitchExtractor: the old raise without resample=True; with it the length checks move to the resampled length (513 samples at 16 kHz)
    px = modules.RmvpePitchExtractor(config=dict(n_blocks=1, inter_layers=1, en_out_channels=8))
    for fn in (px.mel_packed, px.mel, px.packed_from_audio, px.infer_from_audio):
        with pytest.raises(ValueError, match="16000"):
            fn(torch.zeros(1, 24000), sample_rate=24000)
    assert px._wave_lengths(torch.zeros(1, 770), None, 24000, True) == ([770], [514])
    with pytest.raises(ValueError):
        px.mel_packed(torch.zeros(1, 768), sample_rate=24000, resample=True)  # 512 samples at 16 kHz
    with pytest.raises(ValueError):
        px.infer_from_audio(torch.zeros(1, 160 * 15 * 3 // 2), sample_rate=24000, resample=True)  # 16 frames: below mel2hidden's reflect padding
    with pytest.raises(NotImplementedError):
        px.infer_from_audio(torch.zeros(1, 24000), sample_rate=24000, resample=True, use_viterbi=True)


def test_convert_audio_refuses_a_bad_sample_rate_on_the_host(cfg):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules
    from stylish_tts_amd.config import hubert_dims
    from stylish_tts_amd.pipeline import VoiceConverter

    hd, sd = hubert_dims(cfg)
    vc = VoiceConverter(types.SimpleNamespace(cfg=cfg, device=torch.device("cpu")))
    hub = modules.AdaptiveHubert(config=dict(hidden_size=hd, num_hidden_layers=1, num_attention_heads=hd // 64, intermediate_size=64, conv_dim=(32,) * 7,
                                             num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=hd // 48))
    spk = torch.zeros(1, sd)
    with pytest.raises(ValueError, match="sample_rate 0 must be a positive integer"):
        vc.convert_audio(torch.zeros(1, 24000), [24000], [80], spk, ssl=hub, sample_rate=0)
    with pytest.raises(ValueError, match="sample_rate 22050.5"):
        vc.convert_audio(torch.zeros(1, 24000), [24000], [80], spk, ssl=hub, sample_rate=22050.5)
    with pytest.raises(ValueError):  # 598 samples at 24 kHz are 399 at 16 kHz: below the content encoder's receptive field
        vc.convert_audio(torch.zeros(1, 598), [598], [3], spk, ssl=hub, sample_rate=24000)
