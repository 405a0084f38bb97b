"""No GPU: the host side of the log-mel front end - the library's mel filter table against tests/logmel64.py's, the structure of the table, the
three frame-count policies, tests/logmel64.py against the float64 arrays of the fixtures (tests/golden/gen_golden_logmel.py: the reference's
calculate_mel / preprocess / log_norm / compute_log_mel_stats run in float64), and the ValueError paths that need no device."""
import types

import numpy as np
import pytest

import logmel64 as L64
from conftest import load_golden

GEOMS = [(256, 80, 24000), (2048, 80, 24000), (512, 48, 16000), (4096, 128, 48000), (1024, 256, 44100), (256, 1, 8000)]


@pytest.mark.parametrize("n_fft,n_mels,sr", GEOMS)
def test_filter_table_is_logmel64s_rounded_to_fp32(n_fft, n_mels, sr):
    from stylish_tts_amd import log_mel

    w, band = log_mel.filter_table(n_fft, n_mels, sr)
    ref = L64.filters(n_fft, n_mels, sr)
    assert w.shape == ref.shape == (n_mels, n_fft // 2 + 1) and w.dtype == np.float32 and band.shape == (n_mels, 2)
    # float64 rounded once: half an ulp of fp32 at each weight (two float64 builds may differ in their last bits, hence not ==)
    assert (np.abs(w.astype(np.float64) - ref) <= np.maximum(np.abs(ref) * 2.0**-24, 1e-30) * 1.001).all()
    assert w.min() >= 0.0 and w.max() <= 1.0
    for m in range(n_mels):
        nz = np.nonzero(w[m])[0]
        if nz.size == 0:
            assert band[m, 0] == band[m, 1]
        else:  # the band is the filter's nonzero bins, with no hole in it
            assert (band[m, 0], band[m, 1]) == (nz[0], nz[-1] + 1) and nz.size == nz[-1] + 1 - nz[0]
    assert (w > 0).sum(axis=0).max() <= 2  # a bin lies in at most two filters


def test_filter_table_structure_at_the_edge_geometries():
    from stylish_tts_amd import log_mel

    w, _ = log_mel.filter_table(256, 80, 24000)
    per = (w > 0).sum(axis=1)
    assert (per == 0).sum() == 5 and (per == 1).sum() == 23
    w, _ = log_mel.filter_table(2048, 80, 24000)
    assert ((w > 0).sum(axis=1) >= 2).all()


def test_filter_table_refuses_bad_arguments():
    from stylish_tts_amd import log_mel

    for bad in [(1000, 80, 24000), (128, 80, 24000), (8192, 80, 24000), (2048, 0, 24000), (2048, 257, 24000), (2048, 80, 0)]:
        with pytest.raises(ValueError):
            log_mel.filter_table(*bad)


@pytest.mark.parametrize("hop", [1, 64, 300])
def test_frame_policies(hop):
    from stylish_tts_amd import log_mel

    for L in [5 * hop, 6 * hop, 5 * hop + hop // 2 + 1, 6 * hop + hop - 1 if hop > 1 else 7]:
        n = L // hop + 1
        assert log_mel.frames(L, hop, "even") == n - n % 2 == L64.frames(L, hop, "even")
        assert log_mel.frames(L, hop, "drop_last") == L // hop == L64.frames(L, hop, "drop_last")
        assert log_mel.frames(L, hop, "all") == n == L64.frames(L, hop, "all")
    assert log_mel.frames(5 * hop, hop, "even") == 6 and log_mel.frames(6 * hop, hop, "even") == 6
    with pytest.raises(ValueError, match="one of"):
        log_mel.frames(1000, hop, "odd")


@pytest.mark.parametrize("case", sorted(L64.CASES))
def test_logmel64_reproduces_the_float64_reference_run(case):
    g = load_golden("logmel_" + case)
    geom, (mean, std) = L64.CASES[case]
    assert tuple(g["geom"]) == geom and tuple(g["norm"]) == (mean, std)
    waves = L64.signals(case)
    assert [w.size for w in waves] == list(g["lengths"]) == L64.lengths(geom) and (np.concatenate(waves) == g["wave"]).all()
    n_fft, _, hop, _, _ = geom
    assert waves[0].size == n_fft // 2 + 1 and waves[1].size % hop == 0 and waves[2].size % hop != 0
    assert (waves[1][waves[1].size // 2 :] == 0).all() and np.abs(waves[0]).max() < 2e-3
    outs = dict(even=lambda w: L64.log_mel(w, geom, mean, std, "even"), drop=lambda w: L64.log_mel(w, geom, mean, std, "drop_last"),
                raw=lambda w: L64.raw_log_mel(w, geom), energy=lambda w: L64.energy(w, geom, mean, std))
    for k, fn in outs.items():
        mine, ref = np.concatenate([fn(w) for w in waves]), g[k + "64"]
        assert mine.shape == ref.shape and ref.dtype == np.float64
        assert np.abs(mine - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), k
        # the fixture's own error figures are those of its two runs
        e = g[k + "32"].astype(np.float64) - ref
        assert np.allclose(g[k + "_err"], [np.abs(e).max(), np.sqrt((e * e).mean())], rtol=1e-12) and g[k + "_err"][0] > 0
    m, s, n = L64.stats(waves, geom)
    assert n == int(g["stats64"][2]) == sum(L64.frames(w.size, hop, "all") for w in waves) * geom[3]
    assert abs(m - g["stats64"][0]) <= 1e-12 * abs(m) and abs(s - g["stats64"][1]) <= 1e-12 * s
    # the floor is reached (the silent half) and the range is wide
    assert g["raw64"].min() == pytest.approx(np.log(1e-5), abs=1e-9) and g["raw64"].max() > 5.0
    p = np.concatenate([L64.partials(w, geom) for w in waves]).sum(axis=0)
    assert abs(p[0] / n - m) <= 1e-12 * abs(m)


def test_too_short_an_utterance_is_a_value_error(cfg):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import log_mel
    from stylish_tts_amd.modules import LogMelSpectrogram

    assert log_mel.frame_counts([1025, 4000], 2048, 300, "all") == [4, 14]
    with pytest.raises(ValueError, match="reflect padding needs more than n_fft / 2 = 1024"):
        log_mel.frame_counts([4000, 1024], 2048, 300, "even")
    with pytest.raises(ValueError, match="leave no frame"):
        log_mel.frame_counts([200], 256, 300, "drop_last")
    front = LogMelSpectrogram(80, 2048, 1200, 300, 24000)
    for fn in (front.forward, front.packed, front.energy):  # refused on the host, before an engine is asked for
        with pytest.raises(ValueError, match="reflect padding"):
            fn(torch.zeros(2, 3000), [3000, 1024])
    with pytest.raises(ValueError, match="reflect padding"):
        front.stats([torch.zeros(3000), torch.zeros(700)])
    with pytest.raises(ValueError, match="do not fit"):
        front.forward(torch.zeros(2, 3000), [3000, 3001])
    for bad in [dict(n_fft=1000), dict(win_length=4096), dict(hop_length=0), dict(n_mels=300), dict(frames="odd")]:
        with pytest.raises(ValueError):
            LogMelSpectrogram(**{**dict(n_mels=80, n_fft=2048, win_length=1200, hop_length=300, sample_rate=24000), **bad})
    cfg_front = LogMelSpectrogram.from_config(cfg, 80, frames="drop_last")
    assert (cfg_front.n_fft, cfg_front.win_length, cfg_front.hop_length, cfg_front.sample_rate, cfg_front.frames) == (2048, 1200, 300, 24000, "drop_last")


def test_voice_converter_refuses_contradictory_audio_keywords(cfg):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd.config import hubert_dims
    from stylish_tts_amd.pipeline import VoiceConverter

    hd, sd = hubert_dims(cfg)
    vc = VoiceConverter(types.SimpleNamespace(cfg=cfg, device=torch.device("cpu")))
    feats, spk, T = torch.zeros(2, hd, 40), torch.zeros(2, sd), [40, 38]
    hop = cfg.hop_length
    with pytest.raises(ValueError, match="ref_mel or ref_wave"):
        vc.convert(feats, T, spk, ref_mel=torch.zeros(2, cfg.n_mels, 40), ref_wave=torch.zeros(2, 12000), f0_log2_stats=(7.4, 0.45))
    with pytest.raises(ValueError, match="energy or energy_wave"):
        vc.convert(feats, T, spk, pitch=torch.zeros(2, 40), energy=torch.zeros(2, 40), energy_wave=torch.zeros(2, 40 * hop))
    # 40 * hop samples give 40 frames ("even": 41 rounded down), 38 * hop give 38; one hop more on the second gives 40: a mismatch
    with pytest.raises(ValueError, match=r"energy_wave gives \[40, 40\] mel frames, lengths are \[40, 38\]"):
        vc.convert(feats, T, spk, pitch=torch.zeros(2, 40), energy_wave=torch.zeros(2, 40 * hop), energy_wave_lengths=[40 * hop, 39 * hop])
    with pytest.raises(ValueError, match="reflect padding"):
        vc.convert(feats, T, spk, ref_wave=torch.zeros(2, 12000), ref_wave_lengths=[12000, 900], f0_log2_stats=(7.4, 0.45))
    with pytest.raises(ValueError, match="f0_log2_stats"):
        vc.convert(feats, T, spk, ref_wave=torch.zeros(2, 12000))
