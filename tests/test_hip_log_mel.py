"""GPU: the log-mel front end (csrc/log_mel.hip.h; HipModel.log_mel / log_mel_stats, modules.LogMelSpectrogram) against the fixtures of
tests/golden/gen_golden_logmel.py - the reference's calculate_mel / preprocess / log_norm / compute_log_mel_stats run in fp32 and in float64 on a
restated torchaudio MelSpectrogram.  The bar, for every output: max-abs and rms error against the float64 run at most 4x the fp32 run's own error
on the same input (the bar of the HuBERT, RMVPE and aligner ports).  Then what no fixture holds: ragged = solo and run-to-run bit equality, the
floor and the empty filters, a geometry without a fixture against tests/logmel64.py, the wiring into MelStyleEncoder / TextAligner / VoiceConverter,
and bit stability beside the split-fp32 frame path on another stream.

Measured on an MI355X (worst ratio of the HIP error to the fp32 run's own error over the four geometries; `pytest -m gpu tests/test_hip_log_mel.py -s`
prints every figure): see DESIGN.md section 5l."""
import copy

import numpy as np
import pytest

import logmel64 as L64
from conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NARROW_HUBERT = {"hidden_dim": 128, "sr": 16000, "arch": {"hidden_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2, "intermediate_size": 256,
                                                          "conv_dim": [64] * 7, "num_conv_pos_embeddings": 32, "num_conv_pos_embedding_groups": 4}}


@pytest.fixture(scope="module")
def eng(cfg):
    from stylish_tts_amd.runtime import HipModel

    e = HipModel(cfg, 0, precision="f32")  # the front end needs no weights
    yield e
    e.close()


def _run(eng, waves, geom, **kw):
    from stylish_tts_amd.runtime import Segments

    flat = torch.from_numpy(np.concatenate(waves)).to(eng.device)
    return eng.log_mel(Segments([w.size for w in waves], eng.device), flat, *geom, **kw)


def _within_bar(name, mine, ref64, err, factor=4.0):
    e = mine.double().cpu().numpy().reshape(ref64.shape) - ref64
    mx, rms = np.abs(e).max(), np.sqrt((e * e).mean())
    print(f"  {name}: HIP vs f64 max {mx:.3e} rms {rms:.3e}; fp32 run vs f64 max {err[0]:.3e} rms {err[1]:.3e}; ratios {mx / err[0]:.3f} {rms / err[1]:.3f}")
    assert mx <= factor * err[0] and rms <= factor * err[1], (name, mx, rms, tuple(err))


@pytest.mark.parametrize("case,own_mels", [("g2048", False), ("g2048", True), ("g512", False), ("g4096", False), ("g256", False)])
def test_parity_with_the_reference(eng, cfg, case, own_mels):
    g = load_golden("logmel_" + case)
    geom, (mean, std) = L64.CASES[case]
    if own_mels:
        geom = geom[:3] + (cfg.n_mels,) + geom[4:]
        assert geom == (cfg.n_fft, cfg.win_length, cfg.hop_length, cfg.n_mels, cfg.sample_rate) == L64.CASES[case][0]
    waves = L64.signals(case)
    n_mels = geom[3]
    rows, seg, en, raw = _run(eng, waves, geom, mean=mean, std=std, frames="even", energy=True, raw=True)
    assert rows.shape == (g["even64"].shape[0], n_mels) and seg.lengths == [L64.frames(w.size, geom[2], "even") for w in waves]
    _within_bar(f"{case} even", rows, g["even64"], g["even_err"])
    _within_bar(f"{case} energy", en, g["energy64"], g["energy_err"])
    # drop_last into rows wider than n_mels: the padding columns keep what they held
    T = sum(L64.frames(w.size, geom[2], "drop_last") for w in waves)
    out = torch.full((T, n_mels + 16), -7.0, device=eng.device)
    rows_d, seg_d = _run(eng, waves, geom, mean=mean, std=std, frames="drop_last", out=out)
    assert rows_d is out and bool((out[:, n_mels:] == -7.0).all()) and seg_d.lengths == [w.size // geom[2] for w in waves]
    _within_bar(f"{case} drop_last", out[:, :n_mels].contiguous(), g["drop64"], g["drop_err"])
    # all frames: the un-normalised log-mel (the optional output of the same launch)
    rows_a, seg_a, raw_a = _run(eng, waves, geom, mean=mean, std=std, frames="all", raw=True)
    assert seg_a.lengths == [w.size // geom[2] + 1 for w in waves]
    _within_bar(f"{case} raw", raw_a, g["raw64"], g["raw_err"])
    # the frames the policies share are the same frames
    o_e, o_a = 0, 0
    for u, w in enumerate(waves):
        ne, na = seg.lengths[u], seg_a.lengths[u]
        assert torch.equal(rows[o_e : o_e + ne], rows_a[o_a : o_a + ne]) and torch.equal(raw[o_e : o_e + ne], raw_a[o_a : o_a + ne])
        o_e, o_a = o_e + ne, o_a + na


def test_stats_against_the_reference(eng):
    from stylish_tts_amd.modules import LogMelSpectrogram

    for case in ("g2048", "g256"):
        g = load_golden("logmel_" + case)
        geom, _ = L64.CASES[case]
        front = LogMelSpectrogram(geom[3], *geom[:3], geom[4], engine=eng)
        waves = [torch.from_numpy(w) for w in L64.signals(case)]
        m, s, n = front.stats(waves)
        m64, s64, n64 = g["stats64"]
        print(f"  {case} stats: HIP vs f64 mean {abs(m - m64):.3e} std {abs(s - s64):.3e}; fp32 run vs f64 {g['stats_err'][0]:.3e} {g['stats_err'][1]:.3e}")
        assert n == int(n64) and abs(m - m64) <= 4.0 * g["stats_err"][0] and abs(s - s64) <= 4.0 * g["stats_err"][1]
        assert front.stats(waves) == (m, s, n)  # bit-identical from run to run


def test_ragged_equals_solo_and_repeats_bit_for_bit(eng):
    from stylish_tts_amd.runtime import Segments

    for case in ("g2048", "g256"):
        geom, (mean, std) = L64.CASES[case]
        waves = L64.signals(case)
        rows, seg, en, raw = _run(eng, waves, geom, mean=mean, std=std, frames="all", energy=True, raw=True)
        again = _run(eng, waves, geom, mean=mean, std=std, frames="all", energy=True, raw=True)
        assert torch.equal(rows, again[0]) and torch.equal(en, again[2]) and torch.equal(raw, again[3])
        flat = torch.from_numpy(np.concatenate(waves)).to(eng.device)
        st = eng.log_mel_stats(Segments([w.size for w in waves], eng.device), flat, *geom, return_partials=True)
        for u, w in enumerate(waves):
            r1, s1, e1, w1 = _run(eng, [w], geom, mean=mean, std=std, frames="all", energy=True, raw=True)
            sl = slice(int(seg.host[u]), int(seg.host[u + 1]))
            assert torch.equal(rows[sl], r1) and torch.equal(en[sl], e1) and torch.equal(raw[sl], w1), (case, u)
            p1 = eng.log_mel_stats(Segments([w.size], eng.device), torch.from_numpy(w).to(eng.device), *geom, return_partials=True)[3]
            assert torch.equal(st[3][sl], p1), (case, u)
        # the partials are the float64 sums of the raw log-mel over the mel axis: the fp32 rounding of the filter weights moves each of the n_mels
        # logarithms by at most 2^-24, so a sum by n_mels 2^-24 and a sum of squares by 2 * 11.6 times that (|log| <= 11.6 here)
        p64 = np.concatenate([L64.partials(w, geom) for w in waves])
        assert np.abs(st[3].cpu().numpy() - p64).max() <= geom[3] * 2.0**-24 * 24.0


def test_floor_and_empty_filters(eng):
    from stylish_tts_amd import log_mel

    geom, (mean, std) = L64.CASES["g256"]
    n_mels = geom[3]
    const = (np.log(1e-5) - mean) / std
    ulp = float(np.spacing(np.float32(abs(const))))
    zero = [np.zeros(1000, np.float32)]
    rows, _, en, raw = _run(eng, zero, geom, mean=mean, std=std, frames="all", energy=True, raw=True)
    assert np.abs(rows.double().cpu().numpy() - const).max() <= 2 * ulp
    assert np.abs(raw.double().cpu().numpy() - np.log(1e-5)).max() <= 2 * float(np.spacing(np.float32(11.5)))
    g = load_golden("logmel_g256")
    assert np.abs(en.double().cpu().numpy() - n_mels * 1e-5**0.33).max() <= 4.0 * g["energy_err"][0]
    # an empty filter sums nothing: the same constant under any input
    w, _ = log_mel.filter_table(geom[0], n_mels, geom[4])
    empty = np.nonzero((w > 0).sum(axis=1) == 0)[0]
    assert empty.size == 5
    rows, _ = _run(eng, L64.signals("g256"), geom, mean=mean, std=std, frames="all")
    r = rows.cpu().numpy()
    assert (r[:, empty] == np.float32(const)).all() and (r[:, [m for m in range(n_mels) if m not in empty]] != np.float32(const)).any()


def test_a_geometry_without_a_fixture_against_logmel64(eng):
    """win < n_fft, an odd hop, a mel count that is no multiple of 64, 22.05 kHz.  No fp32 reference run exists for it, so the bound is that of the
    number formats: the kernel computes in fp64 and rounds once (2^-24 relative), and its filter weights are float64 weights rounded to fp32, which
    moves a mel by at most 2^-24 relative and its logarithm by at most 2^-24 absolute; 2^-23 leaves a factor two for the fp64 arithmetic in between."""
    geom, mean, std = (1024, 1000, 171, 57, 22050), -4.0, 4.0
    waves = [L64.signal(f"nofix.{i}", n, geom[4]) for i, n in enumerate([513, 171 * 30, 171 * 21 + 5])]
    waves[1][waves[1].size // 2 :] = 0.0
    rows, seg, en, raw = _run(eng, waves, geom, mean=mean, std=std, frames="all", energy=True, raw=True)
    ref = np.concatenate([L64.raw_log_mel(w, geom) for w in waves])
    assert raw.shape == ref.shape
    assert (np.abs(raw.double().cpu().numpy() - ref) <= 2.0**-24 * np.abs(ref) + 2.0**-23).all()
    refn = (ref - mean) / std
    assert (np.abs(rows.double().cpu().numpy() - refn) <= 2.0**-24 * np.abs(refn) + 2.0**-23 / std).all()
    refe = np.concatenate([L64.energy(w, geom, mean, std, "all") for w in waves])
    assert (np.abs(en.double().cpu().numpy() - refe) <= 2.0**-23 * np.abs(refe)).all()  # 0.33 * 2^-24 per term from the weights, 2^-24 from the rounding


def test_refusals(eng):
    from stylish_tts_amd.runtime import Segments

    geom = L64.CASES["g2048"][0]
    with pytest.raises(ValueError, match="reflect padding"):
        _run(eng, [np.zeros(1024, np.float32)], geom)
    with pytest.raises(ValueError, match="ld 64 < n_mels 80"):
        _run(eng, [np.zeros(3000, np.float32)], geom, ld=64)
    # the library itself refuses the same (a caller of the C ABI gets a status, not a fault)
    lib, C = eng.lib, __import__("ctypes")
    s, r = Segments([1024], eng.device), Segments([4], eng.device)
    wave, out = torch.zeros(1024, device=eng.device), torch.zeros(4, 80, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.stts_log_mel_forward(eng.ctx, None, 1, s.host_ptr, p(s.dev), r.host_ptr, p(r.dev), p(wave), 2048, 1200, 300, 80, 24000, -4.0, 4.0, p(out), 80, None, None)
    assert rc != 0 and b"reflect padding" in lib.stts_last_error()
    s = Segments([3000], eng.device)
    r = Segments([12], eng.device)  # 3000 // 300 + 1 = 11 frames at the most
    wave = torch.zeros(3000, device=eng.device)
    rc = lib.stts_log_mel_forward(eng.ctx, None, 1, s.host_ptr, p(s.dev), r.host_ptr, p(r.dev), p(wave), 2048, 1200, 300, 80, 24000, -4.0, 4.0, p(out), 80, None, None)
    assert rc != 0 and b"12 frames" in lib.stts_last_error()


# ------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def vc_setup():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import DEFAULT_MODEL, load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    raw = copy.deepcopy(DEFAULT_MODEL)
    raw["hubert"] = copy.deepcopy(NARROW_HUBERT)
    cfg = load_model_config(raw)
    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, hubert=True, cfm_pitch=True, mel_style=True, aligner=True)
    vc = VoiceConverter(eng, [mods["hubert_speech_predictor"], mods["hubert_pitch_energy_predictor"], mods["cfm_pitch_predictor"]])
    hop = cfg.hop_length
    S = [40 * hop, 40 * hop + 7]  # 2 utterances of 40 frames under "even" (41 rounded down) and under "drop_last"
    w = torch.zeros(2, S[1])
    for b, n in enumerate(S):
        w[b, :n] = torch.from_numpy(L64.signal(f"wiring.{b}", n, cfg.sample_rate))
    yield cfg, eng, mods, vc, w, S, synth
    eng.close()


def test_mel_style_from_audio_is_forward_on_the_front_ends_mel(vc_setup):
    from stylish_tts_amd.modules import LogMelSpectrogram

    cfg, eng, mods, vc, w, S, synth = vc_setup
    enc = mods["pe_mel_style_encoder"]
    stats = (-3.5, 3.9)
    front = LogMelSpectrogram.from_config(cfg, mean=stats[0], std=stats[1], engine=eng)
    mel, mel_len = front(w, S)
    assert mel.shape == (2, cfg.n_mels, 40) and mel_len.tolist() == [40, 40]
    want = enc(mel[:, None], mel_len).clone()
    got = enc.from_audio(w, S, stats)
    assert got.shape == (2, cfg.style_dim) and torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_align_audio_is_align_on_the_drop_last_mel(vc_setup):
    from stylish_tts_amd.modules import LogMelSpectrogram

    cfg, eng, mods, vc, w, S, synth = vc_setup
    al = mods["text_aligner"]
    stats = (-4.0, 4.0)
    front = LogMelSpectrogram.from_config(cfg, al.n_mels, mean=stats[0], std=stats[1], frames="drop_last", engine=eng)
    mel, mel_len = front(w, S)
    assert mel_len.tolist() == [40, 40]
    PL = [9, 12]
    text = torch.zeros(2, 12, dtype=torch.int64)
    for b, p in enumerate(PL):
        text[b, :p] = torch.from_numpy(np.clip((synth.uniform(f"wiring.tok.{b}", (p,)) * al.num_symbols).astype(np.int64), 0, al.num_symbols - 1))
    want = al.align(mel.transpose(1, 2).contiguous(), mel_len, text, PL)
    want = [[t.clone() for t in part] for part in want]
    got = al.align_audio(w, S, text, PL, mel_stats=stats)
    for a, b in zip(want, got):
        assert len(a) == len(b) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(s[0].sum()) == 40 for s in got[0])


def test_convert_with_ref_wave_and_energy_wave(vc_setup):
    from stylish_tts_amd.modules import LogMelSpectrogram
    from stylish_tts_amd.pipeline import VoiceConverter

    cfg, eng, mods, vc, w, S, synth = vc_setup
    T = [40, 40]
    feats = torch.from_numpy(synth.normal("wiring.feats", (2, vc.hubert_dim, 40)).astype(np.float32))
    spk = torch.from_numpy(synth.normal("wiring.spk", (2, vc.spk_dim)) * 0.5)
    R4 = 4 * sum(T)
    noise = dict(prior_noise=torch.from_numpy(synth.normal("wiring.vpn", (R4, 128))).cuda(), src_noise=torch.from_numpy(synth.normal("wiring.vsn", (R4 * eng.hop4,))).cuda(),
                 init_phase=torch.zeros(1).cuda())
    stats, f0s = (-3.5, 3.9), (7.4, 0.45)
    front = LogMelSpectrogram.from_config(cfg, mean=stats[0], std=stats[1], engine=eng)
    mel, mel_len = front(w, S)
    a, da = vc.convert(feats, T, spk, noise=noise, return_details=True, ref_mel=mel, ref_mel_lengths=mel_len, f0_log2_stats=f0s)
    b, db = vc.convert(feats, T, spk, noise=noise, return_details=True, ref_wave=w, ref_wave_lengths=S, mel_stats=stats, f0_log2_stats=f0s)
    assert torch.equal(da["pitch"], db["pitch"]) and torch.equal(da["energy"], db["energy"]) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x).all()) for x in b)
    en = front.energy(w, S)
    assert en.shape == (2, 40) and bool((en > 0).all())
    pitch = torch.from_numpy(synth.pitch_curve("wiring.f0", 2, 40))
    c, dc = vc.convert(feats, T, spk, noise=noise, return_details=True, pitch=pitch, energy=en)
    d, dd = vc.convert(feats, T, spk, noise=noise, return_details=True, pitch=pitch, energy_wave=w, energy_wave_lengths=S, mel_stats=stats)
    assert torch.equal(dc["energy"], dd["energy"]) and torch.equal(dc["energy"], torch.cat([en[0], en[1]])) and all(torch.equal(x, y) for x, y in zip(c, d))
    with pytest.raises(ValueError, match="mel frames, lengths are"):
        vc.convert(feats, [40, 38], spk, pitch=pitch, energy_wave=w, energy_wave_lengths=S)
    assert VoiceConverter.host_syncs_per_call == 0


# ------------------------------------------------------------------------------------------------ beside other streams
def test_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    geom, (mean, std) = L64.CASES["g2048"]
    waves = L64.signals("g2048")
    flat = dev(np.concatenate(waves))
    seg_s = Segments([w.size for w in waves], devid)
    L = [240] * 4
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("lmc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("lmc.f0", (R,))) * 60 + 120), energy=dev(synth.normal("lmc.en", (R,))),
              style=dev(synth.normal("lmc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("lmc.pn", (R, 128))), sn=dev(synth.normal("lmc.sn", (R * 75,))),
              ph=dev(synth.uniform("lmc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    def run():
        rows, _, en, raw = eng.log_mel(seg_s, flat, *geom, mean=mean, std=std, frames="all", energy=True, raw=True)
        return rows, en, raw

    solo = [t.clone() for t in run()]
    torch.cuda.synchronize()
    g = load_golden("logmel_g2048")
    _within_bar("g2048 raw (solo)", solo[2], g["raw64"], g["raw_err"])
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(4):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def mels():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [run() for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    with ThreadPoolExecutor(2) as ex:
        f = ex.submit(frames)
        got = ex.submit(mels).result()
        f.result()
    for j, out in enumerate(got):
        assert all(torch.equal(x, y) for x, y in zip(out, solo)), j
    eng.close()
