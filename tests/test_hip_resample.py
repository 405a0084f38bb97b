"""GPU: the windowed-sinc resampler (csrc/resample.hip.h; HipModel.resample, modules.Resample) against tests/resample64.py, the float64 restatement
that tests/test_resample_cpu.py pins to the fixtures' float64 runs.  The bar, for every output sample:

    |got - want64| <= 2^-24 |want64| + 1e-10 max|x|

The first term is the one rounding to fp32.  The second is the fp64 table's and sum's own error: at most ~1200 taps at a few ulp of fp64 each, about
1e-12 of the input scale, with a hundredfold margin.  The fp32 run's own error (torchaudio's arithmetic, from the fixtures) is printed beside it with
``-s``; it is not the bar.  Then the bit identities (ragged = solo, run to run, placement in the packed buffer, equal rates) and the wiring into
AdaptiveHubert, RmvpePitchExtractor and VoiceConverter.convert_audio, each against the reference's fixture at the standing bar of its own tests (4 x
the reference fp32 run's own error against float64) and against the composed steps bit for bit."""
import copy

import numpy as np
import pytest

import resample64 as R64
from conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BAR = 4.0
NARROW_SSL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7, num_conv_pos_embeddings=32,
                  num_conv_pos_embedding_groups=4)
NARROW_RMVPE = dict(n_blocks=1, inter_layers=1, en_out_channels=8)
NARROW_HUBERT = {"hidden_dim": 128, "sr": 16000, "arch": {"hidden_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2, "intermediate_size": 256,
                                                          "conv_dim": [64] * 7, "num_conv_pos_embeddings": 32, "num_conv_pos_embedding_groups": 4}}


@pytest.fixture(scope="module")
def eng(cfg):
    from stylish_tts_amd.runtime import HipModel

    e = HipModel(cfg, 0, precision="f32")  # the resampler needs no weights
    yield e
    e.close()


def _kw(case):
    orig, new, lpw, rolloff, method, beta = R64.CASES[case]
    return (orig, new), dict(lowpass_filter_width=lpw, rolloff=rolloff, resampling_method=method, beta=beta)


def _run(eng, waves, case):
    from stylish_tts_amd.runtime import Segments

    rates, kw = _kw(case)
    flat = torch.from_numpy(np.concatenate(waves)).to(eng.device)
    out, seg = eng.resample(Segments([w.size for w in waves], eng.device), flat, *rates, **kw)
    return out, seg


def _want(w, case):
    orig, new, lpw, rolloff, method, beta = R64.CASES[case]
    return R64.resample(w, orig, new, lpw, rolloff, method, beta)


def _within_bound(name, got, want, x):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    bound = 2.0**-24 * np.abs(want) + 1e-10 * np.abs(x).max()
    worst = float((err / bound).max())
    assert (err <= bound).all(), (name, worst, float(err.max()))
    return float(err.max()), worst


@pytest.mark.parametrize("case", sorted(R64.CASES))
def test_accuracy_against_float64(eng, case):
    from stylish_tts_amd import resample

    orig, new = R64.CASES[case][:2]
    tile = resample.tile(orig, new)
    waves = R64.signals(case, tile)
    L = [w.size for w in waves]
    o, n = R64.reduced(orig, new)
    width = R64.geometry(*R64.CASES[case][:4])[2]
    M = [R64.out_length(s, orig, new) for s in L]
    # the lengths the issue names: 1, shorter than the width, around a multiple of o, a tile and one past it (the first count >= it when upsampling)
    assert L[0] == 1 and L[1] == 5 < width and [s % o for s in L[2:5]] == [(o - 1) % o, 0, 1 % o]
    assert M[5] >= tile and M[6] >= tile + 1 and (o < n or (M[5], M[6]) == (tile, tile + 1)) and M[7] > 4 * tile
    assert np.abs(waves[3]).max() < 2e-3 and not waves[-1][waves[-1].size // 2 :].any()
    out, seg = _run(eng, waves, case)
    assert seg.lengths == M and out.shape == (sum(M),) and out.dtype == torch.float32
    worst = [0.0, 0.0]
    for u, w in enumerate(waves):
        e, r = _within_bound(f"{case} u{u}", out[int(seg.host[u]) : int(seg.host[u + 1])], _want(w, case), w)
        worst = [max(worst[0], r), max(worst[1], e)]
    g = load_golden("resample_cases")
    print(f"  {case}: HIP vs f64 worst {worst[0]:.3f} of the bound (max-abs {worst[1]:.2e}); torchaudio's fp32 arithmetic vs f64 on the fixture: max {g[case + '_err'][0]:.2e} "
          f"rms {g[case + '_err'][1]:.2e}")


@pytest.mark.parametrize("case", ["r24_16_w128", "r441_160", "r441_160_w128", "r160_441", "kaiser"])
def test_the_fixtures_float64_runs(eng, case):
    """The same bound against the generator's own float64 run (restated torchaudio on F.conv1d), not through tests/resample64.py."""
    g = load_golden("resample_cases")
    L = list(g[case + "_lengths"])
    waves = np.split(g[case + "_wave"], np.cumsum(L)[:-1])
    out, seg = _run(eng, waves, case)
    ref = np.split(g[case + "_out64"], np.cumsum(seg.lengths)[:-1])
    mine = np.split(out.double().cpu().numpy(), np.cumsum(seg.lengths)[:-1])
    for u, w in enumerate(waves):
        assert (np.abs(mine[u] - ref[u]) <= 2.0**-24 * np.abs(ref[u]) + 1e-10 * np.abs(w).max()).all(), (case, u)
    e = np.abs(out.double().cpu().numpy() - g[case + "_out64"])
    print(f"  {case}: HIP vs f64 max {e.max():.2e} rms {np.sqrt((e * e).mean()):.2e}; fp32 run vs f64 max {g[case + '_err'][0]:.2e} rms {g[case + '_err'][1]:.2e}")


@pytest.mark.parametrize("case", ["r24_16_w6", "r24_16_w128", "r441_160", "r441_160_w128", "r160_441", "r16_24", "kaiser_b9"])
def test_bit_identities(eng, case):
    from stylish_tts_amd import resample
    from stylish_tts_amd.runtime import Segments

    orig, new = R64.CASES[case][:2]
    waves = R64.signals(case, resample.tile(orig, new))
    out, seg = _run(eng, waves, case)
    again, _ = _run(eng, waves, case)
    assert torch.equal(out, again)  # run to run
    solo = [_run(eng, [w], case)[0] for w in waves]
    for u in range(len(waves)):  # a ragged batch is its solo runs
        assert torch.equal(out[int(seg.host[u]) : int(seg.host[u + 1])], solo[u]), (case, u)
    # an utterance that starts mid-tile in the packed buffers (after 5 samples in, a few out) is itself first in the buffer
    for u in (6, 7):
        moved, seg_m = _run(eng, [waves[1], waves[u], waves[2]], case)
        assert 0 < seg_m.host[1] < resample.tile(orig, new) and torch.equal(moved[int(seg_m.host[1]) : int(seg_m.host[2])], solo[u]), (case, u)
    # equal rates: the input's bits, whatever the other arguments
    flat = torch.from_numpy(np.concatenate(waves)).to(eng.device)
    same, seg_s = eng.resample(Segments([w.size for w in waves], eng.device), flat, orig, orig, lowpass_filter_width=R64.CASES[case][2])
    assert seg_s.lengths == [w.size for w in waves] and torch.equal(same, flat) and same.data_ptr() != flat.data_ptr()


def test_module_forward_shapes_and_padding(eng):
    from stylish_tts_amd.modules import Resample

    rs = Resample(24000, 16000, engine=eng)
    x = torch.from_numpy(np.stack([R64.signal(f"mod.{i}", 301, 24000) for i in range(6)])).reshape(2, 3, 301)
    y = rs(x)
    assert y.shape == (2, 3, 201) and y.device == eng.device  # ceil(2 * 301 / 3)
    for i in range(2):
        for j in range(3):
            _within_bound(f"dense {i}{j}", y[i, j], R64.resample(x[i, j].numpy(), 24000, 16000), x[i, j].numpy())
    L = torch.tensor([[301, 7, 150], [1, 300, 299]])
    z = rs(x, L)
    assert z.shape == (2, 3, 201)
    for i in range(2):
        for j in range(3):
            n, m = int(L[i, j]), R64.out_length(int(L[i, j]), 24000, 16000)
            assert not bool(z[i, j, m:].any()) and torch.equal(z[i, j, :m], rs(x[i, j, :n]))  # alone, bit for bit; zeros past its length
    rows, seg = rs.packed(x.reshape(6, 301), L.reshape(-1))
    assert seg.lengths == [R64.out_length(int(v), 24000, 16000) for v in L.reshape(-1)] and torch.equal(rows[: seg.lengths[0]], z[0, 0])
    same = Resample(16000, 16000, engine=eng)(x)
    assert torch.equal(same.cpu(), x)
    # the library itself checks the output offsets: a status, not a fault
    import ctypes as C

    from stylish_tts_amd.runtime import Segments

    si, so = Segments([7], eng.device), Segments([4], eng.device)
    w, o = torch.zeros(7, device=eng.device), torch.zeros(4, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = eng.lib.stts_resample_forward(eng.ctx, None, 24000, 16000, 6, 0.99, 0, 0.0, 1, si.host_ptr, p(si.dev), so.host_ptr, p(so.dev), p(w), p(o))
    assert rc != 0 and b"the formula gives 5" in eng.lib.stts_last_error()


# ------------------------------------------------------------------------------------------------ composition
class _HostReads:
    """Counts the reads of DEVICE tensors by the host that go through torch while the block runs (.cpu / .item / .tolist / .numpy / bool() / int() /
    float() / .to(cpu)): what ``host_syncs_per_call == 0`` declares.  The library itself copies nothing back after a table's first use."""

    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__")

    def __enter__(self):
        self.seen = []
        for name in self.NAMES:
            setattr(torch.Tensor, name, self._wrap(name, getattr(torch.Tensor, name)))
        inner = torch.Tensor.to

        def to(t, *a, **k):
            out = inner(t, *a, **k)
            if t.is_cuda and not out.is_cuda:
                self.seen.append("to(cpu)")
            return out

        torch.Tensor.to = to
        return self.seen

    def _wrap(self, name, inner):
        def fn(t, *a, **k):
            if t.is_cuda:
                self.seen.append(name)
            return inner(t, *a, **k)

        return fn

    def __exit__(self, *exc):
        for name in self.NAMES + ("to",):
            delattr(torch.Tensor, name)  # the base class's own method shows through again


def _ratio(name, mine, f64, err):
    e = mine - f64
    mx, rms = np.abs(e).max(), np.sqrt((e * e).mean())
    print(f"  {name}: HIP vs f64 max {mx:.3e} rms {rms:.3e}; reference fp32 run vs f64 max {err[0]:.3e} rms {err[1]:.3e}; ratios {mx / err[0]:.3f} {rms / err[1]:.3f}")
    assert mx <= BAR * err[0] and rms <= BAR * err[1], (name, mx, rms, tuple(err))


def test_adaptive_hubert_from_the_models_rate(eng):
    """The reference's AdaptiveHubert(model_sr=24000, hubert_sr=16000).forward: resample, then the network."""
    from stylish_tts_amd import modules

    g = load_golden("resample_ssl")
    m = modules.AdaptiveHubert(config=NARROW_SSL, model_sr=24000, hubert_sr=16000, engine=eng).load_synthetic(0)
    w = torch.from_numpy(g["wave"])
    rs = modules.Resample(m.model_sr, m.sr, engine=eng)
    w16 = rs(w)
    _within_bound("ssl resample", w16[0], g["res64"][0], g["wave"][0])
    want = m(w16, 40).clone()
    got = m(w, 40, sample_rate=m.model_sr)
    assert got.shape == (1, 128, 40) and torch.equal(got, want)
    assert torch.equal(m(w16, 40, sample_rate=16000), want) and torch.equal(m(w16, 40, sample_rate=None), want)
    _ratio("AdaptiveHubert(24 kHz)", got.double().cpu().numpy(), g["out64"], g["out_err"])
    # ragged: each utterance is its solo run, the lengths at the recording's rate
    w2 = torch.zeros(2, 12000)
    w2[0], w2[1, :9001] = w[0], w[0, 2000:11001]
    both = m.packed(w2, [40, 30], [12000, 9001], sample_rate=24000)
    assert torch.equal(both[:40, :128], got[0].t()) and torch.equal(both[40:, :128], m.packed(w2[1:, :9001], [30], sample_rate=24000)[:, :128])


def test_rmvpe_infer_from_audio_at_another_rate(eng):
    """The reference's RMVPE.infer_from_audio(audio, sample_rate=24000): its width-128 resampler, the log-mel, the network, the decoding."""
    from stylish_tts_amd import modules

    g = load_golden("resample_rmvpe")
    px = modules.RmvpePitchExtractor(config=NARROW_RMVPE, engine=eng).load_synthetic(0)
    w = torch.from_numpy(g["audio"])[None]
    rs = modules.Resample(24000, 16000, lowpass_filter_width=128, engine=eng)
    w16 = rs(w)
    _within_bound("rmvpe resample", w16[0], g["res64"][0], g["audio"])
    want = px.infer_from_audio(w16).clone()
    got = px.infer_from_audio(w, sample_rate=24000, resample=True)
    assert got.shape == (1, 51) and torch.equal(got, want)
    assert torch.equal(px.mel(w, sample_rate=24000, resample=True), px.mel(w16))
    hid = px.mel2hidden(px.mel(w, sample_rate=24000, resample=True))
    _ratio("RMVPE salience (24 kHz)", hid.double().cpu().numpy(), g["hidden64"], g["hidden_err"])
    f0, f64 = got[0].double().cpu().numpy(), g["f064"]
    v = f64 > 0
    assert np.array_equal(f0 > 0, v)
    rel = np.abs(f0[v] / f64[v] - 1).max()
    print(f"  RMVPE f0 (24 kHz): HIP max rel {rel:.3e}; reference fp32 run {g['f0_err'][0]:.3e}; ratio {rel / g['f0_err'][0]:.3f}")
    assert rel <= BAR * g["f0_err"][0]
    with pytest.raises(ValueError, match="16000"):  # without the keyword: the old refusal
        px.infer_from_audio(w, sample_rate=24000)
    # frames= and ragged lengths pass through
    fr = px.infer_from_audio(w, [12000], frames=[40], sample_rate=24000, resample=True)
    assert torch.equal(fr, px.infer_from_audio(w16, [8000], frames=[40]))


def test_convert_audio_from_one_recording_at_the_models_rate():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import DEFAULT_MODEL, load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    raw = copy.deepcopy(DEFAULT_MODEL)
    raw["hubert"] = copy.deepcopy(NARROW_HUBERT)
    cfg = load_model_config(raw)
    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, hubert=True, ssl=True, cfm_pitch=True)
    px = modules.RmvpePitchExtractor(config=NARROW_RMVPE, engine=eng).load_synthetic(0)
    ssl = mods["hubert"]
    vc = VoiceConverter(eng, [mods["hubert_speech_predictor"], mods["hubert_pitch_energy_predictor"], mods["cfm_pitch_predictor"], ssl])
    sr, hop = cfg.sample_rate, cfg.hop_length
    assert sr == 24000 and ssl.sr == 16000
    S, T = [40 * hop, 36 * hop + 7], [40, 36]  # the "even" frame counts of the log-mel front end at these lengths
    w = torch.zeros(2, S[0])
    for b, n in enumerate(S):
        w[b, :n] = torch.from_numpy(R64.signal(f"vc.{b}", n, sr))
    spk = torch.from_numpy(synth.normal("rsvc.spk", (2, vc.spk_dim)) * 0.5)
    R4 = 4 * sum(T)
    noise = dict(prior_noise=torch.from_numpy(synth.normal("rsvc.vpn", (R4, 128))).cuda(), src_noise=torch.from_numpy(synth.normal("rsvc.vsn", (R4 * eng.hop4,))).cuda(),
                 init_phase=torch.zeros(1).cuda())
    hid = px.mel2hidden(px.mel(w[:1], sample_rate=sr, resample=True))
    px.thred = float(hid.max(dim=-1)[0].median())  # voiced and unvoiced frames from the synthetic network
    # the composed steps: each consumer's own resampling of the ORIGINAL recording, then the existing calls
    S16 = [R64.out_length(n, sr, 16000) for n in S]
    w6 = modules.Resample(sr, 16000, engine=eng)(w, S)
    w128 = modules.Resample(sr, 16000, lowpass_filter_width=128, engine=eng)(w, S)
    assert not torch.equal(w6, w128)
    feats = ssl.packed(w6, T, S16).clone()
    f0 = px.packed_from_audio(w128, S16, T).clone()
    assert bool((f0 == 0).any()) and bool((f0 > 0).any())
    want, dw = vc.convert(None, T, spk, noise=noise, return_details=True, _packed_feats=feats, _packed_pitch=f0)
    got, dg = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px, sample_rate=sr)
    assert torch.equal(dg["pitch"], f0) and torch.equal(dg["pitch"], dw["pitch"]) and torch.equal(dg["energy"], dw["energy"])
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(bool(torch.isfinite(a).all()) for a in got)
    # with the tables built, the whole call - two resamplings, content encoder, pitch extractor, convert() - reads nothing back
    with _HostReads() as reads:
        vc.convert_audio(w, S, T, spk, noise=noise, pitch_extractor=px, sample_rate=sr)
        modules.Resample(sr, 16000, lowpass_filter_width=128, engine=eng).packed(w, S)
        during = list(reads)
        bool(torch.zeros(1, device=eng.device).sum() == 0)  # the counter does see a read
    assert during == [] and reads == ["__bool__"], (during, reads)
    # without a pitch extractor only the content encoder's resampling runs
    a = vc.convert_audio(w, S, T, spk, noise=noise, sample_rate=sr)
    b = vc.convert(None, T, spk, noise=noise, _packed_feats=feats)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the one-recording call: the same wave is the source, the reference speaker's recording and the energy's source
    stats, f0s = (-3.5, 3.9), (7.4, 0.45)
    one, d1 = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px, sample_rate=sr, ref_wave=w, ref_wave_lengths=S, energy_wave=w,
                               energy_wave_lengths=S, mel_stats=stats, f0_log2_stats=f0s)
    two, d2 = vc.convert(None, T, spk, noise=noise, return_details=True, _packed_feats=feats, _packed_uv=(f0 == 0).to(torch.float32), ref_wave=w, ref_wave_lengths=S,
                         energy_wave=w, energy_wave_lengths=S, mel_stats=stats, f0_log2_stats=f0s)
    assert torch.equal(d1["pitch"], d2["pitch"]) and torch.equal(d1["pitch"] == 0, f0 == 0) and all(torch.equal(x, y) for x, y in zip(one, two))
    assert all(bool(torch.isfinite(x).all()) for x in one)
    # audio already at 16 kHz with the keyword is the call without it
    c = vc.convert_audio(w6, S16, T, spk, noise=noise, pitch_extractor=px, sample_rate=16000)
    d = vc.convert_audio(w6, S16, T, spk, noise=noise, pitch_extractor=px)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    assert VoiceConverter.host_syncs_per_call == 0
    eng.close()
