"""The voice-conversion models (HubertPitchEnergyPredictor, HubertSpeechPredictor, VoiceConverter) on the GPU library against the
reference fixtures of tests/golden/gen_golden_hubert.py.  Inputs are regenerated from their names (``inputs``, the generator's recipe)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def inputs(name, T, hubert_dim=768, spk_dim=10240, h=75):
    from stylish_tts_amd import synth

    tag = "hb." + name
    return dict(feats=synth.normal(tag + ".feats", (1, hubert_dim, T)), spk=synth.normal(tag + ".spk", (1, spk_dim)),
                pitch=synth.pitch_curve(tag + ".pitch", 1, T), energy=(synth.uniform(tag + ".energy", (1, T)) * 2.0 + 2.0).astype(F32),
                nz=synth.path_noise(name, 1, 4 * T, hop4=h))


def make_engine(precision="f32"):
    """An engine with both HuBERT models bound through their shims (synthetic weights, seed 0, as the fixtures)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.runtime import HipModel

    cfg = load_model_config()
    eng = HipModel(cfg, 0, precision=precision)
    m = modules.build_inference_modules(cfg, engine=eng, hubert=True)
    sp, pe = m["hubert_speech_predictor"].load_synthetic(0), m["hubert_pitch_energy_predictor"].load_synthetic(0)
    _, _ = sp.engine, pe.engine  # bind (finalize) both
    return eng, sp, pe


@pytest.fixture(scope="module")
def hub():
    eng, sp, pe = make_engine()
    yield eng, sp, pe
    eng.close()


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def front(eng, ins, T):
    from stylish_tts_amd.runtime import Segments

    s = Segments([T], eng.device)
    feats = eng.to_time_major(dev(ins["feats"]))
    style, pe_style = eng.speaker_style(dev(ins["spk"]))
    return s, feats, style, pe_style


# ------------------------------------------------------------------------------------------------ 1. pitch / energy vs reference
@pytest.mark.parametrize("T", [60, 272])
def test_pitch_energy_matches_reference(hub, T):
    eng = hub[0]
    g = load_golden("hubert_pe")
    s, feats, _, pe_style = front(eng, inputs(f"pe{T}", T), T)
    f0, en, pros = eng.hubert_pitch_energy(s, feats, pe_style, taps=True)
    eng.check_status()
    kr = g[f"keep_rows_{T}"]
    errs = dict(F0=rel(f0.cpu().numpy(), g[f"F0_{T}"][0]), N=rel(en.cpu().numpy(), g[f"N_{T}"][0]), style=rel(pe_style.cpu().numpy(), g[f"style_{T}"]),
                prosody=rel(pros.cpu().numpy()[kr], g[f"prosody_rows_{T}"]))
    print(f"\n[hubert_pe T={T}]", {k: f"{v:.1e}" for k, v in errs.items()})
    assert errs["F0"] < 2e-4 and errs["style"] < 2e-4 and errs["prosody"] < 2e-4 and errs["N"] < 5e-4, errs


# ------------------------------------------------------------------------------------------------ 2. encoder at > 1024 positions
def test_encoder_long_matches_reference(hub):
    """4T = 1088 positions: RoPE past position 1023 and the matrix-core attention past 1024 keys (heads of 16)."""
    eng = hub[0]
    g = load_golden("hubert_sp_long")
    T = int(g["T"])
    s, feats, style, _ = front(eng, inputs("hubert_sp_long", T), T)
    asr = eng.hubert_encoder(s, feats)
    assert asr.shape == (4 * T, 128)
    kr = g["keep_rows"]
    assert kr.max() == 4 * T - 1
    e = rel(asr.cpu().numpy()[kr], g["enc_rows"])
    print(f"\n[encoder 4T={4 * T}] {e:.1e}")
    assert e < 2e-4
    assert rel(style.cpu().numpy(), g["style"]) < 2e-4


# ------------------------------------------------------------------------------------------------ 3. speech predictor vs reference
def staged(eng, s, asr, style, pitch, energy, nz, hint=None):
    """decoder -> prior / flow -> source -> STFT -> vocoder at 4T rows, optionally adopting the reference's branch ties (test_hip_geometry)."""
    from oracle import stylish_oracle as O
    from stylish_tts_amd.runtime import Segments

    s4 = s.scaled(4)
    T4, bins = s4.rows, eng.n_bins
    p4, e4 = eng.upsample4(s, s4, pitch), eng.upsample4(s, s4, energy)
    x = eng.decoder(s4, asr, p4, e4, style)
    mel, zp, _ = eng.prior_flow(s4, x, style, dev(nz["prior_noise"][0].T), return_z=True)
    spec, phase = eng.harmonic_stft(s4, p4, dev(nz["src_noise"].reshape(-1)), dev(nz["init_phase"].reshape(-1)))
    raw = eng.vocoder(s4, mel, style, spec, phase)
    if hint is not None:
        sp, ph = spec.cpu().numpy()[:, :bins].T[None], phase.cpu().numpy()[:, :bins].T[None]
        ph, bad = O.align_branch(ph, hint, sp, return_bad=True)
        assert bad == 0
        phz = np.zeros((T4, eng.har_ld), F32)
        phz[:, :bins] = ph[0].T
        phase = dev(phz)
    audio = eng.vocoder(s4, mel, style, spec, phase)
    eng.check_status()
    assert isinstance(s4, Segments)
    return dict(x=x, z=zp, mel=mel, audio=audio, raw=raw)


@pytest.mark.parametrize("name", ["hubert_sp_short", "hubert_sp_long"])
def test_speech_predictor_matches_reference(hub, name):
    eng = hub[0]
    g = load_golden(name)
    T = int(g["T"])
    ins = inputs(name, T)
    s, feats, style, _ = front(eng, ins, T)
    asr = eng.hubert_encoder(s, feats)
    out = staged(eng, s, asr, style, dev(ins["pitch"][0]), dev(ins["energy"][0]), ins["nz"], (g["cut_idx"].astype(np.int64), g["cut_phase"].astype(F32)))
    kr = g["keep_rows"]
    errs = dict(enc=rel(asr.cpu().numpy()[kr], g["enc_rows"]), style=rel(style.cpu().numpy(), g["style"]))
    if "x_rows" in g:
        errs.update(x=rel(out["x"].cpu().numpy()[kr], g["x_rows"]), z=rel(out["z"].cpu().numpy()[kr], g["z_rows"]),
                    mel=rel(out["mel"].cpu().numpy()[kr], g["mel_rows"]))
    errs["audio"] = float(np.abs(out["audio"].cpu().numpy() - g["audio"].reshape(-1)).max())
    print(f"\n[{name}]", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(v for k, v in errs.items() if k != "audio") < 2e-4 and errs["audio"] < 1e-3, errs


# ------------------------------------------------------------------------------------------------ 4. VoiceConverter
def test_voice_converter_matches_reference(hub):
    from stylish_tts_amd.pipeline import VoiceConverter

    eng, sp, pe = hub
    g = load_golden("hubert_convert")
    T = int(g["T"])
    ins = inputs("cv60", T)
    nz = ins["nz"]
    packed = dict(prior_noise=dev(nz["prior_noise"][0].T), src_noise=dev(nz["src_noise"].reshape(-1)), init_phase=dev(nz["init_phase"].reshape(-1)))
    vc = VoiceConverter(eng, modules=[sp, pe])
    waves, det = vc.convert(torch.from_numpy(ins["feats"]), [T], torch.from_numpy(ins["spk"]), noise=packed, return_details=True)
    assert len(waves) == 1 and waves[0].shape == (4 * T * eng.hop4,)
    ef0, en = rel(det["pitch"].cpu().numpy(), g["F0"][0]), rel(det["energy"].cpu().numpy(), g["N"][0])
    assert ef0 < 2e-4 and en < 5e-4, (ef0, en)
    # shim by shim: the same stages one call each give the fused frame path's waveform bit for bit (branch ties as they fall)
    s, feats, style, _ = front(eng, ins, T)
    asr = eng.hubert_encoder(s, feats)
    hint = (g["cut_idx"].astype(np.int64), g["cut_phase"].astype(F32))
    out = staged(eng, s, asr, style, det["pitch"], det["energy"], nz, hint)
    assert torch.equal(waves[0], out["raw"])
    # the waveform against the reference's is compared on the reference's F0 / N: the harmonic source integrates F0, so the 2e-6
    # relative difference of the predicted curves alone moves the waveform by ~1e-2 after 0.6 s (measured on MI355X)
    F0g, Ng = dev(g["F0"][0]), dev(g["N"][0])
    w2 = vc.convert(torch.from_numpy(ins["feats"]), [T], torch.from_numpy(ins["spk"]), pitch=F0g[None], energy=Ng[None], noise=packed)
    out2 = staged(eng, s, asr, style, F0g, Ng, nz, hint)
    assert torch.equal(w2[0], out2["raw"])
    ea = float(np.abs(out2["audio"].cpu().numpy() - g["audio"].reshape(-1)).max())
    print(f"\n[convert] F0 {ef0:.1e} N {en:.1e} audio {ea:.1e}")
    assert ea < 1e-3
    # the shims on the same inputs give the same curves and waveform
    F0, N = pe(torch.from_numpy(ins["feats"]), torch.tensor([T]), torch.from_numpy(ins["spk"]))
    assert torch.equal(F0.reshape(-1), det["pitch"]) and torch.equal(N.reshape(-1), det["energy"])
    pred = sp(torch.from_numpy(ins["feats"]), torch.tensor([T]), torch.from_numpy(ins["spk"]), F0, N, noise=nz)
    assert torch.equal(pred.audio.reshape(-1), waves[0])
    pcm = vc.convert_int16(torch.from_numpy(ins["feats"]), [T], torch.from_numpy(ins["spk"]), noise=packed)
    assert pcm[0].dtype == np.int16 and np.array_equal(pcm[0], np.multiply(waves[0].cpu().numpy(), 32768).astype(np.int16))


# ------------------------------------------------------------------------------------------------ 5. speaker-style kernel
def _mish64(x):
    return x * np.tanh(np.log1p(np.exp(x)))


def test_speaker_style_float64_and_batch_invariance(hub):
    from stylish_tts_amd import synth

    eng, sp, pe = hub
    W = {k: v.numpy().astype(np.float64) for k, v in sp.state_dict().items() if k.startswith("style_encoder.")}
    Wp = {k: v.numpy().astype(np.float64) for k, v in pe.state_dict().items() if k.startswith("style_encoder.")}
    X = synth.normal("hb.spk.batch", (64, 10240)).astype(F32)
    x64 = X.astype(np.float64)
    pe_ref = x64 @ Wp["style_encoder.weight"].T + Wp["style_encoder.bias"]
    pe_bound = 1e-6 * (np.abs(x64) @ np.abs(Wp["style_encoder.weight"]).T)
    h = _mish64(x64 @ W["style_encoder.0.weight"].T + W["style_encoder.0.bias"])
    h = _mish64(h @ W["style_encoder.3.weight"].T + W["style_encoder.3.bias"])
    sp_ref = h @ W["style_encoder.6.weight"].T + W["style_encoder.6.bias"]
    alone = [eng.speaker_style(dev(X[i : i + 1])) for i in range(64)]
    for n in (1, 3, 17, 64):
        s, p = eng.speaker_style(dev(X[:n]))
        s, p = s.cpu().numpy(), p.cpu().numpy()
        assert np.all(np.abs(p - pe_ref[:n]) <= pe_bound[:n]), n
        assert rel(s, sp_ref[:n]) < 1e-5, n
        for i in range(n):
            assert np.array_equal(s[i], alone[i][0].cpu().numpy()[0]) and np.array_equal(p[i], alone[i][1].cpu().numpy()[0]), (n, i)
    # null outputs are honoured: either style alone equals its row of the joint call
    s_only, none1 = eng.speaker_style(dev(X[:3]), pe_style=False)
    none2, p_only = eng.speaker_style(dev(X[:3]), style=False)
    s, p = eng.speaker_style(dev(X[:3]))
    assert none1 is None and none2 is None and torch.equal(s_only, s) and torch.equal(p_only, p)
    # Mish at large inputs is x, not NaN
    big = np.zeros((1, 10240), F32)
    big[0, :] = 1e4
    s, p = eng.speaker_style(dev(big))
    assert torch.isfinite(s).all() and torch.isfinite(p).all()


# ------------------------------------------------------------------------------------------------ 6. ragged batch
def test_ragged_batch_matches_single_calls(hub):
    """Three utterances of different T in one packed call vs three single calls.  Speaker styles: bit-identical (the kernel promises it).
    Encoder (matrix-core attention: the same kernel at any batch) and pitch / energy: the contractions may split K differently for a
    different total row count, so within 1e-6 of scale."""
    from stylish_tts_amd.runtime import Segments

    eng = hub[0]
    lens = [60, 37, 90]
    ins = [inputs(f"rag{i}", L) for i, L in enumerate(lens)]
    feats = torch.cat([eng.to_time_major(dev(x["feats"])) for x in ins])
    spk = dev(np.concatenate([x["spk"] for x in ins]))
    s = Segments(lens, eng.device)
    style, pe_style = eng.speaker_style(spk)
    asr = eng.hubert_encoder(s, feats)
    f0, en = eng.hubert_pitch_energy(s, feats, pe_style)
    eng.check_status()
    for i, L in enumerate(lens):
        s1, ft1, st1, ps1 = front(eng, ins[i], L)
        assert torch.equal(st1[0], style[i]) and torch.equal(ps1[0], pe_style[i])
        a1 = eng.hubert_encoder(s1, ft1)
        g1, n1 = eng.hubert_pitch_energy(s1, ft1, ps1)
        o, o4 = s.host[i], 4 * s.host[i]
        for what, got, want in (("asr", asr[o4 : o4 + 4 * L], a1), ("f0", f0[o : o + L], g1), ("energy", en[o : o + L], n1)):
            want = want.cpu().numpy()
            assert np.abs(got.cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max(), (what, i)


# ------------------------------------------------------------------------------------------------ 7. re-binding
def test_speech_predictor_and_hubert_share_one_engine(hub):
    """SpeechPredictor and HubertSpeechPredictor own the same frame-path components; called alternately, each re-binds its weights
    and reproduces what it gives alone (SpeechPredictor on a fresh engine; HubertSpeechPredictor against hubert_sp_short)."""
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.runtime import HipModel

    eng, hsp, _ = hub
    cfg = load_model_config()
    P, T = 12, 40
    texts = torch.from_numpy(synth.tokens("hb.rebind.tokens", 1, P, 178).astype(np.int64))
    dur = synth.durations_for("hb.rebind.dur", P, T)
    align = torch.from_numpy(synth.alignment_from_durations(dur)[None].astype(F32))
    pitch = torch.from_numpy(synth.pitch_curve("hb.rebind.pitch", 1, T))
    energy = torch.from_numpy((synth.uniform("hb.rebind.energy", (1, T)) * 2.0 + 2.0).astype(F32))
    nz = {k: torch.from_numpy(v) for k, v in synth.path_noise("hb.rebind", 1, 4 * T).items()}
    solo_eng = HipModel(cfg, 0)
    solo = modules.SpeechPredictor(cfg, engine=solo_eng).load_synthetic(0)
    want_sp = solo(texts, torch.tensor([P]), align, pitch, energy, noise=nz).audio.cpu()
    solo_eng.close()
    spm = modules.SpeechPredictor(cfg, engine=eng).load_synthetic(0)
    g = load_golden("hubert_sp_short")
    Th = int(g["T"])
    ins = inputs("hubert_sp_short", Th)
    nzh = {k: torch.from_numpy(v) for k, v in ins["nz"].items()}
    _ = hsp.engine  # bound: the stages below run on its frame-path weights
    s, feats, style, _ = front(eng, ins, Th)
    ref = staged(eng, s, eng.hubert_encoder(s, feats), style, dev(ins["pitch"][0]), dev(ins["energy"][0]), ins["nz"],
                 (g["cut_idx"].astype(np.int64), g["cut_phase"].astype(F32)))
    assert float(np.abs(ref["audio"].cpu().numpy() - g["audio"].reshape(-1)).max()) < 1e-3
    want_h = ref["raw"].cpu()
    for _ in range(2):
        got = spm(texts, torch.tensor([P]), align, pitch, energy, noise=nz).audio.cpu()
        assert torch.equal(got, want_sp)
        a = hsp(torch.from_numpy(ins["feats"]), torch.tensor([Th]), torch.from_numpy(ins["spk"]), torch.from_numpy(ins["pitch"]),
                torch.from_numpy(ins["energy"]), noise=nzh).audio.cpu()
        assert torch.equal(a.reshape(-1), want_h)


# ------------------------------------------------------------------------------------------------ 8. precision modes
def test_bf16_front_ends_are_fp32(hub):
    eng32 = hub[0]
    eng16, _, _ = make_engine("bf16")
    try:
        g = load_golden("hubert_sp_short")
        T = int(g["T"])
        ins = inputs("hubert_sp_short", T)
        r = {}
        for nm, e in (("f32", eng32), ("bf16", eng16)):
            s, feats, style, pe_style = front(e, ins, T)
            f0, en = e.hubert_pitch_energy(s, feats, pe_style)
            r[nm] = dict(style=style, pe_style=pe_style, asr=e.hubert_encoder(s, feats), f0=f0, en=en)
        for k in r["f32"]:
            assert torch.equal(r["f32"][k].cpu(), r["bf16"][k].cpu()), k
        s, _, style, _ = front(eng16, ins, T)
        out = staged(eng16, s, r["bf16"]["asr"], style, dev(ins["pitch"][0]), dev(ins["energy"][0]), ins["nz"],
                     (g["cut_idx"].astype(np.int64), g["cut_phase"].astype(F32)))
        ea = float(np.abs(out["audio"].cpu().numpy() - g["audio"].reshape(-1)).max())
        print(f"\n[bf16 audio] {ea:.1e}")
        assert ea < 1.2e-2
    finally:
        eng16.close()


# ------------------------------------------------------------------------------------------------ 9. errors
def test_errors_name_the_width(hub):
    from stylish_tts_amd.pipeline import VoiceConverter

    eng, sp, pe = hub
    vc = VoiceConverter(eng, modules=[sp, pe])
    feats, spk = torch.zeros(1, 768, 40), torch.zeros(1, 10240)
    with pytest.raises(ValueError, match="width 512.*hubert.hidden_dim is 768"):
        vc.convert(torch.zeros(1, 512, 40), [40], spk)
    with pytest.raises(ValueError, match="width 256.*speaker_embedder.hidden_dim is 10240"):
        vc.convert(feats, [40], torch.zeros(1, 256))
    with pytest.raises(ValueError, match="hubert.hidden_dim"):
        pe(torch.zeros(1, 700, 40), torch.tensor([40]), spk)
    with pytest.raises(ValueError, match="speaker_embedder.hidden_dim"):
        sp(feats, torch.tensor([40]), torch.zeros(1, 100), torch.zeros(1, 40), torch.zeros(1, 40))
    with pytest.raises(NotImplementedError):
        sp(feats, torch.tensor([40]), spk, torch.zeros(1, 40), torch.zeros(1, 40), audio_gt=torch.zeros(1, 1, 12000))
    # 2 frames = 600 samples: too short for the STFT's reflect padding (n_fft / 2 = 1024): the existing check refuses it before any launch
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        vc.convert(torch.zeros(1, 768, 2), [2], spk, pitch=torch.full((1, 2), 120.0), energy=torch.ones(1, 2))
    eng.check_status()
