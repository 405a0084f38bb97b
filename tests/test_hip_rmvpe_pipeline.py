"""GPU: the RMVPE pitch extractor inside the voice-conversion chain (VoiceConverter.convert_audio(pitch_extractor=...)) and beside the fp32
frame path on another stream of the same engine (DESIGN.md sections 5d, 5j)."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NARROW = dict(n_blocks=1, inter_layers=1, en_out_channels=8)
NARROW_HUBERT = {"hidden_dim": 128, "sr": 16000, "arch": {"hidden_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2, "intermediate_size": 256,
                                                          "conv_dim": [64] * 7, "num_conv_pos_embeddings": 32, "num_conv_pos_embedding_groups": 4}}


def test_hidden_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    px = modules.RmvpePitchExtractor(engine=eng).load_synthetic(0)
    px.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    mel = torch.from_numpy((synth.normal("rmvpe.mel.f100", (1, 128, 100)) * 2.0 - 5.0).astype(np.float32)).cuda()
    L = [240] * 4
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("rvc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("rvc.f0", (R,))) * 60 + 120), energy=dev(synth.normal("rvc.en", (R,))),
              style=dev(synth.normal("rvc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("rvc.pn", (R, 128))), sn=dev(synth.normal("rvc.sn", (R * 75,))),
              ph=dev(synth.uniform("rvc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    solo_h, solo_f = px.mel2hidden(mel).clone(), px(mel).clone()
    torch.cuda.synchronize()
    g = np.load(os.path.join(GOLD, "rmvpe_full_b.npz"))
    idx, f32, f64 = g["f100_hidden_idx"].astype(np.int64), g["f100_hidden_f32"].astype(np.float64), g["f100_hidden_f64"]
    mine = solo_h.cpu().double().numpy().ravel()[idx]
    assert np.abs(mine - f64).max() <= 4.0 * np.abs(f32 - f64).max()
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(4):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def pitch():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [(px.mel2hidden(mel), px(mel)) for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    with ThreadPoolExecutor(2) as ex:
        f = ex.submit(frames)
        got = ex.submit(pitch).result()
        f.result()
    for j, (h, f0) in enumerate(got):
        assert torch.equal(h, solo_h) and torch.equal(f0, solo_f), j
    eng.close()


def test_convert_audio_with_a_pitch_extractor():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import DEFAULT_MODEL, load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    raw = copy.deepcopy(DEFAULT_MODEL)
    raw["hubert"] = copy.deepcopy(NARROW_HUBERT)
    cfg = load_model_config(raw)
    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, hubert=True, ssl=True, cfm_pitch=True)
    px = modules.RmvpePitchExtractor(config=NARROW, engine=eng).load_synthetic(0)
    vc = VoiceConverter(eng, [mods["hubert_speech_predictor"], mods["hubert_pitch_energy_predictor"], mods["cfm_pitch_predictor"], mods["hubert"]])
    S, T = [16000, 8000], [80, 40]
    w = torch.zeros(2, 16000)
    for b, n in enumerate(S):
        w[b, :n] = torch.from_numpy((synth.normal(f"rvc.wave{b}", (n,)) * 0.1).astype(np.float32))
    spk = torch.from_numpy(synth.normal("rvc.spk", (2, vc.spk_dim)) * 0.5)
    R4 = 4 * sum(T)
    noise = dict(prior_noise=torch.from_numpy(synth.normal("rvc.vpn", (R4, 128))).cuda(), src_noise=torch.from_numpy(synth.normal("rvc.vsn", (R4 * eng.hop4,))).cuda(),
                 init_phase=torch.zeros(1).cuda())
    # a threshold at which the synthetic network's salience leaves both voiced and unvoiced frames
    hid = px.mel2hidden(px.mel(w[:1]))
    px.thred = float(hid.max(dim=-1)[0].median())
    own = px.packed_from_audio(w, S, T).clone()
    assert own.shape == (sum(T),) and bool((own == 0).any()) and bool((own > 0).any())
    base = vc.convert_audio(w, S, T, spk, noise=noise)
    # without ref_mel: the extracted curve is the pitch; energy is predicted
    waves, det = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px)
    assert torch.equal(det["pitch"], own)
    _, det0 = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True)
    assert torch.equal(det["energy"], det0["energy"]) and not torch.equal(det["pitch"], det0["pitch"])
    assert all(torch.isfinite(x).all() for x in waves) and [x.numel() for x in waves] == [x.numel() for x in base]
    # with ref_mel: uv = (extracted f0 == 0) on the device
    ref = torch.from_numpy(synth.normal("rvc.ref", (2, cfg.n_mels, 40)).astype(np.float32))
    stats = (7.4, 0.45)
    _, dr = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px, ref_mel=ref, f0_log2_stats=stats)
    assert torch.equal(dr["pitch"] == 0, own == 0) and bool((dr["pitch"][own > 0] >= 50).all())
    uv = torch.zeros(2, 80)
    _, du = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px, ref_mel=ref, f0_log2_stats=stats, uv=uv)
    assert bool((du["pitch"] > 0).all())  # a given uv wins
    # without the keyword nothing changed: the same bits as before, and convert()'s own errors
    again = vc.convert_audio(w, S, T, spk, noise=noise)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    feats = mods["hubert"](w, 80, S)
    with pytest.raises(ValueError, match="give both pitch and energy, or neither"):
        vc.convert(feats, [80, 80], spk, pitch=torch.zeros(2, 80))
    with pytest.raises(ValueError, match="not both"):
        vc.convert_audio(w, S, T, spk, pitch_extractor=px, pitch=torch.zeros(2, 80), energy=torch.zeros(2, 80))
    assert VoiceConverter.host_syncs_per_call == 0
    eng.close()
