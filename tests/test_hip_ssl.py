"""AdaptiveHubert on the engine (csrc/ssl.hip.h) against the reference fixtures of tests/golden/gen_golden_ssl.py.

Accuracy is judged against the FLOAT64 run of the reference module: for every tap the fixture holds the reference's own fp32 values and the
float64 values at the same sampled indices, and the engine's max-abs and rms error against float64 must be at most BAR = 4 x the
reference fp32 run's own error there.  The 4 is 2 x 2: two independent fp32 evaluations with different summation orders can sit on
opposite sides of the truth, and the 19-layer chain gives a different ordering room to grow once more.
Inputs are regenerated from their names (``wave``, the generator's recipe)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
NARROW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7, num_conv_pos_embeddings=32,
              num_conv_pos_embedding_groups=4)


def wave(name, B, L):
    from stylish_tts_amd import synth

    return torch.from_numpy((synth.normal("ssl.wave." + name, (B, L)) * 0.3).astype(np.float32))


_ENGINES, _MODS = {}, {}


def hubert(narrow=False, precision="f32"):
    """The content encoder with the fixtures' synthetic weights (seed 0) on an engine of the given precision (one engine per precision)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import HipModel

    if precision not in _ENGINES:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
    key = (narrow, precision)
    if key not in _MODS:
        _MODS[key] = modules.AdaptiveHubert(config=NARROW if narrow else None, engine=_ENGINES[precision]).load_synthetic(0)
    return _MODS[key]


def engine_taps(m, w, time_dim, lengths=None):
    """{tap: [per-utterance flat fp64 arrays]} in the fixtures' layouts (time-major [frames, C]; out: [C, time_dim])."""
    B = w.shape[0]
    feats, t = m.packed(w, [time_dim] * B, lengths, taps=True)
    fr = t["frames"]
    off = np.concatenate([[0], np.cumsum(fr)])
    c0 = t["conv0_off"].cpu().numpy()
    L = [w.shape[1]] * B if lengths is None else lengths
    H = m.hidden
    out = {k: [] for k in ("conv0", "conv_last", "proj", "pos", "out")}
    nl = t["layers"].shape[0]
    for k in range(1, nl + 1):
        out[f"layer{k}"] = []
    for b in range(B):
        n0 = (L[b] - m.arch["conv_kernel"][0]) // m.arch["conv_stride"][0] + 1
        out["conv0"].append(t["conv0"][c0[b] : c0[b] + n0].cpu().double().numpy().ravel())
        for k in ("conv_last", "proj", "pos"):
            out[k].append(t[k][off[b] : off[b + 1]].cpu().double().numpy().ravel())
        for k in range(1, nl + 1):
            out[f"layer{k}"].append(t["layers"][k - 1, off[b] : off[b + 1]].cpu().double().numpy().ravel())
        out["out"].append(feats[b * time_dim : (b + 1) * time_dim, :H].t().cpu().double().numpy().ravel())
    assert torch.equal(t["hidden"], t["layers"][nl - 1])
    return out


def check_run(g, run, got, label):
    """Engine error against float64 <= BAR x the reference fp32 run's own error, max-abs and rms, on every tap of the fixture run."""
    bad = []
    for key in sorted(k for k in g.files if k.startswith(run + "_") and k.endswith("_idx")):
        tap = key[len(run) + 1 : -4]
        idx, f32, f64 = g[key].astype(np.int64), g[f"{run}_{tap}_f32"].astype(np.float64), g[f"{run}_{tap}_f64"]
        mine = np.concatenate(got[tap])[idx]
        ref_e, my_e = f32 - f64, mine - f64
        ref_max, ref_rms = np.abs(ref_e).max(), np.sqrt((ref_e**2).mean())
        my_max, my_rms = np.abs(my_e).max(), np.sqrt((my_e**2).mean())
        print(f"{label} {run:>7s} {tap:>9s}: engine max {my_max:.2e} rms {my_rms:.2e} | reference fp32 max {ref_max:.2e} rms {ref_rms:.2e} | ratio {my_max / ref_max:.2f} {my_rms / ref_rms:.2f}")
        if not (my_max <= BAR * ref_max and my_rms <= BAR * ref_rms):
            bad.append((tap, my_max, ref_max, my_rms, ref_rms))
    assert not bad, bad


@pytest.mark.parametrize("case,run,samples,time_dim", [("base_3s", "b3s", 48000, 240), ("base_10s", "b10s", 160000, 800), ("base_short", "b400", 400, 3),
                                                        ("base_short", "b720", 720, 7)])
def test_base_network_against_float64(case, run, samples, time_dim):
    g = np.load(os.path.join(GOLD, f"ssl_{case}.npz"))
    m = hubert()
    check_run(g, run, engine_taps(m, wave(run, 1, samples), time_dim), "base")


def test_dense_batch_equals_the_reference_batch_call():
    g = np.load(os.path.join(GOLD, "ssl_base_dense.npz"))
    check_run(g, "bdense", engine_taps(hubert(), wave("bdense", 2, 16000), 80), "base")


@pytest.mark.parametrize("run,B,samples,time_dim", [("n1s", 1, 16000, 80), ("n720", 1, 720, 5), ("ndense", 2, 8000, 33)])
def test_narrow_configuration(run, B, samples, time_dim):
    g = np.load(os.path.join(GOLD, "ssl_narrow.npz"))
    check_run(g, run, engine_taps(hubert(narrow=True), wave(run, B, samples), time_dim), "narrow")


def test_ragged_batch_equals_solo_runs_bit_for_bit():
    m = hubert()
    L, T = [48000, 720, 160000, 400], [240, 7, 800, 3]
    w = torch.zeros(4, max(L))
    for b, n in enumerate(L):
        w[b, :n] = wave(f"rag{b}", 1, n)[0]
    rows = m.packed(w, T, L).clone()
    off = np.concatenate([[0], np.cumsum(T)])
    for b, n in enumerate(L):
        solo = m.packed(w[b : b + 1, :n], [T[b]])
        assert torch.equal(rows[off[b] : off[b + 1]], solo), b
    assert torch.isfinite(rows).all() and float(rows[:, : m.hidden].std()) > 0.5


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_16_bit_engines_give_the_fp32_bits(precision):
    w = wave("prec", 2, 16000)
    a = hubert()(w, 80)
    b = hubert(precision=precision)(w, 80)
    assert torch.equal(a, b)


def test_short_utterance_and_zero_time_dim_are_error_statuses():
    import ctypes as C

    from stylish_tts_amd.runtime import Segments

    m = hubert()
    eng = m.engine
    good = torch.zeros(4000, device=eng.device)
    with pytest.raises(RuntimeError, match="fewer than one frame"):
        eng.hubert_ssl(Segments([399], eng.device), good[:399], Segments([3], eng.device))
    with pytest.raises(RuntimeError, match="fewer than one frame"):
        eng.hubert_ssl(Segments([2000, 399], eng.device), good[:2399], Segments([3, 3], eng.device))
    s, t = Segments([2000], eng.device), Segments([3], eng.device)
    t.host[1] = 0  # a time_dim of 0
    with pytest.raises(RuntimeError, match="time_dim of 0"):
        eng.hubert_ssl(s, good[:2000], t)
    torch.cuda.synchronize()
    assert eng.hubert_ssl(s, good[:2000], Segments([3], eng.device)).shape == (3, 768)
    with pytest.raises(ValueError, match="receptive field"):
        m(torch.zeros(1, 399), 3)
    assert C.sizeof(C.c_int) == 4


def test_module_round_trips_the_reference_state_dict_and_matches_the_golden():
    import json

    from stylish_tts_amd import modules, params

    gm = np.load(os.path.join(GOLD, "ssl_misc.npz"))
    keys, shapes = json.loads(str(gm["keys"])), json.loads(str(gm["shapes"]))
    src = hubert()
    sd = src.state_dict()
    assert list(sd.keys()) == keys and [list(v.shape) for v in sd.values()] == shapes
    m2 = modules.AdaptiveHubert(engine=src._engine)
    m2.load_state_dict(sd)
    # the legacy weight-norm spelling loads too
    q = "model.encoder.pos_conv_embed.conv."
    legacy = {k.replace(q + "parametrizations.weight.original0", q + "weight_g").replace(q + "parametrizations.weight.original1", q + "weight_v"): v
              for k, v in sd.items()}
    m3 = modules.AdaptiveHubert(engine=src._engine)
    m3.load_state_dict(legacy)
    w = wave("bdense", 2, 16000)
    y = m2(w, 80)
    assert tuple(y.shape) == (2, 768, 80)
    assert torch.equal(y, m3(w, 80)) and torch.equal(y, src(w, 80))
    g = np.load(os.path.join(GOLD, "ssl_base_dense.npz"))
    idx, f32, f64 = g["bdense_out_idx"].astype(np.int64), g["bdense_out_f32"].astype(np.float64), g["bdense_out_f64"]
    mine = y.cpu().double().numpy().ravel()[idx]
    assert np.abs(mine - f64).max() <= BAR * np.abs(f32 - f64).max()
    assert params.count_params(params.hubert_ssl_spec()) == sum(int(np.prod(s)) for s in shapes)


def test_convert_audio_equals_convert_on_the_modules_features(cfg):
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, hubert=True, ssl=True)
    vc = VoiceConverter(eng, [mods["hubert_speech_predictor"], mods["hubert_pitch_energy_predictor"], mods["hubert"]])
    B, S, T = 2, 16000, 80
    w = wave("vc", B, S)
    spk = torch.from_numpy(synth.normal("ssl.spk", (B, vc.spk_dim)) * 0.5)
    R = 4 * B * T
    noise = dict(prior_noise=torch.from_numpy(synth.normal("ssl.pn", (R, 128))).cuda(), src_noise=torch.from_numpy(synth.normal("ssl.sn", (R * eng.hop4,))).cuda(),
                 init_phase=torch.from_numpy(synth.uniform("ssl.ph", (1,))).cuda())
    feats = mods["hubert"](w, T)
    a = vc.convert(feats, [T] * B, spk, noise=noise)
    b = vc.convert_audio(w, [S] * B, [T] * B, spk, noise=noise)
    assert VoiceConverter.host_syncs_per_call == 0
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
