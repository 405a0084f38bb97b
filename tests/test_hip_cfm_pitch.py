"""CfmPitchPredictor on the engine (csrc/cfm_pitch.hip.h + the spk_emb MelStyleEncoder) against the reference fixtures of
tests/golden/gen_golden_cfm_pitch.py and a float64 restatement written here, layer by layer; the fused denorm_f0_zscore; ragged
batches; VoiceConverter(ref_mel=...).  Inputs are regenerated from their names (``asr`` / ``mel``, the generator's recipe)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cfm_pitch.npz")
MEL_LEN = {1: 33, 3: 40, 33: 33, 240: 240, 803: 300, 1100: 120}
BAR = 1e-5  # max-abs error over max |reference|


def asr(name, B, T):
    from stylish_tts_amd import synth

    return torch.from_numpy(synth.normal("cp.asr." + name, (B, 768, T)))


def mel(name, B, T):
    from stylish_tts_amd import synth

    return torch.from_numpy(synth.normal("cp.mel." + name, (B, 80, T)))


_ENGINES = {}


def engine(precision="f32"):
    from stylish_tts_amd.runtime import HipModel

    if precision not in _ENGINES:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
    return _ENGINES[precision]


def predictor(precision="f32"):
    from stylish_tts_amd import modules

    return modules.CfmPitchPredictor(768, 80, engine=engine(precision)).load_synthetic(0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def ragged(names_T):
    """a zero-padded batch of (name, T, Tm) utterances -> (asr, mel, asr lengths, mel lengths)"""
    B, T, Tm = len(names_T), max(t for _, t, _ in names_T), max(m for _, _, m in names_T)
    a, m = torch.zeros(B, 768, T), torch.zeros(B, 80, Tm)
    for b, (n, t, tm) in enumerate(names_T):
        a[b, :, :t] = asr(n, 1, t)[0]
        m[b, :, :tm] = mel(n, 1, tm)[0]
    return a, m, [t for _, t, _ in names_T], [tm for _, _, tm in names_T]


@pytest.mark.parametrize("precision", ["f32", "f32_native", "bf16", "f16"])
def test_goldens(precision):
    g = np.load(GOLD)
    m = predictor(precision)
    worst = {"dense": rel(m(asr("dense", 2, 240), mel("dense", 2, 240)).cpu(), g["dense_normed"])}
    for T, Tm in MEL_LEN.items():
        out, _, taps = m.run(asr(f"T{T}", 1, T), mel(f"T{T}", 1, Tm), taps=T == 240)
        assert out.shape == (1, 1, T)
        worst[f"T{T}"] = rel(out.cpu(), g[f"normed_{T}"])
        if taps:
            for k in range(5):
                flat = taps[k][0].reshape(-1)
                worst[f"tap{k}"] = rel(flat[torch.from_numpy(g[f"tap{k}_idx"]).to(flat.device)].cpu(), g[f"tap{k}"])
    print(precision, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= BAR, worst


def test_16bit_engines_return_the_f32_bits():
    a, m, La, Lm = ragged([("T240", 240, 240), ("T33", 33, 33), ("T3", 3, 40)])
    want = predictor("f32")(a, m, La, Lm)
    for p in ("bf16", "f16"):
        assert torch.equal(predictor(p)(a, m, La, Lm), want), p


# ------------------------------------------------------------------------------------------------ float64 restatement, layer by layer
def _sd64(m):
    return {k: v.to("cuda", torch.float64) for k, v in m.state_dict().items()}


def asr_emb64(sd, x):  # x [asr_dim, T]
    h = F.conv1d(x[None], sd["asr_emb.0.weight"], sd["asr_emb.0.bias"])
    return F.conv1d(F.mish(h), sd["asr_emb.2.weight"], sd["asr_emb.2.bias"])[0]


def block64(sd, i, x, spk):  # generator.ConvNeXtBlock (models/generator.py:441-499) with AdaptiveLayerNorm (ada_norm.py:185-201)
    q = f"blocks.{i}."
    y = F.conv1d(x[None], sd[q + "dwconv.weight"], sd[q + "dwconv.bias"], padding=3, groups=x.shape[0])[0].t()
    h = spk @ sd[q + "norm.fc.weight"].t() + sd[q + "norm.fc.bias"]
    gamma, beta = h[:256], h[256:]
    y = (1 + gamma) * F.layer_norm(y, (256,), eps=1e-6) + beta
    y = F.silu(y @ sd[q + "pwconv1.weight"].t() + sd[q + "pwconv1.bias"])
    gx = torch.norm(y, p=2, dim=0, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    y = sd[q + "grn.gamma"][0] * (y * nx) + sd[q + "grn.beta"][0] + y
    y = y @ sd[q + "pwconv2.weight"].t() + sd[q + "pwconv2.bias"]
    return x + y.t()


def out64(sd, x):
    return sd["out_proj.weight"][0, :, 0] @ x + sd["out_proj.bias"]


@pytest.mark.parametrize("case", ["ragged", "long"])
def test_layers_against_float64(case):
    m = predictor()
    sd = _sd64(m)
    spec = [("L240", 240, 240), ("L37", 37, 33), ("L5", 5, 40)] if case == "ragged" else [("L1100", 1100, 120)]
    a, mm, La, Lm = ragged(spec)
    normed, _, taps = m.run(a, mm, La, Lm, taps=True)
    spk = m.speaker_style(mm, Lm).to(torch.float64)
    worst = {}
    for b, T in enumerate(La):
        x = a[b, :, :T].to("cuda", torch.float64)
        steps = [("asr_emb", asr_emb64(sd, x), taps[0][b])]
        for i in range(4):
            steps.append((f"block{i}", block64(sd, i, taps[i][b].to(torch.float64), spk[b]), taps[i + 1][b]))
        steps.append(("out_proj", out64(sd, taps[4][b].to(torch.float64)), normed[b, 0, :T]))
        for name, want, got in steps:
            e = rel(got.cpu(), want.cpu())
            worst[name] = max(worst.get(name, 0.0), e)
        assert (normed[b, 0, T:] == 0).all()
    print(case, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 2e-6, worst


def test_ragged_batch_equals_each_utterance_alone():
    m = predictor()
    spec = [(f"T{T}", T, Tm) for T, Tm in MEL_LEN.items()]
    a, mm, La, Lm = ragged(spec)
    got = m(a, mm, La, Lm)
    assert got.shape == (len(La), 1, max(La))
    bits, worst = True, 0.0
    for b, (n, T, Tm) in enumerate(spec):
        solo = m(asr(n, 1, T), mel(n, 1, Tm))[0, 0]
        worst = max(worst, rel(got[b, 0, :T].cpu(), solo.cpu()))
        bits = bits and torch.equal(got[b, 0, :T], solo)
        assert (got[b, 0, T:] == 0).all()
    print(f"ragged vs solo: max rel {worst:.2e}, bit-identical {bits}")
    assert worst <= BAR


def test_two_identical_calls_give_identical_bits():
    m = predictor()
    a, mm, La, Lm = ragged([("T803", 803, 300), ("T240", 240, 240), ("T1", 1, 33)])
    stats = (7.4, 0.45)
    n1, h1, _ = m.run(a, mm, La, Lm, f0_log2_stats=stats)
    n2, h2, _ = m.run(a, mm, La, Lm, f0_log2_stats=stats)
    assert torch.equal(n1, n2) and torch.equal(h1, h2)


@pytest.mark.parametrize("stats", [(7.4, 0.45), (7.0, 2.5)])
def test_fused_denorm_equals_host_helper(stats):
    from stylish_tts_amd import modules, synth

    m = predictor()
    a, mm, La, Lm = ragged([("T1", 1, 33), ("T240", 240, 240), ("T33", 33, 33)])
    B, T = len(La), max(La)
    uv = torch.from_numpy((synth.uniform("cp.uvgpu", (B, T)) > 0.6).astype(np.float32))
    normed, hz, _ = m.run(a, mm, La, Lm, f0_log2_stats=stats, uv=uv)
    mean, std = torch.tensor(stats[0]), torch.tensor(stats[1])
    for b, L in enumerate(La):
        want = modules.denorm_f0_zscore(normed[b, 0, :L].cpu(), uv[b, :L], mean, std)
        got = hz[b, 0, :L].cpu()
        ulp = 2 * np.finfo(np.float32).eps * want.abs()
        assert ((got - want).abs() <= ulp).all(), (b, float((got - want).abs().max()))
        assert (got[uv[b, :L] > 0] == 0).all()
        assert (hz[b, 0, L:] == 0).all()
    h = hz[hz > 0]
    if stats[1] > 1:  # wide statistics: both clamp ends are reached by the synthetic network
        assert float(h.min()) == 50.0 and float(h.max()) == 1200.0
    _, hz_nouv, _ = m.run(a, mm, La, Lm, f0_log2_stats=stats)
    assert (hz_nouv[0, 0, :1] >= 50).all()  # T = 1, no uv: voiced


def test_loading_the_full_component_leaves_the_spk_emb_encoder_unchanged():
    from stylish_tts_amd import modules

    eng = engine()
    enc = modules.MelStyleEncoder(80, 256, 1024, True, engine=eng, component="cfm_pitch_predictor.spk_emb").load_synthetic(0)
    x = mel("spk", 2, 240)[:, None]
    before = enc(x, lengths=[240, 77]).clone()
    m = predictor()
    m(asr("dense", 2, 240), mel("dense", 2, 240))
    assert torch.equal(m.speaker_style(x[:, 0], [240, 77]), before)  # the same weights under the same keys
    assert torch.equal(enc(x, lengths=[240, 77]), before)


# ------------------------------------------------------------------------------------------------ VoiceConverter(ref_mel=...)
def test_voice_converter_takes_f0_from_the_cfm_pitch_predictor():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    cfg = load_model_config()
    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, hubert=True, cfm_pitch=True)
    sp, pe, cp = (mods[k].load_synthetic(0) for k in ("hubert_speech_predictor", "hubert_pitch_energy_predictor", "cfm_pitch_predictor"))
    vc = VoiceConverter(eng, modules=[sp, pe, cp])
    L, Lm = [60, 37], [40, 33]
    feats = torch.zeros(2, 768, 60)
    for b, t in enumerate(L):
        feats[b, :, :t] = torch.from_numpy(synth.normal(f"cp.vc.feats{b}", (768, t)))
    spk = torch.from_numpy(synth.normal("cp.vc.spk", (2, 10240)))
    ref = torch.zeros(2, 80, 40)
    for b, t in enumerate(Lm):
        ref[b, :, :t] = torch.from_numpy(synth.normal(f"cp.vc.mel{b}", (80, t)))
    uv = torch.from_numpy((synth.uniform("cp.vc.uv", (2, 60)) > 0.8).astype(np.float32))
    stats = (7.4, 0.45)
    R4 = 4 * sum(L)
    noise = dict(prior_noise=torch.from_numpy(synth.normal("cp.vc.pn", (R4, 128))).cuda(),
                 src_noise=torch.from_numpy(synth.normal("cp.vc.sn", (R4 * eng.hop4,))).cuda(), init_phase=torch.zeros(1).cuda())
    waves, det = vc.convert(feats, L, spk, noise=noise, return_details=True, ref_mel=ref, ref_mel_lengths=Lm, f0_log2_stats=stats, uv=uv)
    _, hz, _ = cp.run(feats, ref, L, Lm, f0_log2_stats=stats, uv=uv)
    want_f0 = torch.cat([hz[b, 0, : L[b]] for b in range(2)])
    assert torch.equal(det["pitch"], want_f0)
    _, want_en = eng.hubert_pitch_energy(*_front(eng, feats, L, spk))
    assert torch.equal(det["energy"], want_en)
    pitch = torch.zeros(2, 60)
    energy = torch.zeros(2, 60)
    for b in range(2):
        pitch[b, : L[b]] = hz[b, 0, : L[b]].cpu()
        energy[b, : L[b]] = want_en[sum(L[:b]) : sum(L[: b + 1])].cpu()
    w2 = vc.convert(feats, L, spk, pitch=pitch, energy=energy, noise=noise)
    for a, b in zip(waves, w2):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        vc.convert(feats, L, spk, pitch=pitch, energy=energy, ref_mel=ref, f0_log2_stats=stats)
    with pytest.raises(ValueError):
        vc.convert(feats, L, spk, ref_mel=ref)  # no statistics
    assert VoiceConverter.host_syncs_per_call == 0
    eng.close()


def _front(eng, feats, L, spk):
    from stylish_tts_amd.modules import _pack_rows
    from stylish_tts_amd.runtime import Segments

    st = Segments(L, eng.device)
    _, pe_style = eng.speaker_style(spk.cuda().float().contiguous(), style=False)
    return st, _pack_rows(eng, feats, L), pe_style
