"""MelStyleEncoder on the engine (csrc/mel_style.hip.h) against the reference fixtures of tests/golden/gen_golden_mel_style.py and a
float64 restatement, in both configurations: pe_mel_style_encoder (80, 64, 384) and cfm_pitch_predictor.spk_emb (80, 256, 1024).
Inputs are regenerated from their names (``mel``, the generator's recipe)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CONFIGS = {"pe": ((80, 64, 384, True), "pe_mel_style_encoder"), "cfm": ((80, 256, 1024, True), "cfm_pitch_predictor.spk_emb")}
LENGTHS = (33, 37, 47, 240, 803)


def mel(name, B, n_mels, T):
    from stylish_tts_amd import synth

    return torch.from_numpy(synth.normal("ms." + name, (B, 1, n_mels, T)))


_ENGINES = {}


def encoder(cfg, precision="f32"):
    """The encoder `cfg` with the fixtures' synthetic weights (seed 0) on an engine of the given precision (one engine per precision)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import HipModel

    if precision not in _ENGINES:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
    args, comp = CONFIGS[cfg]
    return modules.MelStyleEncoder(*args, engine=_ENGINES[precision], component=comp).load_synthetic(0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("precision", ["f32", "f32_native"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_goldens(cfg, precision):
    g = np.load(os.path.join(GOLD, f"mel_style_{cfg}.npz"))
    enc = encoder(cfg, precision)
    worst = {}
    for T in LENGTHS:
        style, taps = enc.run(mel(f"{cfg}{T}", 1, 80, T), taps=True)
        worst[f"style_{T}"] = rel(style.cpu(), g[f"style_{T}"])
        for b in range(4):
            tp = taps[b][0]
            assert tuple(tp.shape) == tuple(g[f"tap{b}_shape_{T}"]), (T, b, tp.shape)
            worst[f"tap{b}_{T}"] = rel(tp.reshape(-1)[torch.from_numpy(g[f"tap{b}_idx_{T}"]).to(tp.device)].cpu(), g[f"tap{b}_{T}"])
    print(cfg, precision, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-5, worst


def test_dense_batch_and_unconverged_uv():
    g = np.load(os.path.join(GOLD, "mel_style_misc.npz"))
    enc = encoder("pe")
    assert rel(enc(mel("pe_b2", 2, 80, 240)).cpu(), g["style_pe_b2_240"]) <= 1e-5
    from stylish_tts_amd import params

    sd = dict(enc.state_dict())
    for k in list(sd):
        if k.endswith(".weight_u"):
            base = k[: -len(".weight_u")]
            u, v = params.spectral_uv(sd[base + ".weight_orig"].numpy(), "pe_mel_style_encoder." + base, 0, iters=1)
            sd[base + ".weight_u"], sd[base + ".weight_v"] = torch.from_numpy(u), torch.from_numpy(v)
    enc.load_state_dict(sd)
    got = enc(mel("pe47", 1, 80, 47)).cpu()
    assert rel(got, g["style_pe_unconverged_47"]) <= 1e-5
    conv = encoder("pe")(mel("pe47", 1, 80, 47)).cpu()
    assert rel(conv, g["style_pe_unconverged_47"]) > 1e-3  # the case tells the folds apart


def test_16bit_modes_equal_f32_bits():
    x = mel("pe240", 1, 80, 240)
    ref = encoder("pe", "f32")(x).cpu()
    for p in ("bf16", "f16"):
        assert torch.equal(encoder("pe", p)(x).cpu(), ref), p


def _f64_forward(sd, args, x):
    """The reference's arithmetic restated in float64 (CPU): the ResBlk outputs and the style."""
    from stylish_tts_amd import params

    def w(p):
        return torch.from_numpy(params.fold_spectral_norm(sd[p + ".weight_orig"].numpy(), sd[p + ".weight_u"].numpy(), sd[p + ".weight_v"].numpy()))

    def b(p):
        return sd[p + ".bias"].double()

    lr = lambda t: F.leaky_relu(t, 0.2)  # noqa: E731
    dim_in, _, max_conv, skip = args
    h = F.conv2d(x.double(), w("shared.0"), b("shared.0"), padding=1)
    taps, c = [], dim_in
    for i in range(4):
        co, q = min(2 * c, max_conv), f"shared.{i + 1}."
        down = not (i == 3 and skip)
        s = F.conv2d(h, w(q + "conv1x1")) if c != co else h
        if down:
            if s.shape[-1] % 2:
                s = torch.cat([s, s[..., -1:]], -1)
            s = F.avg_pool2d(s, 2)
        r = F.conv2d(lr(h), w(q + "conv1"), b(q + "conv1"), padding=1)
        if down:
            r = F.conv2d(r, w(q + "downsample_res.conv"), b(q + "downsample_res.conv"), stride=2, padding=1, groups=c)
        r = F.conv2d(lr(r), w(q + "conv2"), b(q + "conv2"), padding=1)
        h = (s + r) / np.sqrt(2.0)
        taps.append(h)
        c = co
    h = F.conv2d(lr(h), w("shared.6"), b("shared.6"))
    h = lr(h.mean(dim=(2, 3)))
    return F.linear(h, sd["unshared.weight"].double(), sd["unshared.bias"].double()), taps


@pytest.mark.parametrize("cfg,B,T", [("pe", 8, 240), ("cfm", 8, 240), ("cfm", 1, 803)])
def test_float64_layer_by_layer(cfg, B, T):
    """Each ResBlk output and the style against float64: within the f32 matrix cores' class (fp32 products, fp32 sums over K <= 25 600)."""
    enc = encoder(cfg)
    x = mel(f"f64_{cfg}{T}", B, 80, T)
    style, taps = enc.run(x, taps=True)
    ref_style, ref_taps = _f64_forward(enc.state_dict(), CONFIGS[cfg][0], x)
    errs = []
    for b in range(4):
        got = torch.stack([t.double().cpu() for t in taps[b]])
        errs.append(rel(got, ref_taps[b]))
    errs.append(rel(style.cpu(), ref_style))
    print(cfg, B, T, [f"{e:.2e}" for e in errs])
    assert max(errs) <= 4e-6, errs


def test_ragged_batch_equals_each_alone():
    enc = encoder("cfm")
    L = [33, 803, 47, 240, 37, 100, 34, 511]
    x = torch.zeros(len(L), 1, 80, max(L))
    for i, t in enumerate(L):
        x[i, :, :, :t] = mel(f"rag{i}", 1, 80, t)[0]
    both = enc(x, lengths=L).cpu()
    for i, t in enumerate(L):
        assert torch.equal(both[i : i + 1], enc(x[i : i + 1, :, :, :t]).cpu()), (i, t)


def test_too_short_raises_and_engine_stays_usable():
    enc = encoder("pe")
    x = mel("pe33", 1, 80, 33)
    before = enc(x).cpu()
    with pytest.raises(RuntimeError, match="33"):
        enc(mel("short", 1, 80, 32))
    with pytest.raises(RuntimeError):
        enc(torch.cat([mel("a", 1, 80, 64), mel("b", 1, 80, 64)]), lengths=[64, 20])
    assert torch.equal(enc(x).cpu(), before)
