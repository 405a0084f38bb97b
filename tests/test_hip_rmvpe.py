"""The RMVPE pitch extractor on the engine (csrc/rmvpe.hip.h) against the reference fixtures of tests/golden/gen_golden_rmvpe.py.

Accuracy is judged against the FLOAT64 run of the reference: for every tap the fixture holds the reference's own fp32 values and the float64
values at the same sampled indices, and the engine's max-abs and rms error against float64 must be at most BAR = 4 x the reference fp32 run's
own error there (the bar and the reasoning of tests/test_hip_ssl.py: two fp32 evaluations can sit on opposite sides of the truth, and a deep
chain gives a different ordering room once more).  Inputs are regenerated from their names (the generator's recipes)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
NARROW = dict(n_blocks=1, inter_layers=1, en_out_channels=8)
TAPS = [f"enc{l}" for l in range(5)] + ["inter"] + [f"dec{i}" for i in range(5)] + ["cnn", "gru"]


def mel_input(run, B, T):
    from stylish_tts_amd import synth

    return torch.from_numpy((synth.normal("rmvpe.mel." + run, (B, 128, T)) * 2.0 - 5.0).astype(np.float32))


def audio_input(n):
    from stylish_tts_amd import synth

    return torch.from_numpy((synth.normal(f"rmvpe.audio.{n}", (1, n)) * 0.1).astype(np.float32))


_ENGINES, _MODS = {}, {}


def extractor(narrow=False, precision="f32"):
    """The extractor with the fixtures' synthetic weights (seed 0) on an engine of the given precision (one engine per precision)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import HipModel

    if precision not in _ENGINES:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
    key = (narrow, precision)
    if key not in _MODS:
        _MODS[key] = modules.RmvpePitchExtractor(config=NARROW if narrow else None, engine=_ENGINES[precision]).load_synthetic(0)
    return _MODS[key]


def engine_taps(m, mel):
    """{tap: flat fp64 array in the fixtures' layout} of a dense batch mel [B, 128, T]."""
    from stylish_tts_amd.runtime import Segments

    B, _, T = mel.shape
    eng = m.engine
    seg = Segments([T] * B, eng.device)
    hid, f0, flat = eng.rmvpe(seg, m._pack_mel(mel, [T] * B), taps=True)
    Tp, c0 = 32 * ((T - 1) // 32 + 1), m.dims["en_out_channels"]
    flat = flat.cpu().double().numpy()
    shapes = [(Tp >> (l + 1), 64 >> l, c0 << l) for l in range(5)] + [(Tp >> 5, 4, c0 << 5)] + [(Tp >> (4 - i), 8 << i, c0 << (4 - i)) for i in range(5)]
    out, pos = {}, 0
    for tap, (t, f, c) in zip(TAPS[:11], shapes):
        ld = (c + 15) // 16 * 16
        a = flat[pos : pos + B * t * f * ld].reshape(B, t, f, ld)
        assert not a[..., c:].any(), f"{tap}: pad channels are not zero"
        out[tap] = a[..., :c].transpose(0, 3, 1, 2).ravel()  # [B, C, T', F']
        pos += B * t * f * ld
    a = flat[pos : pos + B * Tp * 128 * 4].reshape(B, Tp, 128, 4)
    assert not a[..., 3].any()
    out["cnn"] = a[..., :3].transpose(0, 3, 1, 2).ravel()
    pos += B * Tp * 128 * 4
    out["gru"] = flat[pos : pos + B * Tp * 512]
    assert pos + B * Tp * 512 == flat.size
    out["hidden"] = hid.cpu().double().numpy().ravel()  # [B, T, 360]: packed rows of equal lengths
    return out


def check_run(g, run, got, label, worst):
    """Engine error against float64 <= BAR x the reference fp32 run's own error, max-abs and rms, on every tap of the fixture run."""
    bad = []
    for key in sorted(k for k in g.files if k.startswith(run + "_") and k.endswith("_idx")):
        tap = key[len(run) + 1 : -4]
        idx, f32, f64 = g[key].astype(np.int64), g[f"{run}_{tap}_f32"].astype(np.float64), g[f"{run}_{tap}_f64"]
        mine = got[tap][idx]
        ref_e, my_e = f32 - f64, mine - f64
        ref_max, ref_rms = np.abs(ref_e).max(), np.sqrt((ref_e**2).mean())
        my_max, my_rms = np.abs(my_e).max(), np.sqrt((my_e**2).mean())
        worst[0], worst[1] = max(worst[0], my_max / ref_max), max(worst[1], my_rms / ref_rms)
        print(f"{label} {run:>7s} {tap:>7s}: engine max {my_max:.2e} rms {my_rms:.2e} | reference fp32 max {ref_max:.2e} rms {ref_rms:.2e} | ratio {my_max / ref_max:.2f} {my_rms / ref_rms:.2f}")
        if not (my_max <= BAR * ref_max and my_rms <= BAR * ref_rms):
            bad.append((tap, my_max, ref_max, my_rms, ref_rms))
    print(f"{label} {run}: worst ratio max-abs {worst[0]:.2f} rms {worst[1]:.2f}")
    assert not bad, bad


@pytest.mark.parametrize("case,run,B,T", [("full_a", "f17", 1, 17), ("full_a", "f32", 1, 32), ("full_b", "f33", 1, 33), ("full_b", "f100", 1, 100), ("dense", "fdense", 2, 64)])
def test_full_network_every_tap_against_float64(case, run, B, T):
    g = np.load(os.path.join(GOLD, f"rmvpe_{case}.npz"))
    check_run(g, run, engine_taps(extractor(), mel_input(run, B, T)), "full", [0.0, 0.0])


@pytest.mark.parametrize("run,T", [("n17", 17), ("n33", 33), ("n100", 100)])
def test_narrow_network_every_tap_against_float64(run, T):
    g = np.load(os.path.join(GOLD, "rmvpe_narrow.npz"))
    check_run(g, run, engine_taps(extractor(narrow=True), mel_input(run, 1, T)), "narrow", [0.0, 0.0])


def test_decode_of_the_crafted_salience():
    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))
    m = extractor(narrow=True)
    sal = torch.from_numpy(g["decode_sal"])
    for k, th in enumerate(g["decode_thred"]):
        f32, f64 = g[f"decode_f32_{k}"].astype(np.float64), g[f"decode_f64_{k}"]
        got = m.decode(sal, thred=float(th)).cpu().double().numpy()
        assert got.shape == f64.shape == (2, 64)  # no frame is left out
        voiced = f64 > 0
        assert np.array_equal(got > 0, voiced) and np.array_equal(f32 > 0, voiced), "voiced / unvoiced pattern"
        assert (got[~voiced] == 0).all()
        ref_rel = np.abs(f32[voiced] / f64[voiced] - 1).max()
        my_rel = np.abs(got[voiced] / f64[voiced] - 1).max()
        print(f"decode thred {th}: {int(voiced.sum())} voiced; engine max rel {my_rel:.2e} | reference fp32 {ref_rel:.2e} | ratio {my_rel / ref_rel:.2f}")
        assert my_rel <= BAR * ref_rel
    assert (g["decode_f64_0"] > 0).sum() > (g["decode_f64_1"] > 0).sum()  # the second threshold silences a frame the first keeps
    with pytest.raises(NotImplementedError):
        m.decode(sal, use_viterbi=True)


@pytest.mark.parametrize("n", [513, 1600, 16000])
def test_log_mel_against_float64(n):
    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))
    m = extractor(narrow=True)
    rows, seg, lin = m.mel_packed(audio_input(n), linear=True)
    lin64, lin32 = g[f"mel_{n}_lin64"], g[f"mel_{n}_lin32"].astype(np.float64)
    assert seg.lengths == [n // 160 + 1] and tuple(rows.shape) == (n // 160 + 1, 128)
    mine = lin.cpu().double().numpy().T  # [128, frames]
    ref_e, my_e = lin32 - lin64, mine - lin64
    ratio = np.abs(my_e).max() / np.abs(ref_e).max(), np.sqrt((my_e**2).mean()) / np.sqrt((ref_e**2).mean())
    print(f"mel {n}: engine max {np.abs(my_e).max():.2e} | reference fp32 {np.abs(ref_e).max():.2e} | ratio {ratio[0]:.2f} {ratio[1]:.2f}")
    assert ratio[0] <= BAR and ratio[1] <= BAR
    keep = lin64 > 1e-4
    assert keep.mean() >= 0.95
    log64, log32 = g[f"mel_{n}_log64"], g[f"mel_{n}_log32"].astype(np.float64)
    mylog = rows.cpu().double().numpy().T
    assert np.abs(mylog - log64)[keep].max() <= BAR * np.abs(log32 - log64)[keep].max()
    assert torch.equal(m.mel(audio_input(n))[0].t().contiguous(), rows)


@pytest.mark.parametrize("n_in,n_out", [(100, 80), (17, 13)])
def test_interpolation_against_float64(n_in, n_out):
    from stylish_tts_amd import synth
    from stylish_tts_amd.runtime import Segments

    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))
    eng = extractor(narrow=True).engine
    x = torch.from_numpy(synth.pitch_curve(f"rmvpe.curve.{n_in}", 1, n_in)[0].astype(np.float32)).to(eng.device)
    want = g[f"interp_{n_in}_{n_out}"]
    got = eng.rmvpe_resample(Segments([n_in], eng.device), x, Segments([n_out], eng.device)).cpu().double().numpy()
    assert (want == 0).any() and (want > 50).any()
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), np.abs(got - want).max()
    # two utterances in one call: each is its own curve
    both = eng.rmvpe_resample(Segments([n_in, n_in], eng.device), torch.cat([x, x]), Segments([n_out, n_in], eng.device)).cpu().double().numpy()
    assert np.array_equal(both[:n_out], got) and np.array_equal(both[n_out:], x.cpu().double().numpy())


def test_ragged_batch_equals_solo_runs_bit_for_bit():
    m = extractor()
    L = [17, 64, 33, 100]
    mel = torch.zeros(4, 128, max(L))
    for b, n in enumerate(L):
        mel[b, :, :n] = mel_input(f"rag{b}", 1, n)[0]
    hid = m.mel2hidden(mel, L).clone()
    f0 = m(mel, L).clone()
    assert tuple(hid.shape) == (4, 100, 360) and tuple(f0.shape) == (4, 100)
    for b, n in enumerate(L):
        assert torch.equal(hid[b, :n], m.mel2hidden(mel[b : b + 1, :, :n])[0]), b
        assert torch.equal(f0[b, :n], m(mel[b : b + 1, :, :n])[0]), b
        assert not hid[b, n:].any() and not f0[b, n:].any()
        assert torch.equal(m.decode(hid[b : b + 1, :n])[0], f0[b, :n]), b
    assert torch.isfinite(hid).all() and float(hid[1, :64].std()) > 0.05


def test_infer_from_audio_equals_the_steps_bit_for_bit():
    m = extractor(narrow=True)
    S = [16000, 4000]
    w = torch.zeros(2, max(S))
    for b, n in enumerate(S):
        w[b, :n] = audio_input(16000)[0, :n] * (1 + b)
    f0 = m.infer_from_audio(w, S)
    for b, n in enumerate(S):
        mel = m.mel(w[b : b + 1, :n])
        assert tuple(mel.shape) == (1, 128, n // 160 + 1)
        step = m.decode(m.mel2hidden(mel))
        assert torch.equal(f0[b, : n // 160 + 1], step[0]), b
    fr = m.infer_from_audio(w, S, frames=[80, 20])
    assert tuple(fr.shape) == (2, 80) and not fr[1, 20:].any()
    with pytest.raises(ValueError, match="16000"):
        m.infer_from_audio(w, S, sample_rate=24000)
    with pytest.raises(ValueError, match="512"):
        m.mel(torch.zeros(1, 512))
    with pytest.raises(ValueError, match="17"):
        m.infer_from_audio(torch.zeros(1, 160 * 15))


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_16_bit_engines_give_the_fp32_bits(precision):
    mel = mel_input("prec", 2, 40)
    a, b = extractor(narrow=True), extractor(narrow=True, precision=precision)
    assert torch.equal(a.mel2hidden(mel), b.mel2hidden(mel)) and torch.equal(a(mel), b(mel))
    w = audio_input(1600)
    assert torch.equal(a.mel(w), b.mel(w))


def test_short_utterance_is_an_error_status_and_the_module_round_trips(tmp_path):
    import json

    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import Segments

    m = extractor(narrow=True)
    eng = m.engine
    rows = torch.zeros(40, 128, device=eng.device)
    with pytest.raises(RuntimeError, match="at least 17"):
        eng.rmvpe(Segments([16], eng.device), rows[:16])
    with pytest.raises(RuntimeError, match="at least 17"):
        eng.rmvpe(Segments([20, 16], eng.device), rows[:36])
    torch.cuda.synchronize()
    for n in (15, 16):
        with pytest.raises(ValueError, match="17"):
            m.mel2hidden(torch.zeros(1, 128, n))
    assert tuple(m.mel2hidden(torch.zeros(1, 128, 17)).shape) == (1, 17, 360)
    # the full module carries the reference's key list, and a safetensors checkpoint of it loads
    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))
    full = extractor()
    sd = full.state_dict()
    assert list(sd.keys()) == json.loads(str(g["keys"])) and [list(v.shape) for v in sd.values()] == json.loads(str(g["shapes"]))
    st = pytest.importorskip("safetensors.torch")
    nsd = m.state_dict()
    st.save_file({k: v.contiguous() for k, v in nsd.items()}, str(tmp_path / "rmvpe.safetensors"))
    m2 = modules.RmvpePitchExtractor.from_safetensors(str(tmp_path / "rmvpe.safetensors"), config=NARROW, engine=eng)
    mel = mel_input("n33", 1, 33)
    assert torch.equal(m2(mel), m(mel))
