"""WavLM and the "slm" distance on the engine (csrc/wavlm.hip.h) against the reference fixtures of tests/golden/gen_golden_wavlm.py.

Taps: the engine's max-abs and rms error against the reference's FLOAT64 run, at the fixture's sampled indices, must be at most BAR = 4 x the
reference fp32 run's own error there (the standing bar of tests/test_hip_ssl.py).  Score: |slm_engine - slm64| <= the bar the generator stored,
4 x mean over the 13 states of (rms fp32 error of x's state + rms fp32 error of y's state) - what the tap bar implies, since
||a - b| - |a' - b'|| <= |a - a'| + |b - b'| and a mean of absolute values is at most the rms.  Inputs are regenerated from their names."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
NARROW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7, num_conv_pos_embeddings=32,
              num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40)


def wave(name, B, L):
    from stylish_tts_amd import synth

    return torch.from_numpy((synth.normal("wavlm.wave." + name, (B, L)) * 0.3).astype(np.float32))


def pair(name, B, L, eps=0.01):
    from stylish_tts_amd import synth

    x = wave(name, B, L).numpy()
    return torch.from_numpy(x), torch.from_numpy((x + np.float32(eps) * synth.normal("wavlm.noise." + name, (B, L)).astype(np.float32)).astype(np.float32))


_ENGINES, _MODS = {}, {}


def net(narrow=False, precision="f32"):
    """WavLM with the fixtures' synthetic weights (seed 0) on an engine of the given precision (one engine per precision)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import HipModel

    if precision not in _ENGINES:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
    key = (narrow, precision)
    if key not in _MODS:
        _MODS[key] = modules.WavLM(config=NARROW if narrow else None, engine=_ENGINES[precision]).load_synthetic(0)
    return _MODS[key]


def check_run(g, run, got, label):
    bad = []
    for key in sorted(k for k in g.files if k.startswith(run + "_") and k.endswith("_idx")):
        tap = key[len(run) + 1 : -4]
        idx, f32, f64 = g[key].astype(np.int64), g[f"{run}_{tap}_f32"].astype(np.float64), g[f"{run}_{tap}_f64"]
        mine = got[tap][idx]
        ref_e, my_e = f32 - f64, mine - f64
        ref_max, ref_rms = np.abs(ref_e).max(), np.sqrt((ref_e**2).mean())
        my_max, my_rms = np.abs(my_e).max(), np.sqrt((my_e**2).mean())
        print(f"{label} {run:>7s} {tap:>8s}: engine max {my_max:.2e} rms {my_rms:.2e} | reference fp32 max {ref_max:.2e} rms {ref_rms:.2e} | ratio {my_max / ref_max:.2f} {my_rms / ref_rms:.2f}")
        if not (my_max <= BAR * ref_max and my_rms <= BAR * ref_rms):
            bad.append((tap, my_max, ref_max, my_rms, ref_rms))
    assert not bad, bad


def engine_taps(m, w, bias=False):
    """{tap: flat float64} in the fixtures' layouts: state<k> and gate0 [B, frames, C]; bias [heads, frames, frames] of a single utterance, formed
    from the engine's gate, the engine's bucket table and the module's rel_attn_embed."""
    states, g0 = m.hidden_states(w, gate=True)
    got = {f"state{k}": s.cpu().double().numpy().ravel() for k, s in enumerate(states)}
    got["gate0"] = g0.cpu().double().numpy().ravel()
    if bias:
        T = states[0].shape[0]
        tab = m.engine.wavlm_bucket_table(T)
        emb = m.state_dict()["encoder.layers.0.attention.rel_attn_embed.weight"].double().numpy()  # [buckets, heads]
        q = np.arange(T)
        b = emb[tab[(q[None, :] - q[:, None]) + T]].transpose(2, 0, 1)  # [heads, q, j]
        got["bias"] = (g0.cpu().double().numpy().T[:, :, None] * b).ravel()
    return got


@pytest.mark.parametrize("run,B,samples", [("n1s", 1, 16000), ("n720", 1, 720), ("ndense", 2, 8000)])
def test_narrow_network_against_float64(run, B, samples):
    g = np.load(os.path.join(GOLD, "wavlm_narrow.npz"))
    check_run(g, run, engine_taps(net(narrow=True), wave(run, B, samples), bias=run == "n1s"), "narrow")


@pytest.mark.parametrize("case,run,samples", [("base_3s", "b3s", 48000), ("base_17s", "b17s", 272000)])
def test_base_network_against_float64(case, run, samples):
    g = np.load(os.path.join(GOLD, f"wavlm_{case}.npz"))
    check_run(g, run, engine_taps(net(), wave(run, 1, samples)), "base")


@pytest.mark.parametrize("narrow,nb,md", [(True, 32, 40), (False, 320, 800)])
def test_bucket_table_equals_the_reference_integers(narrow, nb, md):
    want = np.load(os.path.join(GOLD, "wavlm_misc.npz"))[f"buckets_{nb}_{md}"]
    got = net(narrow=narrow).engine.wavlm_bucket_table(4095)
    assert got.dtype == np.int32 and np.array_equal(got, want)  # |d| <= D exactly; beyond it the clamp, which is what the reference saturates to
    d = np.arange(-4095, 4096)
    assert np.array_equal(got[np.abs(d) > md], np.where(d[np.abs(d) > md] > 0, got[d == md][0], got[d == -md][0]))


def score_check(label, mine, f32, f64, bar):
    print(f"{label}: engine {mine:.9e} float64 {f64:.9e} | engine |diff| {abs(mine - f64):.2e} | reference fp32 |diff| {abs(f32 - f64):.2e} | bar {bar:.2e}")
    assert abs(mine - f64) <= bar


@pytest.mark.parametrize("narrow,case,name,samples", [(True, "narrow", "npair", 16000), (False, "base_3s", "bpair", 48000)])
def test_score_against_float64(narrow, case, name, samples):
    from stylish_tts_amd import modules

    g = np.load(os.path.join(GOLD, f"wavlm_{case}.npz"))
    loss = modules.WavLMLoss(net(narrow=narrow), 16000)
    x, y = pair(name, 1, samples)
    s = loss(x, y[:, None])
    assert s.dim() == 0 and s.dtype == torch.float64
    score_check(name, float(s), float(g[f"slm_{name}_f32"]), float(g[f"slm_{name}_f64"]), float(g[f"slm_{name}_bar"]))
    assert float(loss([x[0]], [y[0]])) == float(s)  # lists of 1-D waveforms: the same call


def test_identical_pair_scores_exactly_zero():
    from stylish_tts_amd import modules

    for narrow, n in ((True, 16000), (False, 48000)):
        x, y = pair("nsame", 1, n, 0.0)
        assert torch.equal(x, y)
        assert float(modules.WavLMLoss(net(narrow=narrow), 16000)(x, y)) == 0.0


def test_resampled_path_against_float64():
    from stylish_tts_amd import modules

    g = np.load(os.path.join(GOLD, "wavlm_misc.npz"))
    x, y = pair("r24k", 1, 12000)
    s = float(modules.WavLMLoss(net(narrow=True), 24000)(x, y))
    score_check("r24k at 24 kHz", s, float(g["resampled_slm32"]), float(g["resampled_slm64"]), float(g["resampled_bar"]))


def test_l1_reduction_alone_against_fsum_and_repeats_bit_for_bit():
    import ctypes as C

    from stylish_tts_amd import synth
    from stylish_tts_amd.runtime import Segments

    eng = net(narrow=True).engine
    L, Cn = [1, 149, 130], 768
    seg = Segments(L, eng.device)
    a = synth.normal("wavlm.l1.a", (seg.rows, Cn)).astype(np.float32)
    b = (a + 0.1 * synth.normal("wavlm.l1.b", (seg.rows, Cn))).astype(np.float32)
    b[0] = a[0]  # the one-row utterance: an exact zero
    ad, bd = torch.from_numpy(a).to(eng.device), torch.from_numpy(b).to(eng.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def run():
        part = torch.full((seg.n * ((max(L) + 7) // 8),), float("nan"), dtype=torch.float64, device=eng.device)
        sums = torch.empty(seg.n, dtype=torch.float64, device=eng.device)
        fr = torch.empty(seg.n, dtype=torch.int32, device=eng.device)
        rc = eng.lib.stts_op_wavlm_l1(C.c_void_p(torch.cuda.current_stream().cuda_stream), seg.n, seg.host_ptr, ptr(seg.dev), ptr(ad), ptr(bd), Cn, Cn, ptr(part), ptr(sums), ptr(fr))
        assert rc == 0, eng.lib.stts_last_error()
        assert fr.cpu().tolist() == L
        return sums.cpu()

    s1, s2 = run(), run()
    assert torch.equal(s1, s2)
    diff = np.abs(a - b)  # fp32 differences
    for u in range(seg.n):
        rows = diff[seg.host[u] : seg.host[u + 1]].astype(np.float64).ravel()
        want = math.fsum(rows.tolist())
        n = rows.size
        print(f"utterance {u}: {n} terms, engine {float(s1[u]):.17e} fsum {want:.17e} relative {abs(float(s1[u]) - want) / max(want, 1e-300):.2e} (bound {n * 2.0**-53:.2e})")
        assert abs(float(s1[u]) - want) <= n * 2.0**-53 * want
    assert float(s1[0]) == 0.0


def test_ragged_batch_equals_solo_runs_bit_for_bit():
    L = [48000, 720, 16000, 400]
    w = torch.zeros(4, max(L))
    for b, n in enumerate(L):
        w[b, :n] = wave(f"rag{b}", 1, n)[0]
    for narrow in (True, False):
        m = net(narrow=narrow)
        fr = [m.frames(n) for n in L]
        off = np.concatenate([[0], np.cumsum(fr)])
        states = [s.clone() for s in m.hidden_states(w, L)]
        keep = range(len(states)) if narrow else [len(states) - 1]
        for b, n in enumerate(L):
            solo = m.hidden_states(w[b : b + 1, :n])
            for k in keep:
                assert torch.equal(states[k][off[b] : off[b + 1]], solo[k]), (narrow, b, k)
        assert all(torch.isfinite(s).all() for s in states) and float(states[-1].std()) > 0.5
    # ... and the distance of a ragged batch is each pair's own run: sums bit for bit
    from stylish_tts_amd import modules

    loss = modules.WavLMLoss(net(narrow=True), 16000)
    y = w + 0.01 * torch.from_numpy(np.random.default_rng(0).standard_normal(w.shape).astype(np.float32))
    sums, frs = loss.sums(w, y, L)
    for b, n in enumerate(L):
        s1, f1 = loss.sums(w[b : b + 1, :n], y[b : b + 1, :n])
        assert torch.equal(sums[b], s1[0]) and int(frs[b]) == int(f1[0]) == net(narrow=True).frames(n)
    slm, utt = loss.scores(w, y, L)
    tot = sums.cpu().double()
    assert slm == math.fsum(math.fsum(r) for r in tot.tolist()) / (3 * sum(fr) * 128) and len(utt) == 4


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_16_bit_engines_give_the_fp32_bits(precision):
    w = wave("prec", 2, 16000)
    for narrow in (True, False):
        a = net(narrow=narrow).hidden_states(w)
        b = net(narrow=narrow, precision=precision).hidden_states(w)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), narrow


def test_validation_scores_slm_equals_the_loss_and_is_optional(cfg):
    from stylish_tts_amd import modules
    from stylish_tts_amd.pipeline import validation_scores

    m = net(narrow=True)
    eng = m.engine
    loss = modules.WavLMLoss(m, eng.cfg.sample_rate)
    gt, pred = pair("val", 2, 24000)
    L = [24000, 18000]
    plain = validation_scores(eng, pred, gt, L)
    assert sorted(plain) == ["mel", "mel_r", "mel_utt"]
    out = validation_scores(eng, pred, gt, L, slm=loss)
    assert sorted(out) == ["mel", "mel_r", "mel_utt", "slm", "slm_utt"]
    assert all(out[k] == plain[k] for k in plain)
    want, utt = loss.scores(gt, pred, L)
    assert out["slm"] == want == float(loss(gt, pred, L)) and out["slm_utt"] == utt and len(utt) == 2 and want > 0


def test_short_recordings_and_unequal_pairs_are_refused_before_any_launch():
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import Segments

    m = net(narrow=True)
    eng = m.engine
    z = torch.zeros(4000, device=eng.device)
    with pytest.raises(RuntimeError, match="fewer than one frame"):
        eng.wavlm_states(Segments([2000, 399], eng.device), z[:2399])
    with pytest.raises(RuntimeError, match="unequal lengths"):
        eng.wavlm_l1(Segments([2000, 1999], eng.device), z[:3999])
    with pytest.raises(RuntimeError, match="fewer than one frame"):
        eng.wavlm_l1(Segments([399, 399], eng.device), z[:798])
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="receptive field"):
        m.hidden_states(torch.zeros(1, 399))
    with pytest.raises(ValueError, match="one length"):
        modules.WavLMLoss(m, 16000)(torch.zeros(1, 2000), torch.zeros(1, 1999))
    assert len(m.hidden_states(torch.zeros(1, 400))) == 3
