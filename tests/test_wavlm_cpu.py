"""CPU side of WavLM and the "slm" distance: the float64 restatement tests/wavlm64.py against the reference's float64 run
(tests/golden/gen_golden_wavlm.py), the bucket rule against the reference's integers, the parameter inventory, the module's state_dict round trip,
config handling, and the C ABI's statuses (a stand-alone sanitizer program against the HIP runtime stub, tests/asan/wavlm_driver.cpp).

wavlm64 against the float64 fixtures: the bar is 1e-10 of each tap's scale - double-precision agreement between two orders of summation.  Measured
worst case here: 1.5e-14 of the scale (state2 of the one-second run), so nothing needs writing next to the bar."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import wavlm64

GOLD = os.path.join(ROOT, "tests", "golden")
NARROW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7, num_conv_pos_embeddings=32,
              num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40)
BAR = 1e-10


def wave(name, B, L):
    from stylish_tts_amd import synth

    return (synth.normal("wavlm.wave." + name, (B, L)) * 0.3).astype(np.float32)


def pair(name, B, L, eps=0.01):
    from stylish_tts_amd import synth

    x = wave(name, B, L)
    return x, (x + np.float32(eps) * synth.normal("wavlm.noise." + name, (B, L)).astype(np.float32)).astype(np.float32)


@pytest.fixture(scope="module")
def misc():
    return np.load(os.path.join(GOLD, "wavlm_misc.npz"))


@pytest.fixture(scope="module")
def narrow():
    """(arch, weights, fixture) of the narrow network."""
    from stylish_tts_amd import params, wavlm

    a = wavlm.arch(NARROW)
    return a, params.synth_state_dict(params.wavlm_spec(a), 0, prefix="wavlm."), np.load(os.path.join(GOLD, "wavlm_narrow.npz"))


@pytest.mark.parametrize("nb,md", [(320, 800), (32, 40)])
def test_bucket_equals_the_reference_integers(misc, nb, md):
    from stylish_tts_amd import wavlm

    d = np.arange(-4095, 4096)
    want = misc[f"buckets_{nb}_{md}"]
    assert np.array_equal(wavlm64.bucket(d, nb, md), want)
    assert np.array_equal(wavlm.bucket(d, nb, md), want)
    # monotone in |d| on either side, saturated by max_bucket_distance: what lets the engine clamp the distance there
    assert np.array_equal(want[d >= md], np.full((d >= md).sum(), nb - 1)) and np.array_equal(want[d <= -md], np.full((d <= -md).sum(), nb // 2 - 1))
    assert (np.diff(want[d >= 1]) >= 0).all() and (np.diff(want[d <= 0]) <= 0).all()
    if (nb, md) == (32, 40):
        assert want[d == 33][0] == nb - 1 and want[d == 32][0] < nb - 1  # saturates at distance 33 already


def test_wavlm64_reproduces_the_float64_reference_on_the_narrow_network(narrow):
    a, sd, g = narrow
    worst = 0.0
    for run, B, L in (("n1s", 1, 16000), ("n720", 1, 720), ("ndense", 2, 8000)):
        w = wave(run, B, L)
        outs = [wavlm64.forward(sd, a, w[b]) for b in range(B)]
        got = {f"state{k}": np.concatenate([o["states"][k].ravel() for o in outs]) for k in range(3)}
        got["gate0"] = np.concatenate([o["gate0"].ravel() for o in outs])
        if B == 1:
            got["bias"] = outs[0]["bias0"].ravel()
        for key in sorted(k for k in g.files if k.startswith(run + "_") and k.endswith("_idx")):
            tap = key[len(run) + 1 : -4]
            want = g[f"{run}_{tap}_f64"]
            err = np.abs(got[tap][g[key].astype(np.int64)] - want).max() / max(np.abs(want).max(), 1.0)
            worst = max(worst, err)
            print(f"{run:>7s} {tap:>7s}: {err:.2e} of the scale")
            assert err <= BAR, (run, tap, err)
    for nm, eps in (("npair", 0.01), ("nsame", 0.0)):
        x, y = pair(nm, 1, 16000, eps)
        s = wavlm64.l1_mean(wavlm64.forward(sd, a, x[0])["states"], wavlm64.forward(sd, a, y[0])["states"])
        want = float(g[f"slm_{nm}_f64"])
        print(f"slm {nm}: {s:.12e} reference {want:.12e}")
        assert abs(s - want) <= BAR * max(want, 1.0) and (eps or s == 0.0)
    print(f"worst {worst:.2e}")


def test_spec_equals_the_reference_key_list(misc):
    from stylish_tts_amd import params, wavlm

    for tag, a in (("", wavlm.arch(NARROW)), ("_base", wavlm.arch())):
        keys, shapes = json.loads(str(misc["keys" + tag])), json.loads(str(misc["shapes" + tag]))
        spec = params.wavlm_spec(a)
        assert [n for n, _, _ in spec] == keys
        assert [list(s) for _, s, _ in spec] == shapes
    assert "encoder.layers.0.attention.rel_attn_embed.weight" in keys and "encoder.layers.1.attention.rel_attn_embed.weight" not in keys
    sd = params.synth_state_dict(params.wavlm_spec(wavlm.arch(NARROW)), 0, prefix="wavlm.")
    c = sd["encoder.layers.0.attention.gru_rel_pos_const"]
    assert np.abs(c - 1.0).max() <= 0.1  # near its initial value


def test_module_round_trips_the_state_dict_and_rejects_bad_keys():
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules

    src = modules.WavLM(config=NARROW).load_synthetic(0)
    sd = src.state_dict()
    m = modules.WavLM(config=NARROW)
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    q = "encoder.pos_conv_embed.conv."
    legacy = {k.replace(q + "parametrizations.weight.original0", q + "weight_g").replace(q + "parametrizations.weight.original1", q + "weight_v"): v for k, v in sd.items()}
    m.load_state_dict(legacy)
    missing = {k: v for k, v in sd.items() if k != "encoder.layers.1.attention.gru_rel_pos_linear.weight"}
    with pytest.raises(RuntimeError, match="gru_rel_pos_linear"):
        m.load_state_dict(missing)
    bad = dict(sd)
    bad["encoder.layers.0.attention.rel_attn_embed.weight"] = torch.zeros(320, 2)
    with pytest.raises(RuntimeError, match="shape mismatch for encoder.layers.0.attention.rel_attn_embed.weight"):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))
    assert m.frames(16000) == 49 and m.n_states == 3 and m.hidden == 128


@pytest.mark.parametrize("field,value", [("feat_extract_norm", "layer"), ("do_stable_layer_norm", True), ("conv_bias", True), ("hidden_act", "relu"),
                                         ("feat_extract_activation", "relu"), ("add_adapter", True), ("num_attention_heads", 8), ("num_buckets", 30),
                                         ("num_buckets", 0), ("max_bucket_distance", 4096), ("max_bucket_distance", 80), ("hidden_size", 770),
                                         ("conv_kernel", (10, 3, 3, 3, 3, 2)), ("intermediate_size", 100), ("num_hidden_layers", 0),
                                         ("num_conv_pos_embedding_groups", 5)])
def test_arch_rejects_unsupported_fields_by_name(field, value):
    from stylish_tts_amd import wavlm

    name = "conv_dim" if field == "conv_kernel" else field
    with pytest.raises(ValueError, match=rf"wavlm\.arch\.{name}"):
        wavlm.arch({field: value})


def test_arch_defaults_and_accepted_fields():
    from stylish_tts_amd import wavlm

    a = wavlm.arch()
    assert (a["num_buckets"], a["max_bucket_distance"], a["hidden_size"], a["num_attention_heads"]) == (320, 800, 768, 12)
    b = wavlm.arch(dict(NARROW, masked_spec_embed=[0.0], model_type="wavlm", num_buckets=64, max_bucket_distance=17))
    assert (b["num_buckets"], b["max_bucket_distance"]) == (64, 17) and "masked_spec_embed" not in b
    d = wavlm.dims_struct(b)
    assert (d.ssl.hidden_size, d.num_buckets, d.max_bucket_distance) == (128, 64, 17)
    assert wavlm.score([[1.0, 2.0, 3.0], [3.0, 0.0, 0.0]], [2, 1], 2) == (9.0 / 18.0, [6.0 / 12.0, 3.0 / 6.0])


@pytest.mark.timeout(900)
def test_c_abi_statuses_under_asan_ubsan(tmp_path):
    """Stand-alone program only (nothing here is loaded into python): bucket table, workspace walks, and an unequal pair or a recording under 400
    samples as error statuses before any launch."""
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs the ROCm clang toolchain")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "wavlm_build_and_run.py"), str(tmp_path / "build")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=850)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert "wavlm driver: all cases ran" in tail and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, tail
    assert "buckets : 8191 distances equal the reference's" in tail
    for what in ("unequal pair", "pair of 399 samples", "states of 399 samples", "states below the least workspace", "l1_sums below the least workspace"):
        assert f"rejected {what} : " in tail, (what, tail)
