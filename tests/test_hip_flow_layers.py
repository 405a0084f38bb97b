"""The reverse flow's WaveNet kernels against float64, one layer at a time (tests/flow64.py), per kernel variant.

Teacher forcing: STTS_WN_DEBUG = +-k (csrc/flow.hip.h WnDebugStop) stops the flow after WaveNet layer k = 4 (7 - f) + i + 1 and hands
back h (+k) or `out` (-k); after a coupling layer's last WaveNet layer (i = 3) +k is the next coupling layer's h_0 = pre(z) and -k the whole z.
Every layer k is recomputed in float64 from the GPU's OWN h and `out` after layer k - 1, so each comparison sees one layer's error only:
  - layers i = 0 .. 2: h' and out';
  - the tail (i = 3: the last res/skip, proj_mean / proj_logstd, the coupling (z1 - m) exp(-ls)): the updated half of z, from the GPU's h and
    `out` after layer 2 and the GPU's z after the previous coupling layer (the prior's z before the first), and the half it must not touch;
  - `pre`: the next h_0 against float64 pre of the GPU's own z;
  - wn_block_x3_kernel (one launch per coupling layer) per coupling layer: h_0 in, z and the next h_0 out.
The first coupling layer's h_0 is the engine's own `pre` of the prior's z (k = 0), checked against float64 like the other `pre`s.

Bars (split-fp32 variants): per layer and quantity, the error is within 1.25 x the error of the f32-matrix-core kernel with the same block
rows (wn_fused_kernel M = 1 / 2 / 4; the generic path: precision "f32_native") on the same batch, plus a floor, in max and rms, and below an
absolute bar in units of the layer's output scale.  The two forms are NOT run on bit-identical inputs: each is teacher-forced on its own
trajectory, and the two trajectories differ by fp32 noise, so the f32 error is that of the same layer on inputs equal to within that noise; the
floor absorbs the difference.  Why the bars sit where they do: see RATIO below.
"""
import contextlib
import os

import numpy as np
import pytest

import flow64 as F
from test_hip_frame_path import dev, hip, segs  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# ragged lengths that straddle the 16-, 32- and 64-row blocks and the conv's +-2-row reach; the second batch has more than kWnSegInline = 64
# utterances (wn_fused.hip.h), so the per-launch kernels read seg_off instead of their inlined offsets
# (47 / 49 / 97: around wn_block_x3_kernel<4>'s 48-row output blocks)
# (BATCHES and VARIANTS are written out a second time where Python cannot be imported - tests/asan/asan_driver.cpp flow_section, whose launch traces
#  tests/test_asan_host.py FLOW_CASES / _VARIANTS lists: a new batch or variant goes there too)
BATCHES = {"ragged": [1, 2, 15, 16, 17, 31, 33, 47, 49, 63, 65, 97, 130], "many": [1, 2, 15, 16, 17, 31, 33, 63, 65, 130] * 7}

_ENV = ("STTS_WN_M", "STTS_WN_X3", "STTS_WN_X3B", "STTS_WN_X3_WAVES", "STTS_WN_DEBUG")
_X3 = {f"x{rt}w{nw}": dict(STTS_WN_M="2", STTS_WN_X3=str(rt), STTS_WN_X3_WAVES=str(nw)) for rt in (1, 2, 4) for nw in (8, 4)}
VARIANTS = {
    **_X3,                                                          # wn_fused_x3_kernel<RT, LAST, NW>: 16 / 32 / 64-row blocks, 8 / 4 waves
    "b3": dict(STTS_WN_M="2", STTS_WN_X3="2", STTS_WN_X3B="3"),     # wn_block_x3_kernel<3>: 32 output rows per block
    "b4": dict(STTS_WN_M="2", STTS_WN_X3="2", STTS_WN_X3B="4"),     # wn_block_x3_kernel<4>: 48
    "m1": dict(STTS_WN_M="1", STTS_WN_X3="-1"),                     # wn_fused_kernel<M> on the f32 matrix cores: direct form, 16-row blocks
    "m2": dict(STTS_WN_M="2", STTS_WN_X3="-1"),                     # F(2,5), 32-row blocks
    "m4": dict(STTS_WN_M="4", STTS_WN_X3="-1"),                     # F(4,5), 64-row blocks
    "m16": dict(STTS_WN_M="16", STTS_WN_X3="-1"),                   # the staged 16-row kernel (wn_layer_small.hip.h)
}
# split variant -> the f32-matrix-core kernel it is held to (the same rows per block; wn_block_x3 replaces the 32-row per-layer kernels)
NATIVE_OF = {**{v: f"m{v[1]}" for v in _X3}, "b3": "m2", "b4": "m2"}
SPLIT_CASES = [(b, v) for b in BATCHES for v in NATIVE_OF if b == "ragged" or v.startswith("x")]
NATIVE_CASES = [(b, v) for b in BATCHES for v in ("m1", "m2", "m4", "m16") if b == "ragged" or v != "m16"]

# The bars, in units of each quantity's output scale (max |float64|).  Measured on the MI355X, worst over the 32 layers and every quantity
# (h, out, z, pre), max / rms: every wn_fused_x3 variant 4.3e-7 / 7.3e-8 (ragged batch) and 5.4e-7 / 6.8e-8 (70 utterances); wn_block_x3
# per coupling layer 3.0e-7 / 2.7e-8; the f32 kernels M = 1 6.7e-7 / 6.6e-8, M = 2 (F(2,5)) 9.7e-7 / 1.5e-7, M = 4 (F(4,5)) 1.9e-6 / 2.3e-7;
# the generic path at width 96 4.9e-7 / 8.1e-8 split vs 5.3e-7 / 8.2e-8 f32.  The split form is held to 1.25 x the f32 kernel's error at the same layer + a floor of ~0.3 of its typical per-layer
# error (1.5e-7 / 1.5e-8: the per-layer maxima of two fp32 computations differ by that much), and to an absolute 1.2e-6 / 1.5e-7 (about 2 x its
# worst layer); the f32 kernels to 3e-6 / 3e-7.  Why this is tight enough: a wn_fused_x3_kernel with one small cross product dropped from its
# six (x1 w1, which a CPU emulation of one 640-term conv output puts at 2.5 x the correct error) measured 4.3e-6 / 8.5e-7 on the first
# layer's `out` - over every bar here, and 70 x under test_hip_frame_path.py's 2e-4 of max-abs, which it passes.
RATIO, MAX_FLOOR, RMS_FLOOR = 1.25, 1.5e-7, 1.5e-8
SPLIT_MAX, SPLIT_RMS = 1.2e-6, 1.5e-7
F32_MAX, F32_RMS = 3e-6, 3e-7


@contextlib.contextmanager
def flow_env(env, debug=None):
    saved = {k: os.environ.get(k) for k in _ENV}
    try:
        for k in _ENV:
            os.environ.pop(k, None)
        os.environ.update(env)
        if debug is not None:
            os.environ["STTS_WN_DEBUG"] = str(debug)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def batch_inputs(lens, dh, fh, tag):
    from stylish_tts_amd import synth

    rows = sum(lens)
    x = synth.normal(f"wnl.{tag}.x", (rows, dh))
    st = (synth.normal(f"wnl.{tag}.s", (len(lens), 64)) * 0.7).astype(np.float32)
    nz = synth.normal(f"wnl.{tag}.n", (rows, fh))
    return x, st, nz


def run_flow(eng, s, inp, env, debug=None):
    x, st, nz = inp
    with flow_env(env, debug):
        _, zp, zf = eng.prior_flow(s, dev(x), dev(st), dev(nz), return_z=True)
        torch.cuda.synchronize()
    return zp.cpu().numpy().astype(np.float64), zf.cpu().numpy().astype(np.float64)


def err(gpu, ref):
    e = np.abs(gpu - ref)
    scale = np.abs(ref).max()
    assert np.isfinite(gpu).all()
    return float(e.max() / scale), float(np.sqrt((e ** 2).mean()) / scale)


def layer_errors(eng, lens, inp, fws, env, block=False):
    """[(k, quantity, max err / scale, rms err / scale)] over the whole flow, teacher-forced layer by layer."""
    s = segs(lens)
    zp, z_final = run_flow(eng, s, inp, env)
    half = zp.shape[1] // 2
    grab = lambda k: run_flow(eng, s, inp, env, k)[1]  # noqa: E731
    res = []
    z_prev, h_prev = zp, grab(0)
    res.append((0, "pre", *err(h_prev, F.pre(fws[7], zp, 1))))
    for f in reversed(range(8)):
        p, cw = f & 1, fws[f]
        gc = F.cond_columns(cw, inp[1])
        h, out = h_prev, None
        for i in range(3):
            k = 4 * (7 - f) + i + 1
            h_ref, out_ref = F.wn_layer(cw, i, h, out, gc, lens)
            if block:  # one launch per coupling layer: nothing to see between its WaveNet layers
                h, out = h_ref, out_ref
                continue
            h, out = grab(k), grab(-k)
            res += [(k, "h", *err(h, h_ref)), (k, "out", *err(out, out_ref))]
        k = 4 * (7 - f) + 4
        z_ref, _ = F.tail(cw, None, h, out, z_prev, gc, lens, p)
        z = grab(-k)
        keep, upd = slice(p * half, (p + 1) * half), slice((1 - p) * half, (2 - p) * half)
        assert np.array_equal(z[:, keep], z_prev[:, keep]), f"layer {k}: the half the coupling reads changed"
        res.append((k, "z", *err(z[:, upd], z_ref[:, upd])))
        if f > 0:
            h_prev = grab(k)
            res.append((k, "pre", *err(h_prev, F.pre(fws[f - 1], z, 1 - p))))
        else:
            assert np.array_equal(z, z_final), "the hand-back at the last layer is the flow's z_out"
        z_prev = z
    return res


_CACHE = {}


def measured(eng, fws, batch, variant, block=False):
    """block: checked per coupling layer only (wn_block_x3, and the f32 kernel it is held to)."""
    key = (batch, variant, block)
    if key not in _CACHE:
        lens = BATCHES[batch]
        _CACHE[key] = layer_errors(eng, lens, batch_inputs(lens, 512, 128, batch), fws, VARIANTS[variant], block=block)
        print(f"\n[flow layers] {batch} {variant}{' per coupling layer' if block else ''} (k quantity max/rms of the scale): "
              + "; ".join(f"{k}{q} {m:.2e}/{r:.2e}" for k, q, m, r in _CACHE[key]))
    return _CACHE[key]


@pytest.fixture(scope="module")
def fws(weights):
    return F.flow_weights(weights["speech_predictor"])


def check_absolute(errs, what, max_abs=F32_MAX, rms_abs=F32_RMS):
    for k, q, m, r in errs:
        assert m <= max_abs and r <= rms_abs, f"{what}: layer {k} {q}: max {m:.2e} rms {r:.2e} of the scale"


def check_against_native(split, native, what):
    assert [e[:2] for e in split] == [e[:2] for e in native]
    worst = max(split, key=lambda e: e[2])
    print(f"\n[flow layers] {what}: worst layer {worst[0]} {worst[1]} max {worst[2]:.2e} rms {worst[3]:.2e} of the scale; "
          f"max over layers split {max(e[2] for e in split):.2e} native {max(e[2] for e in native):.2e}, "
          f"rms split {max(e[3] for e in split):.2e} native {max(e[3] for e in native):.2e}")
    for (k, q, m, r), (_, _, mn, rn) in zip(split, native):
        assert m <= RATIO * mn + MAX_FLOOR, f"{what}: layer {k} {q}: max err {m:.2e} > {RATIO} x native {mn:.2e} + {MAX_FLOOR:.0e}"
        assert r <= RATIO * rn + RMS_FLOOR, f"{what}: layer {k} {q}: rms err {r:.2e} > {RATIO} x native {rn:.2e} + {RMS_FLOOR:.0e}"
    check_absolute(split, what, SPLIT_MAX, SPLIT_RMS)


@pytest.mark.parametrize("batch,variant", NATIVE_CASES, ids=[f"{b}-{v}" for b, v in NATIVE_CASES])
def test_f32_flow_kernels_per_layer_against_float64(hip, fws, batch, variant):
    check_absolute(measured(hip, fws, batch, variant), f"{batch} {variant}")


@pytest.mark.parametrize("batch,variant", SPLIT_CASES, ids=[f"{b}-{v}" for b, v in SPLIT_CASES])
def test_split_flow_kernels_per_layer_against_float64(hip, fws, batch, variant):
    block = variant.startswith("b")
    split = measured(hip, fws, batch, variant, block)
    native = measured(hip, fws, batch, NATIVE_OF[variant], block)
    check_against_native(split, native, f"{batch} {variant} vs {NATIVE_OF[variant]}")


def test_generic_flow_path_per_layer_against_float64():
    """Flow width 96 (the narrow model.yml of tests/test_hip_config_dims.py): every layer is two contractions with the EPI_GATE / EPI_SPLIT_ACC
    epilogues and the coupling runs in EPI_COUPLE (csrc/gemm.hip.h); split fp32 against the f32 matrix cores."""
    from stylish_tts_amd import params
    from stylish_tts_amd.runtime import HipModel
    from test_oracle_golden import narrow_cfg

    cfg, _ = narrow_cfg()
    dh, fh = cfg.decoder.hidden_dim, cfg.decoder.hidden_dim // 4
    assert fh == 96
    w = params.synth_state_dict(params.module_spec("speech_predictor", cfg), 0, prefix="speech_predictor.")
    fw = F.flow_weights(w)
    lens = BATCHES["ragged"]
    inp = batch_inputs(lens, dh, fh, "narrow")
    errs = {}
    for prec in ("f32", "f32_native"):
        eng = HipModel(cfg, 0, precision=prec)
        eng.load_weights({"speech_predictor": w}, which=7)
        errs[prec] = layer_errors(eng, lens, inp, fw, {})
        eng.check_status()
        eng.close()
        print(f"\n[flow layers] generic {prec}: " + "; ".join(f"{k}{q} {m:.2e}/{r:.2e}" for k, q, m, r in errs[prec]))
    check_absolute(errs["f32_native"], "generic f32_native")
    check_against_native(errs["f32"], errs["f32_native"], "generic f32 vs f32_native")
