"""wn_fused_x3_kernel at every block shape and wave count on exposed operands (tests/test_flow_x3_cpu.py: every output of a WaveNet layer, of the
tail and of `pre` is one product and a short fp32 chain), element by element against float64 under the per-element bound of that module, which
its CPU twin shows rejects a dropped cross product, a wrong or truncated bf16 plane, a bias read twice, a halo row from the neighbouring
utterance, a tap off by one, swapped gate halves, the wrong cond column, `out` accumulated on layer 0, swapped m / ls, exp(+ls) and `pre`
reading the wrong half.  Teacher-forced through STTS_WN_DEBUG like tests/test_hip_flow_layers.py: every layer from the GPU's own inputs."""
import numpy as np
import pytest

from test_flow_x3_cpu import HALF, LENS, edge_inputs, exposed_flow, exposed_weights, layer_ref, pre_ref, tail_ref
from test_hip_flow_layers import run_flow
from test_hip_frame_path import segs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def exposed(cfg, weights):
    from stylish_tts_amd.runtime import HipModel

    E = exposed_flow()
    m = HipModel(cfg, 0)
    m.load_weights({"speech_predictor": exposed_weights(weights["speech_predictor"], E)}, which=7)
    yield m, E
    m.close()


def ratio(gpu, ref, bound):
    assert np.isfinite(gpu).all()
    return float((np.abs(gpu - ref) / bound).max())


@pytest.mark.parametrize("rt", [1, 2, 4])
@pytest.mark.parametrize("nw", [8, 4])
def test_wn_fused_x3_exposed_operands_per_element(exposed, rt, nw):
    eng, E = exposed
    env = dict(STTS_WN_M="2", STTS_WN_X3=str(rt), STTS_WN_X3_WAVES=str(nw))
    s = segs(LENS)
    inp = edge_inputs()
    zp, z_final = run_flow(eng, s, inp, env)
    grab = lambda k: run_flow(eng, s, inp, env, k)[1]  # noqa: E731
    h = grab(0)
    worst = {"pre": ratio(h, *pre_ref(E[7], zp, 1))}
    n_near0 = n_sat = 0
    ls_lo, ls_hi = np.inf, -np.inf
    z_prev = zp
    for f in reversed(range(8)):
        p, out = f & 1, None
        for i in range(3):
            k = 4 * (7 - f) + i + 1
            hr, dh, orf, do, a = layer_ref(E[f], i, h, out, LENS)
            h, out = grab(k), grab(-k)
            worst[f"{k}h"], worst[f"{k}out"] = ratio(h, hr, dh), ratio(out, orf, do)
            n_near0 += int((np.abs(a) < 1e-3).sum())
            n_sat += int((np.abs(a) > 20).sum())
        k = 4 * (7 - f) + 4
        zr, dz, ls = tail_ref(E[f], h, out, z_prev, p, LENS)
        ls_lo, ls_hi = min(ls_lo, ls.min()), max(ls_hi, ls.max())
        z = grab(-k)
        q = (1 - p) * HALF
        assert np.array_equal(z[:, p * HALF : (p + 1) * HALF], z_prev[:, p * HALF : (p + 1) * HALF])
        worst[f"{k}z"] = ratio(z[:, q : q + HALF], zr, dz)
        if f > 0:
            h = grab(k)
            worst[f"{k}pre"] = ratio(h, *pre_ref(E[f - 1], z, 1 - p))
        else:
            assert np.array_equal(z, z_final)
        z_prev = z
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"\n[flow x3 exposed] RT {rt} NW {nw}: worst |err| / bound " + ", ".join(f"{n} {v:.2f}" for n, v in top)
          + f"; gate pre-activations |a| < 1e-3: {n_near0}, |a| > 20: {n_sat}; ls in [{ls_lo:.2f}, {ls_hi:.2f}]")
    assert n_near0 > 1000 and n_sat > 1000 and ls_lo < -3 and ls_hi > 3
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, f"outputs over the per-element bound: {bad}"
