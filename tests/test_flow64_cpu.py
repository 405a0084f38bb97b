"""tests/flow64.py (the float64 restatement of the reverse flow the per-layer GPU tests measure against) reproduces the reference's golden
(tests/golden/flow.npz, z -> z_out) and the fp32 oracle to fp32 noise, and its layer pieces compose to the whole flow.  CPU only."""
import numpy as np

import flow64 as F
from conftest import load_golden
from oracle import stylish_oracle as O


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_flow64_reproduces_the_golden_and_the_oracle(weights):
    g = load_golden("flow")
    w = weights["speech_predictor"]
    fws = F.flow_weights(w)
    z = g["z"][0].T
    z64 = F.flow_reverse(fws, z, g["style"], [64])
    ref = g["z_out"][0].T
    ora = O.flow_reverse(g["z"], g["style"][:, :, None], w)[0].T
    e_golden, e_oracle, e_ref = rel(z64, ref), rel(z64, ora), rel(ora, ref)
    print(f"\n[flow64] z_out: float64 vs golden {e_golden:.2e}, vs the fp32 oracle {e_oracle:.2e}; oracle vs golden {e_ref:.2e} (of the scale)")
    # 32 fp32 WaveNet layers in the reference and in the oracle: measured 3.6e-7 / 2.7e-7 / 2.6e-7 of the scale
    assert e_golden < 2e-6 and e_oracle < 2e-6
    # the same with the Flip left out (the halves' roles never swap) is nowhere near
    def no_flip(z):
        z = np.array(z, np.float64)
        for f in reversed(range(8)):
            cw = fws[f]
            gc = F.cond_columns(cw, g["style"])
            h, out = F.pre(cw, z, 1), None
            for i in range(3):
                h, out = F.wn_layer(cw, i, h, out, gc, [64])
            z, _ = F.tail(cw, None, h, out, z, gc, [64], 1)
        return z
    assert rel(no_flip(z), ref) > 1e-2


def test_flow64_layer_pieces_compose_on_ragged_batches(weights):
    """tail() with the next layer's pre, chained layer by layer on a ragged batch, equals flow_reverse; each utterance equals its own run (no row
    reads across an utterance edge) and the fp32 oracle's."""
    from stylish_tts_amd import synth

    lens = [1, 2, 17, 33, 5]
    w = weights["speech_predictor"]
    fws = F.flow_weights(w)
    z = synth.normal("flow64.z", (sum(lens), 128))
    st = (synth.normal("flow64.s", (len(lens), 64)) * 0.7).astype(np.float32)
    whole = F.flow_reverse(fws, z, st, lens)
    zz, h = np.array(z, np.float64), F.pre(fws[7], z, 1)
    for f in reversed(range(8)):
        gc = F.cond_columns(fws[f], st)
        out = None
        for i in range(3):
            h, out = F.wn_layer(fws[f], i, h, out, gc, lens)
        zz, h = F.tail(fws[f], fws[f - 1] if f else None, h, out, zz, gc, lens, f & 1)
    assert h is None and np.array_equal(zz, whole)
    lo = 0
    for u, L in enumerate(lens):
        one = F.flow_reverse(fws, z[lo : lo + L], st[u : u + 1], [L])
        assert np.abs(one - whole[lo : lo + L]).max() <= 1e-12 * np.abs(one).max()
        ora = O.flow_reverse(z[lo : lo + L].T[None], st[u : u + 1, :, None], w)[0].T
        assert rel(ora, one) < 2e-6, (u, L, rel(ora, one))
        lo += L
