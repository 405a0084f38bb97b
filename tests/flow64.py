"""Float64 restatement of the reverse flow (ResidualCouplingBlock.forward(reverse=True), models/flow.py:132-151; the coupling layer :196-218;
WN :63-88), usable one WaveNet layer at a time.  Test infrastructure: fp32 inputs in, every operation in float64.

Layout is the engine's: time-major rows [rows, C] packed utterance after utterance (`lengths` rows each), z [rows, 2 half].  The order of
csrc/flow.hip.h prior_flow_forward: coupling layers f = 7 .. 0, each preceded by a Flip, so layer f reads half p = f & 1 of z (through `pre`)
and updates the other half in place; after layer 0 the halves are in their natural order.  oracle/stylish_oracle.py flow_reverse is the
same computation in fp32 on [B, C, T] arrays.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
N_LAYERS, K = 4, 5


def weight_norm64(g, v):
    """torch weight_norm (dim 0) in float64: w = g v / ||v||, the norm over every dim but 0."""
    v = np.asarray(v, F64)
    nrm = np.sqrt((v ** 2).reshape(v.shape[0], -1).sum(1))
    return v * (np.asarray(g, F64).reshape(-1) / nrm).reshape((-1,) + (1,) * (v.ndim - 1))


def coupling_weights(w, f, p="flow."):
    """The float64 parameters of coupling layer f (flows.{2 f}): pre, the four WaveNet layers, cond_layer, proj_mean / proj_logstd."""
    q = p + f"flows.{2 * f}."
    e = q + "enc."
    d = lambda k: np.asarray(w[k], F64)  # noqa: E731
    return dict(
        pre=(d(q + "pre.weight"), d(q + "pre.bias")),
        inw=[(weight_norm64(w[e + f"in_layers.{i}.weight_g"], w[e + f"in_layers.{i}.weight_v"]), d(e + f"in_layers.{i}.bias")) for i in range(N_LAYERS)],
        rs=[(weight_norm64(w[e + f"res_skip_layers.{i}.weight_g"], w[e + f"res_skip_layers.{i}.weight_v"]), d(e + f"res_skip_layers.{i}.bias"))
            for i in range(N_LAYERS)],
        cond=(weight_norm64(w[e + "cond_layer.weight_g"], w[e + "cond_layer.weight_v"]), d(e + "cond_layer.bias")),
        proj_m=(d(q + "proj_mean.weight"), d(q + "proj_mean.bias")),
        proj_s=(d(q + "proj_logstd.weight"), d(q + "proj_logstd.bias")),
    )


def flow_weights(w, p="flow.", n_flows=8):
    return [coupling_weights(w, f, p) for f in range(n_flows)]


def linear(x, wb):
    wt, b = wb
    return np.asarray(x, F64) @ wt.reshape(wt.shape[0], -1).T + b


def cond_columns(cw, style):
    """cond_layer (a 1x1 conv of the style vector, one column per utterance) -> [n_utt, 2 H n_layers]; layer i reads [2 H i, 2 H (i + 1))."""
    return linear(style, cw["cond"])


def rows_of(lengths):
    """the utterance of every packed row."""
    return np.repeat(np.arange(len(lengths)), lengths)


def conv_same(h, wb, lengths, k=K):
    """'same' conv of kernel k per utterance (zero padding at every utterance edge) on packed rows h [rows, cin], w [cout, cin, k]."""
    wt, b = wb
    pad = (k - 1) // 2
    h = np.asarray(h, F64)
    out, lo = [], 0
    for L in lengths:
        xi = np.zeros((L + 2 * pad, h.shape[1]), F64)
        xi[pad : pad + L] = h[lo : lo + L]
        y = np.zeros((L, wt.shape[0]), F64)
        for t in range(k):
            y += xi[t : t + L] @ wt[:, :, t].T
        out.append(y + b)
        lo += L
    return np.concatenate(out)


def gate(a, hidden):
    """fused_add_tanh_sigmoid_multiply (flow.py:7-14)."""
    return np.tanh(a[:, :hidden]) / (1.0 + np.exp(-a[:, hidden:]))


def pre(cw, z, p):
    """h_0 = pre(z half p) (flow.py:199)."""
    half = z.shape[1] // 2
    return linear(np.asarray(z, F64)[:, p * half : (p + 1) * half], cw["pre"])


def wn_layer(cw, i, h, out, gc, lengths):
    """WaveNet layer i (flow.py:72-87): (h, out) -> (h', out').  gc = cond_columns(cw, style); `out` is ignored on layer 0 (it starts at 0).
    The last layer's res/skip has only the skip half: h' = h there."""
    hidden = cw["inw"][i][0].shape[1]
    a = conv_same(h, cw["inw"][i], lengths) + gc[rows_of(lengths), 2 * hidden * i : 2 * hidden * (i + 1)]
    rs = linear(gate(a, hidden), cw["rs"][i])
    h = np.asarray(h, F64)
    o = 0.0 if i == 0 else np.asarray(out, F64)
    if i < N_LAYERS - 1:
        return h + rs[:, :hidden], o + rs[:, hidden:]
    return h, o + rs


def coupling(cw, z, out, p):
    """proj_mean / proj_logstd of the finished `out` and the reverse coupling z1 = (z1 - m) exp(-ls) (flow.py:205-209) of the half p does not
    read; returns the whole z."""
    half = z.shape[1] // 2
    m, ls = linear(out, cw["proj_m"]), linear(out, cw["proj_s"])
    z = np.array(z, F64)
    q = (1 - p) * half
    z[:, q : q + half] = (z[:, q : q + half] - m) * np.exp(-ls)
    return z


def tail(cw, cw_next, h, out, z, gc, lengths, p):
    """The fused kernels' last launch of a coupling layer: the last WaveNet layer's res/skip, the projections, the coupling and the next coupling
    layer's `pre` (cw_next None: the last coupling layer).  h, out: after WaveNet layer 2.  Returns (z', h_0 of the next coupling layer or None)."""
    _, out = wn_layer(cw, N_LAYERS - 1, h, out, gc, lengths)
    z = coupling(cw, z, out, p)
    return z, (pre(cw_next, z, 1 - p) if cw_next is not None else None)


def flow_reverse(fws, z, style, lengths):
    """The whole reverse flow on packed rows z [rows, 2 half], style [n_utt, gin] -> z [rows, 2 half]."""
    z = np.array(z, F64)
    for f in reversed(range(len(fws))):
        p, cw = f & 1, fws[f]
        gc = cond_columns(cw, style)
        h, out = pre(cw, z, p), None
        for i in range(N_LAYERS - 1):
            h, out = wn_layer(cw, i, h, out, gc, lengths)
        z, _ = tail(cw, None, h, out, z, gc, lengths, p)
    return z
