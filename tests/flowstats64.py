"""Float64 restatement of the flow statistics: ResidualCouplingBlock.forward in both directions with the three streams z / mean / logstd
(models/flow.py:132-151, the coupling layer :196-218, WN :63-88), PriorEncoder.forward (:311-315) and the two KL formulas of
train/losses.py:157-202.  Test infrastructure: fp32 inputs in, every operation in float64.  The WaveNet pieces are tests/flow64.py's
(pre, wn_layer, cond_columns); layout is the engine's: time-major rows [rows, C] packed utterance after utterance.

reverse = False: layers 0 .. 7, each followed by a Flip; reverse = True: Flip, layer 7, ..., Flip, layer 0.  In both orders layer f reads half
p = f & 1 of z (through `pre`) and updates the other half of all three streams; after eight layers the halves are in their natural order.

`mut` names one deliberate mistake (tests/test_flowstats_cpu.py shows that each moves a tap past the GPU tests' bar); None = the real thing.
"""
from __future__ import annotations

import numpy as np

import flow64 as F

F64 = np.float64
MUTANTS = ("forward_on_reverse", "mean_no_exp", "logstd_sign", "layer_order", "halves_swapped", "neighbour_rows", "halo_1", "cond_next_layer",
           "pre_wrong_next", "kl_mask_per_channel")


def err(a, b):
    """(max-abs, rms) of a - b."""
    d = np.asarray(a, F64) - np.asarray(b, F64)
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


def _conv_mut(h, wb, lengths, mut, block=16):
    """flow64.conv_same with one of the two padding mistakes a blocked kernel can make: `neighbour_rows` reads the packed neighbours where an
    utterance's zero padding belongs; `halo_1` gives every block of `block` rows one halo row each side where k = 5 needs two."""
    wt, b = wb
    h = np.asarray(h, F64)
    R = h.shape[0]
    y = np.zeros((R, wt.shape[0]), F64)
    lo = 0
    for L in lengths:
        for t in range(L):
            b0 = t // block * block
            for k in range(5):
                src = t + k - 2
                if mut == "neighbour_rows":
                    ok = 0 <= lo + src < R
                else:  # halo_1
                    ok = 0 <= src < L and b0 - 1 <= src < b0 + block + 1
                if ok:
                    y[lo + t] += wt[:, :, k] @ h[lo + src]
        lo += L
    return y + b


def wn(cw, h, gc, lengths, mut=None):
    """The four WaveNet layers from h_0 -> the finished `out`."""
    out = None
    for i in range(F.N_LAYERS):
        if mut in ("neighbour_rows", "halo_1"):
            hidden = cw["inw"][i][0].shape[1]
            a = _conv_mut(h, cw["inw"][i], lengths, mut) + gc[F.rows_of(lengths), 2 * hidden * i : 2 * hidden * (i + 1)]
            rs = F.linear(F.gate(a, hidden), cw["rs"][i])
            o = 0.0 if i == 0 else out
            h, out = (h + rs[:, :hidden], o + rs[:, hidden:]) if i < F.N_LAYERS - 1 else (h, o + rs)
        elif mut == "cond_next_layer":
            j = (i + 1) % F.N_LAYERS
            hidden = cw["inw"][i][0].shape[1]
            shifted = np.array(gc)
            shifted[:, 2 * hidden * i : 2 * hidden * (i + 1)] = gc[:, 2 * hidden * j : 2 * hidden * (j + 1)]
            h, out = F.wn_layer(cw, i, h, out, shifted, lengths)
        else:
            h, out = F.wn_layer(cw, i, h, out, gc, lengths)
    return out


def coupling_layer(cw, z, mean, logstd, style, lengths, f, reverse, mut=None):
    """Coupling layer f on the three streams -> (z, mean, logstd): the half f & 1 is read, the other updated (flow.py:196-218)."""
    z, mean, logstd = (np.array(a, F64) for a in (z, mean, logstd))
    half = z.shape[1] // 2
    p = f & 1
    if mut == "halves_swapped":
        p = 1 - p
    out = wn(cw, F.pre(cw, z, p), F.cond_columns(cw, style), lengths, mut)
    m, s = F.linear(out, cw["proj_m"]), F.linear(out, cw["proj_s"])
    q = slice((1 - p) * half, (2 - p) * half)
    fwd = not reverse or mut == "forward_on_reverse"
    sgn = -1.0 if mut == "logstd_sign" else 1.0
    if fwd:
        z[:, q] = m + z[:, q] * np.exp(s)
        mean[:, q] = m + mean[:, q] * (1.0 if mut == "mean_no_exp" else np.exp(s))
        logstd[:, q] = logstd[:, q] + sgn * s
    else:
        z[:, q] = (z[:, q] - m) * np.exp(-s)
        mean[:, q] = (mean[:, q] - m) * (1.0 if mut == "mean_no_exp" else np.exp(-s))
        logstd[:, q] = logstd[:, q] - sgn * s
    return z, mean, logstd


def next_layer(f, reverse):
    """The coupling layer that runs after f in the call's order (None after the last)."""
    n = f - 1 if reverse else f + 1
    return n if 0 <= n < 8 else None


def layer_with_next(fws, f, z, mean, logstd, style, lengths, reverse, mut=None):
    """What a fused form's four launches of coupling layer f leave: the three streams and the next coupling layer's h_0 (None after the last)."""
    z, mean, logstd = coupling_layer(fws[f], z, mean, logstd, style, lengths, f, reverse, mut)
    n = next_layer(f, reverse)
    if n is None:
        return z, mean, logstd, None
    if mut == "pre_wrong_next":
        return z, mean, logstd, F.pre(fws[(n + 2) % 8], z, n & 1)
    return z, mean, logstd, F.pre(fws[n], z, n & 1)


def flow(fws, z, mean, logstd, style, lengths, reverse, mut=None):
    """The whole block on packed rows [rows, 2 half], style [n_utt, gin] -> (z, mean, logstd)."""
    order = list(range(len(fws)))
    if reverse != (mut == "layer_order"):
        order.reverse()
    for f in order:
        z, mean, logstd = coupling_layer(fws[f], z, mean, logstd, style, lengths, f, reverse, mut)
    return z, mean, logstd


def prior(w, x, noise, p="prior_encoder."):
    """PriorEncoder.forward: x [rows, in] -> (z, mean, logstd), z = mean + noise exp(logstd)."""
    d = lambda k: np.asarray(w[k], F64)  # noqa: E731
    mean = F.linear(x, (d(p + "proj_mean.weight"), d(p + "proj_mean.bias")))
    logstd = F.linear(x, (d(p + "proj_logstd.weight"), d(p + "proj_logstd.bias")))
    return mean + np.asarray(noise, F64) * np.exp(logstd), mean, logstd


def kl_pieces(kind, a, b, c, d):
    """The additive pieces of the per-element KL term: (d - b - 0.5, 0.5 var exp(-2 d)); kind 0 = kl_loss (a = z_p: var = (a - c)^2), kind 1 =
    kl_loss_normal (a = m_q: var = exp(2 b) + (a - c)^2); b = logs_q, c = m_p, d = logs_p (losses.py:174-175, :198-199)."""
    a, b, c, d = (np.asarray(v, F64) for v in (a, b, c, d))
    var = (a - c) ** 2 + (np.exp(2.0 * b) if kind == 1 else 0.0)
    return d - b - 0.5, 0.5 * var * np.exp(-2.0 * d)


def kl_sums(kind, a, b, c, d, off):
    """Per-utterance sums over rows and channels -> [n_utt]."""
    p0, p1 = kl_pieces(kind, a, b, c, d)
    t = (p0 + p1).sum(1)
    return np.array([t[off[u] : off[u + 1]].sum() for u in range(len(off) - 1)], F64)


def kl_score(kind, a, b, c, d, mut=None):
    """The reference's score: sum / sum(z_mask); the mask [B, 1, T] sums to the rows, not rows x channels."""
    p0, p1 = kl_pieces(kind, a, b, c, d)
    n = p0.size if mut == "kl_mask_per_channel" else p0.shape[0]
    return float((p0 + p1).sum() / n)
