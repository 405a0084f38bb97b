"""The posterior encoder (reference: train/models/flow.py:17-88, :234-293) restated in numpy float64, from given spectra, and a single
WaveNet layer of it.  Rows are time-major and packed: utterance u owns rows [off[u], off[u + 1]) and is its own sequence with zero
padding at its ends (the reference at B = 1, x_mask = 1).  ``mutant`` names one deliberate mistake (MUTANTS); tests/test_posterior_cpu.py
shows that each of them moves a tap past the GPU tests' bar, so those tests would catch it.
"""
from __future__ import annotations

import numpy as np

MUTANTS = ("neighbour_row", "last_like_rest", "cond_next", "cond_prev", "gate_swapped", "x0_swapped", "logstd_sign", "out_not_cleared", "last_frame_kept")

F64 = np.float64


def fold(sd, p):
    """The layer's effective weight in float64: weight_g * weight_v / ||weight_v|| (norm over all dims but 0; either weight-norm flavour), or .weight."""
    for g, v in ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1")):
        if p + g in sd:
            vv = np.asarray(sd[p + v], F64)
            n = np.sqrt((vv.reshape(vv.shape[0], -1) ** 2).sum(1)).reshape((-1,) + (1,) * (vv.ndim - 1))
            return np.asarray(sd[p + g], F64).reshape(n.shape) * vv / n
    return np.asarray(sd[p + ".weight"], F64)


class Weights:
    """Folded float64 weights of a PosteriorEncoder state_dict (keys without a prefix)."""

    def __init__(self, sd, dtype=F64):
        self.n_layers = sum(1 for k in sd if k.startswith("enc.in_layers.") and k.endswith(".bias"))
        c = lambda a: np.asarray(a, F64).astype(dtype)  # noqa: E731
        self.pre_spec, self.pre_phase = c(fold(sd, "pre_spec")[:, :, 0]), c(fold(sd, "pre_phase")[:, :, 0])
        self.b_spec, self.b_phase = c(sd["pre_spec.bias"]), c(sd["pre_phase.bias"])
        self.win = [c(fold(sd, f"enc.in_layers.{i}")) for i in range(self.n_layers)]  # [2H, H, k]
        self.bin = [c(sd[f"enc.in_layers.{i}.bias"]) for i in range(self.n_layers)]
        self.wrs = [c(fold(sd, f"enc.res_skip_layers.{i}")) for i in range(self.n_layers)]
        self.brs = [c(sd[f"enc.res_skip_layers.{i}.bias"]) for i in range(self.n_layers)]
        self.has_cond = "enc.cond_layer.bias" in sd
        if self.has_cond:
            self.wc, self.bc = c(fold(sd, "enc.cond_layer")), c(sd["enc.cond_layer.bias"])
        self.wm, self.bm = c(sd["proj_mean.weight"]), c(sd["proj_mean.bias"])
        self.wl, self.bl = c(sd["proj_logstd.weight"]), c(sd["proj_logstd.bias"])
        self.hidden = self.win[0].shape[1]


def cond_rows(W: Weights, style):
    """cond_layer(style) [n_utt, 2 H n_layers]; style None (g=None): zeros."""
    return style.astype(W.wc.dtype) @ W.wc.T + W.bc


def layer(W: Weights, i, h, out, cond, off, out_acc=None, mutant=None):
    """WaveNet layer i on packed rows: (h, out, cond [n_utt, 2 H L]) -> (h', out').  out_acc None: layer 0 starts `out`."""
    H, k = W.hidden, W.win[i].shape[2]
    pad = k // 2
    last = i == W.n_layers - 1 and mutant != "last_like_rest"
    acc = (i > 0 or mutant == "out_not_cleared") if out_acc is None else out_acc
    ci = i + 1 if mutant == "cond_next" else i - 1 if mutant == "cond_prev" else i
    ci = min(max(ci, 0), W.n_layers - 1)
    h2, out2 = h.copy(), (out.copy() if acc else np.zeros_like(out))
    for u in range(len(off) - 1):
        lo, hi = int(off[u]), int(off[u + 1])
        x = np.zeros((hi - lo + 2 * pad, H), h.dtype)
        x[pad : pad + hi - lo] = h[lo:hi]
        if mutant == "neighbour_row":  # the rows next to the utterance in the packed buffer instead of its zero padding
            for j in range(pad):
                if lo - 1 - j >= 0:
                    x[pad - 1 - j] = h[lo - 1 - j]
                if hi + j < h.shape[0]:
                    x[pad + hi - lo + j] = h[hi + j]
        xin = sum(x[j : j + hi - lo] @ W.win[i][:, :, j].T for j in range(k)) + W.bin[i]
        xin = xin + cond[u, ci * 2 * H : (ci + 1) * 2 * H]
        a, b = (xin[:, H:], xin[:, :H]) if mutant == "gate_swapped" else (xin[:, :H], xin[:, H:])
        acts = np.tanh(a) * (1.0 / (1.0 + np.exp(-b)))
        if last:
            out2[lo:hi] += acts @ W.wrs[i].T + W.brs[i]
        else:
            rs = acts @ W.wrs[i][: 2 * H].T + W.brs[i][: 2 * H] if W.wrs[i].shape[0] >= 2 * H else None
            if rs is None:  # (mutant last_like_rest on the last layer: it has H outputs only - treat them as res, skip gets nothing new)
                h2[lo:hi] += acts @ W.wrs[i].T + W.brs[i]
            else:
                h2[lo:hi] += rs[:, :H]
                out2[lo:hi] += rs[:, H:]
    return h2, out2


def forward(W: Weights, har_spec, har_phase, style, noise, off, mutant=None, post_flow=None):
    """The stage from spectra [rows, bins]: -> dict x0, wn, mean, logstd, z (and mel = post_flow(z) with post_flow = (weight, bias))."""
    dt = W.pre_spec.dtype
    spec, phase = np.asarray(har_spec).astype(dt), np.asarray(har_phase).astype(dt)
    xs, xp = spec @ W.pre_spec.T + W.b_spec, phase @ W.pre_phase.T + W.b_phase
    x0 = np.concatenate([xp, xs] if mutant == "x0_swapped" else [xs, xp], axis=1)
    n_utt = len(off) - 1
    cond = cond_rows(W, np.asarray(style)) if style is not None else np.zeros((n_utt, 2 * W.hidden * W.n_layers), dt)
    h, out = x0, np.full_like(x0, 0.37) if mutant == "out_not_cleared" else np.zeros_like(x0)
    for i in range(W.n_layers):
        h, out = layer(W, i, h, out, cond, off, mutant=mutant)
    mean, logstd = out @ W.wm.T + W.bm, out @ W.wl.T + W.bl
    z = mean + np.asarray(noise).astype(dt) * np.exp(-logstd if mutant == "logstd_sign" else logstd)
    o = dict(x0=x0, wn=out, mean=mean, logstd=logstd, z=z)
    if post_flow is not None:
        o["mel"] = z @ np.asarray(post_flow[0]).astype(dt).T + np.asarray(post_flow[1]).astype(dt)
    return o


def stft_frames(audio, n_fft, win, hop, frames):
    """torch.stft(center=True, reflect, periodic Hann(win) centred in n_fft) in float64: (|X|, atan2(Im, Re)) of the given frame indices, [len(frames), bins]."""
    x = np.pad(np.asarray(audio, F64), n_fft // 2, mode="reflect")
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo : lo + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    X = np.stack([np.fft.rfft(x[t * hop : t * hop + n_fft] * w) for t in frames])
    return np.abs(X), np.arctan2(X.imag, X.real)


def forward_last_frame_kept(W: Weights, har_spec, har_phase, audio, geom, style, noise, off):
    """The mutant that keeps the STFT's last frame: every utterance runs with one more row (its frame T, from the audio); -> the taps of rows [0, T)."""
    n_fft, win, hop = geom
    off = np.asarray(off)
    sp, ph, nz, off2 = [], [], [], [0]
    for u in range(len(off) - 1):
        lo, hi = int(off[u]), int(off[u + 1])
        m, p = stft_frames(audio[hop * lo : hop * hi], n_fft, win, hop, [hi - lo])
        sp += [har_spec[lo:hi], m]
        ph += [har_phase[lo:hi], p]
        nz += [noise[lo:hi], np.zeros((1, noise.shape[1]))]
        off2.append(off2[-1] + hi - lo + 1)
    o = forward(W, np.concatenate(sp), np.concatenate(ph), style, np.concatenate(nz), off2)
    keep = np.concatenate([np.arange(off2[u], off2[u + 1] - 1) for u in range(len(off) - 1)])
    return {k: v[keep] for k, v in o.items()}


def recording(seed, samples):
    """A synthetic recording: a few sinusoids plus noise at 0.1 (no STFT bin near zero magnitude), fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(samples) / 24000.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip(rng.uniform(0.05, 0.25, 4), rng.uniform(90.0, 5000.0, 4), rng.uniform(0, 6.28, 4)))
    return (x + 0.1 * rng.standard_normal(samples)).astype(np.float32)


def err(a, ref):
    """(max-abs, rms) of a - ref in float64."""
    d = np.asarray(a, F64) - np.asarray(ref, F64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))
