"""Shared by tests/test_flowstats_cpu.py and tests/test_hip_flow_stats.py: the fixtures of tests/golden/gen_golden_flowstats.py, and the cases of one
coupling layer alone - inputs, the float64 reference (tests/flowstats64.py) and the error of the same layer computed in fp32 by torch on the CPU from
the same inputs - computed once per (batch, layer, direction) and left unchanged."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
import flow64 as F  # noqa: E402
import flowstats64 as S  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0  # the project's standing margin over the reference's own fp32 rounding
STREAMS = ("z", "mean", "logstd")
# crosses every block height (16 / 32 / 64) and the k = 5 conv's two halo rows; the second batch is 40 one-row utterances
BATCHES = {"ragged": [1, 2, 3, 15, 16, 17, 31, 33, 47, 64, 66, 130], "ones": [1] * 40}

_S = {}


def weights(cfg):
    """(the speech predictor's synthetic state dict, seed 0; its eight coupling layers in float64)."""
    if "w" not in _S:
        from stylish_tts_amd import params

        _S["w"] = params.synth_state_dict(params.speech_predictor_spec(cfg), 0, prefix="speech_predictor.")
        _S["fws"] = F.flow_weights(_S["w"])
    return _S["w"], _S["fws"]


def fixture():
    if "gold" not in _S:
        g = {}
        for part in ("in", "fwd", "rev", "prior"):
            g.update(np.load(os.path.join(GOLD, f"flowstats_{part}.npz")))
        for v in g.values():
            v.setflags(write=False)
        _S["gold"] = g
    return _S["gold"]


def draw(rng, lengths, fh=128, gin=64):
    """Inputs with the fixture's distributions: mean = 0.5 N, logstd = 0.3 N - 0.5, z = mean + N exp(logstd), style = 0.5 N (fp32)."""
    R = int(sum(lengths))
    mean = (0.5 * rng.standard_normal((R, fh))).astype(np.float32)
    logstd = (0.3 * rng.standard_normal((R, fh)) - 0.5).astype(np.float32)
    z = (mean.astype(np.float64) + rng.standard_normal((R, fh)) * np.exp(logstd.astype(np.float64))).astype(np.float32)
    style = (0.5 * rng.standard_normal((len(lengths), gin))).astype(np.float32)
    return z, mean, logstd, style


def layer_torch32(w, f, z, mean, logstd, style, lengths, reverse):
    """Coupling layer f in fp32 by torch on the CPU, per utterance at B = 1 as the reference runs it (weight_norm folded in fp32 as torch does)
    -> (z, mean, logstd, the next coupling layer's h_0 or None)."""
    Fn = torch.nn.functional
    t = lambda k: torch.from_numpy(np.asarray(w[k], np.float32))  # noqa: E731
    wn = lambda p: torch._weight_norm(t(p + ".weight_v"), t(p + ".weight_g"), 0)  # noqa: E731
    q = f"flow.flows.{2 * f}."
    half = z.shape[1] // 2
    p = f & 1
    cs = slice((1 - p) * half, (2 - p) * half)
    outs = [torch.from_numpy(a.copy()) for a in (z, mean, logstd)]
    zin = torch.from_numpy(z)
    cond_w = wn(q + "enc.cond_layer")
    H = 2 * half
    lo = 0
    with torch.no_grad():
        for u, L in enumerate(lengths):
            rows = slice(lo, lo + L)
            h = Fn.linear(zin[rows, p * half : (p + 1) * half], t(q + "pre.weight"), t(q + "pre.bias")).T[None]
            g = Fn.linear(torch.from_numpy(style[u]), cond_w.reshape(cond_w.shape[0], -1), t(q + "enc.cond_layer.bias"))
            out = torch.zeros_like(h)
            for i in range(4):
                xin = Fn.conv1d(h, wn(q + f"enc.in_layers.{i}"), t(q + f"enc.in_layers.{i}.bias"), padding=2) + g[i * 2 * H : (i + 1) * 2 * H][None, :, None]
                acts = torch.tanh(xin[:, :H]) * torch.sigmoid(xin[:, H:])
                rs = Fn.linear(acts.mT, wn(q + f"enc.res_skip_layers.{i}"), t(q + f"enc.res_skip_layers.{i}.bias")).mT
                if i < 3:
                    h = h + rs[:, :H]
                    out = out + rs[:, H:]
                else:
                    out = out + rs
            m = Fn.linear(out.mT, t(q + "proj_mean.weight"), t(q + "proj_mean.bias"))[0]
            s = Fn.linear(out.mT, t(q + "proj_logstd.weight"), t(q + "proj_logstd.bias"))[0]
            if reverse:
                outs[0][rows, cs] = (outs[0][rows, cs] - m) * torch.exp(-s)
                outs[1][rows, cs] = (outs[1][rows, cs] - m) * torch.exp(-s)
                outs[2][rows, cs] = outs[2][rows, cs] - s
            else:
                outs[0][rows, cs] = m + outs[0][rows, cs] * torch.exp(s)
                outs[1][rows, cs] = m + outs[1][rows, cs] * torch.exp(s)
                outs[2][rows, cs] = outs[2][rows, cs] + s
            lo += L
        n = S.next_layer(f, reverse)
        h0 = None
        if n is not None:
            qn = f"flow.flows.{2 * n}."
            h0 = Fn.linear(outs[0][:, (n & 1) * half : ((n & 1) + 1) * half], t(qn + "pre.weight"), t(qn + "pre.bias")).numpy()
    return outs[0].numpy(), outs[1].numpy(), outs[2].numpy(), h0


def layer_case(cfg, batch, f, reverse):
    """-> dict: lengths, the fp32 inputs, ref = (z, mean, logstd, h0) in float64, err = {tap: (max-abs, rms) of torch fp32}."""
    key = ("layer", batch, f, bool(reverse))
    if key not in _S:
        w, fws = weights(cfg)
        lengths = BATCHES[batch]
        z, mean, logstd, style = draw(np.random.default_rng(2000 + 31 * f + 7 * int(reverse) + len(lengths)), lengths)
        ref = S.layer_with_next(fws, f, z, mean, logstd, style, lengths, reverse)
        t32 = layer_torch32(w, f, z, mean, logstd, style, lengths, reverse)
        half = z.shape[1] // 2
        cs = slice((1 - (f & 1)) * half, (2 - (f & 1)) * half)
        err = {k: S.err(t32[j][:, cs], ref[j][:, cs]) for j, k in enumerate(STREAMS)}
        if ref[3] is not None:
            err["h0"] = S.err(t32[3], ref[3])
        c = dict(lengths=lengths, z=z, mean=mean, logstd=logstd, style=style, ref=ref, err=err, coupled=cs)
        for v in (z, mean, logstd, style) + tuple(a for a in ref if a is not None):
            v.setflags(write=False)
        _S[key] = c
    return _S[key]


def layer_worst_ratio(c, got):
    """Worst ratio (max-abs and rms) of got = (z, mean, logstd[, h0]) over the case's torch-fp32 error, on the coupled half and h0; prints each."""
    worst = 0.0
    cs = c["coupled"]
    for j, k in enumerate(STREAMS + ("h0",)):
        if j >= len(got) or got[j] is None or k not in c["err"]:
            continue
        a, b = (got[j], c["ref"][j]) if k == "h0" else (got[j][:, cs], c["ref"][j][:, cs])
        emax, erms = S.err(a, b)
        rmax, rrms = c["err"][k]
        print(f"    {k:6s}: max {emax:.2e} rms {erms:.2e} | torch fp32 max {rmax:.2e} rms {rrms:.2e} | ratio {emax / rmax:.2f} {erms / rrms:.2f}")
        worst = max(worst, emax / rmax, erms / rrms)
    return worst
