"""Exposed-operand parity of the reverse flow's split-fp32 WaveNet kernels (csrc/wn_fused_x3.hip.h): the operands, the per-element bound, and
the CPU twin that shows the bound rejects every named bug.  tests/test_hip_flow_x3_edges.py runs the GPU side on these very weights.

Exposed weights (exposed_flow): every in_layers gate channel reads ONE full-significand input channel at ONE tap (weight_v rows of +-1 with a
single nonzero, the full-significand value in weight_g: the folded weight norm is exact), cond_layer has zero weight and a full-significand bias
(the cond column is the bias, exactly), and res_skip, proj_mean / proj_logstd and `pre` have one weight per output.  So every output of a layer
is one product followed by a short chain of fp32 operations, and its error can be bounded element by element (layer_ref / tail_ref):
  1. the product: six of nine bf16 cross products + fp32 accumulation, 2^-21 |x w| (tests/test_split_fp32_cpu.py EXPOSED_REL);
  2. the gate: 1 - 2 rcp(exp2(2 a log2 e) + 1) and rcp(1 + exp2(-b log2 e)) have an ABSOLUTE error (relative precision is lost near 0, as
     intended): ET / ES allow 2^-20 plus the argument's rounding;
  3. the res/skip product and its additions, the projections;
  4. the coupling's __expf (exp2 of a rounded argument), EE.
Gate channels come in four classes (j mod 4 of the channel within its half): ordinary, pre-activations near 0, saturated (|a| > 20), ordinary;
proj_logstd puts ls across [-4, 4].
"""
from __future__ import annotations

import numpy as np

import flow64 as F
from test_split_fp32_cpu import F32, full_mantissa, mutants, split3, x3_sum

H, HALF, NL, TAPS = 128, 64, 4, 5
U = 2.0 ** -24
LENS = [1, 2, 15, 16, 17, 31, 33, 47, 49, 63, 65, 97, 130]  # the GPU test's batch (tests/test_hip_flow_x3_edges.py)
SEED = 4242


# ------------------------------------------------------------------------------------------------ operands
def _signed(rng, n, lo, hi):
    return full_mantissa(rng, n, lo, hi)


def exposed_coupling(f, seed=SEED):
    rng = np.random.default_rng(seed + f)
    n = np.arange(2 * H) % H
    cls = n % 4  # 0 / 3 ordinary, 1 near 0, 2 saturated
    E = dict(pre_c=(37 * np.arange(H) + 5) % HALF, pre_w=_signed(rng, H, -1, 0), pre_b=_signed(rng, H, -4, -3), inl=[], rs=[])
    for i in range(NL):
        g = np.where(cls == 1, _signed(rng, 2 * H, -14, -12), np.where(cls == 2, _signed(rng, 2 * H, 5, 6), _signed(rng, 2 * H, -2, 0)))
        b = np.where(cls == 1, _signed(rng, 2 * H, -17, -15), _signed(rng, 2 * H, -6, -4))
        cb = np.where(cls == 1, _signed(rng, 2 * H, -17, -15), _signed(rng, 2 * H, -6, -4))
        sign = np.where(rng.integers(0, 2, 2 * H) == 0, -1, 1).astype(F32)
        E["inl"].append(dict(pi=(37 * np.arange(2 * H) + 5 + 11 * i) % H, tau=(np.arange(2 * H) + i) % TAPS, sign=sign, g=g.astype(F32),
                             w=(sign * g).astype(F32), b=b.astype(F32), cb=cb.astype(F32)))
        N = 2 * H if i < NL - 1 else H
        s2 = np.where(rng.integers(0, 2, N) == 0, -1, 1).astype(F32)
        g2 = _signed(rng, N, -1, 0)
        E["rs"].append(dict(q=(41 * np.arange(N) + 3 + 7 * i) % H, sign=s2, g=g2, w=(s2 * g2).astype(F32), b=_signed(rng, N, -6, -4)))
    E["m_c"], E["m_w"], E["m_b"] = (29 * np.arange(HALF) + 1) % H, _signed(rng, HALF, -1, 0), _signed(rng, HALF, -6, -4)
    E["s_c"], E["s_w"], E["s_b"] = (29 * np.arange(HALF) + 2) % H, _signed(rng, HALF, -3, -2), _signed(rng, HALF, 0, 1)
    return E


def exposed_flow(seed=SEED):
    return [exposed_coupling(f, seed) for f in range(8)]


def exposed_weights(base, E, p="flow."):
    """base (the name-keyed speech_predictor weights) with every flow.* tensor replaced by the exposed layout of E."""
    w = dict(base)
    for f, e in enumerate(E):
        q = p + f"flows.{2 * f}."
        pre = np.zeros((H, HALF), F32)
        pre[np.arange(H), e["pre_c"]] = e["pre_w"]
        w[q + "pre.weight"], w[q + "pre.bias"] = pre, e["pre_b"]
        for i in range(NL):
            L = e["inl"][i]
            v = np.zeros((2 * H, H, TAPS), F32)
            v[np.arange(2 * H), L["pi"], L["tau"]] = L["sign"]
            w[q + f"enc.in_layers.{i}.weight_v"], w[q + f"enc.in_layers.{i}.weight_g"] = v, L["g"].reshape(-1, 1, 1)
            w[q + f"enc.in_layers.{i}.bias"] = L["b"]
            R = e["rs"][i]
            v2 = np.zeros((len(R["q"]), H), F32)
            v2[np.arange(len(R["q"])), R["q"]] = R["sign"]
            w[q + f"enc.res_skip_layers.{i}.weight_v"], w[q + f"enc.res_skip_layers.{i}.weight_g"] = v2, R["g"].reshape(-1, 1)
            w[q + f"enc.res_skip_layers.{i}.bias"] = R["b"]
        gshape = base[q + "enc.cond_layer.weight_g"].shape
        w[q + "enc.cond_layer.weight_g"] = np.zeros(gshape, F32)
        w[q + "enc.cond_layer.weight_v"] = np.ones(base[q + "enc.cond_layer.weight_v"].shape, F32)
        w[q + "enc.cond_layer.bias"] = np.concatenate([e["inl"][i]["cb"] for i in range(NL)])
        for k, c, wt, b in (("proj_mean", "m_c", "m_w", "m_b"), ("proj_logstd", "s_c", "s_w", "s_b")):
            m = np.zeros((HALF, H), F32)
            m[np.arange(HALF), e[c]] = e[wt]
            w[q + k + ".weight"], w[q + k + ".bias"] = m, e[b]
    return w


def gather_rows(x, lens, off, cols, neighbour=False):
    """x[row + off_j, cols_j] per output j, 0 outside the row's utterance (the conv's zero padding); neighbour: the packed row instead (a halo row
    taken from the next / previous utterance)."""
    R = x.shape[0]
    starts = np.repeat(np.cumsum([0] + list(lens[:-1])), lens)
    ends = starts + np.repeat(lens, lens)
    r = np.arange(R)[:, None] + off[None, :]
    ok = (r >= 0) & (r < R) if neighbour else (r >= starts[:, None]) & (r < ends[:, None])
    return np.where(ok, x[np.clip(r, 0, R - 1), cols[None, :]], F32(0)).astype(F32)


def edge_inputs():
    """the GPU test's prior inputs: decoder-like rows x [rows, 512], style [n_utt, 64], prior noise [rows, 128]."""
    from stylish_tts_amd import synth

    rows = sum(LENS)
    return (synth.normal("wnx.x", (rows, 512)), (synth.normal("wnx.s", (len(LENS), 64)) * 0.7).astype(F32), synth.normal("wnx.n", (rows, H)))


# ------------------------------------------------------------------------------------------------ float64 reference + per-element bound
def _gate_ref(a):
    with np.errstate(over="ignore"):
        return np.tanh(a[:, :H]), 1.0 / (1.0 + np.exp(-a[:, H:]))


def ET(a, t):
    return 2.0 ** -20 * (1.0 + np.abs(a) * (1.0 - t * t))


def ES(b, s):
    return 2.0 ** -20 * (1.0 + np.abs(b) * (1.0 - s))


def EE(ls):
    return 2.0 ** -21 + 2.0 ** -22 * np.abs(ls)


def layer_ref(e, i, h, out, lens):
    """float64 WaveNet layer i on fp32 inputs and the bound of every output: (h', dh', out', dout') (i = 3: h' is None)."""
    L, R_ = e["inl"][i], e["rs"][i]
    x = gather_rows(np.asarray(h, F32), lens, L["tau"] - 2, L["pi"]).astype(np.float64)
    p = x * L["w"]
    a = p + L["b"] + L["cb"]
    da = 2.0 ** -21 * np.abs(p) + U * (np.abs(p + L["b"]) + np.abs(a))
    t, s = _gate_ref(a)
    act = t * s
    dact = s * ((1 - t * t) * da[:, :H] + ET(a[:, :H], t)) + np.abs(t) * s * ((1 - s) * da[:, H:] + ES(a[:, H:], s)) + U * np.abs(act)
    ag, dag = act[:, R_["q"]], dact[:, R_["q"]]
    pr = ag * R_["w"]
    rs = pr + R_["b"]
    drs = np.abs(R_["w"]) * dag + 2.0 ** -21 * np.abs(pr) + U * np.abs(rs)
    o = 0.0 if i == 0 else np.asarray(out, np.float64)
    if i < NL - 1:
        h2, o2 = np.asarray(h, np.float64) + rs[:, :H], o + rs[:, H:]
        return h2, drs[:, :H] + U * np.abs(h2) + 1e-38, o2, drs[:, H:] + U * np.abs(o2) + 1e-38, a
    o2 = o + rs
    return None, None, o2, drs + U * np.abs(o2) + 1e-38, a


def pre_ref(e, z, p, dz=0.0):
    zc = np.asarray(z, np.float64)[:, p * HALF : (p + 1) * HALF][:, e["pre_c"]]
    dzc = (dz[:, e["pre_c"]] if np.ndim(dz) else 0.0)
    pr = zc * e["pre_w"]
    h0 = pr + e["pre_b"]
    return h0, np.abs(e["pre_w"]) * dzc + 2.0 ** -21 * np.abs(pr) + U * np.abs(h0) + 1e-38


def tail_ref(e, h, out, z, p, lens):
    """The last WaveNet layer, the projections and the coupling: (z' half updated, its bound, ls)."""
    _, _, o, do, _ = layer_ref(e, NL - 1, h, out, lens)
    pm, ps = o[:, e["m_c"]] * e["m_w"], o[:, e["s_c"]] * e["s_w"]
    m, ls = pm + e["m_b"], ps + e["s_b"]
    dm = np.abs(e["m_w"]) * do[:, e["m_c"]] + 2.0 ** -21 * np.abs(pm) + U * np.abs(m)
    dls = np.abs(e["s_w"]) * do[:, e["s_c"]] + 2.0 ** -21 * np.abs(ps) + U * np.abs(ls)
    q = (1 - p) * HALF
    z1 = np.asarray(z, np.float64)[:, q : q + HALF]
    zn = (z1 - m) * np.exp(-ls)
    dz = np.exp(-ls) * (dm + U * np.abs(z1 - m)) + np.abs(zn) * (dls + EE(ls)) + U * np.abs(zn) + 1e-38
    return zn, dz, ls


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernel, and its mutants
LAYER_MUTANTS = ([f"conv: {m}" for m in ("drop x2w0", "drop x0w2", "drop x1w1", "drop x1w0", "drop x0w1", "drop x0w0", "x planes 1 / 2 swapped",
                                         "x planes 0 / 1 swapped", "w planes 1 / 2 swapped", "x term 0 truncated", "x term 1 truncated",
                                         "w term 0 truncated", "w term 1 truncated", "x plane 1 from the next channel",
                                         "x plane 2 from the next channel", "w plane 1 from the next channel", "w plane 2 from the next channel")]
                 + [f"res/skip: {m}" for m in ("drop x2w0", "drop x0w2", "drop x1w1", "drop x1w0", "drop x0w1", "drop x0w0", "x planes 1 / 2 swapped",
                                               "x term 0 truncated", "x term 1 truncated", "w term 0 truncated", "w term 1 truncated")]
                 + ["halo row from the neighbouring utterance", "tap off by one", "tanh and sigmoid halves swapped", "cond column of the next layer",
                    "in_layers bias added twice", "out accumulated on layer 0"])
TAIL_MUTANTS = ["m and ls swapped", "exp(+ls)", "pre reads the wrong half"]


def _x3(x, w, xn, mut):
    """six-product sums of x w (elementwise), or the named mutant (tests/test_split_fp32_cpu.py mutants)."""
    x, w = np.asarray(x, F32), np.broadcast_to(np.asarray(w, F32), np.shape(x)).astype(F32)
    if mut is None:
        return x3_sum(split3(x), split3(w))
    return mutants(x, w, np.asarray(xn, F32))[mut]


def f32(v):
    return np.asarray(v, F32)


def emulate_layer(e, i, h, out, lens, mut=None, e_cond=None):
    """fp32 emulation of wn_fused_x3_kernel's arithmetic for WaveNet layer i: (h', out')."""
    L, R_ = e["inl"][i], e["rs"][i]
    h = f32(h)
    tau = L["tau"] + (1 if mut == "tap off by one" else 0)
    x = gather_rows(h, lens, tau - 2, L["pi"], neighbour=mut == "halo row from the neighbouring utterance")
    xn = gather_rows(np.concatenate([h, h[:, :1]], 1), lens, tau - 2, L["pi"] + 1)
    conv_mut = mut[len("conv: "):] if mut and mut.startswith("conv: ") else None
    acc = _x3(x, L["w"], xn, conv_mut)
    cb = e_cond["inl"][(i + 1) % NL]["cb"] if mut == "cond column of the next layer" else L["cb"]
    va = f32(acc + L["b"])
    if mut == "in_layers bias added twice":
        va = f32(va + L["b"])
    va = f32(va + cb)
    a, b = va[:, :H], va[:, H:]
    if mut == "tanh and sigmoid halves swapped":
        a, b = b, a
    with np.errstate(over="ignore"):
        th = f32(F32(1) - F32(2) * f32(F32(1) / f32(np.exp2(f32(F32(2.885390082) * a)) + F32(1))))
        sg = f32(F32(1) / f32(F32(1) + np.exp2(f32(F32(-1.442695041) * b))))
    act = f32(th * sg)
    ag = act[:, R_["q"]]
    agn = np.concatenate([act, act[:, :1]], 1)[:, R_["q"] + 1]
    rs_mut = mut[len("res/skip: "):] if mut and mut.startswith("res/skip: ") else None
    rs = f32(_x3(ag, R_["w"], agn, rs_mut) + R_["b"])
    if i == 0:
        o = f32(out) if mut == "out accumulated on layer 0" else np.zeros((h.shape[0], rs.shape[1] - (H if i < NL - 1 else 0)), F32)
    else:
        o = f32(out)
    if i < NL - 1:
        return f32(h + rs[:, :H]), f32(o + rs[:, H:])
    return None, f32(o + rs)


def emulate_pre(e, z, p):
    zc = f32(z)[:, p * HALF : (p + 1) * HALF][:, e["pre_c"]]
    return f32(_x3(zc, e["pre_w"], zc, None) + e["pre_b"])


def emulate_tail(e, e_next, h, out, z, p, lens, mut=None):
    """the last WaveNet layer + proj + coupling (+ the next coupling layer's pre): (z', h_0 next, out final)."""
    _, o = emulate_layer(e, NL - 1, h, out, lens)
    m = f32(_x3(o[:, e["m_c"]], e["m_w"], o[:, e["m_c"]], None) + e["m_b"])
    ls = f32(_x3(o[:, e["s_c"]], e["s_w"], o[:, e["s_c"]], None) + e["s_b"])
    if mut == "m and ls swapped":
        m, ls = ls, m
    q = (1 - p) * HALF
    z = f32(z).copy()
    with np.errstate(over="ignore"):
        ex = f32(np.exp(ls if mut == "exp(+ls)" else -ls))
    z[:, q : q + HALF] = f32(f32(z[:, q : q + HALF] - m) * ex)
    h0 = emulate_pre(e_next, z, p if mut == "pre reads the wrong half" else 1 - p) if e_next is not None else None
    return z, h0, o


def worst(y, ref, bound):
    return float((np.abs(np.asarray(y, np.float64) - ref) / bound).max())


# ------------------------------------------------------------------------------------------------ the CPU twin
def twin_operands(base):
    """The GPU test's operands up to coupling layer 6's first WaveNet layer, emulated: the prior's z (fp32 of float64, from the GPU test's inputs),
    then the correct emulation of coupling layer 7."""
    E = exposed_flow()
    x, st, nz = edge_inputs()
    mean = x.astype(np.float64) @ np.asarray(base["prior_encoder.proj_mean.weight"], np.float64).T + base["prior_encoder.proj_mean.bias"]
    lstd = x.astype(np.float64) @ np.asarray(base["prior_encoder.proj_logstd.weight"], np.float64).T + base["prior_encoder.proj_logstd.bias"]
    z = f32(mean + nz * np.exp(lstd))
    h = emulate_pre(E[7], z, 1)
    hs, outs = [h], [None]
    out = None
    for i in range(NL - 1):
        h, out = emulate_layer(E[7], i, h, out, LENS)
        hs.append(h)
        outs.append(out)
    z6, h6, out7 = emulate_tail(E[7], E[6], h, out, z, 1, LENS)
    return E, z, hs, outs, z6, h6, out7


def test_exposed_layout_is_what_the_bound_assumes(weights):
    """The folded weight norm of the exposed weights is the exact signed value; cond_layer folds to zero; the gate classes and ls are where the
    docstring puts them."""
    E = exposed_flow()
    w = exposed_weights(weights["speech_predictor"], E)
    for f in (0, 7):
        cw = F.coupling_weights(w, f)
        for i in range(NL):
            wt = cw["inw"][i][0]
            assert np.array_equal(wt[np.arange(2 * H), E[f]["inl"][i]["pi"], E[f]["inl"][i]["tau"]], E[f]["inl"][i]["w"].astype(np.float64))
            assert np.count_nonzero(wt) == 2 * H
            assert np.array_equal(cw["rs"][i][0][np.arange(len(E[f]["rs"][i]["q"])), E[f]["rs"][i]["q"]], E[f]["rs"][i]["w"].astype(np.float64))
        assert not cw["cond"][0].any()
        # the engine folds in fp32: g * (v / ||v||) with ||v|| = 1 exactly
        g, v = w[f"flow.flows.{2 * f}.enc.in_layers.0.weight_g"], w[f"flow.flows.{2 * f}.enc.in_layers.0.weight_v"]
        nrm = np.sqrt((v.astype(np.float64) ** 2).reshape(v.shape[0], -1).sum(1)).astype(F32)
        assert (nrm == 1).all()


def test_the_flow_bound_rejects_every_mutant(weights):
    """On the GPU test's weights and inputs (emulated layer inputs): the correct fp32 emulation of wn_fused_x3_kernel passes the per-element bound
    of layer_ref / tail_ref / pre_ref, and every named mutant fails it somewhere."""
    base = weights["speech_predictor"]
    E, z, hs, outs, z6, h6, out7 = twin_operands(base)
    # one WaveNet layer: coupling layer 6's first (its `out` buffer still holds coupling layer 7's final `out`: the layer-0 accumulate mutant reads it)
    h2, dh2, o2, do2, a = layer_ref(E[6], 0, h6, None, LENS)
    assert (np.abs(a) < 1e-3).sum() > 100 and (np.abs(a) > 20).sum() > 100, "gate pre-activations near 0 and in saturation"
    hc, oc = emulate_layer(E[6], 0, h6, out7, LENS)
    assert worst(hc, h2, dh2) <= 1 and worst(oc, o2, do2) <= 1
    # and the middle layers of coupling layer 7 (out accumulated)
    for i in (1, 2):
        r = layer_ref(E[7], i, hs[i], outs[i], LENS)
        y = emulate_layer(E[7], i, hs[i], outs[i], LENS)
        assert worst(y[0], r[0], r[1]) <= 1 and worst(y[1], r[2], r[3]) <= 1, i
    missed = []
    for mut in LAYER_MUTANTS:
        hm, om = emulate_layer(E[6], 0, h6, out7, LENS, mut=mut, e_cond=E[6])
        if max(worst(hm, h2, dh2), worst(om, o2, do2)) <= 1:
            missed.append(mut)
    # one tail: coupling layer 7's (z and the next h_0)
    zr, dz, ls = tail_ref(E[7], hs[3], outs[3], z, 1, LENS)
    assert ls.min() < -3 and ls.max() > 3 and np.abs(ls).max() < 8, (ls.min(), ls.max())
    assert worst(z6[:, :HALF], zr, dz) <= 1
    assert np.array_equal(z6[:, HALF:], z[:, HALF:])
    h0r, dh0 = pre_ref(E[6], z6, 0)
    assert worst(h6, h0r, dh0) <= 1
    for mut in TAIL_MUTANTS:
        zm, hm, _ = emulate_tail(E[7], E[6], hs[3], outs[3], z, 1, LENS, mut=mut)
        if max(worst(zm[:, :HALF], zr, dz), worst(hm, *pre_ref(E[6], zm, 0))) <= 1:
            missed.append(mut)
    assert not missed, f"mutants the bound does not reject: {missed}"
    assert len(LAYER_MUTANTS) + len(TAIL_MUTANTS) == 37
