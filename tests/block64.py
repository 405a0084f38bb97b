"""Float64 restatement of the AdaptiveDecoderBlock, the bounds the HIP block forms are held to, and the cases both tests/test_block64_cpu.py (numpy
models, no GPU) and tests/test_hip_block_forms.py (the forms of csrc/adain_block.hip.h through stts_op_adain_chain) run.  Test infrastructure.

The restatement follows the reference module's text (models/ada_norm.py:129-182), not the kernels:
  style fc        h = s W^T + b, gamma = h[:C], beta = h[C:]
  InstanceNorm1d  (x - mean_t) / sqrt(var_t + 1e-5), biased variance over the utterance's frames
  AdaIN           (1 + gamma) * InstanceNorm(x) + beta
  residual        conv2(lrelu(AdaIN2(conv1(lrelu(AdaIN1(x)))))), LeakyReLU slope 0.2, both convs k = 3 with one zero frame on either side of the UTTERANCE,
                  weights g v / ||v|| (weight_norm over every dim but the first; the fp32 tensor torch forms, see weight_norm64)
  shortcut        the bias-free 1 x 1 conv of x where the widths differ, else x
  out             (residual + shortcut) / sqrt(2)
on packed ragged batches x [rows, >= cin] with utterance u in rows off[u] .. off[u + 1].

`round_to` ("bf16" / "f16") puts round-to-nearest-even (through fp32, as the engine holds every tensor in fp32 before it rounds) at the engine's
rounding points and accumulates in float64: both operands of every contraction (the activations after AdaIN -> LeakyReLU, the copy of x the learned
shortcut reads, and the weights); the identity residual stays the unrounded x; y16 = round(y).

BOUNDS (nothing here is fitted to a kernel's output).  The error of a result is max |got - want| over an utterance divided by max |want| over that
utterance; the bar is 4 x the same figure of a plain fp32 evaluation on the same inputs (`FOUR`):
  fp32 direct forms            oracle.adaptive_decoder_block in float32 against block64
  fp32 Winograd / bridge       the float32 numpy model of F(6,3) below (interpolation points 0, +-1, +-2, +-1/2 and infinity) against block64
  16-bit forms                 the oracle under OPERAND_ROUND against block64(round_to=...): it rounds where the engine rounds, so it carries the same
                               double-rounding flips (an fp32 value a few ulps off can land on the other side of a 16-bit rounding boundary)
An utterance's bar is FOUR x the WORST of the reference's figures over the batch's utterances, not FOUR x the reference's figure on that utterance: a
single utterance's own figure is a sample of one rounding pattern (512 outputs for the 1-row utterance); the batch's worst is the size of the error such
an evaluation makes on these inputs.

FLIPS AND SEEDS.  In the 16-bit modes the reference's own error is not noise but a count of rare events: an fp32 activation that is a few fp32 ulps off
lands on the other side of a 16-bit rounding boundary with probability (its fp32 error) / (the 16-bit spacing), about 1e-5 in bf16 for the oracle, and
one such operand moves three rows of outputs by spacing16(a) * w.  In bf16 a batch holds about five of them, so one batch's worst figure is a noisy sample
(4e-5, 1.2e-4 and 2.3e-4 on the three blocks).  The bar stays FOUR x the reference's error and nothing else; for the blocks whose inputs are drawn here
the reference's error is the MEAN of its worst figure over SEEDS draws of the inputs (the test's own draw first), same lengths, widths and weights.  An
input that a run produced (block B of a pair, the decoder) has one draw only.  The 16-bit forms are held to a SECOND bar of the same kind as well, with
the root mean square over the utterance in place of the maximum: flips are sparse and barely move it, a missing rounding point moves every output (in f16
an unrounded operand costs 1.6e-4 at its worst element, no more than a large flip, and only the rms tells them apart).

INPUTS.  Channels cycle through standard deviations 1, 0.3, 3 and 0.01 with means of at most one standard deviation.  The low-variance channels make
eps matter (var = 1e-4 against eps = 1e-5).  The means stay small on purpose: every form applies AdaIN as x * scale + shift, whose rounding error grows with
|mean| / std, while the oracle normalises in float64; that conditioning is held by tests/norm64.py's bounds (cancel_case), not by a bar relative to the oracle.
"""
from __future__ import annotations

import numpy as np

from norm64 import EPS_IN, F32, F64, LRELU, chunk_rows_of, offsets

FOUR = 4.0
SQRT2 = float(np.sqrt(2.0))
# the batch of the GPU tests: edges of a Winograd group (6 rows), of the 24-row statistics chunk, of the 128-row chunk and of the 64 / 128-row tiles; one
# utterance past 64 groups
LENGTHS = [1, 5, 6, 7, 23, 24, 25, 143, 385]
# narrow input + learned shortcut | the decoder's concat width | identity shortcut.  The identity block is 512 wide, not narrower: in the 16-bit modes the
# reference's own error is made of rare events (an operand that rounds the other way, about one in 10^4); at 128 channels the whole batch sees at most one,
# and no multiple of a zero-or-one count bounds another evaluation's; at 512 there are dozens.
WIDTHS = {"enc": (130, 512), "dec": (578, 512), "id": (512, 512)}
WINO_M = 6


# ------------------------------------------------------------------------------------------------ rounding
def to_bits16(a, mode, truncate=False):
    """fp32 values -> the 16-bit patterns of `mode` (uint16), round-to-nearest-even (truncate: toward zero, a mutant)."""
    a = np.ascontiguousarray(a, F32)
    if mode == "f16":
        if truncate:
            h = a.astype(np.float16)
            over = np.abs(h.astype(F32)) > np.abs(a)
            return np.where(over, h.view(np.uint16) - 1, h.view(np.uint16)).astype(np.uint16)
        return a.astype(np.float16).view(np.uint16)
    assert mode == "bf16", mode
    u = a.view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def from_bits16(b, mode):
    b = np.ascontiguousarray(b).view(np.uint16)
    if mode == "f16":
        return b.view(np.float16).astype(F32)
    return (b.astype(np.uint32) << 16).view(F32)


def rnd(a, mode, truncate=False):
    """Round to `mode` through fp32; None: unchanged.  Returns the dtype it was given."""
    if mode is None:
        return a
    a = np.asarray(a)
    return from_bits16(to_bits16(a.astype(F32), mode, truncate), mode).astype(a.dtype).reshape(a.shape)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def weight_norm64(g, v):
    """The conv's weight operand: the fp32 tensor v * (g / ||v||) that torch's weight_norm parametrization hands to the conv (formed in fp32 from the fp32
    parameters, the norm itself accumulated in float64), as float64 values.  It is data of the block like x: the restatement starts from it."""
    v = np.asarray(v, F32)
    n = np.sqrt((v.astype(F64) ** 2).reshape(v.shape[0], -1).sum(1)).astype(F32)
    return (v * (np.asarray(g, F32).reshape(-1) / n).reshape((-1,) + (1,) * (v.ndim - 1))).astype(F32).astype(F64)


def block_weights(w, p):
    """The block's tensors in float64 from a state dict with the reference's keys: conv weights [cout, cin, k] already weight-normed."""
    wn = lambda q: weight_norm64(w[q + ".parametrizations.weight.original0"], w[q + ".parametrizations.weight.original1"])  # noqa: E731
    o = {"w1": wn(p + ".conv1"), "b1": np.asarray(w[p + ".conv1.bias"], F64), "w2": wn(p + ".conv2"), "b2": np.asarray(w[p + ".conv2.bias"], F64)}
    o["wsc"] = wn(p + ".conv1x1")[:, :, 0] if (p + ".conv1x1.parametrizations.weight.original0") in w else None
    for n in ("norm1", "norm2"):
        o[n] = (np.asarray(w[f"{p}.{n}.fc.weight"], F64), np.asarray(w[f"{p}.{n}.fc.bias"], F64))
    return o


def style_fc(style, fc):
    """-> gamma, beta [n_utt, C]"""
    h = np.asarray(style, F64) @ fc[0].T + fc[1]
    C = h.shape[1] // 2
    return h[:, :C], h[:, C:]


def adain_lrelu64(x, gamma, beta):
    n = (x - x.mean(0)) / np.sqrt(x.var(0) + EPS_IN)
    v = (1.0 + gamma) * n + beta
    return np.where(v >= 0.0, v, LRELU * v)


def conv3(a, w, b):
    """a [L, cin], w [cout, cin, 3]: y[t] = b + sum_k w[:, :, k] a[t + k - 1], zeros outside the utterance.  dtype of a."""
    L = a.shape[0]
    ap = np.zeros((L + 2, a.shape[1]), a.dtype)
    ap[1 : L + 1] = a
    y = np.zeros((L, w.shape[0]), a.dtype)
    for k in range(3):
        y += ap[k : k + L] @ np.ascontiguousarray(w[:, :, k].T)
    return y + b


def block64(x, lengths, style, wt, round_to=None):
    """x [rows, cin] packed, style [n_utt, style_dim], wt = block_weights(...).  -> y [rows, cout] float64 (y16 = rnd(y, round_to))."""
    x = np.asarray(x, F64)
    off = offsets(lengths)
    g1, b1 = style_fc(style, wt["norm1"])
    g2, b2 = style_fc(style, wt["norm2"])
    w1, w2 = rnd(wt["w1"], round_to), rnd(wt["w2"], round_to)
    y = np.zeros((x.shape[0], w1.shape[0]))
    for u in range(len(lengths)):
        xu = x[off[u] : off[u + 1]]
        a1 = rnd(adain_lrelu64(xu, g1[u], b1[u]), round_to)
        h = conv3(a1, w1, wt["b1"])
        a2 = rnd(adain_lrelu64(h, g2[u], b2[u]), round_to)
        h = conv3(a2, w2, wt["b2"])
        sc = xu if wt["wsc"] is None else rnd(xu, round_to) @ rnd(wt["wsc"], round_to).T
        y[off[u] : off[u + 1]] = (h + sc) / SQRT2
    return y


# ------------------------------------------------------------------------------------------------ F(6,3) in float32
def wino_matrices():
    """Toom-Cook F(6,3) from the points 0, +-1, +-2, +-1/2 and infinity, in float64: y = At [(G g) * (Bt d)] for 8 input rows d, 3 taps g, 6 outputs y.
    Bt holds the Lagrange basis polynomials of the points (and the node polynomial for infinity), G and At the plain powers."""
    pts = [0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5]
    n = 8
    At, G, Bt = np.zeros((WINO_M, n)), np.zeros((n, 3)), np.zeros((n, n))
    for j, pj in enumerate(pts):
        At[:, j] = pj ** np.arange(WINO_M)
        G[j] = pj ** np.arange(3)
        others = [q for q in pts if q != pj]
        Bt[j, : n - 1] = np.poly(others)[::-1] / np.prod([pj - q for q in others])
    At[WINO_M - 1, n - 1] = 1.0
    G[n - 1, 2] = 1.0
    Bt[n - 1] = np.poly(pts)[::-1]
    return At, G, Bt


def conv3_wino32(a, w, b):
    """conv3 through F(6,3) in float32: input transform, one contraction per component, output transform (the weights' transform in float64, stored fp32)."""
    At, G, Bt = wino_matrices()
    a = np.asarray(a, F32)
    L, cin = a.shape
    ng = -(-L // WINO_M)
    ap = np.zeros((ng * WINO_M + 2, cin), F32)
    ap[1 : L + 1] = a
    d = np.stack([ap[WINO_M * g : WINO_M * g + 8] for g in range(ng)])  # [ng, 8, cin]
    V = np.einsum("jq,gqc->jgc", Bt.astype(F32), d).astype(F32)
    U = np.einsum("jk,ock->joc", G, np.asarray(w, F64)).astype(F32)  # [8, cout, cin]
    M = np.stack([V[j] @ U[j].T for j in range(8)]).astype(F32)  # [8, ng, cout]
    y = np.einsum("ij,jgo->gio", At.astype(F32), M).astype(F32).reshape(ng * WINO_M, -1)[:L]
    return (y + np.asarray(b, F32)).astype(F32)


# ------------------------------------------------------------------------------------------------ numpy fp32 model of the engine's forms (and its mutants)
MUTANTS = ("unbiased_var", "eps_outside", "gamma_no_one", "tap_crosses", "no_sqrt2", "sc_unrounded", "operand_unrounded", "residual_hbuf", "last_chunk_dropped",
           "const_stats_missing", "m2_equal_chunks", "slope_001", "y16_truncated")


def chunk_stats32(xu, chunk):
    """(means, m2s, ncs) of the chunks of one utterance, float32, two-pass per chunk (norm64.py bound (a))."""
    ncs = chunk_rows_of(xu.shape[0], chunk)
    means, m2s = [], []
    for i, nc in enumerate(ncs):
        r = xu[i * chunk : i * chunk + nc].astype(F32)
        m = (r.sum(0, dtype=F32) / F32(nc)).astype(F32)
        means.append(m)
        m2s.append(((r - m) ** 2).sum(0, dtype=F32))
    return np.array(means, F32), np.array(m2s, F32), np.array(ncs)


def affine32(xu, gamma, beta, chunk, mutant=None, const_from=None):
    """AdaIN as (scale, shift) per channel from chunk statistics merged in float32 (norm64.py bound (b)); const_from: the columns from there on are the
    pair's constant columns, whose statistics come from a pass of their own."""
    means, m2s, ncs = chunk_stats32(xu, chunk)
    if mutant == "const_stats_missing" and const_from is not None:
        means[:, const_from:] = 0
        m2s[:, const_from:] = 0
    if mutant == "last_chunk_dropped" and len(ncs) > 1:
        means, m2s, ncs = means[:-1], m2s[:-1], ncs[:-1]
    n = F32(ncs.sum())
    wk = np.full(len(ncs), chunk, F32) if mutant == "m2_equal_chunks" else ncs.astype(F32)
    nn = F32(wk.sum())
    mean = ((wk[:, None] * means).sum(0, dtype=F32) / nn).astype(F32)
    m2 = (m2s + wk[:, None] * (means - mean) ** 2).sum(0, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (m2 / (n - F32(1) if mutant == "unbiased_var" else n)).astype(F32)
        rstd = F32(1) / (np.sqrt(var) + F32(EPS_IN)) if mutant == "eps_outside" else F32(1) / np.sqrt(var + F32(EPS_IN))
    g = gamma.astype(F32) if mutant == "gamma_no_one" else F32(1) + gamma.astype(F32)
    scale = (rstd * g).astype(F32)
    return scale, (beta.astype(F32) - mean * scale).astype(F32)


def model32(x, lengths, style, wt, prec=None, conv="direct", chunk=128, rows16=False, mutant=None, const_from=None):
    """The block as the engine's forms compute it, in numpy float32: AdaIN as an affine from chunk statistics, LeakyReLU, the contraction's operands rounded
    to `prec`, conv = "direct" | "wino" (fp32 only).  rows16: the learned shortcut reads the rounded copy of x (the model's numbers do not depend on it: the
    operand is rounded either way; it decides what the sc_unrounded mutant means).  -> (y float32, y16 bits or None, hbuf float32)."""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x, F32)
    off = offsets(lengths)
    slope = F32(0.01) if mutant == "slope_001" else F32(LRELU)
    g1, b1 = style_fc(style, wt["norm1"])
    g2, b2 = style_fc(style, wt["norm2"])
    opr = (lambda a: a) if mutant == "operand_unrounded" else (lambda a: rnd(a, prec))
    w1, w2 = rnd(wt["w1"].astype(F32), prec), rnd(wt["w2"].astype(F32), prec)
    cv = conv3_wino32 if conv == "wino" else conv3

    def act(xu, gamma, beta, cf=None):
        sc, sh = affine32(xu, gamma, beta, chunk, mutant, cf)
        v = (xu * sc + sh).astype(F32)
        return np.where(v >= 0, v, v * slope).astype(F32)

    def conv_batch(a, w, b):  # per utterance; the tap_crosses mutant convolves the packed rows as one utterance
        if mutant == "tap_crosses":
            return cv(a, w, b.astype(F32)).astype(F32)
        return np.concatenate([cv(a[off[u] : off[u + 1]], w, b.astype(F32)) for u in range(len(lengths))]).astype(F32)

    a1 = np.concatenate([act(x[off[u] : off[u + 1]], g1[u], b1[u], const_from) for u in range(len(lengths))])
    h = conv_batch(opr(a1), w1, wt["b1"])
    a2 = np.concatenate([act(h[off[u] : off[u + 1]], g2[u], b2[u]) for u in range(len(lengths))])
    r = conv_batch(opr(a2), w2, wt["b2"])
    if wt["wsc"] is None:
        sc = h if mutant == "residual_hbuf" else x[:, : r.shape[1]]
    else:
        xs = x if (mutant == "sc_unrounded" and rows16) else rnd(x, prec)
        sc = (xs @ rnd(wt["wsc"].astype(F32), prec).T).astype(F32)
    y = (r + sc).astype(F32)
    if mutant != "no_sqrt2":
        y = (y * F32(1.0 / SQRT2)).astype(F32)
    y16 = to_bits16(y, prec, truncate=mutant == "y16_truncated") if prec else None
    return y, y16, h


# ------------------------------------------------------------------------------------------------ cases, errors and bars
def inputs(seed, lengths, cin):
    """x [rows, cin] fp32 (module docstring: INPUTS) and style [n_utt, 64]."""
    from stylish_tts_amd import synth

    rows = int(np.sum(lengths))
    std = np.array([1.0, 0.3, 3.0, 0.01])[np.arange(cin) % 4]
    mean = np.array([0.0, 0.5, -1.0])[np.arange(cin) % 3] * std
    x = synth.normal(f"blk.x.{seed}.{rows}.{cin}", (rows, cin)).astype(F64) * std + mean
    style = (synth.normal(f"blk.s.{seed}", (len(lengths), 64)) * 0.7).astype(F32)
    return x.astype(F32), style


def weights(name):
    """(state dict with the reference's keys under the prefix "blk.<name>", the prefix)."""
    from stylish_tts_amd import params

    cin, cout = WIDTHS[name]
    return params.synth_state_dict(params.adaptive_decoder_block_spec(f"blk.{name}", cin, cout, 64), 0), f"blk.{name}"


def utt_errors(got, want, lengths, rms=False):
    """per utterance: max |got - want| / max |want| (rms: root mean square of the difference / max |want|); a non-finite result counts as infinite."""
    off = offsets(lengths)
    out = []
    for u in range(len(lengths)):
        g, w = np.asarray(got[off[u] : off[u + 1]], F64), np.asarray(want[off[u] : off[u + 1]], F64)
        e = np.sqrt(np.mean((g - w) ** 2)) if rms else np.abs(g - w).max()
        out.append(float(e / max(np.abs(w).max(), 1e-30)) if np.isfinite(g).all() else np.inf)
    return np.array(out)


def oracle32(x, lengths, style, w, p, round_to=None):
    """oracle.adaptive_decoder_block per utterance on the packed batch (under OPERAND_ROUND = round_to) -> y [rows, cout] float32."""
    from oracle import stylish_oracle as O

    off = offsets(lengths)
    was = O.OPERAND_ROUND
    O.OPERAND_ROUND = round_to
    try:
        ys = [O.adaptive_decoder_block(np.ascontiguousarray(x[off[u] : off[u + 1]].T[None], F32), style[u : u + 1], w, p)[0].T for u in range(len(lengths))]
    finally:
        O.OPERAND_ROUND = was
    return np.concatenate(ys).astype(F32)


def bar(ref_y, want, lengths, rms=False):
    """FOUR x the worst per-utterance error of the reference evaluation `ref_y` (module docstring: BOUNDS)."""
    return FOUR * float(utt_errors(ref_y, want, lengths, rms).max())


def ref_errors16(x, lengths, style, w, p, mode, want=None):
    """the reference's own error in a 16-bit mode: (worst max-abs figure, worst rms figure) of the oracle under OPERAND_ROUND against block64."""
    want = block64(x, lengths, style, block_weights(w, p), mode) if want is None else want
    ref = oracle32(x, lengths, style, w, p, mode)
    return float(utt_errors(ref, want, lengths).max()), float(utt_errors(ref, want, lengths, rms=True).max())


def bars16(errs):
    """(max-abs bar, rms bar) = FOUR x the mean of the reference's figures over the draws in `errs` (a list of ref_errors16 results)."""
    return FOUR * float(np.mean([e[0] for e in errs])), FOUR * float(np.mean([e[1] for e in errs]))


SEEDS = 4


def seeded_bars16(name, lengths, mode):
    """bars16 of block `name` on `lengths`: the draw inputs(name, ...) that the tests run, and SEEDS - 1 further draws."""
    w, p = weights(name)
    errs = []
    for k in range(SEEDS):
        x, style = inputs(name if k == 0 else f"{name}.draw{k}", lengths, WIDTHS[name][0])
        errs.append(ref_errors16(x, lengths, style, w, p, mode))
    return bars16(errs)


def reference(x, lengths, style, w, p, mode=None, conv="direct", name=None):
    """What a GPU result of one block is held to: (want = block64, bars for `ratios`), the reference evaluation chosen as the module docstring says.
    name: x is inputs(name, lengths, ...), so a 16-bit bar averages the reference over the draws; else x came out of a run and is the only draw."""
    wt = block_weights(w, p)
    want = block64(x, lengths, style, wt, mode)
    if mode:
        return want, (seeded_bars16(name, tuple(lengths), mode) if name else bars16([ref_errors16(x, lengths, style, w, p, mode, want)]))
    if conv == "wino":
        return want, bar(model32(x, lengths, style, wt, conv="wino", chunk=24)[0], want, lengths)
    return want, bar(oracle32(x, lengths, style, w, p), want, lengths)


def decoder64(asr, pitch, energy, style, w, mode, p="decoder."):
    """Decoder.forward (models/decoder.py:47-60) of ONE utterance in float64 with block64's rounding points: asr [T, 128], pitch / energy [T], style [1, 64].
    F0 / N = the one-channel k = 3 convs (no matrix-core contraction: unrounded), asr_res = the 1 x 1 conv (a contraction: operands rounded), x = encode([asr |
    F0 | N]), then four times x = decode_i([x | asr_res | F0 | N]).  -> x [T, hidden] float64."""
    T = [asr.shape[0]]
    wn = lambda q: weight_norm64(w[q + ".parametrizations.weight.original0"], w[q + ".parametrizations.weight.original1"])  # noqa: E731
    F0 = conv3(np.asarray(pitch, F64)[:, None], wn(p + "F0_conv"), np.asarray(w[p + "F0_conv.bias"], F64))
    N = conv3(np.asarray(energy, F64)[:, None], wn(p + "N_conv"), np.asarray(w[p + "N_conv.bias"], F64))
    asr = np.asarray(asr, F64)
    res = rnd(asr, mode) @ rnd(wn(p + "asr_res.0")[:, :, 0], mode).T + np.asarray(w[p + "asr_res.0.bias"], F64)
    x = np.concatenate([asr, F0, N], 1)
    for i, q in enumerate(["encode"] + [f"decode.{j}" for j in range(4)]):
        wt = block_weights(w, p + q)
        x = block64(x.astype(F32) if mode else x, T, style, wt, mode)  # (16-bit modes: the engine holds y in fp32 between the blocks)
        if i < 4:
            x = np.concatenate([x, res, F0, N], 1)
    return x


def ratios(y, want, lengths, bars):
    """worst error / bar of a result: one figure for an fp32 form (bars: a number), (max-abs, rms) for a 16-bit form (bars: bars16's pair)."""
    if not isinstance(bars, tuple):
        return float(utt_errors(y, want, lengths).max() / bars)
    return float(utt_errors(y, want, lengths).max() / bars[0]), float(utt_errors(y, want, lengths, rms=True).max() / bars[1])


def within(r):
    return all(v <= 1.0 for v in (r if isinstance(r, tuple) else (r,)))


def decoder_reference(asr, pitch, energy, style, w, mode):
    """What the decoder's output of one utterance is held to in a 16-bit mode (oracle layout: asr [1, 128, T], pitch / energy [1, T], style [1, 64]):
    (want = decoder64 [T, hidden], bars16 of the oracle under OPERAND_ROUND against it - one draw -, ref = the oracle's output [T, hidden], e = its max-abs
    figure).  A result inside the max-abs bar is within FOUR e of want, and the oracle is e away from want: against the ORACLE it is within (FOUR + 1) e."""
    from oracle import stylish_oracle as O

    want = decoder64(asr[0].T, pitch[0], energy[0], style, w, mode)
    was = O.OPERAND_ROUND
    O.OPERAND_ROUND = mode
    try:
        ref = O.decoder_forward(asr, pitch, energy, style, w)[0].T
    finally:
        O.OPERAND_ROUND = was
    T = [want.shape[0]]
    e = (float(utt_errors(ref, want, T).max()), float(utt_errors(ref, want, T, rms=True).max()))
    return want, bars16([e]), ref, e[0]
