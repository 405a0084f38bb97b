"""Float64 restatements of the operations BETWEEN the contractions, the bounds their HIP kernels are held to, and the cases both
tests/test_norm64_cpu.py (numpy fp32 emulations, no GPU) and tests/test_hip_norm_kernels.py (the kernels, through stts_op_adain / _wino_stat /
_row_layernorm / _dwconv / _grn) run.  Test infrastructure.

The restatements follow the reference modules' formulas, not the kernels:
  InstanceNorm1d(affine=False)  (x - mean_t) / sqrt(var_t + 1e-5), biased variance over time       models/ada_norm.py:129-139
  AdaIN                         (1 + gamma) * InstanceNorm(x) + beta
  Snake1D                       x + sin(alpha x)^2 / alpha                                          models/ada_norm.py:114,117
  LayerNorm                     (x - mean_c) / sqrt(var_c + eps) * g + b, adaptive: g = 1 + gamma   models/ada_norm.py:193-201, text_encoder.py:24-33
  depthwise Conv1d              y[t, c] = b[c] + sum_k w[c, k] x[t + k - (K - 1) / 2, c], zeros outside the utterance   models/generator.py:449-455
  GRN                           Gx = ||x||_2 over time, factor = gamma * Gx / (mean_c Gx + 1e-6) + 1   models/generator.py:496-499
Constants the reference holds in fp32 (1e-5, 1e-6, LeakyReLU's 0.2) are the fp32 numbers here too: both sides multiply by the same value.

BOUNDS.  u = 2^-24 (fp32 unit roundoff).  Every bound counts the roundings of the kernel's expression, in ANY summation order, to first order; a factor
1.01 covers the second-order terms.  Nothing here was fitted to a kernel's output.  The checks are staged so each count stays short:

 (a) chunk table vs float64 of the rows X the kernel read (nc rows, A = sum |v|, M2 = sum (v - mean64)^2):
       mean = fl(fl(sum v) / nc):  |s - S| <= (nc - 1) u A, the division adds u |S| / nc  =>  |mean - mean64| <= nc u A / nc; the bar is
              dm = (nc + 1) u A / nc  (the bar of the 16-bit epilogue's statistics, test_hip_gemm16_epilogues.py assertion 5).
       M2 (two-pass: fl(sum fl(fl(v - mean)^2))):  with delta = mean - mean64 EXACTLY  sum (v - mean)^2 = M2 + nc delta^2  (the cross term is
              2 delta sum (v - mean64) = 0), so the computed mean's offset costs at most off = nc dm^2; each term then sees the subtraction, the
              square and at most nc - 1 additions: (nc + 2) u relative, on non-negative terms.  Bar: off + (nc + 4) u (M2 + off).
       Chan (winograd_output_kernel<N, true>: per-group (mean_w, M2_w) over <= 6 rows, merged as M2 = sum M2_w + n_w (mean_w - mean)^2): the error e_w of a
              group mean does NOT cancel: 2 sum n_w (mean_w - mean) e_w <= 2 sqrt(M2) sqrt(sum n_w e_w^2), e_w <= (n_w + 1) u A_w / n_w  =>
              sqrt(sum n_w e_w^2) <= 7 u A; the bar adds 2 sqrt(M2) 8 u A.
     A one-pass M2 = s2 - mean s1 is (3 nc + 4) u sum v^2 away instead: at mean^2 / var = 2.6e4 that is 1e-2 of M2 and fails this bar by three
     orders of magnitude (test_norm64_cpu.py::test_one_pass_m2_fails_bound_a).
 (b) merged scale / shift vs a float64 merge OF THE TABLE THE KERNEL PRODUCED (K chunks of n_k rows, n rows in all):
       mean = fl(sum fl(n_k m_k)) / n:  dm = (K + 1) u sum n_k |m_k| / n.   M2: as in (a), offset n dm^2 exactly, terms non-negative, each with the
       subtraction, two products and <= K additions: dM2 = n dm^2 + (K + 5) u (M2 + n dm^2).   var + eps: the division and the addition, 2 u.
       rstd = rsqrtf(.): half the relative error of its argument + rho_rsqrt u.   scale = rstd * fl(1 + g): 2 u.
       => dscale = 1.01 |scale| (0.5 (dM2 / (n (var + eps)) + 2 u) + (rho_rsqrt + 2) u),
          dshift = 1.01 (|mean| dscale + dm |scale|) + u (|mean scale| + |shift|).
 (c) Y vs act(x scale64 + shift64) with (scale64, shift64) from (b), per element:  v = fl(x sc + sh): u |x sc| + u |v|, + the propagated table error
       |x| dscale + dshift = dv.   LeakyReLU: one product, Lipschitz 1: dv + u |y|.   Snake: t = fl(al v): |al| dv + u |t|; s = sinf(t): + E_sin;
       q = fl(fl(s s) / al): (2 |s| ds + ds^2 + 2 u s^2) / |al|;  y = fl(v + q): dv + dq + u |y|.
 LayerNorm (per row, C channels): (a) with nc = C for mean and M2, rstd as in (b), y = fl(fl(fl(d rstd) g) + b): |g| rstd dd + |d rstd g| (rr + 3 u) + u |y|
       with dd = dm + u |d|; an input that is itself uncertain by e[c] (the fused depthwise conv) adds mean(e) to dm, e[c] + mean(e) to dd and
       2 sqrt(M2) ||e||_2 + ||e||_2^2 to dM2.
 depthwise conv: K products and K additions onto the bias in tap order: (K + 1) u (|b| + sum |w x|).  SiLU = v * rcp(1 + exp2(-v log2 e)): `silu_bound`.
 GRN: gx = sqrtf(fl(sum of slots)): (slots + 1) u + E_sqrt relative; factor from the kernel's own gx: the channel sum, + 1e-6, the reciprocal, two products
       and the + 1: (C + 6) u |gamma gx inv| + u |factor|; scaled weight with the channel mean exact (the case makes it so): 4 u |w| (|gamma gx inv| + 1).

ULP FIGURES.  The ROCm install has no HIP math documentation, so for rsqrtf, sinf, sqrtf and SiLU's two primitives (exp2 and the reciprocal) the figure is
MEASURED on the CPU: the numpy-fp32 evaluation of the same expression against float64 on the inputs of the check that uses it, times 4
(`four_times_numpy`).  The reference, not the kernel, sets the number.  On the apply / GRN cases (test_norm64_cpu.py::test_measured_ulp_figures, -s) numpy
shows 1.5 u (1 / sqrt), 0.93 u absolute (sin), 1.7 u (exp2), 1.0 u (1 / x), 1.0 u (sqrt), so the kernels are allowed 6.0 u, 3.7 u, 6.8 u, 4.0 u and 4.0 u.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS_IN = float(F32(1e-5))  # InstanceNorm / AdaIN
EPS_GRN = float(F32(1e-6))
LRELU = float(F32(0.2))
ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_LRELU = range(5)  # csrc/gemm.hip.h: enum Act
STAT_CHUNK, WINO_CHUNK, WINO_M = 128, 24, 6
SLACK = 1.01


def round_up(a, b):
    return (a + b - 1) // b * b


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ float64 restatements
def instance_norm64(x):
    """x [T, C] -> (x - mean_t) / sqrt(var_t + 1e-5), biased variance."""
    x = np.asarray(x, F64)
    return (x - x.mean(0)) / np.sqrt(x.var(0) + EPS_IN)


def adain64(x, gamma, beta):
    return (1.0 + np.asarray(gamma, F64)) * instance_norm64(x) + np.asarray(beta, F64)


def adain_affine64(x, gamma, beta):
    """The same as an affine of x: (scale, shift) per channel."""
    x = np.asarray(x, F64)
    scale = (1.0 + np.asarray(gamma, F64)) / np.sqrt(x.var(0) + EPS_IN)
    return scale, np.asarray(beta, F64) - x.mean(0) * scale


def snake64(v, alpha):
    return v + np.sin(alpha * v) ** 2 / alpha


def act64(v, act):
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_LRELU:
        return np.where(v >= 0.0, v, LRELU * v)
    assert act == ACT_NONE, act
    return v


def layernorm64(x, g, b, eps):
    """x [R, C]; g, b [C] or [R, C] (the effective gain: 1 + gamma for the adaptive form)."""
    x = np.asarray(x, F64)
    d = x - x.mean(1, keepdims=True)
    return d / np.sqrt((d * d).mean(1, keepdims=True) + eps) * g + b


def dwconv64(x, lengths, w, b):
    """x [rows, C] packed; w [C, K]; zero padding inside each utterance."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    K = w.shape[1]
    pad = (K - 1) // 2
    y = np.empty_like(x)
    off = offsets(lengths)
    for u, L in enumerate(lengths):
        xp = np.zeros((L + K - 1, x.shape[1]))
        xp[pad : pad + L] = x[off[u] : off[u + 1]]
        acc = np.tile(np.asarray(b, F64), (L, 1))
        for k in range(K):
            acc += w[:, k] * xp[k : k + L]
        y[off[u] : off[u + 1]] = acc
    return y


def grn_gx64(slots):
    """slots [n_slots, C]: partial sums of squares over time -> Gx = ||x||_2."""
    return np.sqrt(np.asarray(slots, F64).sum(0))


def grn_factor64(gx, gamma):
    gx = np.asarray(gx, F64)
    return np.asarray(gamma, F64) * gx / (gx.mean() + EPS_GRN) + 1.0


# ------------------------------------------------------------------------------------------------ measured ULP figures
def four_times_numpy(got32, want64, relative=True):
    """4 x the largest error of a numpy-fp32 evaluation against float64 on the test's own inputs (module docstring: ULP FIGURES)."""
    got, want = np.asarray(got32, F64), np.asarray(want64, F64)
    e = np.abs(got - want)
    if relative:
        nz = want != 0
        e = e[nz] / np.abs(want[nz])
    return 4.0 * float(e.max()) if e.size else 0.0


def rho_rsqrt(v64):
    """Allowed relative error of rsqrtf on arguments v (any shape), IN UNITS OF u."""
    v32 = np.asarray(v64, F64).astype(F32)
    return four_times_numpy(F32(1.0) / np.sqrt(v32), 1.0 / np.sqrt(v32.astype(F64))) / U


def e_sqrt(v64):
    v32 = np.asarray(v64, F64).astype(F32)
    return four_times_numpy(np.sqrt(v32), np.sqrt(v32.astype(F64)))


def e_sin(t64):
    """Allowed ABSOLUTE error of sinf on arguments t."""
    t32 = np.asarray(t64, F64).astype(F32)
    return four_times_numpy(np.sin(t32), np.sin(t32.astype(F64)), relative=False)


def e_exp2_rcp(v64):
    """Allowed relative errors of the two hardware primitives of SiLU, exp2 and the reciprocal, on the arguments SiLU(v) gives them."""
    v32 = np.asarray(v64, F64).astype(F32)
    t = np.clip(-v32 * F32(1.4426950408889634), -120, 120).astype(F32)
    s = (F32(1.0) + np.exp2(t)).astype(F32)
    return four_times_numpy(np.exp2(t), np.exp2(t.astype(F64))), four_times_numpy(F32(1.0) / s, 1.0 / s.astype(F64))


# ------------------------------------------------------------------------------------------------ bounds
def chunk_bound(x, chan=False):
    """Bound (a) for one chunk: x [nc, C] (the stored rows) -> mean64, M2_64, allowed |mean - mean64|, allowed |M2 - M2_64|."""
    x = np.asarray(x, F64)
    nc = x.shape[0]
    A = np.abs(x).sum(0)
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    dm = (nc + 1) * U * A / nc
    off = nc * dm * dm
    d2 = off + (nc + 4) * U * (m2 + off)
    if chan:
        d2 = d2 + 2.0 * np.sqrt(m2) * 8.0 * U * A
    return mean, m2, dm, d2


def merge_bound(means, m2s, ncs, gamma, beta, rho):
    """Bound (b): means, m2s [K, C] (the kernel's own table), ncs [K] rows per chunk -> dict(mean, scale, shift, dscale, dshift) in float64."""
    means, m2s, ncs = np.asarray(means, F64), np.asarray(m2s, F64), np.asarray(ncs, F64)
    K, n = len(ncs), ncs.sum()
    w = ncs[:, None]
    mean = (w * means).sum(0) / n
    m2 = (m2s + w * (means - mean) ** 2).sum(0)
    var = m2 / n + EPS_IN
    scale = (1.0 + np.asarray(gamma, F64)) / np.sqrt(var)
    shift = np.asarray(beta, F64) - mean * scale
    dm = (K + 1) * U * (w * np.abs(means)).sum(0) / n
    off = n * dm * dm
    dm2 = off + (K + 5) * U * (m2 + off)
    rel = 0.5 * (dm2 / n / var + 2 * U) + (rho + 2) * U
    dscale = SLACK * rel * np.abs(scale)
    dshift = SLACK * (np.abs(mean) * dscale + dm * np.abs(scale)) + U * (np.abs(mean * scale) + np.abs(shift))
    return dict(mean=mean, var=var, scale=scale, shift=shift, dscale=dscale, dshift=dshift)


def apply_bound(x, tab, act, alpha=None, esin=0.0):
    """Bound (c): x [T, C] float64, tab from merge_bound -> y64, allowed |y - y64| per element."""
    x = np.asarray(x, F64)
    sc, sh = tab["scale"], tab["shift"]
    v = x * sc + sh
    dv = SLACK * (np.abs(x) * tab["dscale"] + tab["dshift"] + U * np.abs(x * sc) + U * np.abs(v))
    if alpha is not None:
        al = np.asarray(alpha, F64)
        t = al * v
        s = np.sin(t)
        ds = np.abs(al) * dv + U * np.abs(t) + esin
        dq = (2 * np.abs(s) * ds + ds * ds + 2 * U * s * s) / np.abs(al)
        y = v + s * s / al
        return y, SLACK * (dv + dq) + U * np.abs(y)
    y = act64(v, act)
    return y, dv + (U * np.abs(y) if act != ACT_NONE else 0.0)


def ln_bound(x, g, b, eps, rho, act=ACT_NONE, in_err=None):
    """LayerNorm: x [R, C] float64 (g: effective gain) -> y64, allowed |y - y64|; in_err [R, C]: the uncertainty of x itself."""
    x = np.asarray(x, F64)
    C = x.shape[1]
    mean = x.mean(1, keepdims=True)
    d = x - mean
    m2 = (d * d).sum(1, keepdims=True)
    var = m2 / C + eps
    rstd = 1.0 / np.sqrt(var)
    y = d * rstd * g + b
    A = np.abs(x).sum(1, keepdims=True)
    e = np.zeros_like(x) if in_err is None else np.asarray(in_err, F64)
    ebar = e.mean(1, keepdims=True)
    dm0 = (C + 1) * U * A / C
    dd = dm0 + ebar + e + U * np.abs(d)
    l2 = np.sqrt((e * e).sum(1, keepdims=True))
    off = C * dm0 * dm0
    dm2 = off + (C + 4) * U * (m2 + off) + 2 * np.sqrt(m2) * l2 + l2 * l2
    rr = 0.5 * (dm2 / C / var + 2 * U) + rho * U
    dy = SLACK * (np.abs(g) * rstd * dd + np.abs(d * rstd * g) * (rr + 3 * U)) + U * np.abs(y)
    return act64(y, act), dy


def dwconv_bound(x, lengths, w, b):
    """-> y64, allowed |y - y64| = (K + 1) u (|b| + sum |w x|)."""
    K = np.asarray(w).shape[1]
    return dwconv64(x, lengths, w, b), (K + 1) * U * dwconv64(np.abs(x), lengths, np.abs(w), np.abs(b))


def silu_bound(v, dv, eexp2, ercp):
    """act_apply's SiLU = v * rcp(1 + __expf(-v)), __expf(x) = exp2(x * log2 e): the product's rounding (and that of the constant) moves the exponent by
    2 |v| u log2 e, i.e. e = exp(-v) by 2 |v| u relative, + E_exp2; s = 1 + e: e / (1 + e) of that + u; the reciprocal: E_rcp; the last product: u.
    SiLU's slope is at most 1.1.  Where e or 1 / s leave the normal range the result is off by at most (|v| + 1) 2^-126."""
    with np.errstate(over="ignore"):
        y = act64(v, ACT_SILU)
        frac = 1.0 / (1.0 + np.exp(v))  # e / (1 + e)
    rel = (2 * np.abs(v) * U + eexp2) * frac + 2 * U + ercp
    return y, 1.1 * dv + SLACK * rel * np.abs(y) + (np.abs(v) + 1.0) * 2.0 ** -126


def gx_bound(slots, esqrt):
    """-> gx64, allowed |gx - gx64| = ((slots + 1) u + E_sqrt) gx64."""
    gx = grn_gx64(slots)
    return gx, ((len(slots) + 1) * U + esqrt) * gx


def factor_bound(gx, gamma):
    """GRN factor from the kernel's OWN gx [C] -> factor64, allowed error."""
    C = len(gx)
    f = grn_factor64(gx, gamma)
    return f, SLACK * (C + 6) * U * np.abs(f - 1.0) + U * np.abs(f)


# ------------------------------------------------------------------------------------------------ inputs
def ragged(seed, lengths, C, ld, big=1e3, base=1.0):
    """[rows, ld] fp32 rows of N(m_u, s_u) per utterance; every other utterance (the odd ones) and every pad column ~ `big` times larger, so a row or
    a column leaking across a boundary cannot hide."""
    rng = np.random.default_rng(seed)
    off = offsets(lengths)
    x = (rng.standard_normal((int(off[-1]), ld)) * big).astype(F32)
    for u, L in enumerate(lengths):
        s = base * (big if u % 2 else 1.0)
        x[off[u] : off[u + 1], :C] = (rng.standard_normal((L, C)) * s + 0.3 * s * rng.standard_normal(C)).astype(F32)
    x.setflags(write=False)
    return x


def style(seed, n_utt, C, ld=None, col0=0):
    """[n_utt, ld] fp32 style rows: gamma at col0 + c, beta at col0 + C + c (O(0.3) and O(1)); every other column large."""
    rng = np.random.default_rng(seed)
    ld = ld or col0 + 2 * C
    gb = (rng.standard_normal((n_utt, ld)) * 1e3).astype(F32)
    gb[:, col0 : col0 + C] = (0.3 * rng.standard_normal((n_utt, C))).astype(F32)
    gb[:, col0 + C : col0 + 2 * C] = rng.standard_normal((n_utt, C)).astype(F32)
    gb.setflags(write=False)
    return gb


# chunk producers
STAT_LENGTHS = (0, 1, 23, 24, 25, 127, 128, 129, 400)
STAT_C = ((64, 64), (130, 160))  # (C, ldx)
CANCEL_LENGTHS = (128, 129, 400)
CANCEL_CH = (0, 5, 31, 32, 33, 47, 62, 63)
WINO_LENGTHS = (1, 5, 6, 7, 23, 24, 25, 145)
WINO_COUT = (64, 132)
# merges: every lane wrap (16 lanes: > 2 048 rows at chunk 128, > 384 at 24; 4 lanes: > 512 rows)
MERGE_LENGTHS = {STAT_CHUNK: (0, 1, 129, 513, 2100), WINO_CHUNK: (0, 1, 25, 385, 400)}
MERGE_C, MERGE_LD = 130, 160
# apply
APPLY_LENGTHS = (0, 1, 63, 64, 65, 257, 600)
APPLY_C, APPLY_LDX, APPLY_LDY = 130, 160, 192


@lru_cache(maxsize=None)
def stat_case(C, ldx):
    return ragged(100 + C, STAT_LENGTHS, C, ldx)


@lru_cache(maxsize=None)
def cancel_case():
    """C = 64; eight channels with mean 8 and standard deviation 0.05 (mean^2 / var = 2.6e4), the rest N(0, 1)."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((sum(CANCEL_LENGTHS), 64)).astype(F32)
    for c in CANCEL_CH:
        x[:, c] = (8.0 + 0.05 * rng.standard_normal(x.shape[0])).astype(F32)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def merge_case(chunk):
    L = MERGE_LENGTHS[chunk]
    return ragged(200 + chunk, L, MERGE_C, MERGE_LD), style(201 + chunk, len(L), MERGE_C, 2 * MERGE_C + 8, 4)


@lru_cache(maxsize=None)
def apply_case():
    rng = np.random.default_rng(300)
    alpha = rng.uniform(0.1, 3.0, APPLY_C).astype(F32)
    alpha.setflags(write=False)
    return ragged(301, APPLY_LENGTHS, APPLY_C, APPLY_LDX), style(302, len(APPLY_LENGTHS), APPLY_C, 2 * APPLY_C + 8, 4), alpha


def chunk_rows_of(L, chunk):
    """rows of every chunk of an utterance of L rows."""
    return [min(chunk, L - i) for i in range(0, L, chunk)]


# ------------------------------------------------------------------------------------------------ checkers (shared by the CPU emulations and the GPU tests)
def check_chunk_table(x, lengths, C, chunk, table, chan=False, what=""):
    """Bound (a) on a whole table [n_utt, nchunk, 2, >= C] against the rows x [rows, >= C] the producer read (or stored).
    -> (worst |mean err| / bound, worst |M2 err| / bound, worst relative M2 error over full chunks of the channels in CANCEL_CH or all)."""
    off = offsets(lengths)
    wm = w2 = 0.0
    rel = np.zeros(C)
    for u, L in enumerate(lengths):
        for ch, nc in enumerate(chunk_rows_of(L, chunk)):
            rows = x[off[u] + ch * chunk : off[u] + ch * chunk + nc, :C]
            mean, m2, dm, d2 = chunk_bound(rows, chan)
            gm, g2 = table[u, ch, 0, :C].astype(F64), table[u, ch, 1, :C].astype(F64)
            assert np.isfinite(gm).all() and np.isfinite(g2).all(), (what, "chunk not written", u, ch)
            em, e2 = np.abs(gm - mean), np.abs(g2 - m2)
            assert (em <= dm).all(), (what, "mean", u, ch, int(np.argmax(em - dm)), float((em / np.maximum(dm, 1e-300)).max()))
            assert (e2 <= d2).all(), (what, "M2", u, ch, int(np.argmax(e2 - d2)), float((e2 / np.maximum(d2, 1e-300)).max()))
            assert (g2 >= 0).all(), (what, "M2 < 0", u, ch)
            wm = max(wm, float((em / np.maximum(dm, 1e-300)).max()))
            w2 = max(w2, float((e2 / np.maximum(d2, 1e-300)).max()))
            if nc == chunk:
                rel = np.maximum(rel, e2 / np.maximum(m2, 1e-300))
    return wm, w2, rel


def table_of(table, u, L, chunk, C):
    """the (means, m2s, ncs) of utterance u out of a table [n_utt, nchunk, 2, ld]."""
    ncs = chunk_rows_of(L, chunk)
    k = len(ncs)
    return table[u, :k, 0, :C], table[u, :k, 1, :C], ncs


def merge_of(table, u, L, chunk, C, gb, gcol0):
    """bound (b) of utterance u (L > 0 rows) from the kernel's own table: merge_bound's dict, rsqrtf's figure measured on this utterance's variances."""
    means, m2s, ncs = table_of(table, u, L, chunk, C)
    g, b = gb[u, gcol0 : gcol0 + C], gb[u, gcol0 + C : gcol0 + 2 * C]
    return merge_bound(means, m2s, ncs, g, b, rho_rsqrt(merge_bound(means, m2s, ncs, g, b, 0.0)["var"]))


def check_affine(table, lengths, C, chunk, gb, gcol0, aff, what=""):
    """Bound (b) on an affine table aff [n_utt, 2, ld_aff] (pad columns and empty utterances: exactly 0).  -> worst error / bound."""
    worst = 0.0
    for u, L in enumerate(lengths):
        if L == 0:
            assert (aff[u].view(np.uint32) == 0).all(), (what, "empty utterance: scale and shift must be exactly 0", u, aff[u, :, :4])
            continue
        t = merge_of(table, u, L, chunk, C, gb, gcol0)
        es, eh = np.abs(aff[u, 0, :C] - t["scale"]), np.abs(aff[u, 1, :C] - t["shift"])
        assert (es <= t["dscale"]).all(), (what, "scale", u, int(np.argmax(es - t["dscale"])), float((es / t["dscale"]).max()))
        assert (eh <= t["dshift"]).all(), (what, "shift", u, int(np.argmax(eh - t["dshift"])), float((eh / t["dshift"]).max()))
        assert (aff[u, :, C:].view(np.uint32) == 0).all(), (what, "pad columns must be exactly 0", u)
        worst = max(worst, float((es / t["dscale"]).max()), float((eh / t["dshift"]).max()))
    return worst


def check_apply(x, table, lengths, C, gb, gcol0, act, alpha, y, what=""):
    """Bound (c) on fp32 rows y [rows, ldy] (pad columns C .. ldy - 1 exactly 0); the table is the kernel's own (chunks of 128 rows).  -> worst error / bound."""
    off = offsets(lengths)
    worst = 0.0
    for u, L in enumerate(lengths):
        if L == 0:
            continue
        t = merge_of(table, u, L, STAT_CHUNK, C, gb, gcol0)
        xs = x[off[u] : off[u + 1], :C].astype(F64)
        esin = 0.0
        if alpha is not None:
            esin = e_sin(np.asarray(alpha, F64) * (xs * t["scale"] + t["shift"]))
        want, dy = apply_bound(xs, t, act, alpha, esin)
        got = y[off[u] : off[u + 1]]
        e = np.abs(got[:, :C] - want)
        assert (e <= dy).all(), (what, "Y", u, np.argwhere(e > dy)[:2], float((e / dy).max()))
        assert (got[:, C:].view(np.uint32) == 0).all(), (what, "pad columns of Y must be exactly 0", u)
        worst = max(worst, float((e / dy).max()))
    return worst


# ------------------------------------------------------------------------------------------------ row LayerNorm cases
LN_C = (4, 252, 256, 260, 2048)
LN_ROWS = 9
LN_LENGTHS = (2, 3, 4)  # adaptive: three utterances with distinct style rows


@lru_cache(maxsize=None)
def ln_case(C):
    """x [9, ldx = C + 4] (row 7: mean 100, standard deviation 0.01; pad columns large), static gamma / beta, adaptive style rows for two outputs."""
    rng = np.random.default_rng(400 + C)
    x = (rng.standard_normal((LN_ROWS, C + 4)) * 1e3).astype(F32)
    x[:, :C] = (rng.standard_normal((LN_ROWS, C)) * rng.uniform(0.5, 2.0, (LN_ROWS, 1)) + rng.standard_normal((LN_ROWS, 1))).astype(F32)
    x[7, :C] = (100.0 + 0.01 * rng.standard_normal(C)).astype(F32)
    g = (1.0 + 0.3 * rng.standard_normal((2, C))).astype(F32)
    b = rng.standard_normal((2, C)).astype(F32)
    sty = style(401 + C, len(LN_LENGTHS), 2 * C, 4 * C + 8, 4)  # output k: gamma at 4 + 2 C k, beta at 4 + 2 C k + C
    for a in (x, g, b):
        a.setflags(write=False)
    return x, g, b, sty


def ln_gain(C, adaptive, k):
    """effective (g, b) [9 or 1, C] float64 of output k."""
    x, g, b, sty = ln_case(C)
    if not adaptive:
        return g[k].astype(F64)[None], b[k].astype(F64)[None]
    row_utt = np.repeat(np.arange(len(LN_LENGTHS)), LN_LENGTHS)
    c0 = 4 + 2 * C * k
    return 1.0 + sty[row_utt, c0 : c0 + C].astype(F64), sty[row_utt, c0 + C : c0 + 2 * C].astype(F64)


@lru_cache(maxsize=None)
def ln_split_case(C):
    """LnIn: three split-K slices [3, slice_rows = 11, ld_part = C + 4], bias, residual window (ldr = C + 8, rcol0 4), LeakyReLU, alpha 1 / sqrt 2."""
    rng = np.random.default_rng(450 + C)
    part = (rng.standard_normal((3, LN_ROWS + 2, C + 4)) * 1e3).astype(F32)
    part[:, :LN_ROWS, :C] = rng.standard_normal((3, LN_ROWS, C)).astype(F32)
    bias = rng.standard_normal(C).astype(F32)
    r = (rng.standard_normal((LN_ROWS, C + 8)) * 1e3).astype(F32)
    r[:, 4 : 4 + C] = rng.standard_normal((LN_ROWS, C)).astype(F32)
    for a in (part, bias, r):
        a.setflags(write=False)
    return part, bias, r


RSQRT2 = float(F32(0.70710678118654752440))


def split_finish32(part, rows, C, bias, act, r, rcol0, alpha):
    """fp32 restatement IN SLICE ORDER of what splitk_reduce_kernel computes: (act(sum_k partial[k] + bias) [+ R]) * alpha - products and sums of two
    fp32 numbers, each rounded once, so numpy's fp32 arithmetic gives the kernel's bits (LeakyReLU, ReLU or no activation)."""
    v = part[0, :rows, :C].astype(F32).copy()
    for k in range(1, part.shape[0]):
        v = v + part[k, :rows, :C]
    if bias is not None:
        v = v + bias[:C]
    if act == ACT_LRELU:
        v = np.where(v >= 0, v, F32(LRELU) * v)
    elif act == ACT_RELU:
        v = np.maximum(v, F32(0))
    else:
        assert act == ACT_NONE
    if r is not None:
        v = v + r[:rows, rcol0 : rcol0 + C]
    return (v * F32(alpha)).astype(F32)


def check_ln(xin, C, eps, adaptive, k, act, y, rows=LN_ROWS, what=""):
    """y [rows, C] fp32 (output k of case C, input rows xin [rows, C] fp32) against layernorm64 within ln_bound.  -> worst error / bound."""
    g, b = ln_gain(C, adaptive, k)
    g, b = (g[:rows], b[:rows]) if adaptive else (g, b)
    x64 = xin[:rows, :C].astype(F64)
    var = x64.var(1) + eps
    want, dy = ln_bound(x64, g, b, eps, rho_rsqrt(var), act)
    e = np.abs(y[:rows] - want)
    assert (e <= dy).all(), (what, "LayerNorm", np.argwhere(e > dy)[:2], float((e / dy).max()))
    return float((e / dy).max())


# ------------------------------------------------------------------------------------------------ depthwise cases
DW0_C, DW0_K, DW0_LENGTHS = (4, 68, 128), (3, 7, 31), (1, 2, 63, 64, 65, 130)
DWLN_C, DWLN_K, DWLN_LENGTHS = (4, 260, 512), (3, 7, 15, 31), (1, 2, 15, 16, 17, 40)


@lru_cache(maxsize=None)
def dw_case(C, K, fused):
    """x [rows, ldx = C + 4], w [C, K], bias [C], style [n_utt, .] (gamma at 4, beta at 4 + C)."""
    L = DWLN_LENGTHS if fused else DW0_LENGTHS
    rng = np.random.default_rng(500 + 7 * C + K + 1000 * fused)
    x = ragged(501 + 7 * C + K + 1000 * fused, L, C, C + 4)
    w = (rng.standard_normal((C, K)) / np.sqrt(K)).astype(F32)
    b = rng.standard_normal(C).astype(F32)
    sty = style(502 + C + K, len(L), C, 2 * C + 8, 4)
    for a in (w, b):
        a.setflags(write=False)
    return L, x, w, b, sty


def check_dw0(C, K, act, y, what=""):
    L, x, w, b, _ = dw_case(C, K, False)
    want, dv = dwconv_bound(x[:, :C], L, w, b)
    if act == ACT_SILU:
        want, dv = silu_bound(want, dv, *e_exp2_rcp(want))
    e = np.abs(y[:, :C] - want)
    assert (e <= dv).all(), (what, "dwconv", np.argwhere(e > dv)[:2], float((e / dv).max()))
    return float((e / dv).max())


def dwln_ref(C, K):
    """-> y64 [rows, C], allowed error: the conv's own bound carried through the LayerNorm (eps 1e-6)."""
    L, x, w, b, sty = dw_case(C, K, True)
    v, dv = dwconv_bound(x[:, :C], L, w, b)
    row_utt = np.repeat(np.arange(len(L)), L)
    g, be = 1.0 + sty[row_utt, 4 : 4 + C].astype(F64), sty[row_utt, 4 + C : 4 + 2 * C].astype(F64)
    rho = rho_rsqrt(v.var(1) + EPS_GRN)
    return ln_bound(v, g, be, EPS_GRN, rho, ACT_NONE, dv)


# ------------------------------------------------------------------------------------------------ GRN cases
GRN_LENGTHS, GRN_C, GRN_LD = (0, 1, 31, 33, 257, 300), 130, 160
GRN_SW_C, GRN_SW_NPAD = 132, 8  # scale_weight: kc == C, a multiple of 4


@lru_cache(maxsize=None)
def grn_case():
    """slot table [n_utt, ss_stride = 12, ld_ss = 160] (sums of squares of 32 rows of N(0, s_u): non-negative; unused slots and pad columns large), gamma [C]."""
    rng = np.random.default_rng(600)
    n = len(GRN_LENGTHS)
    part = (np.abs(rng.standard_normal((n, 12, GRN_LD))) * 1e6).astype(F32)
    for u, L in enumerate(GRN_LENGTHS):
        ns = (L + 31) // 32
        s = 1e3 if u % 2 else 1.0
        part[u, :ns, :GRN_C] = (rng.chisquare(32, (ns, GRN_C)) * s * s).astype(F32)
    gamma = rng.standard_normal(GRN_C).astype(F32)
    part.setflags(write=False)
    gamma.setflags(write=False)
    return part, gamma


@lru_cache(maxsize=None)
def grn_exact_case():
    """C = 132, lengths (0, 33, 257, 40): slot sums that make gx = j / 4 EXACTLY (every slot a multiple of 2^-10, the total a perfect square), so the
    channel sum of gx is exact in fp32 in any order and 1 / (mean + 1e-6) can be restated in fp32; utterance 3 is all zeros.  w [8, 132]."""
    rng = np.random.default_rng(601)
    lengths = (0, 33, 257, 40)
    C = GRN_SW_C
    part = np.zeros((4, 9, C), F32)
    gx = np.zeros((4, C))
    for u in (1, 2):
        ns = (lengths[u] + 31) // 32
        j = rng.integers(4, 40, C)
        gx[u] = j / 4.0
        rest = rng.integers(1, 64, (ns - 1, C)) / 1024.0
        part[u, 1:ns] = rest
        part[u, 0] = gx[u] ** 2 - rest.sum(0)
        assert (part[u, 0] > 0).all() and (part[u, :ns].astype(F64).sum(0) == gx[u] ** 2).all()
    gamma = rng.standard_normal(C).astype(F32)
    w = rng.standard_normal((GRN_SW_NPAD, C)).astype(F32)
    for a in (part, gamma, w):
        a.setflags(write=False)
    return lengths, part, gx, gamma, w


def scale_weight_ref(gx_row, gamma, w):
    """-> wu64 [npad, C], allowed error 4 u |w| (|gamma gx inv| + 1); inv = 1 / (sum / C + 1e-6) restated in fp32 (the sum is exact, three roundings)."""
    C = len(gx_row)
    s = F32(gx_row.astype(F64).sum())
    assert float(s) == gx_row.astype(F64).sum()
    inv = float(F32(1.0) / (s / F32(C) + F32(1e-6)))
    t = gamma.astype(F64) * gx_row.astype(F64) * inv
    return w.astype(F64) * (t + 1.0), 4 * U * np.abs(w.astype(F64)) * (np.abs(t) + 1.0)
