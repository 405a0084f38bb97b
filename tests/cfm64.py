"""Float64 restatements of the flow-matching estimator's row kernels (csrc/cfm.hip.h) and of the encoders' sequence rotary embedding (rope_kernel,
csrc/phoneme.hip.h), the bounds the HIP kernels are held to, and the cases both tests/test_cfm64_cpu.py (numpy fp32 emulations, no GPU) and
tests/test_hip_cfm_kernels.py (the kernels, through stts_op_cfm_elem / _rms_adaln / _rope / _cfm_small / _cfm_source) run.  Test infrastructure, modelled on
tests/norm64.py.

The restatements follow the reference modules' formulas, not the kernels:
  RMSNorm + shared AdaLN   y = x / sqrt(mean_c x^2 + 1e-6) * w * (scale + 1) + shift                       models/xut/norm.py:25-40, adaln.py:19-27
  gated residual           x = X + T * (gate_prev + 1), X the NORMALISED tensor the branch was fed with     models/xut/transformer.py:67-79
  axial RoPE               pairs (2k, 2k+1) of a head turn by pos * freq[h][k], pos = torch.linspace(-1, 1, n)   models/xut/axial_rope.py:10-29,122-149
  sequence RoPE            pairs (j, j + d/2) of the first d features of a head turn by p * theta_j, theta_j = 10000^(-2j/d), p = row in the utterance
                                                                                                            models/text_encoder.py:146-168
  TimestepEmbedding        cos | sin of (1000 t) f                                                           models/xut/time_emb.py:24-31
  LayerNorm                (x - mean) / sqrt(var + 1e-5) * g + b                                             nn.LayerNorm
  Linear (+ Mish)          x W^T + b;  Mish(v) = v tanh(softplus(v)), softplus(v) = v above 20
  SwiGLU                   silu(a[:, :M]) * a[:, M:]                                                         models/xut/layers.py:23-29
  sine source              tanh(w ((0.1 sin(2 pi frac(sum_i rad_i))) uv + namp noise)), rad_i = fmod(fl(f0_i / 24000), 1), uv = f0 > 0,
                           namp = 0.003 uv + (1 - uv) 0.1 / 3, F0 / N resampled by F.interpolate's 'nearest' rule    models/cfm/cfm_mel_decoder.py:54-104,321-330
Constants the reference holds in fp32 (1e-6, 1e-5, the fp32 pi of `* 2 * np.pi`, 24000, 0.1, 0.003, 0.1 / 3) are the same fp32 numbers on both sides.  Where the
reference forms an ARGUMENT in fp32 before a transcendental (the time-embedding angle, pos * freq, p * theta) the restatement forms the same fp32 argument and
applies the function in float64: otherwise the test would measure the conditioning of sin at 1000 rad, not the kernel.

BOUNDS.  u = 2^-24.  Every bound counts the roundings of the kernel's expression to first order, in ANY summation order and with or without the compiler
contracting a product into the following sum; the factor 1.01 covers second-order terms.  Nothing here was fitted to a kernel's output.  Library functions
(cosf, sinf, expf / log1pf / tanhf as Mish, expf and the division as SiLU, tanhf, powf, sqrtf, the division) get norm64's rule `four_times_numpy`: the error
numpy's fp32 evaluation of the same expression shows against float64 on that check's own inputs, times 4 (rho_*: relative, in units of u; E_*: absolute).  A
result below the smallest normal fp32 number 2^-126 carries an absolute error of that size instead (the relative model does not hold under gradual underflow, and a
library may flush): the Mish and SwiGLU bounds add tiny = 2^-126 times the factor the result is multiplied by.

 rms_adaln      x' = x exactly, or (fused) x' = fl(x + fl(t fl(g + 1))): ex = 2 u |t (g + 1)| + u |x'|  - the bound of Xout and of gated_residual_kernel.
                q = sum x'^2: C products and C - 1 additions on non-negative terms, C u relative; / C and + eps: 2 u  =>  (C + 2) u on the root's argument;
                inv = 1 / sqrtf(.): rel_inv = 0.5 (C + 2) u + (rho_sqrt + rho_div) u.
                y = fl(fl(fl(fl(x' inv) w) fl(scale + 1)) + shift): four roundings on the product, one on the sum:
                   |core| (rel_inv + 4 u) + u |y|,  core = x' / rms w (scale + 1).
                ex reaches y through d(x_c / rms) = dx_c / rms - x_c sum_j x_j dx_j / (C rms^3):  |w (scale + 1)| (ex_c / rms + |x_c| sum_j |x_j| ex_j / (C rms^3)).
 rotary         out0 = fl(fl(a cs) - fl(b sn)), out1 = fl(fl(b cs) + fl(a sn)):  |a| dc + |b| ds + u (|a cs| + |b sn|) + u |out0|, likewise out1, with
                dc = E_cos + dang, ds = E_sin + dang (cos and sin are 1-Lipschitz) and dang the distance of the kernel's fp32 angle from the restatement's:
                axial: step = fl(2 / (n - 1)) is correctly rounded on both sides; pos = fl(-1 + fl(p step)) (or 1 - fl((n - 1 - p) step)) with or without the inner
                   rounding: both lie within u (|p step| + |pos|) of the exact expression, so within 2 u (|p step| + |pos|) of each other; ang = fl(pos freq):
                   dang = |freq| 2 u (|p step| + |pos|) + 2 u |ang|.
                sequence: theta = fl(1 / powf(10000, fl(2j / d))) against the correctly rounded 10000^-e of the same fp32 exponent e: (rho_pow + rho_div + 1) u relative;
                   ang = fl(p theta): dang = |ang| (rho_pow + rho_div + 3) u.
 time embedding a = fl(fl(1000 t) f) is two IEEE products, the same bits in numpy: |E - cos64(a)| <= E_cos, |E - sin64(a)| <= E_sin.
 small LayerNorm one wave per row: every lane adds its ceil(C / 64) elements, then six butterfly steps: an element passes through at most D = ceil(C / 64) + 5
                additions, in any order of either stage (the any-order count C - 1 would allow the mean of the mean-heavy row an error the size of the one-pass
                defect at C = 256).  With that depth norm64's LayerNorm count: dm = (D + 1) u A / C (A = sum |x|), dd = dm + u |d|,
                dM2 = C dm^2 + (D + 3) u (M2 + C dm^2), rr = 0.5 (dM2 / (C (var + eps)) + 2 u) + (rho_sqrt + rho_div) u,
                y = fl(fl(fl(d inv) g) + b):  |g| inv dd + |d inv g| (rr + 3 u) + u |y|.
                A one-pass variance E[x^2] - mean^2 is about 3 u sum x^2 away from M2 instead: at mean^2 / var = 1e4 it fails this bound at every C of the cases.
 small Linear   v = fl(sum_k x_k w_k + b): K products, K - 1 additions, the bias: dv = K u sum |x_k w_k| + u |v|;  Mish (|Mish'| <= 1.09): 1.09 dv + rho_mish u |y| + tiny |v|.
 Mish, SwiGLU   inputs exact: rho_mish u |y| + tiny |x|;  SwiGLU = fl(silu(a) b): (rho_silu + 1) u |y| + tiny |b|.
 sine source    (i) EXACT: rad, the two prefix sums in double (every partial sum of <= 4096 fp32 terms below 1 is exact in 53 bits), fmod of the fp32-rounded sum, the wrap
                flags, the angle fl(fl(fl(c2) 2) pi32) are IEEE operations: `source_exact` reproduces them bit for bit (tests/test_cfm64_cpu.py holds it to torch's CPU
                ops).  Columns 1 (N by the nearest rule) and 2 (t[u]) of har equal it bit for bit, columns 3 .. 31 are zero.
                (ii) IDEAL: the wrap shifts are integers and cancel in exact arithmetic: sine = sin(2 pi frac(sum rad)).  c2 -> fp32 with |c2| <= 1: u; * 2 exact; pi32 is
                1.47 u off pi: 2 * 1.47 u; the product: u |ang| <= 2 pi u  =>  the angle is (2 pi + 2.93 + 2 pi) u = 15.5 u off, then E_sin.  One more rounding belongs to
                the count: the term fl(rad + shift) is an fp32 sum, and rad - 1 in (-1, -0.5) is rounded to a multiple of u: u / 2 per wrap, pi u on the angle, and
                the errors of the W_i wraps up to frame i add up in the prefix sum  =>  ds_i = (15.5 + pi W_i) u + E_sin, W from the restatement's flags.  (Without
                that term the REFERENCE's own arithmetic - torch's CPU ops, which (i) reproduces bit for bit - is 688 u from the ideal at the end of the constant-F0
                utterance of 1100 frames, 219 wraps, where every rounding has the same sign, and 20 u at 4000 frames of a voiced curve: test_cfm64_cpu.py prints both.)
                sw = fl(fl(fl(sine 0.1) uv) + fl(namp noise)):  dsw = 0.1 uv ds + u |0.1 sine uv| + u |namp noise| + u |sw|;  z = fl(sw w): dz = |w| dsw + u |z|;
                tanh is 1-Lipschitz: dz + rho_tanh u |tanh z|.  No element is left out.
                (iii) Column 0 against (i)'s own fp32 angle: the same chain with ds = E_sin alone.  This is the check that sees a wrong wrap flag: an integer shift of c2
                moves the ideal form by nothing and the fp32 angle by the coarser rounding of a larger c2.
"""
from __future__ import annotations

import numpy as np

from norm64 import F32, F64, SLACK, U, four_times_numpy, offsets, round_up  # noqa: F401  (re-exported for the tests)

EPS_RMS, EPS_LN = float(F32(1e-6)), float(F32(1e-5))
PI32 = F32(3.14159265358979323846)
SR32, AMP32, NSTD32, THIRD32 = F32(24000.0), F32(0.1), F32(0.003), F32(3.0)
TINY = 2.0 ** -126
MISH_LIP = 1.09
SENT32 = np.uint32(0x7FC0BEEF)


def ratio(got, want, bound):
    """largest |got - want| / bound; a NaN (a sentinel left in place) or an error on a zero bound counts as infinite."""
    e = np.abs(np.asarray(got, F64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, e / bound, np.where(e == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def _rel(got32, want64):
    """four_times_numpy in units of u, on the results that are normal numbers (below 2^-126 the bound's absolute term takes over)."""
    got, want = np.asarray(got32, F64).ravel(), np.asarray(want64, F64).ravel()
    ok = np.abs(want) >= TINY / U
    return four_times_numpy(got[ok], want[ok]) / U


def rho_sqrt_div(arg64):
    """sqrtf and the division of 1 / sqrtf(arg), relative, in u."""
    a32 = np.asarray(arg64, F64).astype(F32)
    s32 = np.sqrt(a32)
    return _rel(s32, np.sqrt(a32.astype(F64))), _rel(F32(1) / s32, 1.0 / s32.astype(F64))


def e_cos_sin(ang32):
    a = np.asarray(ang32, F32)
    return four_times_numpy(np.cos(a), np.cos(a.astype(F64)), relative=False), four_times_numpy(np.sin(a), np.sin(a.astype(F64)), relative=False)


# ------------------------------------------------------------------------------------------------ Mish, SiLU
def mish64(v):
    v = np.asarray(v, F64)
    with np.errstate(over="ignore"):
        sp = np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 700.0))))
    return v * np.tanh(sp)


def mish32(v):
    """numpy fp32 evaluation of v tanh(softplus(v)), softplus with F.softplus's threshold (the expression four_times_numpy measures)."""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        sp = np.where(v > F32(20), v, np.log1p(np.exp(v)))
        return (v * np.tanh(sp)).astype(F32)


def silu64(a):
    a = np.asarray(a, F64)
    with np.errstate(over="ignore"):
        return a / (1.0 + np.exp(-a))


def silu32(a):
    a = np.asarray(a, F32)
    with np.errstate(over="ignore"):
        return (a / (F32(1) + np.exp(-a))).astype(F32)


def mish_bound(x32):
    """-> mish64(x), bound, rho_mish (u)."""
    want = mish64(x32)
    rho = _rel(mish32(x32), want)
    return want, SLACK * (rho * U * np.abs(want) + TINY * np.abs(np.asarray(x32, F64))), rho


def swiglu64(a, M):
    a = np.asarray(a, F64)
    return silu64(a[:, :M]) * a[:, M:]


def swiglu_bound(a32, M):
    g, b = a32[:, :M], np.asarray(a32[:, M:], F64)
    s = silu64(g)
    rho = _rel(silu32(g), s)
    want = s * b
    return want, SLACK * ((rho + 1) * U * np.abs(want) + TINY * np.abs(b)), rho


# ------------------------------------------------------------------------------------------------ RMSNorm + AdaLN, gated residual
def rows_of(table, lengths):
    """[n_utt, K] per-utterance rows -> [rows, K]."""
    return np.repeat(np.asarray(table, F64), lengths, axis=0)


def gated_residual_bound(h, t, gate):
    """h, t [R, C], gate [R, C] (per row) -> x' = h + t (gate + 1) in float64 and the bound ex."""
    h, t, gate = (np.asarray(a, F64) for a in (h, t, gate))
    g1 = t * (gate + 1.0)
    xp = h + g1
    return xp, SLACK * (2 * U * np.abs(g1) + U * np.abs(xp))


def rms_adaln_bound(x, w, scale, shift, t=None, gate=None):
    """x [R, C], w [C], scale / shift / gate [R, C] (the utterance's AdaLN rows) -> dict(xp, y, bx, by, rho_sqrt, rho_div) in float64."""
    x, w, scale, shift = (np.asarray(a, F64) for a in (x, w, scale, shift))
    C = x.shape[1]
    if t is None:
        xp, ex = x, np.zeros_like(x)
    else:
        xp, ex = gated_residual_bound(x, t, gate)
        ex = ex / SLACK
    arg = (xp * xp).mean(1, keepdims=True) + EPS_RMS
    rms = np.sqrt(arg)
    rs, rd = rho_sqrt_div(arg)
    rel_inv = 0.5 * (C + 2) * U + (rs + rd) * U
    k = w * (scale + 1.0)
    core = xp / rms * k
    y = core + shift
    prop = np.abs(k) * (ex / rms + np.abs(xp) * (np.abs(xp) * ex).sum(1, keepdims=True) / (C * rms ** 3))
    by = SLACK * (np.abs(core) * (rel_inv + 4 * U) + U * np.abs(y) + prop)
    return dict(xp=xp, y=y, bx=SLACK * ex, by=by, rho_sqrt=rs, rho_div=rd)


RMS_C = (32, 96, 128, 512, 1024)
RMS_LENGTHS = (1, 5, 0, 4, 7)
RMS_MODES = ("plain", "fused", "fused_xout", "alias")


def big_rows(lengths):
    """[rows, 1] factor: the odd utterances are 1e3 times larger than the even ones."""
    return np.repeat(np.where(np.arange(len(lengths)) % 2, 1e3, 1.0), lengths)[:, None].astype(F32)


def rms_case(C):
    """x [R + 2, C + 32] (two guard rows, 32 pad columns, all 1e3 large), t [R, C], w, ada / ada_prev [n_utt, 3 C] (distinct tables, distinct rows)."""
    L = RMS_LENGTHS
    R = sum(L)
    rng = np.random.default_rng(1000 + C)
    x = (rng.standard_normal((R + 2, C + 32)) * 1e3).astype(F32)
    x[:R, :C] = rng.standard_normal((R, C)).astype(F32) * big_rows(L)
    t = rng.standard_normal((R, C)).astype(F32) * big_rows(L)
    w = (1.0 + 0.3 * rng.standard_normal(C)).astype(F32)
    ada = (rng.standard_normal((len(L), 3 * C)) * 0.5).astype(F32)
    ada_prev = (rng.standard_normal((len(L), 3 * C)) * 0.5).astype(F32)
    for a in (x, t, w, ada, ada_prev):
        a.setflags(write=False)
    return dict(C=C, lengths=L, R=R, x=x, t=t, w=w, ada=ada, ada_prev=ada_prev)


def rms_check(case, mode, y, xout=None):
    """y [R, C] as the launch left it (xout [R, C] in mode fused_xout) -> dict of error / bound."""
    C, L, R = case["C"], case["lengths"], case["R"]
    a = rows_of(case["ada"], L)
    fused = mode in ("fused", "fused_xout")
    b = rms_adaln_bound(case["x"][:R, :C], case["w"], a[:, :C], a[:, C : 2 * C], case["t"] if fused else None, rows_of(case["ada_prev"], L)[:, 2 * C :] if fused else None)
    out = dict(y=ratio(y, b["y"], b["by"]))
    if xout is not None:
        out["xout"] = ratio(xout, b["xp"], b["bx"])
    return out


GATED_CASES = ((32, (5, 0, 3)), (1024, (1100, 0, 3)))  # (C, lengths); 1100 rows x 256 float4s = 1100 blocks: the grid cap of 1024 is exceeded


def gated_case(C, lengths):
    R = sum(lengths)
    rng = np.random.default_rng(1100 + C)
    h = rng.standard_normal((R + 1, C)).astype(F32)
    h[:R] *= big_rows(lengths)
    t = rng.standard_normal((R + 1, C)).astype(F32)
    ada = (rng.standard_normal((len(lengths), 3 * C)) * 0.5).astype(F32)
    ada[:, : 2 * C] *= F32(1e3)  # scale | shift: a gate read from the wrong third cannot hide
    return dict(C=C, lengths=lengths, R=R, h=h, t=t, ada=ada)


def gated_check(case, y):
    C, L, R = case["C"], case["lengths"], case["R"]
    want, b = gated_residual_bound(case["h"][:R], case["t"][:R], rows_of(case["ada"], L)[:, 2 * C :])
    return ratio(y, want, b)


# ------------------------------------------------------------------------------------------------ rotary embeddings
def linspace32(n):
    """torch.linspace(-1, 1, n) in fp32: ATen's two-sided formula with the product fused into the sum (one rounding; tests/test_cfm64_cpu.py holds this to torch bit
    for bit).  -> pos fp32, |p step| float64 (the bound's term)."""
    if n == 1:
        return np.full(1, -1, F32), np.zeros(1)
    step = F64(F32(2) / F32(n - 1))
    p = np.arange(n)
    lo, hi = (-1.0 + p * step).astype(F32), (1.0 - (n - 1 - p) * step).astype(F32)  # (the product of an integer below 2^24 and an fp32 number is exact in double)
    return np.where(p < n // 2, lo, hi).astype(F32), np.where(p < n // 2, p, n - 1 - p) * step


def axial_angles(lengths, freq32):
    """freq [heads, d/2] fp32 -> ang32 [R, heads, d/2] (fp32 products of the fp32 positions) and dang, the allowed distance of the kernel's angle."""
    pos, ps = zip(*(linspace32(n) for n in lengths if n > 0))
    pos, ps = np.concatenate(pos), np.concatenate(ps)
    ang = (pos[:, None, None] * freq32[None]).astype(F32)
    dang = np.abs(freq32.astype(F64))[None] * (2 * U * (ps + np.abs(pos.astype(F64))))[:, None, None] + 2 * U * np.abs(ang.astype(F64))
    return ang, dang


def seq_angles(lengths, d):
    """-> ang32 [R, d/2] = fl(p theta), theta the correctly rounded 10000^-fl(2j/d), and dang."""
    e32 = (2 * np.arange(d // 2)).astype(F32) / F32(d)
    p64 = np.power(10000.0, e32.astype(F64))
    theta = (1.0 / p64).astype(F32)
    rp = _rel(np.power(F32(10000), e32), p64)
    rd = _rel(F32(1) / p64.astype(F32), 1.0 / p64.astype(F32).astype(F64))
    p = np.concatenate([np.arange(n) for n in lengths]).astype(F32)
    ang = (p[:, None] * theta[None]).astype(F32)
    return ang, np.abs(ang.astype(F64)) * (rp + rd + 3) * U, (rp, rd)


def rotate_bound(a, b, ang32, dang):
    """the pair (a, b) turned by ang: -> out0, out1 (float64 of the fp32 angle), their bounds."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    ec, es = e_cos_sin(ang32)
    ang = ang32.astype(F64)
    cs, sn = np.cos(ang), np.sin(ang)
    o0, o1 = a * cs - b * sn, b * cs + a * sn
    dc, ds = ec + dang, es + dang
    b0 = SLACK * (np.abs(a) * dc + np.abs(b) * ds + U * (np.abs(a * cs) + np.abs(b * sn)) + U * np.abs(o0))
    b1 = SLACK * (np.abs(b) * dc + np.abs(a) * ds + U * (np.abs(b * cs) + np.abs(a * sn)) + U * np.abs(o1))
    return o0, o1, b0, b1


def rope64(x, lengths, kind, col, heads, kc, d, freq32=None):
    """The block [col, col + heads kc) of x [R, ld] turned: -> want [R, heads, d], bound [R, heads, d] (features d .. kc - 1 are not touched)."""
    R = sum(lengths)
    blk = np.asarray(x[:R, col : col + heads * kc], F64).reshape(R, heads, kc)[:, :, :d]
    half = d // 2
    if kind == 0:
        ang, dang = axial_angles(lengths, freq32)
        a, b = blk[:, :, 0::2], blk[:, :, 1::2]
    else:
        ang, dang, _ = seq_angles(lengths, d)
        ang, dang = np.broadcast_to(ang[:, None], (R, heads, half)), np.broadcast_to(dang[:, None], (R, heads, half))
        a, b = blk[:, :, :half], blk[:, :, half:]
    o0, o1, b0, b1 = rotate_bound(a, b, np.ascontiguousarray(ang), dang)
    want, bound = np.empty_like(blk), np.empty_like(blk)
    if kind == 0:
        want[:, :, 0::2], want[:, :, 1::2], bound[:, :, 0::2], bound[:, :, 1::2] = o0, o1, b0, b1
    else:
        want[:, :, :half], want[:, :, half:], bound[:, :, :half], bound[:, :, half:] = o0, o1, b0, b1
    return want, bound


AXIAL_SHAPES = ((2, 64), (4, 64), (8, 64), (2, 8))
AXIAL_LENGTHS = (1, 2, 3, 37, 800)
AXIAL_STRIDE = (8, 64, (1100,))  # 8 heads x 1100 rows x 32 pairs = 1100 blocks of 256: the grid cap of 1024 is exceeded
SEQ_SHAPES = ((8, 16, 8), (2, 96, 48), (2, 160, 80), (8, 40, 20))
SEQ_LENGTHS = (1, 33, 512)


def axial_freq(heads, d):
    """exp(linspace(log pi, log 5 pi)) per head, heads differing (head h scaled by 1 + h / 16)."""
    f = np.exp(np.linspace(np.log(np.pi), np.log(5 * np.pi), d // 2))
    return (f[None] * (1.0 + np.arange(heads)[:, None] / 16.0)).astype(F32)


def rope_case(kind, heads, kc, lengths, two_blocks):
    """x [R + 1, ld]: two_blocks: a q | k | v buffer of ld = 3 dim (col0 0, col1 dim), else ld = dim + 32 with the block at column 16 (col1 -1)."""
    dim, R = heads * kc, sum(lengths)
    rng = np.random.default_rng(1200 + 7 * heads + kc + R + 2 * two_blocks + kind)
    ld, col0, col1 = (3 * dim, 0, dim) if two_blocks else (dim + 32, 16, -1)
    x = (rng.standard_normal((R + 1, ld)) * 1e3).astype(F32)
    for c in (col0, col1):
        if c >= 0:
            x[:R, c : c + dim] = rng.standard_normal((R, dim)).astype(F32) * big_rows(lengths)
    x.setflags(write=False)
    return dict(x=x, ld=ld, col0=col0, col1=col1, R=R, lengths=lengths, heads=heads, kc=kc, kind=kind)


def rope_check(case, d, got, freq32=None):
    """got [R + 1, ld] after the launch: the turned features within their bound, EVERYTHING else bit-identical -> error / bound."""
    x, R, heads, kc = case["x"], case["R"], case["heads"], case["kc"]
    touched = np.zeros(x.shape, bool)
    worst = 0.0
    for col in (case["col0"], case["col1"]):
        if col < 0:
            continue
        want, bound = rope64(x, case["lengths"], case["kind"], col, heads, kc, d, freq32)
        blk = got[:R, col : col + heads * kc].reshape(R, heads, kc)[:, :, :d]
        worst = max(worst, ratio(blk, want, bound))
        m = np.zeros((R, heads, kc), bool)
        m[:, :, :d] = True
        touched[:R, col : col + heads * kc] = m.reshape(R, heads * kc)
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(x).view(np.uint32)
    assert same[~touched].all(), ("written outside the turned features", np.argwhere(~same & ~touched)[:4])
    return worst


# ------------------------------------------------------------------------------------------------ the per-utterance kernels
TIME_HALF, TIME_U, TIME_T = (64, 128, 256), (1, 3), (0.0, 1e-3, 0.5, 1.0)


def time_freqs(half):
    """TimestepEmbedding's table exp(-log(10000) k / half) in fp32."""
    return np.exp(-np.log(10000.0) * np.arange(half) / half).astype(F32)


def time_embed_bound(t32, freqs32):
    """-> want [U, 2 half] (cos | sin in float64 of the fp32 angle), bound (E_cos | E_sin)."""
    a = ((F32(1000) * np.asarray(t32, F32))[:, None] * freqs32[None]).astype(F32)
    ec, es = e_cos_sin(a)
    a = a.astype(F64)
    want = np.concatenate([np.cos(a), np.sin(a)], 1)
    half = freqs32.shape[0]
    return want, SLACK * np.concatenate([np.full((len(t32), half), ec), np.full((len(t32), half), es)], 1)


def layernorm_small_bound(x, g, b):
    """x [rows, C] -> y64, bound (module docstring: small LayerNorm)."""
    x, g, b = (np.asarray(a, F64) for a in (x, g, b))
    C = x.shape[1]
    A = np.abs(x).sum(1, keepdims=True)
    mean = x.mean(1, keepdims=True)
    d = x - mean
    m2 = (d * d).sum(1, keepdims=True)
    var = m2 / C + EPS_LN
    inv = 1.0 / np.sqrt(var)
    rs, rd = rho_sqrt_div(var)
    D = (C + 63) // 64 + 5
    dm = (D + 1) * U * A / C
    dd = dm + U * np.abs(d)
    dm2 = C * dm * dm + (D + 3) * U * (m2 + C * dm * dm)
    rr = 0.5 * (dm2 / (C * var) + 2 * U) + (rs + rd) * U
    y = d * inv * g + b
    return y, SLACK * (np.abs(g) * inv * dd + np.abs(d * inv * g) * (rr + 3 * U) + U * np.abs(y))


LN_C = (32, 100, 256)


def layernorm_case(C):
    """three rows: N(0, 1), a mean-heavy one (mean 100, deviation 1: mean^2 / var = 1e4), one 1e3 times larger; ldx = C + 8 with large pads."""
    rng = np.random.default_rng(1300 + C)
    x = (rng.standard_normal((3, C + 8)) * 1e3).astype(F32)
    x[0, :C] = rng.standard_normal(C)
    x[1, :C] = 100.0 + rng.standard_normal(C)
    x[2, :C] = 1e3 * rng.standard_normal(C)
    g = (1.0 + 0.3 * rng.standard_normal(C)).astype(F32)
    b = rng.standard_normal(C).astype(F32)
    return dict(C=C, x=x, g=g, b=b)


LINEAR_NK = ((256, 48), (5, 100), (3, 64), (64, 10240))
LINEAR_ROWS = (1, 3)


def linear_case(N, K, rows):
    rng = np.random.default_rng(1400 + N + K + rows)
    x = (rng.standard_normal((rows, K + 8)) * 1e3).astype(F32)  # (pad columns 1e3 large)
    # outputs of order 8, of order 32 in the odd row: Mish on both branches of the softplus threshold and on the negative tail
    x[:, :K] = rng.standard_normal((rows, K)).astype(F32) * np.where(np.arange(rows) % 2, 4.0, 1.0)[:, None].astype(F32)
    w = (rng.standard_normal((N, K)) * (8.0 / np.sqrt(K))).astype(F32)
    b = (rng.standard_normal(N) * 4).astype(F32)
    return dict(N=N, K=K, rows=rows, x=x, w=w, b=b)


def linear_bound(x, w, b, act):
    """x [rows, K], w [N, K], b [N] or None -> y64, bound, rho_mish."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    K = x.shape[1]
    v = x @ w.T + (0.0 if b is None else np.asarray(b, F64))
    dv = K * U * (np.abs(x) @ np.abs(w).T) + U * np.abs(v)
    if act == 0:
        return v, SLACK * dv, 0.0
    y = mish64(v)
    rho = _rel(mish32(v.astype(F32)), mish64(v.astype(F32)))
    return y, SLACK * (MISH_LIP * dv + rho * U * np.abs(y) + TINY * np.abs(v)), rho


def mish_grid():
    """[-100, 100]: a uniform grid, 0, -0, 20 and its two fp32 neighbours, the exp overflow edges; padded to a multiple of 4."""
    edge = np.array([0.0, -0.0, 20.0, np.nextafter(F32(20), F32(21)), np.nextafter(F32(20), F32(19)), 88.0, -88.0, 88.8, -88.8, 100.0, -100.0, -103.9, -87.3], F32)
    g = np.concatenate([np.linspace(-100, 100, 4001).astype(F32), edge])
    return np.concatenate([g, np.zeros(-len(g) % 4, F32)])


MISH_LONG = 4 * (2048 * 256 + 3)  # floats: 2048 * 256 + 3 float4s: the capped grid of 2048 blocks strides once and ends on a tail of 3
SWIGLU_CASES = ((4, 5), (512, 7), (2048, 1100))  # (M, rows); 1100 x 512 float4s = 2200 blocks: the grid cap of 2048 is exceeded


def swiglu_case(M, rows):
    rng = np.random.default_rng(1500 + M)
    a = (rng.standard_normal((rows, 2 * M)) * 4).astype(F32)
    a[:, M:] *= F32(3)  # the halves differ in scale: swapped halves cannot hide
    edge = np.array([88.0, -88.0, 100.0, -100.0], F32)
    a[0, :4] = edge
    a[-1, M - 4 : M] = edge
    return a


# ------------------------------------------------------------------------------------------------ sine source
def nearest_idx(n, L):
    """F.interpolate(mode='nearest'): source index of each of n frames on a curve of L points (fp32 scale, floor, clipped)."""
    if L == n:
        return np.arange(n)
    scale = F32(L) / F32(n)
    return np.minimum(np.floor((np.arange(n).astype(F32) * scale).astype(F32)).astype(np.int64), L - 1)


def source_exact(f0r):
    """f0r: fp32 F0 per frame (already resampled).  -> dict(rad, flag, c2 (float64, exact), ang (fp32)): IEEE operations only, bit for bit what torch's CPU ops give
    (tests/test_cfm64_cpu.py) and what cfm_source_kernel's contract states."""
    f0r = np.asarray(f0r, F32)
    n = len(f0r)
    rad = np.fmod((f0r / SR32).astype(F32), F32(1))
    c1 = np.cumsum(rad.astype(F64))
    tmp = np.fmod(c1.astype(F32), F32(1))
    flag = np.zeros(n, bool)
    flag[1:] = (tmp[1:] - tmp[:-1]) < 0
    term = (rad + np.where(flag, F32(-1), F32(0))).astype(F32)
    c2 = np.cumsum(term.astype(F64))
    ang = ((c2.astype(F32) * F32(2)).astype(F32) * PI32).astype(F32)
    return dict(rad=rad, flag=flag, c2=c2, ang=ang)


def noise_amp32(f0r):
    uv = (np.asarray(f0r, F32) > 0).astype(F32)
    return uv, (uv * NSTD32 + ((F32(1) - uv) * AMP32).astype(F32) / THIRD32).astype(F32)


def _source_chain(sine, ds, f0r, noise, w):
    """tanh(w (0.1 sine uv + namp noise)) in float64 and its bound for a sine that is ds off (module docstring, sine source (ii))."""
    uv, namp = noise_amp32(f0r)
    uv, namp, amp, w = uv.astype(F64), namp.astype(F64), float(AMP32), float(F32(w))
    noise = np.asarray(noise, F64)
    sw = sine * amp * uv + namp * noise
    dsw = amp * uv * ds + U * np.abs(sine * amp * uv) + U * np.abs(namp * noise) + U * np.abs(sw)
    z = sw * w
    dz = abs(w) * dsw + U * np.abs(z)
    y = np.tanh(z)
    z32 = z.astype(F32)
    rt = _rel(np.tanh(z32), np.tanh(z32.astype(F64)))
    return y, SLACK * (dz + rt * U * np.abs(y)), rt


def source_angle_bound_u(flag):
    """Allowed distance, in u, of the fp32 angle from 2 pi frac(sum rad) per frame: 15.5 + pi W_i (module docstring)."""
    return 4 * np.pi + 2 * abs(float(PI32) - np.pi) / U + np.pi * np.cumsum(flag)


def source_ideal_bound(f0r, noise, w):
    """Column 0 of har for one utterance: the ideal form and its counted bound (module docstring, sine source (ii))."""
    f0r = np.asarray(f0r, F32)
    e = source_exact(f0r)
    c = np.cumsum(e["rad"].astype(F64))  # exact: <= 4096 fp32 terms below 1
    ang = 2.0 * np.pi * (c - np.floor(c))
    es = four_times_numpy(np.sin(ang.astype(F32)), np.sin(ang.astype(F32).astype(F64)), relative=False)
    y, bound, rt = _source_chain(np.sin(ang), source_angle_bound_u(e["flag"]) * U + es, f0r, noise, w)
    return y, bound, dict(e_sin=es, rho_tanh=rt)


def source_exact_bound(f0r, noise, w):
    """Column 0 against the restatement's own fp32 angle (module docstring, sine source (iii))."""
    e = source_exact(f0r)
    es = four_times_numpy(np.sin(e["ang"]), np.sin(e["ang"].astype(F64)), relative=False)
    y, bound, _ = _source_chain(np.sin(e["ang"].astype(F64)), es, f0r, noise, w)
    return y, bound


SRC_FRAMES = (1, 7, 255, 256, 257, 1100)
SRC_CURVES = (1, 20, 255, 100, 514, 1100)
SRC_WRAP_HZ = F32(0.1999 * 24000.0)  # rad = 0.1999: at 1100 frames (5 per thread) the phase wraps at frame 5 k, the first of thread k, for every k < 220


def source_case(w_sign=1.0):
    """Six utterances in one packed call: frames 1, 7, 255, 256, 257, 1100 (1, 1, 1, 1, 2 and 5 frames per thread) from curves of 1, 20, 255, 100, 514 and 1100
    points.  F0 from synth.pitch_curve (unvoiced stretches); the last utterance has the constant F0 whose phase wraps exactly at every chunk boundary."""
    from stylish_tts_amd import synth

    rng = np.random.default_rng(1600)
    f0 = [synth.pitch_curve(f"cfm64.src.{u}", 1, L, seed=3)[0].astype(F32) for u, L in enumerate(SRC_CURVES)]
    f0[0] = np.array([220.0], F32)
    f0[-1] = np.full(SRC_CURVES[-1], SRC_WRAP_HZ, F32)
    ncurve = [rng.standard_normal(L).astype(F32) * (1e3 if u % 2 else 1.0) for u, L in enumerate(SRC_CURVES)]
    ncurve = [a.astype(F32) for a in ncurve]
    t = rng.uniform(0, 1, len(SRC_FRAMES)).astype(F32)
    noise = [rng.standard_normal(n).astype(F32) for n in SRC_FRAMES]
    return dict(frames=SRC_FRAMES, curves=SRC_CURVES, f0=f0, ncurve=ncurve, t=t, noise=noise, w=F32(w_sign * 0.8))


def source_check(case, u, har):
    """har [n, 32] of utterance u as the launch left it: check (i) on columns 1 .. 31 (bits), checks (ii) and (iii) on column 0 -> their error / bound."""
    n, L = case["frames"][u], case["curves"][u]
    idx = nearest_idx(n, L)
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(har[:, 1]), bits(case["ncurve"][u][idx])), ("column 1 is not N by the nearest rule", u)
    assert np.array_equal(bits(har[:, 2]), bits(np.full(n, case["t"][u], F32))), ("column 2 is not t[u]", u)
    assert (bits(har[:, 3:]) == 0).all(), ("columns 3 .. 31 are not zero", u)
    want, bound, _ = source_ideal_bound(case["f0"][u][idx], case["noise"][u], case["w"])
    want3, bound3 = source_exact_bound(case["f0"][u][idx], case["noise"][u], case["w"])
    return dict(ideal=ratio(har[:, 0], want, bound), exact=ratio(har[:, 0], want3, bound3))
