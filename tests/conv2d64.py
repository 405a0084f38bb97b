"""The 2-D implicit-GEMM convolution (csrc/conv2d.hip.h) restated in float64, the bound its kernels are held to, the packers between dense arrays and
the engine's rows, and the cases tests/test_conv2d64_cpu.py (numpy fp32 emulations, no GPU) and tests/test_hip_conv2d.py (the kernels, through
stts_op_conv2d) both run.  Test infrastructure.

THE OPERATION, per utterance, on dense arrays x_s [T][Fin][C_s] (one per segment) and a base grid of T_b x F positions:
  1. x is zero outside [0, T) x [0, Fin);
  2. tap i of base position (t, f) reads (t + dt[i], f + df[i]);
  3. the operand is cat(x_0, x_1) over channels (w [cout][C_0 + C_1][ntap]);
  4. optionally LeakyReLU(0.2) on the operand (the fp32 number 0.2f on both sides, as in norm64.py);
  5. v = sum + bias; v = act(v) (none, ReLU, sigmoid); v += residual at the OUTPUT position; v /= div;
  6. the result is the output grid's position (t * up + pt, f * up + pf); the output grid is T_b up x F up.
Nothing here follows the kernel: `gather` builds the [T_b][F][ntap][C] operand by slicing, the contraction is one einsum.

ENGINE ROWS.  A level's activation is rows ((off[u] >> sh) + t) * F + f of ld floats, channels first, then pad channels (pack_rows fills them with finite
1e3-scale values: the packed weights there must be zero).  The output rows (t' up + pt) * (F up) + f up + pf, t' the base time row within the batch, are
the dense [sum T_b up][F up][ldy] array of the utterances one after the other in time (pack_grid / the reshape in `expected`).

THE BOUND.  u = 2^-24.  Per output element, S = sum |x_i w_i| over the non-zero products (x after the LeakyReLU):
  accumulation  K is cut into n_chunks chains of `chunk` in the engine's K order (tap-major, per tap ld0 + ld1 columns of which the pad columns multiply
                exact zeros and in-range taps only count).  A chain of n non-zero products is off by at most n u (sum of its |products|) IN ANY ORDER
                and whether or not the products are fused (n - 1 additions, plus one rounding of a product that is not fused), so with L the largest n of
                the element's chains every chain is within L u (its share of S); adding the n_chunks chain sums in any order costs at most n_chunks u S
                more.  LeakyReLU on the operand is ONE rounded product 0.2f * x per negative operand (the constant is the same fp32 number on both sides),
                a relative perturbation of at most u of that product: c = 1 with the LeakyReLU, 0 without.
                   dv = (L + n_chunks + c) u S
  epilogue      one rounding of the running value per step: + bias: u |v|; ReLU: exact, slope <= 1; + residual: u |v|; / div: dv / |div| + u |v| (div = 1:
                exact, nothing added).
  sigmoid       1 / (1 + expf(-v)): slope <= 1 / 4 on the incoming dv; e = expf(-v): E_exp relative, weighted e / (1 + e) in the result; 1 + e: u; the
                reciprocal: E_rcp.  E_exp and E_rcp are 4 x the error numpy's fp32 exp and 1 / x show against float64 on the same arguments (norm64.py:
                ULP FIGURES - the ROCm install documents no figure, so the reference sets the number, not the kernel); + 2^-126 where the result could
                leave the normal range (the cases keep |v| < 80, so it never does).
First order; nothing here was fitted to a kernel's output.  The inputs are of order 1 (and 1e3 in the odd utterances), no product or partial sum is
subnormal, so flush-to-zero is not in play.
"""
from __future__ import annotations

import zlib
from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
LRELU = float(F32(0.2))
ACT_NONE, ACT_RELU, ACT_SIGMOID = range(3)  # csrc/conv2d.hip.h: CONV_ACT_*
BK = 16  # kConvBK: the K step; every row stride is a multiple of it
MAX_TAPS = 25
BIG = 1e3  # the odd utterances and the pad channels


def round_up(a, b):
    return (a + b - 1) // b * b


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ taps
def taps_same(k):
    """k x k, zero padding (k - 1) / 2, row-major as torch's weight[:, :, i, j]."""
    p = (k - 1) // 2
    return [i - p for i in range(k) for _ in range(k)], [j - p for _ in range(k) for j in range(k)]


def taps_valid(k):
    """k x k without padding: the base grid is (T - k + 1) x (Fin - k + 1)."""
    return [i for i in range(k) for _ in range(k)], [j for _ in range(k) for j in range(k)]


def up_axis(p):
    """One axis of ConvTranspose(k = 3, stride = 2, padding = 1, output_padding = 1): input i and kernel index k reach output o = 2 i - 1 + k, so output
    2 t + p takes input t + d with k = p + 1 - 2 d wherever that is a kernel index -> [(d, k)]."""
    return [(d, p + 1 - 2 * d) for d in (-1, 0, 1) if 0 <= p + 1 - 2 * d < 3]


def subpixel(wt, pt, pf):
    """wt [cin][cout][3][3] (ConvTranspose2d's layout) -> dt, df, w [cout][cin][ntap] of the sub-pixel convolution that yields outputs (2 t + pt, 2 f + pf)."""
    dt, df, cols = [], [], []
    for a, ka in up_axis(pt):
        for b, kb in up_axis(pf):
            dt.append(a)
            df.append(b)
            cols.append(wt[:, :, ka, kb].T)
    return dt, df, np.ascontiguousarray(np.stack(cols, axis=2))


# ------------------------------------------------------------------------------------------------ the operation
def gather(x, dt, df, T_out, F):
    """x [T][Fin][C] -> [T_out][F][ntap][C]: tap i of (t, f) is x[t + dt[i], f + df[i]], zero outside [0, T) x [0, Fin)."""
    T, Fin, C = x.shape
    out = np.zeros((T_out, F, len(dt), C), x.dtype)
    for i, (a, b) in enumerate(zip(dt, df)):
        t0, t1, f0, f1 = max(0, -a), min(T_out, T - a), max(0, -b), min(F, Fin - b)
        if t1 > t0 and f1 > f0:
            out[t0:t1, f0:f1, i] = x[t0 + a : t1 + a, f0 + b : f1 + b]
    return out


def operand64(segs, lrelu):
    x = np.concatenate([np.asarray(s, F64) for s in segs], axis=2)
    return np.where(x >= 0.0, x, LRELU * x) if lrelu else x


def sigmoid_figures(v64):
    """Allowed relative errors of expf and of the reciprocal on the arguments the sigmoid of v gives them: 4 x numpy fp32 against float64."""
    v32 = np.asarray(v64, F64).astype(F32)
    e32 = np.exp(-v32)
    s32 = (F32(1.0) + e32).astype(F32)

    def four(got, want):
        return 4.0 * float((np.abs(got.astype(F64) - want) / np.abs(want)).max()) if want.size else 0.0

    return four(e32, np.exp(-v32.astype(F64))), four(F32(1.0) / s32, 1.0 / s32.astype(F64))


def conv2d64(segs, w, dt, df, T_out, F, *, lrelu=False, bias=None, act=ACT_NONE, res=None, div=1.0, up=1, pt=0, pf=0, count=None):
    """One utterance: segs = dense [T][Fin][C_s] arrays, w [cout][sum C_s][ntap] -> the base grid's results [T_out][F][cout] in float64 (position (t, f) is
    the output grid's (t up + pt, f up + pf); res is that grid, [T_out up][F up][cout]).
    count = (L [T_out][F], n_chunks): also the allowed error of the module docstring, -> (result, bound)."""
    w = np.asarray(w, F64)
    A = gather(operand64(segs, lrelu), dt, df, T_out, F)
    v = np.einsum("tfkc,nck->tfn", A, w)
    dv = None
    if count is not None:
        S = np.einsum("tfkc,nck->tfn", np.abs(A), np.abs(w))
        dv = (count[0][:, :, None] + count[1] + (1 if lrelu else 0)) * U * S
    if bias is not None:
        v = v + np.asarray(bias, F64)
        if dv is not None:
            dv = dv + U * np.abs(v)
    if act == ACT_RELU:
        v = np.maximum(v, 0.0)
    elif act == ACT_SIGMOID:
        assert np.abs(v).max(initial=0.0) < 80.0, "the sigmoid cases stay inside expf's normal range"
        y = 1.0 / (1.0 + np.exp(-v))
        if dv is not None:
            e_exp, e_rcp = sigmoid_figures(v)
            dv = 0.25 * dv + (e_exp / (1.0 + np.exp(v)) + U + e_rcp) * y + 2.0 ** -126
        v = y
    else:
        assert act == ACT_NONE, act
    if res is not None:
        v = v + np.asarray(res, F64)[pt::up, pf::up][:T_out, :F]
        if dv is not None:
            dv = dv + U * np.abs(v)
    if div != 1.0:
        v = v / div
        if dv is not None:
            dv = dv / abs(div) + U * np.abs(v)
    return v if count is None else (v, dv)


def k_index(cin0, cin1, ld0, ld1, ntap):
    """The engine's K row of (tap, channel of cat(segment 0, segment 1)) -> [ntap][cin0 + cin1]."""
    ch = np.concatenate([np.arange(cin0), ld0 + np.arange(cin1)])
    return np.arange(ntap)[:, None] * (ld0 + ld1) + ch[None, :]


def chain_counts(T, Fin, dt, df, T_out, F, cin0, cin1, ld0, ld1, chunk):
    """-> (L [T_out][F]: the largest count of non-zero products in one chain of `chunk` K rows, n_chunks)."""
    K = len(dt) * (ld0 + ld1)
    n_chunks = -(-K // chunk)
    per = np.zeros((len(dt), n_chunks))
    for tap, row in enumerate(k_index(cin0, cin1, ld0, ld1, len(dt)) // chunk):
        per[tap] = np.bincount(row, minlength=n_chunks)
    inside = gather(np.ones((T, Fin, 1)), dt, df, T_out, F)[..., 0]
    return np.einsum("tfk,kj->tfj", inside, per).max(-1), n_chunks


# ------------------------------------------------------------------------------------------------ engine rows
def pack_rows(xs, ld, seed):
    """Dense [T_u][F][C] arrays -> the engine's [sum T_u F][ld] fp32 rows; the pad channels hold finite values of the 1e3 scale."""
    C = xs[0].shape[2]
    rows = np.concatenate([np.asarray(x, F32).reshape(-1, C) for x in xs]) if xs else np.zeros((0, C), F32)
    out = (np.random.default_rng(seed).standard_normal((rows.shape[0], ld)) * BIG).astype(F32)
    out[:, :C] = rows
    return out


def grid_of(y, lens, F):
    """Engine rows [sum T_u F][ld] -> dense [T_u][F][ld] per utterance."""
    off = offsets(lens) * F
    return [y[off[u] : off[u + 1]].reshape(L, F, y.shape[1]) for u, L in enumerate(lens)]


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One launch.  lens: the input level's lengths per utterance (the offsets are lens << sh); taps: "3x3" / "1x1" (same), "5x5v" (valid: base grid
    (T - 4) x (Fin - 4)), "up2" (the sub-pixel conv (pt, pf) of the transposed conv)."""

    def __init__(self, name, lens, Fin, cin0, cout, npad, ldy, *, cin1=0, taps="3x3", lrelu=0, chunk=None, sliced=0, sh=0, pt=0, pf=0, act=ACT_NONE, bias=0, res=0,
                 div=1.0, wscale=1.0):
        self.name, self.lens, self.Fin, self.cin0, self.cin1, self.cout, self.npad, self.ldy = name, tuple(lens), Fin, cin0, cin1, cout, npad, ldy
        self.ld0, self.ld1 = round_up(cin0, BK), round_up(cin1, BK)
        self.taps, self.lrelu, self.sliced, self.sh, self.act, self.bias, self.res, self.div, self.wscale = taps, lrelu, sliced, sh, act, bias, res, float(F32(div)), wscale
        self.up, self.pt, self.pf = (2, pt, pf) if taps == "up2" else (1, 0, 0)
        if taps == "5x5v":
            (self.dt, self.df), self.lens_out, self.F = taps_valid(5), tuple(max(L - 4, 0) for L in lens), Fin - 4
        else:
            self.dt, self.df = subpixel(np.zeros((1, 1, 3, 3)), pt, pf)[:2] if taps == "up2" else taps_same(int(taps[0]))
            self.lens_out, self.F = self.lens, Fin
        self.K = len(self.dt) * (self.ld0 + self.ld1)
        self.chunk = chunk or self.K
        # the DATA depend on the convolution alone: the same conv at another tile, chunk or summation path has the same inputs
        self.seed = zlib.crc32(repr((self.lens, Fin, cin0, cin1, cout, taps.replace("up2", "up"), act, bias, res, wscale)).encode())

    def replace(self, **attrs):
        s = Case.__new__(Case)
        s.__dict__.update(self.__dict__)
        s.__dict__.update(attrs)
        return s

    @property
    def rows(self):
        return sum(self.lens_out) * self.F

    @property
    def out_rows(self):
        return sum(self.lens_out) * self.up * self.F * self.up


ROWS_A, F_A = (5, 0, 9, 1), 6  # 90 rows: one partial block in every tile
ROWS_B, F_B = (7, 12, 0, 30), 8  # 392 rows: boundaries inside a block, an empty utterance in the middle, a ragged last block at BM 64, 128 and 256
ROWS_C = (0, 6, 3, 0)  # the first and the last utterance empty
SQRT2 = float(np.sqrt(F32(2.0)))


def _cases():
    c = []
    # tiles, on ROWS_A and (one per BM) on ROWS_B
    tiles = {"n16c3": (3, 16, 4), "n16c16": (16, 16, 16), "n32c17": (17, 32, 32), "n64c33": (33, 64, 48), "n128c70": (70, 128, 80), "n32c16": (16, 32, 16), "n64c16": (16, 64, 16)}
    for t, (cout, npad, ldy) in tiles.items():
        c.append(Case(f"tile_{t}_A", ROWS_A, F_A, 13, cout, npad, ldy))
    c.append(Case("tile_n64c33_lrelu_A", ROWS_A, F_A, 13, 33, 64, 48, lrelu=1))
    for t in ("n16c16", "n32c17", "n64c33"):
        cout, npad, ldy = tiles[t]
        c.append(Case(f"tile_{t}_B", ROWS_B, F_B, 13, cout, npad, ldy))
    c.append(Case("tile_n64c33_lrelu_B", ROWS_B, F_B, 13, 33, 64, 48, lrelu=1, chunk=64))
    c.append(Case("rows_C", ROWS_C, F_A, 13, 33, 64, 48))
    c.append(Case("rows_none", (0, 0), F_A, 13, 16, 16, 16))
    # K: 9 taps x 16 = 144 in chunks of 64 (64, 64, 16), K and beyond K, each in the kernel and as grid slices; two segments: 9 x (16 + 32) = 432
    for chunk in (64, 144, 256):
        for sliced in (0, 1):
            c.append(Case(f"k144_chunk{chunk}_s{sliced}", ROWS_B, F_B, 13, 17, 32, 32, chunk=chunk, sliced=sliced, bias=1))
    for sliced in (0, 1):
        c.append(Case(f"two_segments_s{sliced}", ROWS_A, F_A, 5, 33, 64, 48, cin1=20, chunk=64, sliced=sliced))
        c.append(Case(f"lrelu_chunk64_s{sliced}", ROWS_A, F_A, 13, 33, 64, 48, lrelu=1, chunk=64, sliced=sliced))
    # row maps
    for sliced in (0, 1):
        c.append(Case(f"valid5_s{sliced}", (9, 5, 4, 7), 10, 6, 20, 32, 32, taps="5x5v", chunk=128, sliced=sliced, bias=1))
    c.append(Case("frames_1tap", ROWS_A, 1, 40, 20, 32, 24, taps="1x1", bias=1))
    c.append(Case("shift2", (3, 0, 2, 5), 4, 13, 16, 16, 16, sh=2))
    for pt in (0, 1):
        for pf in (0, 1):
            c.append(Case(f"up2_{pt}{pf}", (3, 0, 4), 5, 7, 10, 16, 16, taps="up2", pt=pt, pf=pf, act=ACT_RELU, bias=1))
    # epilogue
    epi = {"bias": dict(bias=1), "relu": dict(bias=1, act=ACT_RELU), "sigmoid": dict(bias=1, act=ACT_SIGMOID, wscale=1.0 / 64), "res": dict(res=1),
           "res_div": dict(bias=1, res=1, div=SQRT2)}
    for e, kw in epi.items():
        c.append(Case(f"epi_{e}", ROWS_A, F_A, 13, 33, 64, 48, **kw))
    return {x.name: x for x in c}


CASES = _cases()
UP2 = tuple(f"up2_{pt}{pf}" for pt in (0, 1) for pf in (0, 1))
SLICED_PAIRS = tuple((n, n[:-1] + "1") for n in CASES if n.endswith("_s0"))


@lru_cache(maxsize=None)
def data(name):
    """-> dict(x0, x1: per utterance [T][Fin][C] fp32 (x1 None without a second segment), w [cout][cin][ntap] fp32, bias [cout] fp32 or None,
    res: per utterance [T_b up][F up][cout] fp32 or None, wt: the transposed conv's weight of the up2 cases).  Every other utterance is 1e3 times larger."""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    scale = [BIG if u % 2 else 1.0 for u in range(len(c.lens))]

    def level(T, F, C, s):
        return (rng.standard_normal((T, F, C)) * s + 0.3 * s * rng.standard_normal(C)).astype(F32)

    d = dict(x0=[level(T, c.Fin, c.cin0, s) for T, s in zip(c.lens, scale)], x1=None, wt=None, bias=None, res=None)
    if c.cin1:
        d["x1"] = [level(T, c.Fin, c.cin1, s) for T, s in zip(c.lens, scale)]
    cin = c.cin0 + c.cin1
    if c.taps == "up2":
        d["wt"] = (rng.standard_normal((cin, c.cout, 3, 3)) / np.sqrt(cin * 2.25)).astype(F32)
        d["w"] = subpixel(d["wt"], c.pt, c.pf)[2]
    else:
        d["w"] = (rng.standard_normal((c.cout, cin, len(c.dt))) * c.wscale / np.sqrt(cin * len(c.dt))).astype(F32)
    if c.bias:
        d["bias"] = rng.standard_normal(c.cout).astype(F32)
    if c.res:
        d["res"] = [level(T * c.up, c.F * c.up, c.cout, s) for T, s in zip(c.lens_out, scale)]
    for v in d.values():
        for a in v if isinstance(v, list) else [v]:
            if a is not None:
                a.setflags(write=False)
    return d


def segs_of(d, u):
    return (d["x0"][u],) + ((d["x1"][u],) if d["x1"] is not None else ())


@lru_cache(maxsize=None)
def expected(name):
    """-> (want, bound, written): the dense output grid [sum T_b up][F up][cout] of the batch in float64, the allowed error, and which positions the launch
    writes [sum T_b up][F up]."""
    c, d = CASES[name], data(name)
    want, dy, written = [], [], []
    for u, (T, Tb) in enumerate(zip(c.lens, c.lens_out)):
        count = chain_counts(T, c.Fin, c.dt, c.df, Tb, c.F, c.cin0, c.cin1, c.ld0, c.ld1, c.chunk)
        v, dv = conv2d64(segs_of(d, u), d["w"], c.dt, c.df, Tb, c.F, lrelu=c.lrelu, bias=d["bias"], act=c.act, res=None if d["res"] is None else d["res"][u], div=c.div, up=c.up,
                         pt=c.pt, pf=c.pf, count=count)
        g, e, m = np.zeros((Tb * c.up, c.F * c.up, c.cout)), np.zeros((Tb * c.up, c.F * c.up, c.cout)), np.zeros((Tb * c.up, c.F * c.up), bool)
        g[c.pt :: c.up, c.pf :: c.up], e[c.pt :: c.up, c.pf :: c.up], m[c.pt :: c.up, c.pf :: c.up] = v, dv, True
        want.append(g)
        dy.append(e)
        written.append(m)
    out = np.concatenate(want), np.concatenate(dy), np.concatenate(written)
    for a in out:
        a.setflags(write=False)
    return out


def solo(name, u):
    """The same launch on utterance u alone -> (a Case, its data): the slices of the batch's inputs."""
    c, d = CASES[name], data(name)
    s = c.replace(name=f"{name}[{u}]", lens=(c.lens[u],), lens_out=(c.lens_out[u],))
    return s, dict(x0=[d["x0"][u]], x1=None if d["x1"] is None else [d["x1"][u]], w=d["w"], bias=d["bias"], res=None if d["res"] is None else [d["res"][u]], wt=d["wt"])


def worst(got, want, bound):
    """Largest |got - want| / bound over the elements (0 for none); a NaN or an infinity in `got` counts as infinite."""
    if want.size == 0:
        return 0.0
    e = np.abs(np.asarray(got, F64) - want)
    e[~np.isfinite(e)] = np.inf
    return float((e / bound).max())
