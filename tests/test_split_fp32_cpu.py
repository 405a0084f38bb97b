"""Split fp32 (csrc/gemm.hip.h, PREC_X3), the arithmetic fact it rests on, checked on the CPU: an fp32 number is the EXACT sum of three
bf16 numbers, and the three cross products the kernel drops are below fp32 rounding."""
import numpy as np


def bf16_round(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)



def test_three_bf16_terms_are_an_exact_split():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000) * 10.0 ** rng.uniform(-6, 6, 200000), [0.0, 1.0, -1.0, 3.0e38, 1e-30]]).astype(np.float32)
    p0 = bf16_round(x)
    r1 = x - p0
    p1 = bf16_round(r1)
    r2 = r1 - p1
    p2 = bf16_round(r2)
    assert np.array_equal(p2, r2), "the third term must be representable in bf16"
    assert np.array_equal((p0.astype(np.float64) + p1 + p2).astype(np.float32), x)
    assert np.array_equal(p0.astype(np.float64) + p1 + p2, x.astype(np.float64)), "x = p0 + p1 + p2 exactly"
    # the three dropped cross terms (p1 w2 + p2 w1 + p2 w2) against |x w|
    w = rng.standard_normal(x.size).astype(np.float32)
    q0 = bf16_round(w); q1 = bf16_round(w - q0); q2 = bf16_round(w - q0 - q1)
    dropped = p1.astype(np.float64) * q2 + p2.astype(np.float64) * q1 + p2.astype(np.float64) * q2
    ok = (np.abs(x) > 1e-25) & (np.abs(x) < 1e30) & (w != 0)
    rel = dropped[ok] / np.abs(x[ok].astype(np.float64) * w[ok])
    half_ulp = 2.0 ** -24
    assert np.abs(rel).max() <= 2 * half_ulp             # worst case: one fp32 ulp of the product
    assert np.sqrt((rel ** 2).mean()) <= 0.15 * half_ulp  # rms: ~0.1 of half an ulp (a single fp32 rounding of the product has 0.43)
    assert abs(rel.mean()) <= 1e-3 * half_ulp             # and no bias: the remainders of round-to-nearest are zero-mean




# ------------------------------------------------------------------------------------------------ bit-exact twin of the split
# split3_bf16 (csrc/gemm.hip.h: the activations, split_rows_kernel, winograd_input_kernel, wn_fused_x3) and split3_host
# (csrc/model.hip.h: the weights), and the kernel's six-product fp32 sum of one product x * w.  tests/test_hip_split_fp32_edges.py
# builds its operands and its bound from this module.
import pytest  # noqa: E402

F32 = np.float32
TOP_MAX = np.uint32(0x7F7F7FFF).view(np.float32)  # the largest fp32 whose bf16 rounding is finite (0x7F7F8000 and up round to Inf)
PRODUCTS = ("x2w0", "x0w2", "x1w1", "x1w0", "x0w1", "x0w0")  # the kernel's accumulation order (gemm.hip.h frag_mma): smallest terms first


def f32_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def bf16_rne(x):
    """f32_to_bf16 / v_cvt_pk_bf16_f32, back in fp32: round to nearest even, NaN stays NaN."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = np.where((u & 0x7FFFFFFF) > 0x7F800000, ((u >> 16) | 0x40) & 0xFFFF, r)
    return (r << 16).astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x, fixed=True, with_remainders=False):
    """x -> (p0, p1, p2): p0 = RNE bf16 of x clamped to +-TOP_MAX, p1 = RNE bf16 of r1 = x - p0, p2 = RNE bf16 of r2 = r1 - p1, every
    subtraction one fp32 rounding; +-Inf -> (0, 0, +-Inf).  fixed=False: the split before the edges were handled (p0 = RNE bf16 of x)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        inf = np.isinf(x) & fixed
        top = np.where(np.isnan(x), x, np.clip(np.where(inf, F32(0), x), -TOP_MAX, TOP_MAX)).astype(F32) if fixed else x
        p0 = bf16_rne(top)
        r1 = (x - p0).astype(F32)
        p1 = bf16_rne(np.where(inf, F32(0), r1))
        r2 = (r1 - p1).astype(F32)
        p2 = bf16_rne(r2)
    return (p0, p1, p2, top, r1, r2) if with_remainders else (p0, p1, p2)


def x3_sum(xs, ws, drop=None):
    """The kernel's fp32 accumulation of the six products of one x * w (xs / ws: the three bf16 terms), in its order."""
    acc = np.zeros(np.broadcast(xs[0], ws[0]).shape, F32)
    with np.errstate(all="ignore"):
        for name in PRODUCTS:
            if name != drop:
                acc = (acc + (xs[int(name[1])] * ws[int(name[3])]).astype(F32)).astype(F32)
    return acc


def x3_product(x, w):
    return x3_sum(split3(x), split3(w))


# The per-element bound of an output that is ONE product x w (+ b): the three dropped cross terms (<= 2^-23 |x w|), the six accumulations (only the
# last rounds at the scale of |x w|; the earlier partial sums are <= 2^-7 |x w|), room for an accumulator that truncates instead of rounding:
# 2^-21 |x w|; the bias addition rounds once more at |x w + b|; results in the fp32 subnormal range round at 2^-149.
EXPOSED_REL = 2.0 ** -21


def exposed_bound(prod, bias=0.0):
    prod = np.abs(np.asarray(prod, np.float64))
    return EXPOSED_REL * prod + 2.0 ** -24 * (prod + np.abs(bias)) + 2.0 ** -149


def full_mantissa(rng, shape, e_lo=-3, e_hi=2):
    """fp32 values whose 24 significand bits are random (all three bf16 terms populated), random signs, binades [2^e_lo, 2^(e_hi + 1))."""
    m = rng.integers(0, 1 << 23, size=shape, dtype=np.uint32) | np.uint32(1)
    e = (rng.integers(e_lo, e_hi + 1, size=shape) + 127).astype(np.uint32)
    s = rng.integers(0, 2, size=shape, dtype=np.uint32) << np.uint32(31)
    return (s | (e << np.uint32(23)) | m).view(np.float32)


def exposed_layout(cin, cout, k, rows, seed):
    """Exposed-product operands: x [rows, cin] and a weight with ONE nonzero per output channel, w[j, pi_j, tau_j] (tau_j = j mod k,
    pi_j = (37 j + 5) mod cin: every input channel for cout >= cin), so every output is one product of full-significand fp32 values and
    every row, output channel, input channel and tap of a tile is visible on its own."""
    rng = np.random.default_rng(seed)
    x = full_mantissa(rng, (rows, cin))
    j = np.arange(cout)
    pi, tau = (37 * j + 5) % cin, j % k
    w = np.zeros((cout, cin, k), np.float32)
    w[j, pi, tau] = full_mantissa(rng, cout)
    b = full_mantissa(rng, cout, -9, -7)
    return x, w, b, pi, tau


def exposed_operands(x, w, pi, tau, k, dil, lengths):
    """The operand pair of every output [rows, cout] (0 outside the utterance: the conv's zero padding), and the operand's channel
    neighbour (x at pi_j + 1, the next column of the same row)."""
    pad = (k - 1) // 2 * dil
    cout = w.shape[0]
    xo, xn = np.zeros((x.shape[0], cout), np.float32), np.zeros((x.shape[0], cout), np.float32)
    lo = 0
    xe = np.concatenate([x, x[:, :1]], 1)
    for L in lengths:
        r = np.arange(L)[:, None] + (tau[None, :] * dil - pad)
        ok = (r >= 0) & (r < L)
        rr = lo + np.clip(r, 0, L - 1)
        xo[lo : lo + L] = np.where(ok, xe[rr, pi[None, :]], 0)
        xn[lo : lo + L] = np.where(ok, xe[rr, pi[None, :] + 1], 0)
        lo += L
    return xo, w[np.arange(cout), pi, tau], xn


def mutants(xo, wo, xn):
    """name -> the six-product sum of every output under one plausible bug of a rewritten kernel."""
    xs, ws = split3(xo, with_remainders=True), split3(wo, with_remainders=True)
    xn_s = split3(xn)
    x3, w3 = xs[:3], ws[:3]
    out = {f"drop {p}": x3_sum(x3, w3, drop=p) for p in PRODUCTS}
    out["x planes 1 / 2 swapped"] = x3_sum((x3[0], x3[2], x3[1]), w3)
    out["x planes 0 / 1 swapped"] = x3_sum((x3[1], x3[0], x3[2]), w3)
    out["w planes 1 / 2 swapped"] = x3_sum(x3, (w3[0], w3[2], w3[1]))
    # a term stored truncated while the next remainder is taken from the rounded term (the conversion and the remainder disagree)
    out["x term 0 truncated"] = x3_sum((bf16_trunc(xs[3]), x3[1], x3[2]), w3)
    out["x term 1 truncated"] = x3_sum((x3[0], bf16_trunc(xs[4]), x3[2]), w3)
    out["w term 0 truncated"] = x3_sum(x3, (bf16_trunc(ws[3]), w3[1], w3[2]))
    out["w term 1 truncated"] = x3_sum(x3, (w3[0], bf16_trunc(ws[4]), w3[2]))
    # one plane read from the neighbouring channel's slot (x: the next column; w: the next input channel of the packed row, 0 here)
    out["x plane 1 from the next channel"] = x3_sum((x3[0], xn_s[1], x3[2]), w3)
    out["x plane 2 from the next channel"] = x3_sum((x3[0], x3[1], xn_s[2]), w3)
    out["w plane 1 from the next channel"] = x3_sum(x3, (w3[0], np.zeros_like(w3[1]), w3[2]))
    out["w plane 2 from the next channel"] = x3_sum(x3, (w3[0], w3[1], np.zeros_like(w3[2])))
    return out


EDGE_BITS = {  # the fp32 edge set of the split
    "+0": 0x00000000, "-0": 0x80000000, "+inf": 0x7F800000, "-inf": 0xFF800000, "nan": 0x7FC00000,
    "0x7F7F7FFF": 0x7F7F7FFF, "0x7F7F8000": 0x7F7F8000, "-0x7F7F8000": 0xFF7F8000, "FLT_MAX": 0x7F7FFFFF, "-FLT_MAX": 0xFF7FFFFF,
    "min normal": 0x00800000, "max subnormal": 0x007FFFFF, "subnormal 0x00012345": 0x00012345, "min subnormal": 0x00000001,
}


def edge_values():
    v = {n: f32_bits(b) for n, b in EDGE_BITS.items()}
    for e in range(100, 150):  # 2^-100 ... 2^-149 with a full significand where fp32 has the bits
        v[f"2^-{e}"] = F32(np.ldexp(1.0 + 0x5A5A5B / 2.0 ** 23, -e))
    return v


def test_split_of_the_fp32_edge_set():
    """Exact on every finite fp32 down to 2^-110; below that the bf16 terms run out of bits (bf16 subnormals step 2^-133: half the values of the
    2^-111 binade, 3/4 of 2^-112 are off by 2^-134); +-Inf is (0, 0, +-Inf) (test_an_infinite_operand_keeps_its_sign); NaN leaves NaN
    low terms."""
    vals = edge_values()
    names = list(vals)
    x = np.array([vals[n] for n in names], np.float32)
    p0, p1, p2 = split3(x)
    s = p0.astype(np.float64) + p1 + p2
    for n, xi, si, t in zip(names, x, s, zip(p0, p1, p2)):
        if np.isnan(xi):
            assert np.isnan(t[1]) and np.isnan(t[2]), n
        elif np.isinf(xi):
            assert t[0] == 0 and t[1] == 0 and t[2] == xi, n
        elif abs(float(xi)) >= 2.0 ** -110 or xi == 0:
            assert si == float(xi), (n, float(xi), si)
            assert np.isfinite(np.array(t)).all(), n
        else:
            assert abs(si - float(xi)) <= 2.0 ** -134, (n, float(xi), si)  # half a bf16 subnormal step
    # the terms are bf16 numbers, the top one never overflows
    for p in (p0, p1, p2):
        assert np.array_equal(p, bf16_rne(p), equal_nan=True)
    fin = np.isfinite(x)
    assert np.isfinite(p0[fin]).all()
    # before the edges were handled: the top term of |x| >= 0x7F7F8000 rounded to Inf and the split was NaN
    q0, q1, q2 = split3(x, fixed=False)
    big = fin & (np.abs(x) >= f32_bits(0x7F7F8000))
    assert big.sum() == 4 and np.isinf(q0[big]).all() and np.isnan(q2[big]).all()
    # nothing changes below the edge
    rng = np.random.default_rng(3)
    u = rng.integers(0, 0x7F7F8000, 400000, dtype=np.uint32) | (rng.integers(0, 2, 400000, dtype=np.uint32) << np.uint32(31))
    y = u.view(np.float32)
    for a, b in zip(split3(y), split3(y, fixed=False)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_split_is_exact_on_every_finite_fp32_above_2_minus_110():
    rng = np.random.default_rng(4)
    lo = np.uint32(np.float32(2.0 ** -110).view(np.uint32))
    u = rng.integers(lo, 0x7F800000, 2000000, dtype=np.uint32)
    u = np.concatenate([u, np.arange(0x7F7F0000, 0x7F800000, dtype=np.uint32)])  # the whole top bf16 binade
    x = (u | (rng.integers(0, 2, u.size, dtype=np.uint32) << np.uint32(31))).view(np.float32)
    p0, p1, p2 = split3(x)
    assert np.array_equal(p0.astype(np.float64) + p1 + p2, x.astype(np.float64))
    # below: off by at most 2^-134 (half a bf16 subnormal step)
    t = (np.arange(0, 1 << 23, 7, dtype=np.uint32) + np.uint32(np.float32(2.0 ** -112).view(np.uint32))).view(np.float32)
    q = split3(np.concatenate([t, t / 2 ** 20, -t / 2 ** 30]))
    xq = np.concatenate([t, t / 2 ** 20, -t / 2 ** 30]).astype(np.float64)
    assert np.abs(q[0].astype(np.float64) + q[1] + q[2] - xq).max() == 2.0 ** -134
    # the edge binade: top term 0x7F7F, the 16 bits below in the two lower terms
    top = np.abs(x) >= f32_bits(0x7F7F8000)
    assert (np.abs(p0[top]) == f32_bits(0x7F7F0000)).all()


def test_six_products_are_the_fp32_product():
    """x3_product (the kernel's arithmetic for one product) against the float64 product of the same fp32 operands: within the bound the GPU
    test uses, over the full range including the edge binade (products kept finite)."""
    rng = np.random.default_rng(5)
    x = full_mantissa(rng, 300000, -20, 20)
    w = full_mantissa(rng, 300000, -20, 20)
    big = np.concatenate([f32_bits(np.arange(0x7F7F8000, 0x7F800000, 97, dtype=np.uint32)), [f32_bits(0x7F7F7FFF), f32_bits(0x7F7FFFFF)]])
    x = np.concatenate([x, big, -big])
    w = np.concatenate([w, full_mantissa(rng, 2 * big.size, -3, -2)])
    y = x3_product(x, w).astype(np.float64)
    ref = x.astype(np.float64) * w
    assert np.isfinite(y).all()
    err = np.abs(y - ref)
    assert (err <= exposed_bound(ref)).all()
    assert err.max() / np.abs(ref[err.argmax()]) <= 2.0 ** -22  # the emulation itself has room to spare: 2^-21 is for the hardware's accumulator


def test_an_infinite_operand_keeps_its_sign():
    """+-Inf is split (0, 0, +-Inf): the infinite term enters only x2 w0 (w2 x0 on the weight side), so the six products give IEEE's +-Inf for
    every other operand whose top term is nonzero and finite - including bf16 numbers, whose low terms are zero - and NaN where IEEE has Inf * 0.
    The two cases left: Inf * Inf (both infinite terms meet a zero term: NaN), and an fp32 subnormal below 2^-134, whose top term is 0."""
    rng = np.random.default_rng(7)
    w = np.concatenate([full_mantissa(rng, 300000, -126, 126), np.float32([0.5, -1.0, 2.0 ** -133, 3.0e38, -TOP_MAX]),
                        f32_bits([0x7F7FFFFF, 0xFF7F8000])])
    with np.errstate(all="ignore"):
        for inf in (np.float32(np.inf), np.float32(-np.inf)):
            ieee = inf.astype(np.float64) * w.astype(np.float64)
            for y in (x3_product(np.full_like(w, inf), w), x3_product(w, np.full_like(w, inf))):
                assert np.array_equal(y.astype(np.float64), ieee)
        assert np.isnan(x3_product(np.float32(np.inf), np.float32(0)))
        assert np.isnan(x3_product(np.float32(0), np.float32(-np.inf)))
        assert np.isnan(x3_product(np.float32(np.nan), np.float32(0.5)))
        assert np.isnan(x3_product(np.float32(0.5), np.float32(np.nan)))
        # the two exceptions, stated
        assert np.isnan(x3_product(np.float32(np.inf), np.float32(np.inf)))
        assert np.isnan(x3_product(np.float32(np.inf), f32_bits(0x00000001)))
    # before the edges were handled: +-Inf gave NaN against every operand
    with np.errstate(all="ignore"):
        assert np.isnan(x3_sum(split3(np.float32(np.inf), fixed=False), split3(np.float32(0.5), fixed=False)))


def test_truncating_the_last_term_is_the_identity():
    """(Why the mutants truncate only terms 0 and 1: the last remainder is already a bf16 number, so truncating it changes nothing.)"""
    rng = np.random.default_rng(6)
    x = full_mantissa(rng, 200000, -30, 30)
    p = split3(x, with_remainders=True)
    assert np.array_equal(bf16_trunc(p[5]), p[5]) and np.array_equal(p[5], p[2])


def ragged(bn):
    """Utterance lengths that straddle a tile of bn rows."""
    return [1, bn - 1, bn, bn + 1, 2 * bn + 1]


# (cin, cout, k, dil): one K chunk / cout 1025 (a partial M tile), a partial K chunk with dilation 3, the decoder conv, deep K with k = 7
EXPOSED_GEOMETRY = [(32, 1025, 1, 1), (33, 130, 3, 3), (578, 512, 3, 1), (1536, 64, 7, 3)]
# every exposed-product operand set of tests/test_hip_split_fp32_edges.py: (cin, cout, k, dil, lengths, seed)
EXPOSED_SHAPES = [(cin, cout, k, dil, ragged(bn), 1000 * i + bn) for i, (cin, cout, k, dil) in enumerate(EXPOSED_GEOMETRY) for bn in (32, 64, 128, 256)] + [
    (1536, 64, 7, 1, [1, 63], 7001),      # tile 0: 32-row tiles, block split-K over 8 slices + the reduce pass
    (32, 2048, 1, 1, [257] * 16, 7002),   # tile 0: 512 blocks of 256 rows fill the chip twice -> tile 22
    (578, 512, 3, 1, [129, 1, 300], 7003),  # the input-affine / two-segment / Winograd cases
    (128, 64, 3, 1, [20] * 300, 7006),    # tile 0, f32 matrix cores: 300 blocks of 64 rows = 256 whole + a remainder launch of 44 with K cut in 3 + the reduce pass
]


@pytest.mark.parametrize("shape", EXPOSED_SHAPES, ids=[f"{c[0]}x{c[1]}k{c[2]}d{c[3]}n{len(c[4])}s{c[5]}" for c in EXPOSED_SHAPES])
def test_the_gpu_bound_rejects_every_mutant(shape):
    """On the exposed-product operands of the GPU test (the same generator, the same seeds), the correct emulation passes the bound and every
    mutant fails it somewhere: a kernel with any of these bugs cannot pass tests/test_hip_split_fp32_edges.py."""
    cin, cout, k, dil, lengths, seed = shape
    x, w, b, pi, tau = exposed_layout(cin, cout, k, sum(lengths), seed)
    xo, wo, xn = exposed_operands(x, w, pi, tau, k, dil, lengths)
    prod = xo.astype(np.float64) * wo
    bound = exposed_bound(prod, b)
    ref = prod + b

    def y_of(acc):
        return (acc + b).astype(F32).astype(np.float64)

    assert (np.abs(y_of(x3_sum(split3(xo), split3(wo))) - ref) <= bound).all(), shape
    names = set()
    for name, acc in mutants(xo, wo, xn).items():
        worst = (np.abs(y_of(acc) - ref) / bound).max()
        assert worst > 1.0, f"{shape}: mutant '{name}' passes the bound (worst {worst:.2f})"
        names.add(name)
    assert len(names) == 17
