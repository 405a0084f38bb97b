"""Every split-fp32 contraction variant (csrc/gemm.hip.h PREC_X3: tiles, pre-split planes, input affine, two segments, the Winograd form) and
the f32 matrix-core tiles against float64, on operands that expose one product per output, at ragged tile edges and on the fp32 edge set.

Exposed products (tests/test_split_fp32_cpu.py exposed_layout): every output channel reads ONE input channel at ONE tap, so each output is
one product x w + b of full-significand fp32 values, compared with the float64 product under a per-element bound of a few fp32 half-ulps of
that product (exposed_bound).  The CPU twin shows that this bound rejects a dropped cross product, swapped or truncated bf16 terms and a
plane read from the neighbouring channel on these very operands; dense random data cannot see those bugs under fp32 accumulation noise.
"""
import numpy as np
import pytest

from test_hip_frame_path import dev, segs
from test_split_fp32_cpu import (
    EXPOSED_SHAPES, edge_values, exposed_bound, exposed_layout, exposed_operands, f32_bits, full_mantissa, ragged,
)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hip(cfg):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)
    yield m
    m.close()


# forced tile -> rows per tile (BN), and the path launch_conv_gemm takes for it (a forced tile never gets block split-K or a remainder launch)
SPLIT_BN = {  # precision "f32": x3 stays on (tiles 2-6, 8, 20-22 have a split form) -> gemm_dispatch_tile_x3 -> launch_cfg_x3<BM, BN, WM, WN, KS>
    2: 64,    # <128, 64, 2, 2>: 4 waves of 64 x 32
    3: 32,    # no case of its own: the default, <128, 32, 2, 1>
    4: 32,    # <128, 32, 4, 1>: 4 waves of one 32 x 32 tile
    5: 128,   # <128, 128, 4, 2>: 8 waves, the fragment-pipelined loop (FPIPE)
    6: 64,    # <128, 64, 4, 2>
    8: 128,   # <128, 128, 4, 2, KS 2>: 16 waves, two K-groups summed through LDS
    20: 128,  # <128, 128, 2, 2>: 4 waves of 64 x 64
    21: 128,  # <128, 128, 2, 2, KS 2>
    22: 256,  # <128, 256, 2, 4>: 8 waves of 64 x 64
}
PRESPLIT_BN = {  # presplit: x16 on an fp32 call -> launch_cfg_x3<..., X16MODE>, conv_gemm_f32<..., PREC_X3, X16 = true>
    25: 128,  # <128, 128, 4, 2>, register staging
    26: 64,   # <128, 64, 4, 2>, register staging
    27: 128,  # <128, 128, 4, 2>, LDS-DMA (GLDS)
    28: 64,   # <128, 64, 4, 2>, LDS-DMA
}
NATIVE_BN = {  # precision "f32_native": no bf16 planes are packed, x3 is off -> gemm_dispatch_tile<PREC_F32> -> launch_cfg, v_mfma_f32_32x32x2_f32
    2: 64,    # <128, 64, 2, 2>
    4: 32,    # <128, 32, 4, 1>
    5: 128,   # <128, 128, 4, 2>
    6: 64,    # <128, 64, 4, 2>
    8: 128,   # <128, 128, 4, 2, KS 2>
    11: 128,  # <128, 128, 4, 2, GL>: LDS-DMA staging
    13: 64,   # <128, 64, 4, 2, GL>
}


def shape_for(geom, bn):
    return next(s for s in EXPOSED_SHAPES if s[:4] == geom and s[4] == ragged(bn))


def padded(x, ld, rng):
    """x [rows, c] -> [rows, ld] with finite full-significand values in the pad columns (they meet zero weights)."""
    out = full_mantissa(rng, (x.shape[0], ld))
    out[:, : x.shape[1]] = x
    return out


def run_exposed(hip, shape, **kw):
    cin, cout, k, dil, lengths, seed = shape
    s = segs(lengths)
    x, w, b, pi, tau = exposed_layout(cin, cout, k, s.rows, seed)
    xo, wo, _ = exposed_operands(x, w, pi, tau, k, dil, lengths)
    prod = xo.astype(np.float64) * wo
    ld = (cin + 31) // 32 * 32
    xd = padded(x, ld, np.random.default_rng(seed + 1))
    y = hip.op_conv1d_x3(s, dev(xd), cin, w, b, dil=dil, **kw).cpu().numpy()[:, :cout].astype(np.float64)
    return y, prod, b


def check_exposed(y, prod, b, what):
    ref = prod + b
    err = np.abs(y - ref)
    bound = exposed_bound(prod, b)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {bad.sum()} of {bad.size} outputs outside the bound; worst err / bound "
                           f"{np.nanmax(np.where(np.isfinite(err), err / bound, np.inf)):.2f} at {np.unravel_index(np.argmax(np.where(bad, 1, 0)), bad.shape)}")


def geoms():
    return sorted({s[:4] for s in EXPOSED_SHAPES[:16]})


# ------------------------------------------------------------------------------------------------ exposed products, every tile
@pytest.mark.parametrize("geom", geoms())
@pytest.mark.parametrize("tile", list(SPLIT_BN))
def test_split_tile_exposed_products(hip, tile, geom):
    """Forced split tiles: gemm_dispatch_tile_x3 (no block split-K for a forced tile), lengths 1, BN - 1, BN, BN + 1, 2 BN + 1."""
    y, prod, b = run_exposed(hip, shape_for(geom, SPLIT_BN[tile]), force_tile=tile, precision="f32")
    check_exposed(y, prod, b, f"split tile {tile} {geom}")


@pytest.mark.parametrize("geom", geoms())
@pytest.mark.parametrize("tile", list(PRESPLIT_BN))
def test_presplit_tile_exposed_products(hip, tile, geom):
    """Activations split by split_rows_kernel into three bf16 planes, then tiles 25 / 26 (register staging) and 27 / 28 (LDS-DMA)."""
    y, prod, b = run_exposed(hip, shape_for(geom, PRESPLIT_BN[tile]), presplit=True, force_tile=tile, precision="f32")
    check_exposed(y, prod, b, f"pre-split tile {tile} {geom}")


@pytest.mark.parametrize("geom", geoms())
@pytest.mark.parametrize("tile", list(NATIVE_BN))
def test_f32_matrix_core_tile_exposed_products(hip, tile, geom):
    """precision f32_native: no bf16 planes are packed, so the forced tile runs on v_mfma_f32_32x32x2_f32 (gemm_dispatch_tile<PREC_F32>)."""
    y, prod, b = run_exposed(hip, shape_for(geom, NATIVE_BN[tile]), force_tile=tile, precision="f32_native")
    check_exposed(y, prod, b, f"f32 matrix cores tile {tile} {geom}")


# tile 0 on ragged(64) = [1, 63, 64, 65, 129] (322 rows; row tiles: 6 of 128, 8 of 64, 13 of 32, 5 of 256), derived from launch_conv_gemm:
AUTO = [  # geometry, path (the same on both forms unless stated)
    ((32, 1025, 1, 1), "mt 9: 54 blocks of 128 x 128 >= 24; cost 1 round each, 128 vs 64 x 1.03 rows -> tile 6; 1 K iteration: no split-K"),
    ((33, 130, 3, 3), "mt 2: 12 blocks < 24 -> tile 4; 6 K iterations (2 chunks x 3 taps) / 4 < 2: no split-K"),
    ((578, 512, 3, 1), "mt 4: 24 blocks -> tile 6; 57 K iterations over 32 blocks -> block split-K 7 (split: 255 / 32) or 8 (f32 cores) + reduce"),
    ((1536, 64, 7, 3), "mt 1: 6 blocks < 24 -> tile 4; 336 K iterations over 13 blocks -> block split-K 8 + reduce"),
]


@pytest.mark.parametrize("precision", ["f32", "f32_native"])
@pytest.mark.parametrize("geom,path", AUTO, ids=[f"{g[0]}x{g[1]}" for g, _ in AUTO])
def test_auto_tile_exposed_products(hip, geom, path, precision):
    y, prod, b = run_exposed(hip, shape_for(geom, 64), precision=precision)
    check_exposed(y, prod, b, f"auto tile {precision} {geom} ({path})")


@pytest.mark.parametrize("precision", ["f32", "f32_native"])
@pytest.mark.parametrize("shape", EXPOSED_SHAPES[16:18] + EXPOSED_SHAPES[19:20], ids=["splitK", "tile22", "remainder"])
def test_auto_tile_dispatch_paths_exposed_products(hip, shape, precision):
    """1536 -> 64, k 7, lengths [1, 63]: 2 blocks of 128 x 128 < 24 -> tile 4; 3 blocks of 32 rows, 336 K iterations -> block split-K over
    8 slices + splitk_reduce_kernel (both forms).
    32 -> 2048, 16 x 257 rows: mt 16, 768 blocks of 128 rows (3 rounds) against 1 280 of 64 rows (5 rounds x 64 x 1.03) -> tile 6; split fp32:
    1 K iteration keeps tile 6, then 32 row tiles of 256 x 16 = 512 blocks (fills22: >= 440, whole rounds) -> tile 22.  f32 matrix cores: tile 6.
    128 -> 64, k 3, 300 x 20 rows: mt 1, 300 blocks of 128 rows (2 rounds) against 300 of 64 rows -> tile 6; 12 K iterations.  f32 matrix cores: 256 row tiles
    as they are + the other 44 as a second launch with K cut in 3 (min(8, 12 / 4, 256 / 44)) + splitk_reduce_kernel over those rows; split fp32: one whole launch."""
    y, prod, b = run_exposed(hip, shape, precision=precision)
    check_exposed(y, prod, b, f"auto {precision} {shape[:4]}")


# ------------------------------------------------------------------------------------------------ input affine, two segments
AFF_TILES = [0, 2, 3, 4, 5, 6, 8, 20, 21, 22]


def affine_case(cin, lengths, mode, seed):
    """The per-utterance affine table and the fp32 operand it produces (the kernel's arithmetic, xin in gemm.hip.h).  Mode 1: power-of-two
    scales (x * scale exact, so a fused multiply-add and a multiply + add agree) and full-significand shifts, slope 0.2; mode 2: full-significand
    scales, no shift."""
    rng = np.random.default_rng(seed)
    n, ld = len(lengths), (cin + 31) // 32 * 32
    aff = np.zeros((n, 2, ld), np.float32)
    if mode == 1:
        aff[:, 0, :cin] = np.ldexp(1.0, rng.integers(-2, 3, (n, cin))).astype(np.float32) * rng.choice([-1, 1], (n, cin))
        aff[:, 1, :cin] = full_mantissa(rng, (n, cin), -3, 1)
    else:
        aff[:, 0, :cin] = full_mantissa(rng, (n, cin), -2, 1)
    return aff


def apply_affine(x, aff, lengths, mode, slope):
    y = np.empty_like(x)
    lo = 0
    for u, L in enumerate(lengths):
        t = (x[lo : lo + L] * aff[u, 0, : x.shape[1]]).astype(np.float32)
        if mode == 1:
            t = (t + aff[u, 1, : x.shape[1]]).astype(np.float32)
            t = np.where(t >= 0, t, (np.float32(slope) * t).astype(np.float32))
        y[lo : lo + L] = t
        lo += L
    return y


def run_variant(hip, cin, cout, k, lengths, seed, mode=0, cin2=0, tile=0, precision="f32"):
    s = segs(lengths)
    x, w, b, pi, tau = exposed_layout(cin + cin2, cout, k, s.rows, seed)
    rng = np.random.default_rng(seed + 1)
    ld, ld2 = (cin + 31) // 32 * 32, (cin2 + 31) // 32 * 32
    x1, x2 = x[:, :cin], x[:, cin:]
    kw = {}
    xop = x.copy()
    if mode:
        aff = affine_case(cin, lengths, mode, seed + 2)
        kw.update(aff=aff, xaff_mode=mode, slope=0.2 if mode == 1 else 1.0)
        xop[:, :cin] = apply_affine(x1, aff, lengths, mode, kw["slope"])
    if cin2:
        kw.update(x2=dev(padded(x2, ld2, rng)), cin2=cin2)
    xo, wo, _ = exposed_operands(xop, w, pi, tau, k, 1, lengths)
    prod = xo.astype(np.float64) * wo
    y = hip.op_conv1d_x3(s, dev(padded(x1, ld, rng)), cin, w, b, force_tile=tile, precision=precision, **kw).cpu().numpy()[:, :cout]
    return y.astype(np.float64), prod, b


@pytest.mark.parametrize("precision", ["f32", "f32_native"])
@pytest.mark.parametrize("tile", AFF_TILES)
def test_input_affine_exposed_products(hip, tile, precision):
    """XAFF = 1 (lrelu(x * scale + shift), the decoder's AdaIN) on a single segment, 578 -> 512, k 3: conv_gemm_f32<..., PREC_X3, 1, false>."""
    if precision == "f32_native" and tile in (20, 21, 22):
        pytest.skip("split-only tile")
    y, prod, b = run_variant(hip, 578, 512, 3, [129, 1, 300], 7003, mode=1, tile=tile, precision=precision)
    check_exposed(y, prod, b, f"input affine tile {tile} {precision}")


@pytest.mark.parametrize("tile", AFF_TILES)
def test_scale_only_input_affine_exposed_products(hip, tile):
    """XAFF = 2 (x * scale: GRN folded into pwconv2's staging), 512 -> 256, k 1 (cin == ldx): conv_gemm_f32<..., PREC_X3, 2, false>."""
    y, prod, b = run_variant(hip, 512, 256, 1, [129, 1, 300], 7004, mode=2, tile=tile)
    check_exposed(y, prod, b, f"scale-only input affine tile {tile}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tile", AFF_TILES)
def test_two_segments_exposed_products(hip, tile, mode):
    """MSEG: [x (256 + affine) | x2 (322 channels, a partial chunk)] -> 512, k 3, the decoder's concatenated input as two segments of one
    launch: conv_gemm_f32<..., PREC_X3, XAFF, true>; mode 0 without the affine, 1 with it on segment 0."""
    y, prod, b = run_variant(hip, 256, 512, 3, [129, 1, 300], 7005, mode=mode, cin2=322, tile=tile)
    check_exposed(y, prod, b, f"two segments tile {tile} affine {mode}")


# ------------------------------------------------------------------------------------------------ dense data, calibrated on the f32 matrix cores
def conv64(x, w, lengths, k, dil=1):
    out, lo = [], 0
    pad = (k - 1) // 2 * dil
    for L in lengths:
        xi = np.zeros((L + 2 * pad, x.shape[1]), np.float64)
        xi[pad : pad + L] = x[lo : lo + L]
        y = np.zeros((L, w.shape[0]), np.float64)
        for t in range(k):
            y += xi[t * dil : t * dil + L] @ w[:, :, t].T.astype(np.float64)
        out.append(y)
        lo += L
    return np.concatenate(out)


# variant, shape options, split-form run, f32-matrix-core run.  Both forms of a row take the same tile and the same K order, so the error of a
# long fp32 accumulation is compared with the same accumulation (578 -> 512, k 3, lengths [129, 1, 300]: 57 K iterations; at tile 0 the launcher
# cuts them over block split-K slices - 7 for the split form, 8 on the f32 matrix cores - and a pre-split tile never does, so it runs all 57 in
# one chain: a few times the error of the cut form on the same data, the same as an uncut tile 6 on either form)
DENSE = [
    ("tile 0 (tile 6, block split-K)", {}, {}, {}),
    ("tile 6, whole K", {}, {"force_tile": 6}, {"force_tile": 6}),
    ("pre-split tile 28, whole K", {}, {"presplit": True, "force_tile": 28}, {"force_tile": 6}),
    ("pre-split tile 27, whole K", {}, {"presplit": True, "force_tile": 27}, {"force_tile": 5}),
    ("input affine, tile 0", {"mode": 1}, {}, {}),
    ("scale-only affine, tile 0", {"mode": 2}, {}, {}),
    ("two segments, tile 0", {"cin2": 322}, {}, {}),
    ("Winograd k3", {"wino": 3}, {}, {}),
    ("Winograd k7", {"wino": 7}, {}, {}),
]


@pytest.mark.parametrize("name,opt,split_kw,native_kw", DENSE, ids=[d[0] for d in DENSE])
def test_dense_error_per_element_matches_the_f32_matrix_cores(hip, name, opt, split_kw, native_kw):
    """Dense random data: max over elements of |y - ref| / sum |x w|, the split form within 1.25 x the f32 matrix cores' on the same operands
    and the same accumulation order (+ 2^-26, a quarter of the f32 matrix cores' own figure here)."""
    cin, cout, k, lengths = (512, 512, 3, [129, 1, 300]) if opt.get("mode") == 2 else (256 if opt.get("cin2") else 578, 512, opt.get("wino", 3), [129, 1, 300])
    if opt.get("mode") == 2:
        k = 1
    cin2 = opt.get("cin2", 0)
    s = segs(lengths)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((s.rows, cin + cin2)).astype(np.float32)
    w = (rng.standard_normal((cout, cin + cin2, k)) / np.sqrt((cin + cin2) * k)).astype(np.float32)
    ld, ld2 = (cin + 31) // 32 * 32, (cin2 + 31) // 32 * 32
    kw = {}
    xop = x.copy()
    if opt.get("mode"):
        aff = affine_case(cin, lengths, opt["mode"], 12)
        kw.update(aff=aff, xaff_mode=opt["mode"], slope=0.2 if opt["mode"] == 1 else 1.0)
        xop[:, :cin] = apply_affine(x[:, :cin], aff, lengths, opt["mode"], kw["slope"])
    if cin2:
        kw.update(x2=dev(padded(x[:, cin:], ld2, rng)), cin2=cin2)
    ref = conv64(xop, w, lengths, k)
    mag = conv64(np.abs(xop), np.abs(w), lengths, k)
    xd = dev(padded(x[:, :cin], ld, rng))
    errs = {}
    for prec, extra in (("f32", split_kw), ("f32_native", native_kw)):
        if "wino" in opt:
            y = hip.op_conv1d(s, xd, cin, w, None, force_tile=-4, precision=prec)
        else:
            y = hip.op_conv1d_x3(s, xd, cin, w, None, precision=prec, **kw, **extra)
        errs[prec] = (np.abs(y.cpu().numpy()[:, :cout].astype(np.float64) - ref) / np.maximum(mag, 1e-30)).max()
    print(f"\n[split fp32 dense] {name}: max err / sum|xw| split {errs['f32']:.2e}, f32 matrix cores {errs['f32_native']:.2e}")
    assert errs["f32"] <= 1.25 * errs["f32_native"] + 2.0 ** -26
    assert errs["f32"] <= 2.0 ** -16


# ------------------------------------------------------------------------------------------------ the fp32 edge set
EDGE_GROUPS = {  # (tiny magnitudes: their own test)
    "near FLT_MAX": ["0x7F7F7FFF", "0x7F7F8000", "-0x7F7F8000", "FLT_MAX", "-FLT_MAX"],
    "infinite": ["+inf", "-inf"],
    "zero and NaN": ["+0", "-0", "nan"],
}
EDGE_FORMS = [("f32", t) for t in [0, 2, 3, 4, 5, 6, 8, 20, 21, 22]] + [("presplit", t) for t in PRESPLIT_BN] + [("f32_native", t) for t in [0, *NATIVE_BN]]


def edge_case(where, names, seed=21):
    """33 -> 130, k 3, dilation 3, lengths [70, 90, 40]: the exposed layout, weights in [0.25, 0.5) (x w of FLT_MAX stays finite), no bias; the
    edge values sit in utterance 1 (where='x': one input element each, 2 k dil rows apart; 'w': one weight each)."""
    cin, cout, k, dil, lengths = 33, 130, 3, 3, [70, 90, 40]
    x, w, _, pi, tau = exposed_layout(cin, cout, k, sum(lengths), seed)
    x = np.abs(x) * np.float32(0.25) / np.float32(8)  # |x| in [2^-6, 2^-3): products with an edge weight stay finite
    j = np.arange(cout)
    w[j, pi, tau] = np.float32(0.25) + np.abs(full_mantissa(np.random.default_rng(seed), cout, -3, -3))
    vals = edge_values()
    for i, n in enumerate(names):
        if where == "x":
            r, c = 70 + 3 + i * 2 * k * dil % 84, pi[i]
            x[r, c] = vals[n]
        else:
            w[i * 7, pi[i * 7], tau[i * 7]] = vals[n]
    return cin, cout, k, dil, lengths, x, w


def ieee64(x, w, lengths, k, dil):
    """float64 conv of the same fp32 operands with IEEE semantics everywhere (Inf * 0 = NaN): explicit sums, no BLAS."""
    out, lo = [], 0
    pad = (k - 1) // 2 * dil
    with np.errstate(all="ignore"):
        for L in lengths:
            xi = np.zeros((L + 2 * pad, x.shape[1]), np.float64)
            xi[pad : pad + L] = x[lo : lo + L]
            y = np.zeros((L, w.shape[0]), np.float64)
            for t in range(k):
                y = y + np.einsum("rc,jc->rj", xi[t * dil : t * dil + L], w[:, :, t].astype(np.float64), optimize=False)
            out.append(y)
            lo += L
    return np.concatenate(out)


def run_form(hip, form, tile, s, xd, cin, w, dil):
    if form == "presplit":
        return hip.op_conv1d_x3(s, xd, cin, w, None, dil=dil, presplit=True, force_tile=tile, precision="f32").cpu().numpy()
    return hip.op_conv1d_x3(s, xd, cin, w, None, dil=dil, force_tile=tile, precision=form).cpu().numpy()


@pytest.mark.parametrize("group", list(EDGE_GROUPS))
@pytest.mark.parametrize("where", ["x", "w"])
@pytest.mark.parametrize("form,tile", EDGE_FORMS)
def test_edge_operands_keep_their_ieee_class(hip, form, tile, where, group):
    """Finite <-> finite within the exposed bound (the fp32 result does not depend on the order: one nonzero product per output), NaN <-> NaN,
    +-Inf <-> the same Inf, in every form: the split puts +-Inf in its lowest term, which meets only the other operand's top term
    (test_split_fp32_cpu.py::test_an_infinite_operand_keeps_its_sign)."""
    cin, cout, k, dil, lengths, x, w = edge_case(where, EDGE_GROUPS[group])
    s = segs(lengths)
    ld = (cin + 31) // 32 * 32
    xd = dev(padded(x, ld, np.random.default_rng(5)))
    y = run_form(hip, form, tile, s, xd, cin, w, dil)[:, :cout].astype(np.float64)
    ref = ieee64(x, w, lengths, k, dil)
    fin = np.isfinite(ref)
    assert np.isfinite(y[fin]).all(), f"{form} tile {tile}: {(~np.isfinite(y[fin])).sum()} outputs non-finite where IEEE is finite"
    err = np.abs(y[fin] - ref[fin])
    bound = exposed_bound(ref[fin])
    assert (err <= bound).all(), f"{form} tile {tile}: finite outputs off by {np.max(err / bound):.2f} x the bound"
    assert np.isnan(y[np.isnan(ref)]).all()
    inf = np.isinf(ref)
    assert inf.any() == (group == "infinite")
    assert (y[inf] == ref[inf]).all(), f"{form} tile {tile}: {(y[inf] != ref[inf]).sum()} of {inf.sum()} infinite outputs differ from IEEE"


def test_tiny_magnitudes_and_the_bf16_subnormal_inputs(hip):
    """|x| from 2^-100 down to 2^-149 times weights of ~2^40 (products stay normal fp32): the split form's absolute error per product, and
    whether v_mfma_f32_32x32x16_bf16 keeps bf16 subnormal inputs (probe: a weight 2^-130, split on the host into one subnormal bf16 term,
    times x = 2^40 gives 2^-90 if kept, 0 if flushed)."""
    cin, cout, k, lengths = 64, 128, 1, [64]
    s = segs(lengths)
    rng = np.random.default_rng(31)
    j = np.arange(cout)
    tiny = np.array([np.ldexp(1.0 + rng.integers(0, 1 << 23) / 2.0 ** 23, -e) for e in range(100, 150)], np.float32)
    x = np.zeros((64, cin), np.float32)
    x[: tiny.size, 0] = tiny
    x[: tiny.size, 1] = np.float32(2.0 ** 40)
    w = np.zeros((cout, cin, k), np.float32)
    wt = np.float32(2.0 ** 40) * (np.float32(1) + np.abs(full_mantissa(rng, 1, -2, -2))[0])
    w[0, 0, 0] = wt  # output 0 = tiny x * 2^40-ish weight
    w[1, 1, 0] = np.float32(2.0 ** -130)  # output 1 = 2^40 * 2^-130 (a bf16-subnormal weight term)
    w[2, 1, 0] = f32_bits(0x00012345)  # output 2 = 2^40 * an fp32 subnormal weight
    xd = dev(x)
    out = {p: hip.op_conv1d_x3(s, xd, cin, w, None, precision=p).cpu().numpy() for p in ("f32", "f32_native")}
    ref0 = x[: tiny.size, 0].astype(np.float64) * float(wt)
    y0 = out["f32"][: tiny.size, 0].astype(np.float64)
    # the error beyond the fp32 rounding of the product, per product, in units of |w| (= the error of the operand x)
    err = np.maximum(np.abs(y0 - ref0) - exposed_bound(ref0), 0) / float(wt)
    print(f"\n[split fp32 tiny] per-product |error| / |w| beyond fp32 rounding, by exponent of x: "
          + " ".join(f"2^-{100 + i}:{e:.1e}" for i, e in enumerate(err)))
    print(f"[split fp32 tiny] bf16-subnormal weight term: split {out['f32'][0, 1]:.6e} (2^-90 = {2.0 ** -90:.6e}), f32 matrix cores {out['f32_native'][0, 1]:.6e}")
    print(f"[split fp32 tiny] fp32-subnormal weight: split {out['f32'][0, 2]:.6e}, f32 matrix cores {out['f32_native'][0, 2]:.6e}, exact {2.0 ** 40 * float(f32_bits(0x00012345)):.6e}")
    # measured on MI355X: the bf16 MFMA keeps bf16 subnormal inputs (2^40 * 2^-130 = 2^-90 exactly), and the error per product is at most
    # 2^-134 |w| (half a bf16 subnormal step: the CPU twin's split error, nothing flushed) from 2^-111 down; 0 from 2^-110 up
    assert out["f32"][0, 1] == np.float32(2.0 ** -90), "v_mfma_f32_32x32x16_bf16 flushed a bf16 subnormal input"
    assert out["f32_native"][0, 1] == np.float32(2.0 ** -90)
    assert err.max() <= 2.0 ** -134
    assert (err[:11] == 0).all()  # 2^-100 ... 2^-110: the split is exact
    # a weight that is an fp32 subnormal (split on the host): off by at most 2^-134 too
    assert abs(float(out["f32"][0, 2]) - 2.0 ** 40 * float(f32_bits(0x00012345))) <= 2.0 ** 40 * 2.0 ** -134 + exposed_bound(1.2e-28)


# ------------------------------------------------------------------------------------------------ isolation of a poisoned utterance
ISO_FORMS = EDGE_FORMS + [("wino_f32", -4), ("wino_f32_native", -4)]


@pytest.mark.parametrize("form,tile", ISO_FORMS)
def test_non_finite_values_stay_inside_their_receptive_field(hip, form, tile):
    """NaN, Inf and a value near FLT_MAX in one utterance of a ragged batch (dense weights): every other utterance is bit-identical to the clean
    run, and so is every row of that utterance outside the k dil receptive field (direct forms) or outside the F(6, k) groups whose input
    window holds the value (Winograd)."""
    wino = form.startswith("wino")
    cin, cout, k, dil = (64, 130, 3, 1) if wino else (33, 130, 3, 3)
    lengths = [130, 257, 65, 1]
    s = segs(lengths)
    rng = np.random.default_rng(41)
    x = rng.standard_normal((s.rows, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ld = (cin + 31) // 32 * 32
    dirty = x.copy()
    u, lo = 1, s.host[1]
    poison = {60: np.float32(np.nan), 130: np.float32(np.inf), 200: f32_bits(0x7F7FFFFF)}
    for r, v in poison.items():
        dirty[lo + r, 7] = v

    def run(xx):
        xd = dev(padded(xx, ld, np.random.default_rng(6)))
        if wino:
            return hip.op_conv1d(s, xd, cin, w, b, force_tile=-4, precision=form[5:]).cpu().numpy()
        if form == "presplit":
            return hip.op_conv1d_x3(s, xd, cin, w, b, dil=dil, presplit=True, force_tile=tile, precision="f32").cpu().numpy()
        return hip.op_conv1d_x3(s, xd, cin, w, b, dil=dil, force_tile=tile, precision=form).cpu().numpy()

    clean, hit = run(x)[:, :cout], run(dirty)[:, :cout]
    L = lengths[u]
    reached = np.zeros(L, bool)
    pad = (k - 1) // 2 * dil
    for r in poison:
        if wino:
            n = 6 + k - 1
            for g in range((L + 5) // 6):
                if g * 6 - (k - 1) // 2 <= r <= g * 6 - (k - 1) // 2 + n - 1:
                    reached[g * 6 : g * 6 + 6] = True
        else:
            reached[max(0, r - pad) : r + pad + 1] = True
    keep = np.ones(s.rows, bool)
    keep[lo : lo + L] = ~reached
    assert np.array_equal(hit[keep].view(np.uint32), clean[keep].view(np.uint32)), f"{form} tile {tile}: rows outside the reach changed"
    assert not np.isfinite(hit[lo : lo + L][reached]).all(), f"{form} tile {tile}: the poison vanished"
