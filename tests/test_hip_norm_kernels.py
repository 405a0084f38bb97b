"""The kernels BETWEEN the contractions, one at a time, against float64 (tests/norm64.py): the AdaIN chunk statistics' four producers' fp32 forms
(adain_partial_kernel at 128 and 24 rows, adain_partial_reduce_kernel, winograd_output_kernel<8, true>), the three merges (adain_affine_kernel,
adain_affine_lanes_kernel, adain_apply_kernel's preamble), adain_apply_kernel, row_layernorm_kernel, dwconv_kernel / dwconv_ln_kernel, grn_gx_kernel /
grn_xaff_kernel / scale_weight_kernel - through stts_op_adain, _wino_stat, _row_layernorm, _dwconv and _grn.

Every bound is norm64's (derived there from the kernels' arithmetic, met by numpy-fp32 emulations in tests/test_norm64_cpu.py; rsqrtf, sinf, sqrtf,
exp2 and the reciprocal are allowed 4 x the error numpy's fp32 functions show on the same inputs).  Every output buffer is pre-filled with the quiet
NaN 0x7FC0BEEF (16-bit: 0x7FC1) and compared as bits: whatever lies outside the written window must keep it.  In every ragged batch the odd
utterances and all pad columns hold values about 1e3 times larger than the even utterances, so a row or column leaking across a boundary cannot hide.

The rows adain_partial_reduce_kernel finishes are compared BIT FOR BIT with a float32 restatement in slice order of what splitk_reduce_kernel computes
(norm64.split_finish32: sums and products of two fp32 numbers, each rounded once); row_layernorm_kernel's LnIn source, whose finished row never leaves the
kernel, is held to the LayerNorm bound on that restatement.

Measured on an MI355X (-s prints them), largest error as a fraction of its bound:
  adain_partial_kernel       chunk 128: mean 0.07 / 0.09 (C 64 / 130), M2 0.08 / 0.16; chunk 24: mean 0.18 / 0.22, M2 0.23 / 0.29
  cancellation channels      |M2 - M2_64| / M2_64 = 1.5e-7 (0.12 of bound (a)); the one-pass formula: 2.2e-2 in numpy fp32, 2.2e-3 .. 1.2e-2 in the 16-bit epilogue
  adain_partial_reduce       X bit-identical to the restatement (ksplit 2 and 5); mean 0.10 / 0.12, M2 0.11 / 0.12
  winograd_output<8, true>   mean 0.44 / 0.36 (cout 64 / 132), M2 0.07 / 0.06
  merges, bound (b)          serial 0.81, lanes 0.81 (chunk 128), 0.35 / 0.35 (chunk 24); serial against lanes 0.40 / 0.61; apply's four-lane merge 0.63 of bound (c)
  adain_apply, bound (c)     none 0.56, LeakyReLU 0.42, snake 0.36 - the same at rb 64 and 256; 16-bit rows = RNE(fp32 rows); ragged = solo
  row_layernorm              static 0.01 .. 0.19, adaptive up to 0.74 (C 256, the row with mean 100), LnIn 0.002 .. 0.17
  dwconv_kernel              0.07 .. 0.58, SiLU 0.05 .. 0.34;  dwconv + LayerNorm: fused = two launches BIT FOR BIT in all 12 cases (not asserted), 0.02 .. 0.19 of the bound
  GRN                        gx 0.18, factor 0.24, scaled weight 0.45 of 4 u
With `ch += 8` for `ch += 16` in a scratch copy of adain_affine_lanes_kernel both cases of test_merges_against_float64_of_their_own_table fail (scale 2.2e5 bounds off,
at the 2 100-row and the 385-row utterance); nothing else of the file runs that kernel.
"""
import numpy as np
import pytest

import gemm16_ref as G
import norm64 as N

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT32, SENT16 = np.uint32(0x7FC0BEEF), np.uint16(0x7FC1)
F32, F64 = np.float32, np.float64
PREC = {0: None, 1: "bf16", 2: "f16"}


@pytest.fixture(scope="module")
def hip(cfg):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)
    yield m
    m.close()


def seg_of(lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments(lengths, torch.device("cuda", 0))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def sent(shape, bits16=False):
    if bits16:
        return torch.from_numpy(np.full(shape, SENT16, np.uint16).view(np.int16)).cuda()
    return torch.from_numpy(np.full(shape, SENT32, np.uint32).view(np.float32)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def kept(a):
    a = np.ascontiguousarray(a)
    return bool((a == SENT16).all()) if a.dtype == np.uint16 else bool((a.view(np.uint32) == SENT32).all())


def same_bits(a, b):
    v = np.uint32 if a.dtype == np.float32 else a.dtype
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def table_kept(table, lengths, chunk, C_written, what):
    for u, L in enumerate(lengths):
        assert kept(table[u, (L + chunk - 1) // chunk :]), (what, "a chunk past ceil(len / chunk) written", u, L)
    assert kept(table[:, :, :, C_written:]), (what, "columns past the channels written")


# ------------------------------------------------------------------------------------------------ chunk producers
def run_producer(hip, x, lengths, C, producer, extra=None):
    """-> (table [n_utt, nchunk + 1, 2, round_up(C, 32) + 32] as the launch left it, x after the launch)."""
    chunk = N.WINO_CHUNK if producer == 1 else N.STAT_CHUNK
    nchunk = (max(lengths) + chunk - 1) // chunk + 1
    part = sent((len(lengths), nchunk, 2, N.round_up(C, 32) + 32))
    xd = dev(x)
    hip.op_adain(seg_of(lengths), x=xd, ldx=x.shape[1], C=C, producer=producer, consumer=0, part=part, ldp=part.shape[3], nchunk=nchunk, **(extra or {}))
    return host(part), host(xd)


@pytest.mark.parametrize("C,ldx", N.STAT_C)
@pytest.mark.parametrize("producer", (0, 1))
def test_chunk_statistics_against_float64(hip, C, ldx, producer):
    """adain_partial_kernel at 128 and at 24 rows per chunk: bound (a); unused chunks and columns keep the sentinel; X is not written."""
    x = N.stat_case(C, ldx)
    chunk = N.WINO_CHUNK if producer == 1 else N.STAT_CHUNK
    table, xa = run_producer(hip, x, N.STAT_LENGTHS, C, producer)
    assert same_bits(xa, x)
    table_kept(table, N.STAT_LENGTHS, chunk, C, "adain_partial_kernel")
    wm, w2, _ = N.check_chunk_table(x, N.STAT_LENGTHS, C, chunk, table, what=f"producer {producer}")
    print(f"\n[norm] adain_partial_kernel C {C} chunk {chunk}: mean error {wm:.3f} of bound (a), M2 {w2:.3f}")


def test_chunk_statistics_cancellation(hip):
    """Eight channels with mean 8 and standard deviation 0.05: the two-pass formula keeps M2 to bound (a), where a one-pass formula loses 1e-2 of it."""
    x = N.cancel_case()
    table, _ = run_producer(hip, x, N.CANCEL_LENGTHS, 64, 0)
    _, w2, rel = N.check_chunk_table(x, N.CANCEL_LENGTHS, 64, N.STAT_CHUNK, table, what="cancellation")
    r = float(rel[list(N.CANCEL_CH)].max())
    print(f"\n[norm] cancellation channels (mean^2 / var 2.6e4): |M2 - M2_64| / M2_64 = {r:.2e} ({w2:.3f} of bound (a)); the one-pass formula gives 1e-2 (2.2e-2 in fp32 numpy)")
    assert r < 1e-4


@pytest.mark.parametrize("ksplit", (2, 5))
def test_partial_reduce_finishes_x_and_takes_statistics(hip, ksplit):
    """adain_partial_reduce_kernel: channels < 100 of X are finished from `ksplit` slices (LeakyReLU, R at rcol0 8, alpha 1 / sqrt 2) - the bits of the fp32
    restatement in slice order of splitk_reduce_kernel -, channels 100 .. 129 are read; the table meets bound (a) on the X the launch left."""
    C, ldx, n_fin, L = 130, 160, 100, N.STAT_LENGTHS
    R = sum(L)
    rng = np.random.default_rng(700 + ksplit)
    x = np.array(N.stat_case(C, ldx))
    x[:, :n_fin] = np.full((R, n_fin), SENT32, np.uint32).view(F32)
    scale = np.repeat(np.where(np.arange(len(L)) % 2, 1e3, 1.0), L)[:, None].astype(F32)
    part = (rng.standard_normal((ksplit, R + 3, 104)) * 1e3).astype(F32)
    part[:, :R, :n_fin] = rng.standard_normal((ksplit, R, n_fin)).astype(F32) * scale
    bias = rng.standard_normal(n_fin).astype(F32)
    r = (rng.standard_normal((R, 136)) * 1e6).astype(F32)
    r[:, 8 : 8 + n_fin] = rng.standard_normal((R, n_fin)).astype(F32) * scale
    extra = dict(partial=dev(part), ksplit=ksplit, slice_rows=R + 3, ld_part=104, split_n=n_fin, bias=dev(bias), split_act=N.ACT_LRELU, r=dev(r), ldr=136, rcol0=8,
                 split_alpha=N.RSQRT2)
    table, xa = run_producer(hip, x, L, C, 2, extra)
    want = N.split_finish32(part, R, n_fin, bias, N.ACT_LRELU, r, 8, N.RSQRT2)
    assert same_bits(xa[:, :n_fin], want), ("finished X differs from the slice-order restatement", np.argwhere(xa[:, :n_fin] != want)[:4])
    assert same_bits(xa[:, n_fin:], x[:, n_fin:]), "X written outside the finished channels"
    table_kept(table, L, N.STAT_CHUNK, C, "adain_partial_reduce_kernel")
    wm, w2, _ = N.check_chunk_table(xa, L, C, N.STAT_CHUNK, table, what=f"partial_reduce ksplit {ksplit}")
    print(f"\n[norm] adain_partial_reduce_kernel ksplit {ksplit}: X bit-identical to the restatement; mean {wm:.3f} of bound (a), M2 {w2:.3f}")


@pytest.mark.parametrize("cout", N.WINO_COUT)
def test_winograd_output_statistics(hip, cout):
    """winograd_output_kernel<8, true> (k 3): the statistics meet bound (a), with the term of Chan's merge, on the Y the same launch stored; Y is the plain launch's."""
    cin, L = 64, N.WINO_LENGTHS
    R = sum(L)
    rng = np.random.default_rng(800 + cout)
    x = N.ragged(801 + cout, L, cin, cin)
    w = (rng.standard_normal((cout, cin, 3)) / np.sqrt(3 * cin)).astype(F32)
    b = rng.standard_normal(cout).astype(F32)
    seg = seg_of(L)
    nchunk = ((max(L) + 5) // 6 + 3) // 4
    ldy, ld_stat = N.round_up(cout, 32) + 32, N.round_up(cout, 4) + 32
    y, stat = sent((R + 1, ldy)), sent((len(L), nchunk, 2, ld_stat))
    hip.op_wino_stat(seg, x=dev(x), ldx=cin, cin=cin, w_host=w, bias_host=b, cout=cout, k=3, act=N.ACT_NONE, y=y, ldy=ldy, stat=stat, ld_stat=ld_stat, stat_nchunk=nchunk,
                     precision=0)
    y, stat = host(y), host(stat)
    assert kept(y[R:]) and kept(y[:, cout:]), "Y written outside its window"
    assert np.isfinite(y[:R, :cout]).all()
    plain = host(hip.op_conv1d(seg, dev(x), cin, w, b, act=0, force_tile=-4, precision="f32"))
    assert same_bits(plain[:, :cout], y[:R, :cout]), "Y differs from the launch without statistics"
    table_kept(stat, L, N.WINO_CHUNK, N.round_up(cout, 4), "winograd_output_kernel")
    wm, w2, _ = N.check_chunk_table(y, L, cout, N.WINO_CHUNK, stat, chan=True, what=f"winograd cout {cout}")
    print(f"\n[norm] winograd_output_kernel<8, true> cout {cout}: mean {wm:.3f} of bound (a), M2 {w2:.3f}")


# ------------------------------------------------------------------------------------------------ merges
@pytest.mark.parametrize("chunk", (N.STAT_CHUNK, N.WINO_CHUNK))
def test_merges_against_float64_of_their_own_table(hip, chunk):
    """adain_affine_kernel (serial) and adain_affine_lanes_kernel at lengths that reach every lane wrap: bound (b) against the float64 merge of the table the
    launch produced; they agree with each other within that bound; pad columns and the empty utterance are exactly 0.  At chunk 128 adain_apply_kernel's
    four-lane merge too, through bound (c) with no activation."""
    x, gb = N.merge_case(chunk)
    L, C, ld = N.MERGE_LENGTHS[chunk], N.MERGE_C, N.MERGE_LD
    seg, n = seg_of(L), len(L)
    nchunk = (max(L) + chunk - 1) // chunk
    out = {}
    for consumer in (1, 2):
        part, aff = sent((n, nchunk, 2, ld)), sent((n + 1, 2, ld))
        hip.op_adain(seg, x=dev(x), ldx=ld, C=C, producer=0 if chunk == N.STAT_CHUNK else 1, consumer=consumer, part=part, ldp=ld, nchunk=nchunk, gb=dev(gb), ld_gb=gb.shape[1],
                     gcol0=4, aff=aff, ld_aff=ld)
        out[consumer] = (host(part), host(aff))
        assert kept(out[consumer][1][n]), "affine table written past the last utterance"
        w = N.check_affine(out[consumer][0], L, C, chunk, gb, 4, out[consumer][1][:n], what=f"consumer {consumer} chunk {chunk}")
        print(f"\n[norm] {'adain_affine_kernel' if consumer == 1 else 'adain_affine_lanes_kernel'} chunk {chunk}: {w:.3f} of bound (b)")
    assert same_bits(out[1][0], out[2][0])
    gap = 0.0
    for u, Lu in enumerate(L):
        if Lu:
            t = N.merge_of(out[1][0], u, Lu, chunk, C, gb, 4)
            for k, d in ((0, t["dscale"]), (1, t["dshift"])):
                e = np.abs(out[1][1][u, k, :C].astype(F64) - out[2][1][u, k, :C])
                assert (e <= d).all(), ("serial and lanes tables differ by more than bound (b)", u, k, float((e / d).max()))
                gap = max(gap, float((e / d).max()))
    print(f"[norm] serial vs lanes, chunk {chunk}: largest gap {gap:.3f} of bound (b)")
    if chunk == N.STAT_CHUNK:
        part, y = sent((n, nchunk, 2, ld)), sent((sum(L) + 1, ld))
        hip.op_adain(seg, x=dev(x), ldx=ld, C=C, producer=0, consumer=3, part=part, ldp=ld, nchunk=nchunk, gb=dev(gb), ld_gb=gb.shape[1], gcol0=4, y=y, ldy=ld, rb=64,
                     act=N.ACT_NONE, out16=0)
        y = host(y)
        assert kept(y[sum(L) :])
        w = N.check_apply(x, host(part), L, C, gb, 4, N.ACT_NONE, None, y[: sum(L)], what="apply merge")
        print(f"[norm] adain_apply_kernel's merge (lengths to 2 100): {w:.3f} of bound (c)")


# ------------------------------------------------------------------------------------------------ apply
_APPLY32 = {}


def run_apply(hip, rb, mode, out16, only=None):
    """mode: 'none' / 'lrelu' / 'snake'.  -> (table, y [rows + 2, ldy]) as the launch left them."""
    x, gb, alpha = N.apply_case()
    L = N.APPLY_LENGTHS
    if only is not None:
        off = N.offsets(L)
        x, gb, L = x[off[only] : off[only + 1]], gb[only : only + 1], (L[only],)
    nchunk = (max(L) + 127) // 128
    part, y = sent((len(L), nchunk, 2, 160)), sent((sum(L) + 2, N.APPLY_LDY), bits16=out16 != 0)
    hip.op_adain(seg_of(L), x=dev(x), ldx=N.APPLY_LDX, C=N.APPLY_C, producer=0, consumer=3, part=part, ldp=160, nchunk=nchunk, gb=dev(gb), ld_gb=gb.shape[1], gcol0=4, y=y,
                 ldy=N.APPLY_LDY, rb=rb, act=N.ACT_LRELU if mode == "lrelu" else N.ACT_NONE, snake=dev(alpha) if mode == "snake" else None, out16=out16)
    return host(part), host(y)


def apply32(hip, rb, mode):
    if (rb, mode) not in _APPLY32:
        _APPLY32[rb, mode] = run_apply(hip, rb, mode, 0)
    return _APPLY32[rb, mode]


@pytest.mark.parametrize("rb", (64, 256))
@pytest.mark.parametrize("mode", ("none", "lrelu", "snake"))
@pytest.mark.parametrize("out16", (0, 1, 2))
def test_apply_against_float64(hip, rb, mode, out16):
    """adain_apply_kernel, C 130 into ldy 192: fp32 rows meet bound (c) and have zero pad columns; 16-bit rows are RNE of the fp32 launch bit for bit."""
    x, gb, alpha = N.apply_case()
    R = sum(N.APPLY_LENGTHS)
    table, y32 = apply32(hip, rb, mode)
    assert kept(y32[R:])
    if out16 == 0:
        w = N.check_apply(x, table, N.APPLY_LENGTHS, N.APPLY_C, gb, 4, N.ACT_LRELU if mode == "lrelu" else N.ACT_NONE, alpha if mode == "snake" else None, y32[:R],
                          what=f"apply rb {rb} {mode}")
        print(f"\n[norm] adain_apply_kernel rb {rb} {mode}: {w:.3f} of bound (c)")
        return
    t16, y16 = run_apply(hip, rb, mode, out16)
    assert same_bits(t16, table)
    assert kept(y16[R:])
    want = G.round_bits(y32[:R], PREC[out16]).reshape(R, -1)
    assert np.array_equal(y16[:R], want), ("16-bit rows != RNE(fp32 rows)", np.argwhere(y16[:R] != want)[:4])


@pytest.mark.parametrize("mode", ("none", "lrelu", "snake"))
def test_apply_ragged_equals_solo(hip, mode):
    _, y = apply32(hip, 64, mode)
    off = N.offsets(N.APPLY_LENGTHS)
    for u, L in enumerate(N.APPLY_LENGTHS):
        if L:
            _, solo = run_apply(hip, 64, mode, 0, only=u)
            assert same_bits(solo[:L], y[off[u] : off[u + 1]]), (mode, "utterance", u)


# ------------------------------------------------------------------------------------------------ row LayerNorm
def run_ln(hip, C, adaptive, outs, act=0, split=False, n_rows_real=-1):
    """outs: list of (k, prec16, ldy, ycol0) -> list of host arrays [rows + 1, ldy]."""
    x, g, b, sty = N.ln_case(C)
    ys, od = [], []
    styd = dev(sty)
    for k, prec16, ldy, ycol0 in outs:
        y = sent((N.LN_ROWS + 1, ldy), bits16=prec16 != 0)
        ys.append(y)
        if adaptive:
            od.append(dict(y=y, ldy=ldy, ycol0=ycol0, g=styd, ld_g=sty.shape[1], gcol0=4 + 2 * C * k, prec16=prec16))
        else:
            od.append(dict(y=y, ldy=ldy, ycol0=ycol0, g=dev(g[k]), b=dev(b[k]), prec16=prec16))
    f = dict(n_rows=N.LN_ROWS, n_rows_real=n_rows_real, C=C, adaptive=adaptive, act=act, eps=1e-5)
    if split:
        part, bias, r = N.ln_split_case(C)
        f.update(partial=dev(part), ksplit=3, slice_rows=part.shape[1], ld_part=part.shape[2], bias=dev(bias), in_act=N.ACT_LRELU, r=dev(r), ldr=r.shape[1], rcol0=4, in_alpha=N.RSQRT2)
    else:
        f.update(x=dev(x), ldx=x.shape[1])
    hip.op_row_layernorm(seg_of(N.LN_LENGTHS) if adaptive else None, od, **f)
    return [host(y) for y in ys]


@pytest.mark.parametrize("C", N.LN_C)
@pytest.mark.parametrize("adaptive", (0, 1))
def test_row_layernorm_against_float64(hip, C, adaptive):
    """row_layernorm_kernel, 9 rows (one with mean 100, standard deviation 0.01): both outputs of a two-output launch (the second 16-bit at ycol0 32), ReLU,
    the LnIn source (three split-K slices) and the n_rows_dev early-out."""
    x = N.ln_case(C)[0]
    R, p16 = N.LN_ROWS, 1 + adaptive
    y0, y1 = run_ln(hip, C, adaptive, [(0, 0, C + 8, 0), (1, p16, C + 40, 32)])
    (b1,) = run_ln(hip, C, adaptive, [(1, 0, C + 8, 0)])
    for y in (y0, b1):
        assert kept(y[R:]) and kept(y[:, C:])
    w0 = N.check_ln(x, C, 1e-5, adaptive, 0, N.ACT_NONE, y0[:R, :C], what="output 0")
    w1 = N.check_ln(x, C, 1e-5, adaptive, 1, N.ACT_NONE, b1[:R, :C], what="output 1")
    assert kept(y1[R:]) and kept(y1[:, :32]) and kept(y1[:, 32 + C :])
    want = G.round_bits(b1[:R, :C], PREC[p16]).reshape(R, C)
    assert np.array_equal(y1[:R, 32 : 32 + C], want), ("16-bit second output != RNE(fp32 launch)", np.argwhere(y1[:R, 32 : 32 + C] != want)[:4])
    (yr,) = run_ln(hip, C, adaptive, [(1, 0, C + 8, 0)], act=N.ACT_RELU)
    wr = N.check_ln(x, C, 1e-5, adaptive, 1, N.ACT_RELU, yr[:R, :C], what="ReLU")
    assert (yr[:R, :C] == np.maximum(b1[:R, :C], 0)).all(), "ReLU of the same launch's values"
    (ys,) = run_ln(hip, C, adaptive, [(0, 0, C + 8, 0)], split=True)
    part, bias, r = N.ln_split_case(C)
    xin = N.split_finish32(part, R, C, bias, N.ACT_LRELU, r, 4, N.RSQRT2)
    ws = N.check_ln(xin, C, 1e-5, adaptive, 0, N.ACT_NONE, ys[:R, :C], what="LnIn")
    assert kept(ys[R:]) and kept(ys[:, C:])
    (y5,) = run_ln(hip, C, adaptive, [(0, 0, C + 8, 0)], n_rows_real=5)
    assert kept(y5[5:]) and same_bits(y5[:5], y0[:5]), "n_rows_dev = 5: rows 5 .. 8 must keep the sentinel, rows 0 .. 4 the full launch's bits"
    print(f"\n[norm] row_layernorm_kernel C {C} adaptive {adaptive}: outputs {w0:.3f} / {w1:.3f}, ReLU {wr:.3f}, LnIn {ws:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("C", N.DW0_C)
@pytest.mark.parametrize("K", N.DW0_K)
def test_dwconv_against_float64(hip, C, K):
    """dwconv_kernel<31>, no activation and SiLU; pad columns and the row after the batch keep the sentinel."""
    L, x, w, b, _ = N.dw_case(C, K, False)
    R = sum(L)
    e = []
    for act in (N.ACT_NONE, N.ACT_SILU):
        y = sent((R + 1, C + 4))
        hip.op_dwconv(seg_of(L), x=dev(x), ldx=x.shape[1], C=C, K=K, form=0, act=act, w_host=w, bias_host=b, y=y, ldy=C + 4)
        y = host(y)
        assert kept(y[R:]) and kept(y[:, C:])
        e.append(N.check_dw0(C, K, act, y[:R], what=f"dwconv C {C} K {K} act {act}"))
    print(f"\n[norm] dwconv_kernel C {C} K {K}: {e[0]:.3f} of the bound, SiLU {e[1]:.3f}")


@pytest.mark.parametrize("C", N.DWLN_C)
@pytest.mark.parametrize("K", N.DWLN_K)
def test_dwconv_layernorm_fused_and_fallback(hip, C, K):
    """dwconv_ln_kernel<K, 16> (form 1) and dwconv_kernel + row_layernorm_kernel (form 2), utterances shorter than the half-kernel included: both meet the
    float64 bound, their gap lies within the sum of the two bounds; the 16-bit outputs are RNE of the same form's fp32 launch."""
    L, x, w, b, sty = N.dw_case(C, K, True)
    R = sum(L)
    want, dy = N.dwln_ref(C, K)
    ys, ratio = {}, {}
    for form in (1, 2):
        for p16 in (0, 1, 2):
            y = sent((R + 1, C + 4), bits16=p16 != 0)
            hip.op_dwconv(seg_of(L), x=dev(x), ldx=x.shape[1], C=C, K=K, form=form, act=0, w_host=w, bias_host=b, style=dev(sty), ld_style=sty.shape[1], gcol0=4, y=y, ldy=C + 4,
                          prec16=p16)
            y = host(y)
            assert kept(y[R:]) and kept(y[:, C:]), (form, p16)
            if p16 == 0:
                ys[form] = y[:R, :C]
                e = np.abs(ys[form] - want)
                assert (e <= dy).all(), (f"form {form}", np.argwhere(e > dy)[:2], float((e / dy).max()))
                ratio[form] = float((e / dy).max())
            else:
                w16 = G.round_bits(ys[form], PREC[p16]).reshape(R, C)
                assert np.array_equal(y[:R, :C], w16), (form, p16, "16-bit rows != RNE(fp32 rows)")
    gap = np.abs(ys[1].astype(F64) - ys[2])
    assert (gap <= 2 * dy).all(), float((gap / (2 * dy)).max())
    print(f"\n[norm] dwconv + LayerNorm C {C} K {K}: fused {ratio[1]:.3f}, two launches {ratio[2]:.3f} of the bound; largest gap between them {gap.max():.2e} "
          f"({(gap / (2 * dy)).max():.3f} of the sum of their bounds)")


# ------------------------------------------------------------------------------------------------ GRN
def test_grn_gx_and_input_affine(hip):
    """grn_gx_kernel (slot wrap above 256 rows, an empty utterance) and grn_xaff_kernel: gx within (slots + 1) u + sqrtf; the factor within its bound of the
    float64 factor of the kernel's own gx; shift exactly 0, pad scales exactly 0."""
    part, gamma = N.grn_case()
    L, C, ld = N.GRN_LENGTHS, N.GRN_C, N.GRN_LD
    n = len(L)
    gx, xaff = sent((n + 1, ld)), sent((n + 1, 2, ld))
    hip.op_grn(seg_of(L), mode=1, C=C, part=dev(part), ld_ss=ld, ss_stride=part.shape[1], gx=gx, ld_gx=ld, gamma=dev(gamma), xaff=xaff, ld_xaff=ld)
    gx, xaff = host(gx), host(xaff)
    assert kept(gx[n]) and kept(gx[:, C:]) and kept(xaff[n])
    wg = wf = 0.0
    for u, Lu in enumerate(L):
        ns = (Lu + 31) // 32
        want, d = N.gx_bound(part[u, :ns, :C], N.e_sqrt(part[u, :ns, :C].astype(F64).sum(0)))
        e = np.abs(gx[u, :C] - want)
        assert (e <= d).all(), ("gx", u, float((e[d > 0] / d[d > 0]).max()))
        f, df = N.factor_bound(gx[u, :C], gamma)
        ef = np.abs(xaff[u, 0, :C] - f)
        assert (ef <= df).all(), ("factor", u, float((ef / df).max()))
        assert (xaff[u, 1].view(np.uint32) == 0).all(), ("shift must be exactly 0", u)
        assert (xaff[u, 0, C:].view(np.uint32) == 0).all(), ("pad scales must be exactly 0", u)
        if Lu == 0:
            assert (gx[u, :C] == 0).all() and (xaff[u, 0, :C] == 1).all()
        else:
            wg, wf = max(wg, float((e / d).max())), max(wf, float((ef / df).max()))
    print(f"\n[norm] grn_gx_kernel: {wg:.3f} of its bound; grn_xaff_kernel factor: {wf:.3f} of its bound")


def test_grn_scale_weight(hip):
    """scale_weight_kernel<PREC>: fp32 copies within 4 u of W (gamma gx inv + 1) (the case makes the channel mean exact); the 16-bit copies are RNE of the fp32
    launch; an all-zero utterance and an empty one give W back exactly (scale 1, from mean + 1e-6)."""
    lengths, part, gxw, gamma, w = N.grn_exact_case()
    C, npad, n = N.GRN_SW_C, N.GRN_SW_NPAD, 4
    outs = {}
    for prec in (0, 1, 2):
        gx, wu = sent((n, C)), sent((n + 1, npad, C), bits16=prec != 0)
        hip.op_grn(seg_of(lengths), mode=2, C=C, part=dev(part), ld_ss=C, ss_stride=part.shape[1], gx=gx, ld_gx=C, gamma=dev(gamma), w=dev(w), npad=npad, kc=C, prec=prec, wu=wu)
        outs[prec] = host(wu)
        assert kept(outs[prec][n])
        assert (host(gx) == gxw).all(), "gx of the exact case"
    worst = 0.0
    for u in range(n):
        want, d = N.scale_weight_ref(gxw[u].astype(F32), gamma, w)
        e = np.abs(outs[0][u] - want)
        assert (e <= d).all(), (u, float((e / d).max()))
        worst = max(worst, float((e / d).max()))
        if u in (0, 3):
            assert same_bits(outs[0][u], w), ("scale must be exactly 1", u)
        for prec in (1, 2):
            assert np.array_equal(outs[prec][u], G.round_bits(outs[0][u], PREC[prec]).reshape(npad, C)), (u, prec)
    print(f"\n[norm] scale_weight_kernel<f32>: {worst:.3f} of 4 u")
