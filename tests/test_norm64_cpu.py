"""tests/norm64.py without a GPU: numpy-fp32 emulations of each kernel's formula (in one fixed order each) on every case of
tests/test_hip_norm_kernels.py must meet the bounds the kernels are held to - the bounds are not tighter than fp32 arithmetic allows - and a
one-pass M2 must FAIL bound (a) on the cancellation case - the case has teeth.  The float64 restatements are held to torch's own functions.

Measured here (-s): the ULP figures of norm64's docstring, and per family the worst emulation error / bound.
"""
import numpy as np
import pytest

import norm64 as N

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ fp32 emulations
def emu_chunk(x):
    """adain_partial_kernel's formula: mean, then the centred squares (two passes)."""
    nc = F32(x.shape[0])
    mean = x.sum(0, dtype=F32) / nc
    d = x - mean
    return mean, (d * d).sum(0, dtype=F32)


def emu_chunk_one_pass(x):
    """the 16-bit epilogue's formula: M2 = max(s2 - mean s1, 0)."""
    nc = F32(x.shape[0])
    s1, s2 = x.sum(0, dtype=F32), (x * x).sum(0, dtype=F32)
    mean = s1 * (F32(1) / nc)
    return mean, np.maximum(s2 - mean * s1, F32(0))


def emu_chunk_chan(x):
    """winograd_output_kernel<N, true>: groups of six rows, merged by Chan's update in group order."""
    nc = x.shape[0]
    gm, g2, gn = [], [], []
    for i in range(0, nc, N.WINO_M):
        g = x[i : i + N.WINO_M]
        m = g.sum(0, dtype=F32) * (F32(1) / F32(len(g)))
        d = g - m
        gm.append(m), g2.append((d * d).sum(0, dtype=F32)), gn.append(F32(len(g)))
    mean = np.zeros(x.shape[1], F32)
    for m, n in zip(gm, gn):
        mean = mean + n * m
    mean = mean * (F32(1) / F32(nc))
    m2 = np.zeros(x.shape[1], F32)
    for m, q, n in zip(gm, g2, gn):
        dv = m - mean
        m2 = m2 + (q + n * dv * dv)
    return mean, m2


def emu_table(x, lengths, C, chunk, fn):
    off = N.offsets(lengths)
    nchunk = max(1, (max(lengths) + chunk - 1) // chunk)
    t = np.full((len(lengths), nchunk, 2, C), np.nan, F32)
    for u, L in enumerate(lengths):
        for ch, nc in enumerate(N.chunk_rows_of(L, chunk)):
            t[u, ch, 0], t[u, ch, 1] = fn(x[off[u] + ch * chunk : off[u] + ch * chunk + nc, :C])
    return t


def emu_merge(means, m2s, ncs, g, b):
    """adain_scale_shift's formula, chunks in order."""
    n = F32(sum(ncs))
    mean = np.zeros(means.shape[1], F32)
    for m, nc in zip(means, ncs):
        mean = mean + F32(nc) * m
    mean = mean / n
    m2 = np.zeros_like(mean)
    for m, q, nc in zip(means, m2s, ncs):
        d = m - mean
        m2 = m2 + (q + F32(nc) * d * d)
    rstd = F32(1) / np.sqrt(m2 / n + F32(1e-5))
    sc = rstd * (F32(1) + g)
    return sc, b - mean * sc


def emu_affine(table, lengths, C, chunk, gb, gcol0, ld_aff):
    aff = np.zeros((len(lengths), 2, ld_aff), F32)
    for u, L in enumerate(lengths):
        if L:
            aff[u, 0, :C], aff[u, 1, :C] = emu_merge(*N.table_of(table, u, L, chunk, C), gb[u, gcol0 : gcol0 + C], gb[u, gcol0 + C : gcol0 + 2 * C])
    return aff


def emu_apply(x, aff, lengths, C, act, alpha, ldy):
    off = N.offsets(lengths)
    y = np.zeros((x.shape[0], ldy), F32)
    for u in range(len(lengths)):
        v = x[off[u] : off[u + 1], :C] * aff[u, 0, :C] + aff[u, 1, :C]
        if alpha is not None:
            s = np.sin(alpha * v)
            v = v + s * s / alpha
        elif act == N.ACT_LRELU:
            v = np.where(v >= 0, v, F32(0.2) * v)
        y[off[u] : off[u + 1], :C] = v
    return y


def emu_ln(x, g, b, eps, act):
    C = F32(x.shape[1])
    mean = x.sum(1, dtype=F32, keepdims=True) / C
    d = x - mean
    rstd = F32(1) / np.sqrt((d * d).sum(1, dtype=F32, keepdims=True) / C + F32(eps))
    y = d * rstd * g.astype(F32) + b.astype(F32)
    return np.maximum(y, F32(0)) if act == N.ACT_RELU else y


def emu_dwconv(x, lengths, w, b):
    K = w.shape[1]
    pad = (K - 1) // 2
    off = N.offsets(lengths)
    y = np.empty((x.shape[0], w.shape[0]), F32)
    for u, L in enumerate(lengths):
        xp = np.zeros((L + K - 1, w.shape[0]), F32)
        xp[pad : pad + L] = x[off[u] : off[u + 1], : w.shape[0]]
        acc = np.tile(b, (L, 1))
        for k in range(K):
            acc = acc + w[:, k] * xp[k : k + L]
        y[off[u] : off[u + 1]] = acc
    return y


# ------------------------------------------------------------------------------------------------ restatements against torch
def test_restatements_match_torch():
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F

    rng = np.random.default_rng(1)
    x = rng.standard_normal((50, 12))
    g, b = rng.standard_normal(12), rng.standard_normal(12)
    xt = torch.from_numpy(x)
    want = (1 + torch.from_numpy(g)) * F.instance_norm(xt.T[None], eps=N.EPS_IN)[0].T + torch.from_numpy(b)
    assert np.abs(N.adain64(x, g, b) - want.numpy()).max() < 1e-12
    sc, sh = N.adain_affine64(x, g, b)
    assert np.abs(x * sc + sh - want.numpy()).max() < 1e-12
    want = F.layer_norm(xt, (12,), torch.from_numpy(g), torch.from_numpy(b), 1e-6)
    assert np.abs(N.layernorm64(x, g, b, 1e-6) - want.numpy()).max() < 1e-12
    w, bias = rng.standard_normal((12, 7)), rng.standard_normal(12)
    lengths = (3, 40, 7)
    want = torch.cat([F.conv1d(xt[a:e].T[None], torch.from_numpy(w)[:, None], torch.from_numpy(bias), padding=3, groups=12)[0].T
                      for a, e in zip(N.offsets(lengths)[:-1], N.offsets(lengths)[1:])])
    assert np.abs(N.dwconv64(x, lengths, w, bias) - want.numpy()).max() < 1e-12
    gx = torch.norm(xt, p=2, dim=0)
    want = torch.from_numpy(g) * (gx / (gx.mean() + N.EPS_GRN)) + 1
    assert np.abs(N.grn_factor64(N.grn_gx64(x ** 2), g) - want.numpy()).max() < 1e-12
    al = rng.uniform(0.1, 3, 12)
    want = xt + (1 / torch.from_numpy(al)) * torch.sin(torch.from_numpy(al) * xt) ** 2
    assert np.abs(N.snake64(x, al) - want.numpy()).max() < 1e-12


def test_measured_ulp_figures():
    """The figures of norm64's docstring: 4 x numpy-fp32 against float64 on the cases' own inputs."""
    x, gb, alpha = N.apply_case()
    v = N.adain64(x[1:64, : N.APPLY_C], gb[2, 4 : 4 + N.APPLY_C], gb[2, 4 + N.APPLY_C : 4 + 2 * N.APPLY_C])
    figs = dict(rsqrt_u=N.rho_rsqrt(np.abs(x[:, : N.APPLY_C].astype(F64)) ** 2 + N.EPS_IN), sin_u=N.e_sin(alpha * v) / N.U,
                exp2_u=N.e_exp2_rcp(v * 2.0)[0] / N.U, rcp_u=N.e_exp2_rcp(v * 2.0)[1] / N.U, sqrt_u=N.e_sqrt(N.grn_case()[0].astype(F64)) / N.U)
    print("\n[norm64] allowed (= 4 x measured numpy fp32) in units of u:", {k: round(v, 2) for k, v in figs.items()})
    assert 2.0 <= figs["rsqrt_u"] <= 12.0 and 2.0 <= figs["sin_u"] <= 8.0 and 2.0 <= figs["exp2_u"] <= 8.0 and 2.0 <= figs["rcp_u"] <= 4.0 + 1e-9 and 2.0 <= figs["sqrt_u"] <= 4.0 + 1e-9, figs


# ------------------------------------------------------------------------------------------------ the bounds admit fp32
@pytest.mark.parametrize("C,ldx", N.STAT_C)
@pytest.mark.parametrize("chunk", (N.STAT_CHUNK, N.WINO_CHUNK))
def test_two_pass_chunks_meet_bound_a(C, ldx, chunk):
    x = N.stat_case(C, ldx)
    t = emu_table(x, N.STAT_LENGTHS, C, chunk, emu_chunk)
    wm, w2, _ = N.check_chunk_table(x, N.STAT_LENGTHS, C, chunk, t)
    print(f"\n[norm64] two-pass emulation C {C} chunk {chunk}: mean {wm:.3f} of its bound, M2 {w2:.3f}")


def test_cancellation_case_two_pass_passes_one_pass_fails():
    x = N.cancel_case()
    t = emu_table(x, N.CANCEL_LENGTHS, 64, N.STAT_CHUNK, emu_chunk)
    _, w2, rel = N.check_chunk_table(x, N.CANCEL_LENGTHS, 64, N.STAT_CHUNK, t)
    one = emu_table(x, N.CANCEL_LENGTHS, 64, N.STAT_CHUNK, emu_chunk_one_pass)
    with pytest.raises(AssertionError, match="M2"):
        N.check_chunk_table(x, N.CANCEL_LENGTHS, 64, N.STAT_CHUNK, one)
    # how far: relative M2 error of the one-pass formula on the eight channels
    off = N.offsets(N.CANCEL_LENGTHS)
    r1 = 0.0
    for u, L in enumerate(N.CANCEL_LENGTHS):
        for ch, nc in enumerate(N.chunk_rows_of(L, 128)):
            _, m2, _, _ = N.chunk_bound(x[off[u] + 128 * ch : off[u] + 128 * ch + nc])
            if nc == 128:
                r1 = max(r1, float((np.abs(one[u, ch, 1] - m2) / m2)[list(N.CANCEL_CH)].max()))
    print(f"\n[norm64] cancellation channels, relative M2 error: two-pass {rel[list(N.CANCEL_CH)].max():.2e} ({w2:.3f} of the bound), one-pass {r1:.2e}")
    assert r1 > 1e-3 > 100 * rel[list(N.CANCEL_CH)].max()


@pytest.mark.parametrize("cout", N.WINO_COUT)
def test_chan_chunks_meet_bound_a(cout):
    x = N.ragged(900 + cout, N.WINO_LENGTHS, cout, cout)
    t = emu_table(x, N.WINO_LENGTHS, cout, N.WINO_CHUNK, emu_chunk_chan)
    wm, w2, _ = N.check_chunk_table(x, N.WINO_LENGTHS, cout, N.WINO_CHUNK, t, chan=True)
    print(f"\n[norm64] Chan emulation cout {cout}: mean {wm:.3f} of its bound, M2 {w2:.3f}")


@pytest.mark.parametrize("chunk", (N.STAT_CHUNK, N.WINO_CHUNK))
def test_merge_meets_bound_b(chunk):
    x, gb = N.merge_case(chunk)
    L = N.MERGE_LENGTHS[chunk]
    t = emu_table(x, L, N.MERGE_C, chunk, emu_chunk)
    aff = emu_affine(t, L, N.MERGE_C, chunk, gb, 4, N.MERGE_LD)
    w = N.check_affine(t, L, N.MERGE_C, chunk, gb, 4, aff)
    print(f"\n[norm64] merge emulation chunk {chunk}: {w:.3f} of bound (b)")
    bad = aff.copy()
    bad[3, 0, 5] *= F32(1 + 1e-4)
    with pytest.raises(AssertionError, match="scale"):
        N.check_affine(t, L, N.MERGE_C, chunk, gb, 4, bad)


@pytest.mark.parametrize("act,snake", ((N.ACT_NONE, False), (N.ACT_LRELU, False), (N.ACT_NONE, True)))
def test_apply_meets_bound_c(act, snake):
    x, gb, alpha = N.apply_case()
    C, L = N.APPLY_C, N.APPLY_LENGTHS
    t = emu_table(x, L, C, N.STAT_CHUNK, emu_chunk)
    aff = emu_affine(t, L, C, N.STAT_CHUNK, gb, 4, N.APPLY_LDY)
    y = emu_apply(x, aff, L, C, act, alpha if snake else None, N.APPLY_LDY)
    w = N.check_apply(x, t, L, C, gb, 4, act, alpha if snake else None, y)
    print(f"\n[norm64] apply emulation act {act} snake {snake}: {w:.3f} of bound (c)")


@pytest.mark.parametrize("C", N.LN_C)
@pytest.mark.parametrize("adaptive", (0, 1))
def test_layernorm_meets_its_bound(C, adaptive):
    x = N.ln_case(C)[0]
    for k, act in ((0, N.ACT_NONE), (1, N.ACT_RELU)):
        g, b = N.ln_gain(C, adaptive, k)
        w = N.check_ln(x, C, 1e-5, adaptive, k, act, emu_ln(x[:, :C], g, b, 1e-5, act))
    part, bias, r = N.ln_split_case(C)
    xin = N.split_finish32(part, N.LN_ROWS, C, bias, N.ACT_LRELU, r, 4, N.RSQRT2)
    g, b = N.ln_gain(C, adaptive, 0)
    w2 = N.check_ln(xin, C, 1e-5, adaptive, 0, N.ACT_NONE, emu_ln(xin, g, b, 1e-5, N.ACT_NONE))
    print(f"\n[norm64] LayerNorm emulation C {C} adaptive {adaptive}: {w:.3f} / LnIn {w2:.3f} of the bound")


@pytest.mark.parametrize("C", N.DW0_C)
@pytest.mark.parametrize("K", N.DW0_K)
def test_dwconv_meets_its_bound(C, K):
    L, x, w, b, _ = N.dw_case(C, K, False)
    y = emu_dwconv(x, L, w, b)
    e0 = N.check_dw0(C, K, N.ACT_NONE, y)
    with np.errstate(over="ignore"):
        e1 = N.check_dw0(C, K, N.ACT_SILU, y * (F32(1) / (F32(1) + np.exp(-y))))
    print(f"\n[norm64] dwconv emulation C {C} K {K}: {e0:.3f} / SiLU {e1:.3f} of the bound")


@pytest.mark.parametrize("C", N.DWLN_C)
@pytest.mark.parametrize("K", N.DWLN_K)
def test_dwconv_ln_meets_its_bound(C, K):
    L, x, w, b, sty = N.dw_case(C, K, True)
    row_utt = np.repeat(np.arange(len(L)), L)
    y = emu_ln(emu_dwconv(x, L, w, b), 1.0 + sty[row_utt, 4 : 4 + C].astype(F64), sty[row_utt, 4 + C : 4 + 2 * C], N.EPS_GRN, N.ACT_NONE)
    want, dy = N.dwln_ref(C, K)
    e = np.abs(y - want)
    assert (e <= dy).all(), float((e / dy).max())
    print(f"\n[norm64] dwconv + LayerNorm emulation C {C} K {K}: {(e / dy).max():.3f} of the bound")


def test_grn_meets_its_bounds():
    part, gamma = N.grn_case()
    C = N.GRN_C
    for u, L in enumerate(N.GRN_LENGTHS):
        ns = (L + 31) // 32
        gx = np.sqrt(part[u, :ns, :C].sum(0, dtype=F32))
        want, d = N.gx_bound(part[u, :ns, :C], N.e_sqrt(part[u, :ns, :C].astype(F64).sum(0)))
        assert (np.abs(gx - want) <= d).all(), u
        inv = F32(1) / (gx.sum(dtype=F32) / F32(C) + F32(1e-6))
        f, df = N.factor_bound(gx, gamma)
        assert (np.abs(gamma * gx * inv + F32(1) - f) <= df).all(), u
    lengths, part, gx, gamma, w = N.grn_exact_case()
    for u in range(4):
        g32 = np.sqrt(part[u].sum(0, dtype=F32))
        assert (g32 == gx[u]).all()
        inv = F32(1) / (g32.sum(dtype=F32) / F32(N.GRN_SW_C) + F32(1e-6))
        want, d = N.scale_weight_ref(g32, gamma, w)
        got = w * (gamma * g32 * inv + F32(1))
        assert (np.abs(got - want) <= d).all(), u
        if u in (0, 3):
            assert (got == w).all()
