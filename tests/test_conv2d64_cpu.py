"""tests/conv2d64.py on its own, without a GPU: the float64 restatement of the 2-D convolution equals torch's float64 F.conv2d / F.conv_transpose2d; a
numpy-fp32 emulation of the engine's chunked summation (packed rows, the kernel's row maps, K in steps of one fp32 multiply-add, chunk sums in order)
meets the bound on every case tests/test_hip_conv2d.py runs; and each of seven emulated defects - the last 16-wide K step dropped, the last chunk
skipped, the last chunk added twice, a tap's column shifted by one, a boundary row taken from the neighbouring utterance, the bias of channel n + 1, the
parity pt ignored - exceeds its case's bound at least ten times, so none can hide under it.

The emulation, which rounds every product and every addition (the matrix core fuses them), uses 0.025 .. 0.23 of the bound (-s prints each case); the
defects are 3.4e4 times the bound and more (-s)."""
import numpy as np
import pytest

import conv2d64 as V

torch = pytest.importorskip("torch")
F = torch.nn.functional
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the restatement against torch
def t64(x):
    """dense [T][Fin][C] -> torch [1][C][T][Fin] float64"""
    return torch.from_numpy(np.asarray(x, F64)).permute(2, 0, 1)[None]


def dense(y):
    return y[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("k,pad,T,Fin", [(3, 1, 7, 6), (1, 0, 5, 4), (5, 0, 9, 7), (5, 0, 5, 5), (3, 1, 1, 1)])
def test_restatement_equals_torch_conv2d(k, pad, T, Fin):
    rng = np.random.default_rng(k * 100 + T)
    cin, cout = 5, 4
    x, w, b = rng.standard_normal((T, Fin, cin)), rng.standard_normal((cout, cin, k * k)), rng.standard_normal(cout)
    dt, df = V.taps_same(k) if pad else V.taps_valid(k)
    To, Fo = (T, Fin) if pad else (T - k + 1, Fin - k + 1)
    got = V.conv2d64((x,), w, dt, df, To, Fo, bias=b)
    want = dense(F.conv2d(t64(x), torch.from_numpy(w.reshape(cout, cin, k, k)), torch.from_numpy(b), padding=pad))
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-12


def test_restatement_of_two_segments_and_the_epilogue():
    """cat(a, b) as two segments, LeakyReLU on the operand, sigmoid / ReLU, the residual and the division, against torch on the concatenated tensor."""
    rng = np.random.default_rng(5)
    T, Fin, c0, c1, cout = 6, 5, 3, 4, 5
    a, b2 = rng.standard_normal((T, Fin, c0)), rng.standard_normal((T, Fin, c1))
    w, b, r = rng.standard_normal((cout, c0 + c1, 9)), rng.standard_normal(cout), rng.standard_normal((T, Fin, cout))
    dt, df = V.taps_same(3)
    xc = torch.cat([t64(a), t64(b2)], 1)
    wt = torch.from_numpy(w.reshape(cout, c0 + c1, 3, 3))
    for act, fn in ((V.ACT_NONE, lambda v: v), (V.ACT_RELU, torch.relu), (V.ACT_SIGMOID, torch.sigmoid)):
        got = V.conv2d64((a, b2), w, dt, df, T, Fin, lrelu=True, bias=b, act=act, res=r, div=1.25)
        want = dense((fn(F.conv2d(F.leaky_relu(xc, V.LRELU), wt, torch.from_numpy(b), padding=1)) + t64(r)) / 1.25)
        assert np.abs(got - want).max() < 1e-12, act


def test_four_subpixel_launches_equal_conv_transpose2d():
    rng = np.random.default_rng(6)
    T, Fin, cin, cout = 4, 5, 3, 4
    x, wt = rng.standard_normal((T, Fin, cin)), rng.standard_normal((cin, cout, 3, 3))
    out = np.full((2 * T, 2 * Fin, cout), np.nan)
    for pt in (0, 1):
        for pf in (0, 1):
            dt, df, w = V.subpixel(wt, pt, pf)
            assert len(dt) == (1 + pt) * (1 + pf)
            out[pt::2, pf::2] = V.conv2d64((x,), w, dt, df, T, Fin, up=2, pt=pt, pf=pf)
    want = dense(F.conv_transpose2d(t64(x), torch.from_numpy(wt), stride=2, padding=1, output_padding=1))
    assert out.shape == want.shape and np.abs(out - want).max() < 1e-12


def test_the_up2_cases_are_the_transposed_conv():
    """The four up2 cases share their inputs and one ConvTranspose2d weight; together they are relu(conv_transpose2d + bias)."""
    ds = [V.data(n) for n in V.UP2]
    assert all(np.array_equal(d["wt"], ds[0]["wt"]) and np.array_equal(d["bias"], ds[0]["bias"]) for d in ds)
    assert all(np.array_equal(a, b) for d in ds for a, b in zip(d["x0"], ds[0]["x0"]))
    got = np.zeros(V.expected(V.UP2[0])[0].shape)
    seen = np.zeros(got.shape[:2], int)
    for n in V.UP2:
        want, _, written = V.expected(n)
        got[written] = want[written]
        seen += written
    assert (seen == 1).all()
    ref = [dense(torch.relu(F.conv_transpose2d(t64(x), torch.from_numpy(ds[0]["wt"].astype(F64)), torch.from_numpy(ds[0]["bias"].astype(F64)), stride=2, padding=1,
                                               output_padding=1))) for x in ds[0]["x0"] if len(x)]
    assert np.abs(got - np.concatenate(ref)).max() < 1e-9 * V.BIG


# ------------------------------------------------------------------------------------------------ the engine's summation in numpy fp32
def emulate(name, defect=None, out=None):
    """The launch of case `name` in numpy fp32 on the engine's packed rows -> the output rows [out_rows][cout], NaN where nothing is written."""
    c, d = V.CASES[name], V.data(name)
    x = [V.pack_rows(d["x0"], c.ld0, 1)] + ([V.pack_rows(d["x1"], c.ld1, 2)] if c.cin1 else [])
    off_in, off_out = V.offsets(c.lens), V.offsets(c.lens_out)
    m = np.arange(c.rows)
    tr, f = m // c.F, m % c.F
    u = np.searchsorted(off_out, tr, side="right") - 1
    t, in0, T = tr - off_out[u], off_in[u], off_in[u + 1] - off_in[u]
    dt, df = list(c.dt), list(c.df)
    if defect == "column":
        df[1 % len(df)] += 1
    Kt = c.ld0 + c.ld1
    A = np.zeros((c.rows, c.K), F32)
    for tap in range(len(dt)):
        ti, fi = t + dt[tap], f + df[tap]
        ok = (ti >= 0) & (ti < T) & (fi >= 0) & (fi < c.Fin)
        if defect == "neighbour":
            ok = (in0 + ti >= 0) & (in0 + ti < off_in[-1]) & (fi >= 0) & (fi < c.Fin)
        row = np.where(ok, (in0 + ti) * c.Fin + fi, 0)
        k0 = tap * Kt
        for xs, ld in zip(x, (c.ld0, c.ld1)):
            A[:, k0 : k0 + ld] = np.where(ok[:, None], xs[row], F32(0)) if len(xs) else 0
            k0 += ld
    if c.lrelu:
        A = np.where(A > 0, A, F32(0.2) * A).astype(F32)
    W = np.zeros((c.K, c.cout), F32)
    W[V.k_index(c.cin0, c.cin1, c.ld0, c.ld1, len(dt)).reshape(-1)] = d["w"].transpose(2, 1, 0).reshape(-1, c.cout)
    assert np.isfinite(A).all()
    chunks = [(k, min(k + c.chunk, c.K)) for k in range(0, c.K, c.chunk)]
    if defect == "skip_chunk":
        chunks = chunks[:-1]
    elif defect == "double_chunk":
        chunks = chunks + chunks[-1:]
    elif defect == "drop_step":
        chunks[-1] = (chunks[-1][0], chunks[-1][1] - V.BK)
    tot = np.zeros((c.rows, c.cout), F32)
    for k0, k1 in chunks:
        acc = np.zeros((c.rows, c.cout), F32)
        for k in range(k0, k1):
            acc = acc + A[:, k : k + 1] * W[k][None, :]
        tot = tot + acc
    v = tot
    pt = 0 if defect == "parity" else c.pt
    orow = (tr * c.up + pt) * (c.F * c.up) + f * c.up + c.pf
    with np.errstate(over="ignore"):
        if d["bias"] is not None:
            v = v + (np.roll(d["bias"], -1) if defect == "bias" else d["bias"])[None, :]
        if c.act == V.ACT_RELU:
            v = np.maximum(v, F32(0))
        elif c.act == V.ACT_SIGMOID:
            v = F32(1) / (F32(1) + np.exp(-v))
        if d["res"] is not None:
            v = v + np.concatenate([r.reshape(-1, c.cout) for r in d["res"]])[orow]
        v = v / F32(c.div)
    assert v.dtype == F32
    if out is None:
        out = np.full((c.out_rows, c.cout), np.nan, F32)
    out[orow] = v
    return out


def fraction(name, out):
    want, bound, written = V.expected(name)
    out = out.reshape(want.shape)
    return V.worst(out[written], want[written], bound[written])


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_emulation_meets_every_bound(name):
    out = emulate(name)
    want, _, written = V.expected(name)
    assert np.isnan(out.reshape(want.shape)[~written]).all() and np.isfinite(out.reshape(want.shape)[written]).all()
    e = fraction(name, out)
    print(f"\n[conv2d64] {name}: the fp32 emulation uses {e:.3f} of the bound")
    assert e <= 1.0


DEFECTS = [("drop_step", "k144_chunk64_s0"), ("drop_step", "two_segments_s0"), ("drop_step", "k144_chunk144_s0"),
           ("skip_chunk", "k144_chunk64_s0"), ("skip_chunk", "two_segments_s0"), ("skip_chunk", "valid5_s0"),
           ("double_chunk", "k144_chunk64_s0"), ("double_chunk", "two_segments_s0"), ("double_chunk", "valid5_s0"),
           ("column", "tile_n64c33_A"), ("column", "valid5_s0"), ("column", "up2_11"),
           ("neighbour", "tile_n16c16_B"), ("neighbour", "shift2"), ("neighbour", "up2_11"),  # (a valid conv never leaves its utterance)
           ("bias", "epi_bias"), ("bias", "epi_sigmoid"), ("bias", "frames_1tap"), ("bias", "up2_00")]


@pytest.mark.parametrize("defect,name", DEFECTS)
def test_a_defect_cannot_hide_under_the_bound(defect, name):
    e = fraction(name, emulate(name, defect))
    print(f"\n[conv2d64] {name} with the defect '{defect}': {e:.3g} times the bound")
    assert e >= 10.0


def test_an_ignored_parity_cannot_hide():
    """All four sub-pixel launches with pt taken as 0: the rows of parity 1 are never written, and those of parity 0 hold the wrong launch's values."""
    c = V.CASES[V.UP2[0]]
    out = np.full((c.out_rows, c.cout), np.nan, F32)
    for n in V.UP2:
        emulate(n, "parity", out)
    for n in V.UP2:
        e = fraction(n, out)
        print(f"\n[conv2d64] {n} after four launches that ignore pt: {e:.3g} times the bound")
        assert e >= 10.0
    grid = out.reshape(V.expected(V.UP2[0])[0].shape)
    assert np.isnan(grid[1::2]).all() and np.isfinite(grid[0::2]).all()
