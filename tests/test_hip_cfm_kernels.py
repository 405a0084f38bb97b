"""The flow-matching estimator's row kernels (csrc/cfm.hip.h: small_linear, cfm_time_embed, small_layernorm, cfm_source, rms_adaln, axial_rope,
gated_residual, mish, swiglu) and the encoders' sequence rotary embedding (rope_kernel, csrc/phoneme.hip.h), one launch at a time against float64
(tests/cfm64.py), through stts_op_cfm_elem / _rms_adaln / _rope / _cfm_small / _cfm_source - which launch through the helpers cfm_estimator itself uses, so
the grids (their caps of 1024 / 2048 blocks and the stride loops behind them included) are the product's.

Every bound is cfm64's (derived there from the kernels' arithmetic, met by numpy-fp32 emulations and missed by emulated defects in tests/test_cfm64_cpu.py).
Every output buffer is pre-filled with the quiet NaN 0x7FC0BEEF and compared as bits: guard rows and guard columns must keep it; in-place buffers (the rotary
kernels, Mish) must keep every bit outside the features they turn.  Neighbouring utterances and all pad columns hold values 1e3 times larger, so a row or column
leaking across a boundary cannot hide.  -s prints error / bound per case.

Measured on an MI355X (-s prints them), largest error as a fraction of its bound:
  rms_adaln_kernel        plain and Y = X 0.50 - 0.68, fused 0.39 - 0.63, Xout 0.82 - 0.97 (three roundings, all of the bound)
  gated_residual_kernel   0.73 (C 32), 0.97 (C 1024, stride loop)
  axial_rope_kernel       0.11 - 0.14;  rope_kernel 0.19 - 0.30
  cfm_time_embed_kernel   0.25 - 0.36;  small_layernorm_kernel 0.05 - 0.23;  small_linear_kernel 0.000 - 0.025
  mish_kernel             0.20 (grid), 0.16 (stride loop);  swiglu_kernel 0.20 - 0.27
  cfm_source_kernel       ideal form 0.00 - 0.97 (0.97: the constant-F0 utterance, 219 wraps whose roundings all have one sign), own angle 0.05 - 0.24
Sensitivity on scratch copies of the kernels: DESIGN.md 5g.2.
"""
import numpy as np
import pytest

import cfm64 as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
SENT32 = M.SENT32


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


def sent(shape):
    return torch.from_numpy(np.full(shape, SENT32, np.uint32).view(np.float32)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def kept(a):
    return bool((bits(a) == SENT32).all())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def show(what, r):
    print(f"[cfm] {what}: error / bound {r:.3f}")
    assert r < 1.0, (what, r)


# ------------------------------------------------------------------------------------------------ RMSNorm + AdaLN, gated residual
@pytest.mark.parametrize("C", M.RMS_C)
def test_rms_adaln_against_float64(hip, C):
    """plain, fused with the previous branch's gated residual, fused with Xout, and Y aliasing X (the estimator's form): lengths 1, 5, 0, 4, 7, ldx = C + 32."""
    case = M.rms_case(C)
    L, R = case["lengths"], case["R"]
    seg = seg_of(L)
    w, ada, ada_prev, t = dev(case["w"]), dev(case["ada"]), dev(case["ada_prev"]), dev(case["t"])
    print()
    for mode in M.RMS_MODES:
        x = dev(case["x"])
        fused = mode in ("fused", "fused_xout")
        y = x if mode == "alias" else sent((R + 2, C + 16))
        xout = sent((R + 2, C)) if mode == "fused_xout" else None
        hip.op_rms_adaln(seg, x=x, ldx=C + 32, C=C, w=w, ada=ada, y=y, ldy=y.shape[1], t=t if fused else None, ada_prev=ada_prev if fused else None, xout=xout)
        ya = host(y)
        if mode == "alias":
            assert same_bits(ya[R:], case["x"][R:]) and same_bits(ya[:, C:], case["x"][:, C:]), "written outside the rows' C columns"
        else:
            assert kept(ya[R:]) and kept(ya[:, C:]), "Y written outside its window"
            assert same_bits(host(x), case["x"]), "X written"
        xo = None
        if xout is not None:
            xo = host(xout)
            assert kept(xo[R:]), "Xout written past the rows"
            xo = xo[:R]
        for k, r in M.rms_check(case, mode, ya[:R, :C], xo).items():
            show(f"rms_adaln C {C} {mode} {k}", r)


@pytest.mark.parametrize("C,lengths", M.GATED_CASES)
def test_gated_residual_against_float64(hip, C, lengths):
    """C 32 and 1024; at 1100 rows x 256 float4s the grid cap of 1024 blocks is exceeded and the stride loop runs."""
    case = M.gated_case(C, lengths)
    R = case["R"]
    h, t, y = dev(case["h"]), dev(case["t"]), sent((R + 1, C))
    hip.op_cfm_elem(seg_of(lengths), kind=2, C=C, x=h, t=t, ada=dev(case["ada"]), y=y)
    ya = host(y)
    assert kept(ya[R:]) and same_bits(host(h), case["h"]) and same_bits(host(t), case["t"])
    print()
    show(f"gated_residual C {C} lengths {lengths}", M.gated_check(case, ya[:R]))


# ------------------------------------------------------------------------------------------------ rotary embeddings
def run_rope(hip, case, d, freq=None):
    x = dev(case["x"])
    hip.op_rope(seg_of(case["lengths"]), kind=case["kind"], x=x, ldx=case["ld"], col0=case["col0"], col1=case["col1"], heads=case["heads"], kc=case["kc"], d=d,
                freq=None if freq is None else dev(freq))
    return host(x)


@pytest.mark.parametrize("two_blocks", (False, True))
@pytest.mark.parametrize("heads,d", M.AXIAL_SHAPES)
def test_axial_rope_against_float64(hip, heads, d, two_blocks):
    """lengths 1, 2, 3, 37, 800 (pos -1 alone, the two ends, odd n across the p < n / 2 switch); col1 -1, and col1 = dim in a q | k | v buffer whose v block,
    like every guard column and the guard row, must stay bit-identical (cfm64.rope_check asserts it)."""
    freq = M.axial_freq(heads, d)
    case = M.rope_case(0, heads, d, M.AXIAL_LENGTHS, two_blocks)
    print()
    show(f"axial_rope heads {heads} d {d} col1 {case['col1']}", M.rope_check(case, d, run_rope(hip, case, d, freq), freq))


def test_axial_rope_beyond_the_grid_cap(hip):
    """8 heads x 1100 rows x 32 pairs = 1100 blocks of 256: the grid is capped at 1024 and the stride loop runs."""
    heads, d, L = M.AXIAL_STRIDE
    freq = M.axial_freq(heads, d)
    case = M.rope_case(0, heads, d, L, True)
    print()
    show("axial_rope 8 heads x 1100 rows", M.rope_check(case, d, run_rope(hip, case, d, freq), freq))


@pytest.mark.parametrize("two_blocks", (False, True))
@pytest.mark.parametrize("heads,kc,d", M.SEQ_SHAPES)
def test_sequence_rope_against_float64(hip, heads, kc, d, two_blocks):
    """rope_kernel through run_rope: lengths 1, 33, 512, both col1 forms; features d .. kc - 1 of every head stay bit-identical."""
    case = M.rope_case(1, heads, kc, M.SEQ_LENGTHS, two_blocks)
    print()
    show(f"rope heads {heads} kc {kc} d {d} col1 {case['col1']}", M.rope_check(case, d, run_rope(hip, case, d)))


# ------------------------------------------------------------------------------------------------ the per-utterance kernels
@pytest.mark.parametrize("n_utt", M.TIME_U)
@pytest.mark.parametrize("half", M.TIME_HALF)
def test_time_embedding_against_float64(hip, half, n_utt):
    """cos | sin of the fp32 angle (1000 t) f: t 0, 1e-3, 0.5 (and 1 alone); lde = 2 half + 8."""
    f = M.time_freqs(half)
    t = np.array(M.TIME_T[:3] if n_utt == 3 else M.TIME_T[3:], F32)
    want, bound = M.time_embed_bound(t, f)
    e = sent((n_utt + 1, 2 * half + 8))
    hip.op_cfm_small(kind=2, n_rows=n_utt, N=half, x=dev(t), w=dev(f), y=e, ldy=e.shape[1])
    ea = host(e)
    assert kept(ea[n_utt:]) and kept(ea[:, 2 * half :])
    print()
    show(f"time embedding half {half} U {n_utt}", M.ratio(ea[:n_utt, : 2 * half], want, bound))


@pytest.mark.parametrize("C", M.LN_C)
def test_small_layernorm_against_float64(hip, C):
    """three rows, one of them mean-heavy (mean^2 / var = 1e4: a one-pass variance fails here), C 32 (half a wave idle), 100, 256."""
    c = M.layernorm_case(C)
    want, bound = M.layernorm_small_bound(c["x"][:, :C], c["g"], c["b"])
    y = sent((4, C + 4))
    hip.op_cfm_small(kind=1, n_rows=3, N=C, x=dev(c["x"]), ldx=C + 8, w=dev(c["g"]), b=dev(c["b"]), y=y, ldy=C + 4)
    ya = host(y)
    assert kept(ya[3:]) and kept(ya[:, C:])
    print()
    for r, name in enumerate(("N(0, 1)", "mean-heavy", "1e3 large")):
        show(f"small_layernorm C {C} row {name}", M.ratio(ya[r : r + 1, :C], want[r : r + 1], bound[r : r + 1]))


@pytest.mark.parametrize("rows", M.LINEAR_ROWS)
@pytest.mark.parametrize("N,K", M.LINEAR_NK)
def test_small_linear_against_float64(hip, N, K, rows):
    """with and without bias, act 0 and 1, ldx = K + 8, ldy = N + 4; K 48 and 100 leave tail lanes, rows * N is no multiple of the 4 outputs of a block."""
    c = M.linear_case(N, K, rows)
    x, w = dev(c["x"]), dev(c["w"])
    print()
    for act in (0, 1):
        for b in (None, c["b"]):
            want, bound, rho = M.linear_bound(c["x"][:, :K], c["w"], b, act)
            y = sent((rows + 1, N + 4))
            hip.op_cfm_small(kind=0, n_rows=rows, N=N, K=K, act=act, x=x, ldx=K + 8, w=w, b=None if b is None else dev(b), y=y, ldy=N + 4)
            ya = host(y)
            assert kept(ya[rows:]) and kept(ya[:, N:])
            show(f"small_linear N {N} K {K} rows {rows} act {act} bias {b is not None}", M.ratio(ya[:rows, :N], want, bound))


def test_mish_against_float64(hip):
    """the grid over [-100, 100] with 0, -0, 20 and its fp32 neighbours; then 4 (2048 * 256 + 3) floats: the capped grid strides once and ends on a tail of 3."""
    g = M.mish_grid()
    x = torch.cat([dev(g), sent((8,))])
    hip.op_cfm_elem(None, kind=0, x=x, n=len(g) // 4)
    xa = host(x)
    want, bound, rho = M.mish_bound(g)
    assert kept(xa[len(g) :])
    print()
    show(f"mish on the grid (rho_mish {rho:.1f} u)", M.ratio(xa[: len(g)], want, bound))
    big = (np.random.default_rng(7).standard_normal(M.MISH_LONG) * 8).astype(F32)
    x = torch.cat([dev(big), sent((8,))])
    hip.op_cfm_elem(None, kind=0, x=x, n=M.MISH_LONG // 4)
    xa = host(x)
    want, bound, rho = M.mish_bound(big)
    assert kept(xa[M.MISH_LONG :])
    show(f"mish over {M.MISH_LONG // 4} float4s (rho_mish {rho:.1f} u)", M.ratio(xa[: M.MISH_LONG], want, bound))


@pytest.mark.parametrize("Mh,rows", M.SWIGLU_CASES)
def test_swiglu_against_float64(hip, Mh, rows):
    """M 4 and 512; M 2048 at 1100 rows exceeds the grid cap of 2048 blocks; gate inputs include +-88 and +-100."""
    a = M.swiglu_case(Mh, rows)
    want, bound, rho = M.swiglu_bound(a, Mh)
    ad, y = dev(a), sent((rows + 1, Mh))
    hip.op_cfm_elem(None, kind=1, C=Mh, n=rows, x=ad, y=y)
    ya = host(y)
    assert kept(ya[rows:]) and same_bits(host(ad), a)
    print()
    show(f"swiglu M {Mh} rows {rows} (rho_silu {rho:.1f} u)", M.ratio(ya[:rows], want, bound))


# ------------------------------------------------------------------------------------------------ sine source
def run_source(hip, case, utts):
    frames, curves = [case["frames"][u] for u in utts], [case["curves"][u] for u in utts]
    R = sum(frames)
    har = sent((R + 1, 32))
    cat = lambda k: dev(np.concatenate([case[k][u] for u in utts] + [np.full(3, 1e3, F32)]))  # noqa: E731
    hip.op_cfm_source(seg_of(frames), seg_of(curves), f0=cat("f0"), ncurve=cat("ncurve"), t=dev(case["t"][list(utts)]), noise=cat("noise"), har=har, ldh=32,
                      merge_w=float(case["w"]))
    ha = host(har)
    assert kept(ha[R:]), "har written past the rows"
    return np.split(ha[:R], np.cumsum(frames)[:-1])


@pytest.mark.parametrize("w_sign", (1.0, -1.0))
def test_source_against_float64(hip, w_sign):
    """frames 1, 7, 255, 256, 257, 1100 from curves of 1, 20, 255, 100, 514, 1100 points in one packed call: columns 1 .. 31 bit for bit (check (i)), column 0
    within the counted bound of the ideal form (ii) and of the restatement's own fp32 angle (iii); the packed call equals each utterance run alone, bit for bit."""
    case = M.source_case(w_sign)
    packed = run_source(hip, case, range(len(case["frames"])))
    print()
    for u, har in enumerate(packed):
        for k, r in M.source_check(case, u, har).items():
            show(f"cfm_source merge_w {float(case['w']):+.1f} utterance {u} ({case['curves'][u]} -> {case['frames'][u]}) {k}", r)
        solo = run_source(hip, case, (u,))[0]
        assert same_bits(solo, har), ("the packed call differs from the utterance alone", u)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_configurations_leave_the_sentinels(hip):
    """Each configuration outside a kernel's domain, and each buffer shorter than a launch would touch, raises with its message before anything is launched."""
    seg = seg_of((3, 2))
    y = sent((6, 2048))
    buf = lambda *s: dev(np.ones(s, F32))  # noqa: E731

    def refused(match, call, **kw):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
        assert kept(host(y)), match

    rms = dict(x=buf(5, 1056), ldx=1056, w=buf(1028), ada=buf(2, 3 * 1028), y=y, ldy=2048)
    refused("C <= 1024", lambda **k: hip.op_rms_adaln(seg, **k), C=1028, **rms)
    refused("ada .* shorter", lambda **k: hip.op_rms_adaln(seg, **k), C=64, **{**rms, "ada": buf(2 * 3 * 64 - 1)})
    refused("x .* outside", lambda **k: hip.op_rms_adaln(seg, **k), C=64, **{**rms, "x": buf(5 * 1056 - 1000)})
    refused("t and ada_prev come together", lambda **k: hip.op_rms_adaln(seg, **k), C=64, t=buf(5, 64), **rms)
    refused("xout .* shorter", lambda **k: hip.op_rms_adaln(seg, **k), C=64, xout=y[0, : 5 * 64 - 1], **rms)
    from stylish_tts_amd.runtime import Segments

    other = Segments((3, 2), torch.device("cuda", 0), dev=dev(np.array([0, 2, 5], np.int32)))  # host offsets 0, 3, 5
    refused("host and device offsets differ", lambda **k: hip.op_rms_adaln(other, **k), C=64, **rms)
    gr = dict(x=y, t=buf(5, 64), ada=buf(2, 192))
    refused("C % 4 == 0", lambda **k: hip.op_cfm_elem(seg, **k), kind=2, C=62, y=y[1], **gr)
    refused("C % 4 == 0", lambda **k: hip.op_cfm_elem(None, **k), kind=1, C=6, n=2, x=buf(2, 12), y=y[0])
    refused("inside their buffers", lambda **k: hip.op_cfm_elem(None, **k), kind=1, C=8, n=2, x=buf(2, 16), y=y[0, :15])
    refused("at least 4 n", lambda **k: hip.op_cfm_elem(None, **k), kind=0, n=3, x=y[0, :11])
    rope = dict(x=y, ldx=2048, col0=0, col1=-1, heads=2)
    refused("d even", lambda **k: hip.op_rope(seg, **k), kind=0, kc=6, d=3, freq=buf(2, 3), **rope)
    refused("d even", lambda **k: hip.op_rope(seg, **k), kind=1, kc=6, d=3, **rope)
    refused("d even", lambda **k: hip.op_rope(seg, **k), kind=1, kc=8, d=16, **rope)
    refused("kc == d", lambda **k: hip.op_rope(seg, **k), kind=0, kc=16, d=8, freq=buf(2, 4), **rope)
    refused("freq", lambda **k: hip.op_rope(seg, **k), kind=0, kc=8, d=8, freq=buf(7), **rope)
    refused("outside ldx", lambda **k: hip.op_rope(seg, **k), kind=1, kc=16, d=8, **{**rope, "col0": 2048 - 31})
    refused("second column block", lambda **k: hip.op_rope(seg, **k), kind=1, kc=16, d=8, **{**rope, "col1": 2048 - 31})
    refused("second column block", lambda **k: hip.op_rope(seg, **k), kind=1, kc=16, d=8, **{**rope, "col1": 16})
    refused("x .* outside", lambda **k: hip.op_rope(seg, **k), kind=1, kc=16, d=8, **{**rope, "x": y.view(-1)[: 4 * 2048 + 31]})
    sm = dict(x=buf(3, 72), ldx=72, w=buf(5, 64), y=y, ldy=2048, n_rows=3, N=5)
    refused("act 0", lambda **k: hip.op_cfm_small(**k), kind=0, K=64, act=2, **sm)
    refused("w .* shorter", lambda **k: hip.op_cfm_small(**k), kind=0, K=64, **{**sm, "w": buf(5 * 64 - 1)})
    refused("x .* outside", lambda **k: hip.op_cfm_small(**k), kind=0, K=80, **{**sm, "w": buf(5, 80)})
    refused("y .* outside", lambda **k: hip.op_cfm_small(**k), kind=0, K=64, **{**sm, "ldy": 4})
    refused("gamma", lambda **k: hip.op_cfm_small(**k), kind=1, **sm)
    refused("ldy >= 2 N", lambda **k: hip.op_cfm_small(**k), kind=2, **{**sm, "ldy": 9})
    frames, curves = seg_of((4, 3)), seg_of((4, 0))
    src = dict(f0=buf(8), ncurve=buf(8), t=buf(2), noise=buf(7), har=y, merge_w=1.0)
    refused("zero points", lambda **k: hip.op_cfm_source(frames, curves, **k), ldh=32, **src)
    refused("32 columns", lambda **k: hip.op_cfm_source(frames, seg_of((4, 4)), **k), ldh=64, **src)
    refused("shorter", lambda **k: hip.op_cfm_source(frames, seg_of((4, 4)), **k), ldh=32, **{**src, "noise": buf(6)})
    refused("shorter", lambda **k: hip.op_cfm_source(frames, seg_of((4, 4)), **k), ldh=32, **{**src, "har": y[0, : 7 * 32 - 1]})
    refused("shorter", lambda **k: hip.op_cfm_source(frames, seg_of((4, 5)), **k), ldh=32, **src)
