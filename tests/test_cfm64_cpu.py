"""tests/cfm64.py without a GPU: the float64 restatements are held to torch's own float64 functions; the source restatement (i) to torch's fp32 CPU ops bit for
bit; numpy-fp32 emulations of each kernel's expression (one fixed order each) meet every bound on every case of tests/test_hip_cfm_kernels.py - the bounds are not
tighter than fp32 arithmetic allows -; and emulated defects exceed them - the cases have teeth.

Measured here (-s): the ULP figures cfm64's bounds are built from, per family the worst emulation error / bound, and per defect the factor by which it misses.
The source's wrap defects are integer shifts of the phase, which cancel in the ideal form (ii); they are held to the exact check (flags and angle bit patterns,
allowed difference 0) and to check (iii), column 0 against the restatement's own fp32 angle:
  - a wrap flag computed for frame 0 (the `i > 0` guard dropped, here in the vectorised form `tmp - roll(tmp, 1) < 0`) shifts the whole phase by -1: one flag and
    every angle bit pattern differ, column 0 is 2.9 of (iii)'s bound.  In cfm_source_kernel itself the guard is redundant for F0 >= 0: the first frame compares
    fmod(rad) >= 0 with prev = 0, which is never negative;
  - ONE missed wrap moves fl(c2) from [0, 1) to [1, 2): half an ulp coarser.  A kernel that restarts `prev` at 0 in every thread's chunk misses EVERY wrap of the
    constant-F0 utterance (one per chunk, 219 of them): c2 grows to 219, 1095 of 1100 angles differ and column 0 misses (iii)'s bound 386 times - the emulated defect.
Mish without the softplus threshold is harmless in the form v tanh(log1p(exp v)) (exp overflows to inf, tanh(inf) = 1, the result is v): the emulated defect is the
tanh-free form v (n^2 - 1) / (n^2 + 1), n = 1 + exp v, whose square overflows from v = 44 on: inf / inf.
"""
import numpy as np
import pytest

import cfm64 as M

torch = pytest.importorskip("torch")
TF = torch.nn.functional
F32, F64, U = np.float32, np.float64, M.U


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, F64))


def sum32(a, axis=None):
    return np.sum(a, axis=axis, dtype=F32, keepdims=axis is not None)


# ------------------------------------------------------------------------------------------------ fp32 emulations (defect: None or a name)
def emu_gated(h, t, gate):
    return (h + (t * (gate + F32(1))).astype(F32)).astype(F32)


def emu_rms_adaln(case, mode, defect=None):
    C, L, R = case["C"], case["lengths"], case["R"]
    x, w = case["x"][:R, :C], case["w"]
    a = np.repeat(case["ada"], L, axis=0)
    ap = np.repeat(case["ada_prev"], L, axis=0)
    xp = x
    if mode in ("fused", "fused_xout"):
        xp = emu_gated(x, case["t"], (a if defect == "gate_next_table" else ap)[:, 2 * C :])
    q = sum32(xp * xp, 1)
    inv = F32(1) / np.sqrt(q / F32(C) + F32(1e-6))
    sc = a[:, :C] if defect == "no_plus_one" else a[:, :C] + F32(1)
    return (((xp * inv).astype(F32) * w).astype(F32) * sc + a[:, C : 2 * C]).astype(F32), xp


def emu_rope(case, d, freq=None, defect=None):
    x, R, heads, kc, kind, L = case["x"], case["R"], case["heads"], case["kc"], case["kind"], case["lengths"]
    out = np.array(x)
    half = d // 2
    if kind == 0:
        pos = np.concatenate([M.linspace32(n)[0] for n in L if n > 0])
        ang = (pos[:, None, None] * freq[None]).astype(F32)
    else:
        theta = (F32(1) / np.power(F32(10000), (2 * np.arange(half)).astype(F32) / F32(d))).astype(F32)
        p = np.concatenate([np.arange(n) for n in L]).astype(F32)
        ang = np.broadcast_to((p[:, None] * theta[None]).astype(F32)[:, None], (R, heads, half))
    cs, sn = np.cos(ang), np.sin(ang)
    if defect == "sign":
        sn = -sn
    interleaved = (kind == 0) != (defect == "pairing")
    for col in (case["col0"], case["col1"]):
        if col < 0:
            continue
        blk = out[:R, col : col + heads * kc].reshape(R, heads, kc)
        a, b = (blk[:, :, 0:d:2], blk[:, :, 1:d:2]) if interleaved else (blk[:, :, :half], blk[:, :, half:d])
        o0, o1 = ((a * cs).astype(F32) - (b * sn).astype(F32)).astype(F32), ((b * cs).astype(F32) + (a * sn).astype(F32)).astype(F32)
        if interleaved:
            blk[:, :, 0:d:2], blk[:, :, 1:d:2] = o0, o1
        else:
            blk[:, :, :half], blk[:, :, half:d] = o0, o1
        out[:R, col : col + heads * kc] = blk.reshape(R, heads * kc)
    return out


def emu_time(t, f):
    a = ((F32(1000) * t)[:, None] * f[None]).astype(F32)
    return np.concatenate([np.cos(a), np.sin(a)], 1).astype(F32)


def wave_sum32(a):
    """small_layernorm_kernel's order: lane l adds elements l, l + 64, ... in turn, then the xor butterfly over the 64 lanes.  a [rows, C] -> [rows, 1]."""
    rows, C = a.shape
    p = np.zeros((rows, (C + 63) // 64 * 64), F32)
    p[:, :C] = a
    p = p.reshape(rows, -1, 64)
    s = p[:, 0].copy()
    for k in range(1, p.shape[1]):
        s = s + p[:, k]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    return s[:, :1]


def emu_layernorm(x, g, b, defect=None):
    C = F32(x.shape[1])
    mean = wave_sum32(x) / C
    if defect == "one_pass":
        var = np.maximum(wave_sum32(x * x) / C - mean * mean, F32(0))
    else:
        d = x - mean
        var = wave_sum32(d * d) / C
    inv = F32(1) / np.sqrt(var + F32(1e-5))
    return ((((x - mean) * inv).astype(F32) * g).astype(F32) + b).astype(F32)


def emu_linear(x, w, b, act, defect=None):
    K = x.shape[1]
    if defect == "tail_lanes":
        K = K // 64 * 64
    v = sum32(x[:, None, :K] * w[None, :, :K], 2)[:, :, 0]
    if b is not None:
        v = (v + b).astype(F32)
    return M.mish32(v) if act else v


def mish32_no_threshold(v):
    with np.errstate(over="ignore", invalid="ignore"):
        n = F32(1) + np.exp(np.asarray(v, F32))
        n2 = n * n
        return (v * ((n2 - F32(1)) / (n2 + F32(1)))).astype(F32)


def emu_swiglu(a, Mh, defect=None):
    g, b = (a[:, Mh:], a[:, :Mh]) if defect == "halves" else (a[:, :Mh], a[:, Mh:])
    return (M.silu32(g) * b).astype(F32)


def emu_source(f0c, n, noise, w, defect=None):
    """cfm_source_kernel's contract in numpy for one utterance: 256 chunks of `per` frames; -> column 0, flags, angle (fp32)."""
    L = len(f0c)
    idx = M.nearest_idx(n, L)
    if defect == "rint" and L != n:
        idx = np.minimum(np.rint((np.arange(n).astype(F32) * (F32(L) / F32(n))).astype(F32)).astype(np.int64), L - 1)
    f = f0c[idx]
    rad = np.fmod((f / M.SR32).astype(F32), F32(1))
    c1 = np.cumsum(rad.astype(F64))
    tmp = np.fmod(c1.astype(F32), F32(1))
    prev = np.concatenate([[F32(0)], tmp[:-1]]).astype(F32)
    if defect == "chunk_prev":  # every thread's chunk restarts at prev = 0
        per = (n + 255) // 256
        prev[::per] = 0
    flag = (tmp - prev) < 0
    if defect == "no_guard":
        flag = (tmp - np.roll(tmp, 1)) < 0
    else:
        flag[0] = False
    c2 = np.cumsum((rad + np.where(flag, F32(-1), F32(0))).astype(F32).astype(F64))
    ang = ((c2.astype(F32) * F32(2)).astype(F32) * M.PI32).astype(F32)
    uv, namp = M.noise_amp32(f)
    sw = (((np.sin(ang) * M.AMP32).astype(F32) * uv).astype(F32) + (namp * noise).astype(F32)).astype(F32)
    return np.tanh((sw * F32(w)).astype(F32)).astype(F32), flag, ang, idx


# ------------------------------------------------------------------------------------------------ restatements against torch's float64
def close(a, b, tol=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


def test_restatements_agree_with_torch_float64():
    for C in M.RMS_C:
        case = M.rms_case(C)
        L, R = case["lengths"], case["R"]
        a, ap = M.rows_of(case["ada"], L), M.rows_of(case["ada_prev"], L)
        for fused in (False, True):
            b = M.rms_adaln_bound(case["x"][:R, :C], case["w"], a[:, :C], a[:, C : 2 * C], case["t"] if fused else None, ap[:, 2 * C :] if fused else None)
            x = t64(case["x"][:R, :C])
            if fused:
                x = x + t64(case["t"]) * (t64(ap[:, 2 * C :]) + 1)
            y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + M.EPS_RMS) * t64(case["w"])
            if hasattr(TF, "rms_norm"):
                assert close(TF.rms_norm(x, (C,), t64(case["w"]), M.EPS_RMS).numpy(), y.numpy())
            y = y * (t64(a[:, :C]) + 1) + t64(a[:, C : 2 * C])
            assert close(b["y"], y.numpy()) and close(b["xp"], x.numpy()), (C, fused)
    v = np.linspace(-100, 100, 2001)
    assert close(M.mish64(v), TF.mish(t64(v)).numpy()) and close(M.silu64(v), TF.silu(t64(v)).numpy())
    a = M.swiglu_case(4, 5)
    assert close(M.swiglu64(a, 4), (TF.silu(t64(a[:, :4])) * t64(a[:, 4:])).numpy())
    for C in M.LN_C:
        c = M.layernorm_case(C)
        y, _ = M.layernorm_small_bound(c["x"][:, :C], c["g"], c["b"])
        assert close(y, TF.layer_norm(t64(c["x"][:, :C]), (C,), t64(c["g"]), t64(c["b"]), M.EPS_LN).numpy(), 1e-9)
    c = M.linear_case(5, 100, 3)
    y, _, _ = M.linear_bound(c["x"][:, :100], c["w"], c["b"], 1)
    assert close(y, TF.mish(TF.linear(t64(c["x"][:, :100]), t64(c["w"]), t64(c["b"]))).numpy())
    for n in (1, 2, 3, 4, 37, 800, 1100):
        assert np.array_equal(M.linspace32(n)[0].view(np.uint32), torch.linspace(-1, 1, n, dtype=torch.float32).numpy().view(np.uint32)), n
    for n, L in list(zip(M.SRC_FRAMES, M.SRC_CURVES)) + [(800, 799), (799, 800), (3, 1000), (1000, 3), (4000, 1371)]:
        want = TF.interpolate(torch.arange(L, dtype=torch.float32)[None, None], n).numpy()[0, 0].astype(np.int64)
        assert np.array_equal(M.nearest_idx(n, L), want), (n, L)


def test_rotary_restatements_agree_with_torch_float64():
    """axial: interleaved pairs as complex numbers turned by e^{i pos freq}; sequence: x cos + neg_half(x) sin on the first d features - with the restatement's fp32 angles."""
    heads, d, L = 2, 8, (1, 2, 3, 37)
    case = M.rope_case(0, heads, d, L, True)
    freq = M.axial_freq(heads, d)
    want, _ = M.rope64(case["x"], L, 0, 0, heads, d, d, freq)
    ang, _ = M.axial_angles(L, freq)
    z = torch.view_as_complex(t64(case["x"][: case["R"], : heads * d]).reshape(-1, heads, d // 2, 2).contiguous()) * torch.polar(torch.ones(ang.shape, dtype=torch.float64), t64(ang))
    assert close(want, torch.view_as_real(z).reshape(-1, heads, d).numpy())
    heads, kc, d, L = 2, 40, 20, (1, 33)
    case = M.rope_case(1, heads, kc, L, False)
    want, _ = M.rope64(case["x"], L, 1, 16, heads, kc, d)
    ang, _, _ = M.seq_angles(L, d)
    x = t64(case["x"][: case["R"], 16 : 16 + heads * kc]).reshape(-1, heads, kc)[:, :, :d]
    cs, sn = torch.cat([t64(ang).cos()] * 2, -1)[:, None], torch.cat([t64(ang).sin()] * 2, -1)[:, None]
    neg_half = torch.cat([-x[..., d // 2 :], x[..., : d // 2]], -1)
    assert close(want, (x * cs + neg_half * sn).numpy())
    # theta: the correctly rounded 10000^(-2j/d)
    th = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    assert np.abs((M.seq_angles((2,), d)[0][1] - th.numpy()).astype(F64)).max() <= 4 * U


def torch_source(f0r):
    """SineGenerator._f02sine's fp32 CPU ops for one component (cfm_mel_decoder.py:58-81, the initial phase of the fundamental is 0): flags and the sine's argument."""
    f0 = torch.from_numpy(np.asarray(f0r, F32))[None, :, None]
    rad = (f0 / 24000) % 1
    tmp = torch.cumsum(rad, 1) % 1
    idx = (tmp[:, 1:, :] - tmp[:, :-1, :]) < 0
    shift = torch.zeros_like(rad)
    shift[:, 1:, :] = idx * -1.0
    ang = torch.cumsum(rad + shift, dim=1) * 2 * np.pi
    return idx[0, :, 0].numpy(), ang[0, :, 0].numpy()


@pytest.mark.parametrize("n", (1, 7, 255, 256, 257, 1100, 4000))
def test_source_restatement_matches_torch_cpu_bit_for_bit(n):
    from stylish_tts_amd import synth

    worst, wraps = 0.0, 0
    for k, f0 in enumerate((synth.pitch_curve(f"cfm64.cpu.{n}", 1, n, seed=1)[0], np.full(n, M.SRC_WRAP_HZ, F32), synth.pitch_curve(f"cfm64.cpu.b.{n}", 1, n, seed=2, unvoiced=0.0)[0] * 3)):
        e = M.source_exact(f0)
        flag, ang = torch_source(f0)
        nf, na = int((e["flag"][1:] != flag).sum()), int((e["ang"].view(np.uint32) != ang.view(np.uint32)).sum())
        assert nf == 0 and na == 0, (n, k, nf, na)
        assert np.abs(e["c2"]).max() <= 1.0, "the bound's |c2| <= 1"
        c = np.cumsum(e["rad"].astype(F64))
        err = np.abs(np.sin(e["ang"].astype(F64)) - np.sin(2 * np.pi * (c - np.floor(c)))) / U
        worst, wraps = max(worst, float(err.max())), max(wraps, int(e["flag"].sum()))
        assert (err <= M.source_angle_bound_u(e["flag"])).all(), "the restatement's own sine within the counted angle bound 15.5 + pi W"
    print(f"\n[cfm64] source restatement at {n} frames: 0 differing flags, 0 differing angle bit patterns against torch; its own sine is up to {worst:.1f} u from the ideal (up to {wraps} wraps)")


# ------------------------------------------------------------------------------------------------ emulations meet the bounds, defects exceed them
def report(what, r, defect=False):
    print(f"[cfm64] {what}: {'defect misses the bound by a factor of' if defect else 'emulation error / bound'} {r:.3g}")
    assert (r > 1.0) if defect else (r < 1.0), (what, r)


def test_measured_ulp_figures():
    a = np.linspace(0, 1000, 200001).astype(F32)
    ec, es = M.e_cos_sin(a)
    g = np.random.default_rng(1).standard_normal(200000) * 8
    _, _, rm = M.mish_bound(g.astype(F32))
    _, _, rs = M.swiglu_bound(np.stack([g, g], 1).astype(F32), 1)
    rq, rd = M.rho_sqrt_div(np.abs(g) + 1e-3)
    print(f"\n[cfm64] numpy fp32 against float64, times 4: cos / sin on [0, 1000] {ec / U:.2f} / {es / U:.2f} u absolute; Mish on N(0, 8^2) {rm:.1f} u, SiLU {rs:.1f} u, sqrt {rq:.1f} u, 1 / x {rd:.1f} u relative")
    assert 0 < ec < 8 * U and 0 < es < 8 * U and 0 < rm < 64 and 0 < rs < 32


@pytest.mark.parametrize("C", M.RMS_C)
def test_rms_adaln_emulation_and_defects(C):
    case = M.rms_case(C)
    print()
    for mode in M.RMS_MODES:
        y, xp = emu_rms_adaln(case, mode)
        r = M.rms_check(case, mode, y, xp if mode == "fused_xout" else None)
        for k, v in r.items():
            report(f"rms_adaln C {C} {mode} {k}", v)
    report(f"rms_adaln C {C}: gate read from the next branch's table", M.rms_check(case, "fused", emu_rms_adaln(case, "fused", "gate_next_table")[0])["y"], True)
    y, xp = emu_rms_adaln(case, "fused_xout", "gate_next_table")
    report(f"rms_adaln C {C}: the same, on Xout", M.rms_check(case, "fused_xout", y, xp)["xout"], True)
    report(f"rms_adaln C {C}: (scale + 1) without the + 1", M.rms_check(case, "plain", emu_rms_adaln(case, "plain", "no_plus_one")[0])["y"], True)


def test_gated_residual_emulation():
    print()
    for C, L in M.GATED_CASES:
        case = M.gated_case(C, L)
        R = case["R"]
        gate = np.repeat(case["ada"], L, axis=0)[:, 2 * C :]
        report(f"gated_residual C {C}", M.gated_check(case, emu_gated(case["h"][:R], case["t"][:R], gate)))
        report(f"gated_residual C {C}: gate read from the scale third", M.gated_check(case, emu_gated(case["h"][:R], case["t"][:R], np.repeat(case["ada"], L, axis=0)[:, :C])), True)


def test_rotary_emulations_and_defects():
    print()
    for heads, d in M.AXIAL_SHAPES:
        freq = M.axial_freq(heads, d)
        for two in (False, True):
            case = M.rope_case(0, heads, d, M.AXIAL_LENGTHS, two)
            report(f"axial_rope heads {heads} d {d} col1 {case['col1']}", M.rope_check(case, d, emu_rope(case, d, freq), freq))
        report(f"axial_rope heads {heads} d {d}: half-split pairs", M.rope_check(case, d, emu_rope(case, d, freq, "pairing"), freq), True)
        report(f"axial_rope heads {heads} d {d}: rotation sign flipped", M.rope_check(case, d, emu_rope(case, d, freq, "sign"), freq), True)
    for heads, kc, d in M.SEQ_SHAPES:
        for two in (False, True):
            case = M.rope_case(1, heads, kc, M.SEQ_LENGTHS, two)
            report(f"rope heads {heads} kc {kc} d {d} col1 {case['col1']}", M.rope_check(case, d, emu_rope(case, d)))
        report(f"rope heads {heads} kc {kc} d {d}: interleaved pairs", M.rope_check(case, d, emu_rope(case, d, defect="pairing")), True)
        report(f"rope heads {heads} kc {kc} d {d}: rotation sign flipped", M.rope_check(case, d, emu_rope(case, d, defect="sign")), True)


def test_small_kernel_emulations_and_defects():
    print()
    for half in M.TIME_HALF:
        f = M.time_freqs(half)
        t = np.array(M.TIME_T, F32)
        want, bound = M.time_embed_bound(t, f)
        report(f"time embedding half {half}", M.ratio(emu_time(t, f), want, bound))
    for C in M.LN_C:
        c = M.layernorm_case(C)
        y, bound = M.layernorm_small_bound(c["x"][:, :C], c["g"], c["b"])
        report(f"small_layernorm C {C}", M.ratio(emu_layernorm(c["x"][:, :C], c["g"], c["b"]), y, bound))
        report(f"small_layernorm C {C}: one-pass variance, the mean-heavy row", M.ratio(emu_layernorm(c["x"][1:2, :C], c["g"], c["b"], "one_pass"), y[1:2], bound[1:2]), True)
    for N, K in M.LINEAR_NK:
        for rows in M.LINEAR_ROWS:
            c = M.linear_case(N, K, rows)
            for act in (0, 1):
                for b in (None, c["b"]):
                    y, bound, rho = M.linear_bound(c["x"][:, :K], c["w"], b, act)
                    report(f"small_linear N {N} K {K} rows {rows} act {act} bias {b is not None} (rho_mish {rho:.1f} u)", M.ratio(emu_linear(c["x"][:, :K], c["w"], b, act), y, bound))
        if K % 64:
            y, bound, _ = M.linear_bound(c["x"][:, :K], c["w"], c["b"], 0)
            report(f"small_linear N {N} K {K}: tail lanes dropped", M.ratio(emu_linear(c["x"][:, :K], c["w"], c["b"], 0, "tail_lanes"), y, bound), True)


def test_mish_and_swiglu_emulations_and_defects():
    print()
    x = M.mish_grid()
    want, bound, rho = M.mish_bound(x)
    report(f"mish on the grid (rho_mish {rho:.1f} u)", M.ratio(M.mish32(x), want, bound))
    hi = np.array([88.5, 95.0, 100.0], F32)
    want, bound, _ = M.mish_bound(hi)
    report("mish without the softplus threshold (tanh-free form) above 88", M.ratio(mish32_no_threshold(hi), want, bound), True)
    for Mh, rows in M.SWIGLU_CASES[:2]:
        a = M.swiglu_case(Mh, rows)
        want, bound, rho = M.swiglu_bound(a, Mh)
        report(f"swiglu M {Mh} (rho_silu {rho:.1f} u)", M.ratio(emu_swiglu(a, Mh), want, bound))
        report(f"swiglu M {Mh}: halves swapped", M.ratio(emu_swiglu(a, Mh, "halves"), want, bound), True)


def test_source_emulation_and_defects():
    print()
    for sign in (1.0, -1.0):
        case = M.source_case(sign)
        for u, n in enumerate(case["frames"]):
            col0, flag, ang, idx = emu_source(case["f0"][u], n, case["noise"][u], case["w"], None)
            e = M.source_exact(case["f0"][u][idx])
            assert np.array_equal(flag, e["flag"]) and np.array_equal(ang.view(np.uint32), e["ang"].view(np.uint32)), u
            har = np.zeros((n, 32), F32)
            har[:, 0], har[:, 1], har[:, 2] = col0, case["ncurve"][u][idx], case["t"][u]
            for k, v in M.source_check(case, u, har).items():
                report(f"cfm_source merge_w {float(case['w']):+.1f} utterance {u} ({case['curves'][u]} -> {n}) {k}", v)
    case = M.source_case()
    # the wrap of the constant-F0 utterance falls on the first frame of a thread's chunk, every time
    e = M.source_exact(case["f0"][5])
    assert np.array_equal(np.flatnonzero(e["flag"]), 5 * np.arange(1, 220))
    u = 3  # 100 -> 256: rint and floor pick different points
    col0, _, _, idx = emu_source(case["f0"][u], 256, case["noise"][u], case["w"], "rint")
    n_idx = int((idx != M.nearest_idx(256, 100)).sum())
    har = np.zeros((256, 32), F32)
    har[:, 0], har[:, 1], har[:, 2] = col0, case["ncurve"][u][idx], case["t"][u]
    with pytest.raises(AssertionError, match="nearest rule"):
        M.source_check(case, u, har)
    want, bound, _ = M.source_ideal_bound(case["f0"][u][M.nearest_idx(256, 100)], case["noise"][u], case["w"])
    print(f"[cfm64] nearest index by rint: {n_idx} of 256 indices differ, column 1 fails the exact check")
    report("nearest index by rint: column 0", M.ratio(col0, want, bound), True)
    # the exact check: flags and angle bit patterns (allowed difference: 0)
    for u, defect in ((3, "no_guard"), (5, "chunk_prev")):
        n = case["frames"][u]
        col0, flag, ang, idx = emu_source(case["f0"][u], n, case["noise"][u], case["w"], defect)
        e = M.source_exact(case["f0"][u][idx])
        nf, na = int((flag != e["flag"]).sum()), int((ang.view(np.uint32) != e["ang"].view(np.uint32)).sum())
        print(f"[cfm64] source defect {defect}: {nf} differing wrap flags, {na} differing angle bit patterns of {n} (allowed: 0)")
        assert nf > 0 and na > 0
        want, bound = M.source_exact_bound(case["f0"][u][idx], case["noise"][u], case["w"])
        r = M.ratio(col0, want, bound)
        if defect == "chunk_prev":
            report("a wrap missed at every chunk boundary: column 0 against check (iii)", r, True)
        else:
            print(f"[cfm64] source defect {defect}: column 0 is {r:.3g} of check (iii)'s bound (an integer shift of a phase below 1: no error bound can see it)")
