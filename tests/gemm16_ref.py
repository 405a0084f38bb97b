"""Float64 restatement of the store contraction of the 16-bit operand modes (csrc/gemm16.hip.h conv_gemm16_kernel and the 16-bit-row
tiles of csrc/gemm.hip.h conv_gemm_f32) with its epilogue.  Test infrastructure: fp32 inputs in; activations and weights are rounded to the
mode (round-to-nearest-even, the only rounding the kernels' operands see), everything after that is float64:

    v = (act(sum_i conv1d(x_i, w_i) + bias) + R) * alpha

over one or more K segments, each with its own tap count and dilation, the utterance edges being the convs' zero padding.  Layout is the
engine's: time-major rows [rows, C] packed utterance after utterance (`lengths` rows each).

The rounding functions are written out on the bit patterns (no numpy / torch conversion), so that they are an independent statement of
what "rounded to the mode" means; tests/test_gemm16_ref_cpu.py holds them to torch's conversions bit for bit.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_LRELU = range(5)  # csrc/gemm.hip.h: enum Act


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)


def bf16_bits(a):
    """fp32 -> bf16 bit patterns (uint16), round to nearest, ties to even; NaN -> a quiet NaN of the same sign."""
    u = _u32(a)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def f16_bits(a):
    """fp32 -> IEEE binary16 bit patterns (uint16), round to nearest, ties to even: subnormal results below 2^-14, overflow to inf from 65520."""
    u = _u32(a)
    sign = (u >> 16) & 0x8000
    mag = u & 0x7FFFFFFF
    e = (mag >> 23).astype(np.int64) - 127 + 15  # binary16 biased exponent of a normal result
    mant = mag & 0x7FFFFF
    # normal results: 13 bits are dropped; the increment carries into the exponent by itself (up to 0x7C00 = inf)
    hn = (np.clip(e, 1, 31).astype(np.uint64) << 10) | (mant >> 13)
    rem = mant & 0x1FFF
    hn = hn + ((rem > 0x1000) | ((rem == 0x1000) & ((hn & 1) == 1)))
    hn = np.where(e >= 31, 0x7C00, hn)
    # subnormal results (e <= 0): the significand with its hidden bit, shifted right by 14 - e places
    full = mant | 0x800000
    sh = np.clip(14 - e, 14, 40).astype(np.uint64)
    hs = full >> sh
    rs = full & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    hs = hs + ((rs > half) | ((rs == half) & ((hs & 1) == 1)))
    hs = np.where(mag == 0, 0, hs)
    h = np.where(e >= 1, hn, hs)
    h = np.where(mag > 0x7F800000, 0x7E00, h)  # NaN
    h = np.where(mag == 0x7F800000, 0x7C00, h)
    return (sign | h).astype(np.uint16)


def bits_to_f32(bits, mode):
    bits = np.ascontiguousarray(bits, np.uint16)
    if mode == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    assert mode == "f16", mode
    return bits.view(np.float16).astype(np.float32)  # (binary16 -> binary32 is exact)


def round_bits(a, mode):
    return bf16_bits(a) if mode == "bf16" else f16_bits(a)


def round_to(a, mode):
    """fp32 -> the nearest value of the mode ("bf16" / "f16"), as fp32."""
    return bits_to_f32(round_bits(a, mode), mode).reshape(np.shape(a))


def act64(v, act):
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_LRELU:
        return np.where(v >= 0.0, v, 0.2 * v)
    assert act == ACT_NONE, act  # (GELU: no 16-bit launch of the engine uses it)
    return v


def conv_epi64(segments, lengths, bias, mode, act=ACT_NONE, alpha=1.0, r=None):
    """segments: [(x [rows, >= cin] fp32, w [cout, cin, k] fp32, dil)]; bias [cout] or None; r [rows, cout] or None -> float64 [rows, cout]."""
    cout = segments[0][1].shape[0]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    y = np.zeros((int(off[-1]), cout), F64)
    for x, w, dil in segments:
        cin, k = w.shape[1], w.shape[2]
        assert k % 2 == 1 and w.shape[0] == cout
        xr = round_to(np.asarray(x)[:, :cin], mode).astype(F64)
        wr = round_to(w, mode).astype(F64)
        for u, L in enumerate(lengths):
            lo = int(off[u])
            for t in range(k):
                sh = (t - (k - 1) // 2) * dil  # output row j reads input row j + sh of the same utterance, zero outside it
                j0, j1 = max(0, -sh), min(L, L - sh)
                if j1 > j0:
                    y[lo + j0 : lo + j1] += xr[lo + j0 + sh : lo + j1 + sh] @ wr[:, :, t].T
    if bias is not None:
        y += np.asarray(bias, F64)
    y = act64(y, act)
    if r is not None:
        y = y + np.asarray(r, F64)
    return y * F64(np.float32(alpha))  # (the kernels take alpha as an fp32 argument)
