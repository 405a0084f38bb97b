"""tests/gemm16_ref.py against independent statements of the same things (no GPU): its rounding functions against torch's conversions bit
for bit, its single-segment convolution against the oracle's conv1d under OPERAND_ROUND, its two-segment form against one conv over the
channel concatenation."""
import numpy as np
import pytest

import gemm16_ref as G

torch = pytest.importorskip("torch")


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _edge_values():
    rng = np.random.default_rng(7)
    vals = [
        rng.standard_normal(4096).astype(np.float32),
        (rng.standard_normal(4096) * 1e-6).astype(np.float32),  # fp16 subnormal results (below 2^-14 = 6.1e-5) and underflow to 0
        (rng.standard_normal(4096) * 3e4).astype(np.float32),   # fp16 results up to and beyond 65504
        rng.integers(0, 1 << 32, 8192, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern (NaNs are dropped below)
    ]
    bits = []
    for e in (0x3F80, 0x4000, 0x0080, 0x7F00, 0x3300, 0x3800, 0x3880, 0x4700, 0x4770):  # 1, 2, tiny, huge, around 2^-25 / 2^-15 / 2^-14 / 2^15 / 61440
        hi = e << 16
        # bf16 ties (low half 0x8000) on an even and an odd kept bit, and their neighbours; the all-ones significand that rounds up into the next binade
        bits += [hi | 0x8000, hi | 0x18000, hi | 0x7FFF, hi | 0x8001, hi | 0x17FFF, hi | 0x18001, hi | 0x7FFFFF, hi | 0x7F8000, hi | 0x7F7FFF]
        # fp16 ties (13 dropped bits = 0x1000) on an even and an odd kept bit, neighbours, and the round-up into the next binade
        bits += [hi | 0x1000, hi | 0x3000, hi | 0x0FFF, hi | 0x1001, hi | 0x2FFF, hi | 0x3001, hi | 0x7FF000, hi | 0x7FEFFF, hi | 0x7FFFFF]
    # fp16 subnormal ties: 2^-25 (tie between 0 and the smallest subnormal -> 0), 3 * 2^-25 (-> 2 * 2^-24), just above / below them; the largest
    # subnormal's round-up into the smallest normal; overflow: 65504, 65519.996, 65520 (tie -> inf), 65536, fp32 max; infinities and zeros
    bits += [0x33000000, 0x33000001, 0x32FFFFFF, 0x33C00000, 0x33C00001, 0x33BFFFFF, 0x387FC000, 0x387FE000, 0x387FF000, 0x387FFFFF, 0x477FE000, 0x477FEFFF,
             0x477FF000, 0x47800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF]
    b = np.asarray(bits, np.uint32)
    vals += [_f32(b), _f32(b | 0x80000000)]
    v = np.concatenate(vals)
    return v[~np.isnan(v)]


@pytest.mark.parametrize("mode,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_rounding_equals_torch_bit_for_bit(mode, dtype):
    v = _edge_values()
    want = torch.from_numpy(v).to(dtype).view(torch.int16).numpy().view(np.uint16)
    got = G.round_bits(v, mode)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(v[i : i + 1].view(np.uint32)[0])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    back = torch.from_numpy(want.view(np.int16)).view(dtype).to(torch.float32).numpy()
    assert np.array_equal(G.round_to(v, mode).view(np.uint32), back.view(np.uint32))
    # the edge cases are really in the set: ties, a carry into the next binade, and for fp16 subnormals and overflow
    if mode == "f16":
        assert ((want & 0x7C00) == 0).sum() > 100 and ((want & 0x7FFF) == 0x7C00).sum() > 100
        assert G.f16_bits(_f32([0x33000000]))[0] == 0 and G.f16_bits(_f32([0x33C00000]))[0] == 2 and G.f16_bits(_f32([0x477FF000]))[0] == 0x7C00
        assert G.f16_bits(_f32([0x387FF000]))[0] == 0x0400  # the largest subnormal's tie rounds up into the smallest normal
    else:
        assert G.bf16_bits(_f32([0x3F808000]))[0] == 0x3F80 and G.bf16_bits(_f32([0x3F818000]))[0] == 0x3F82 and G.bf16_bits(_f32([0x3FFFFFFF]))[0] == 0x4000


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,k,dil,lengths", [(70, 33, 3, 1, [17, 1, 40]), (24, 20, 7, 3, [5, 30]), (64, 16, 1, 1, [9])])
def test_single_segment_equals_the_rounded_oracle(mode, cin, cout, k, dil, lengths):
    from oracle import stylish_oracle as O
    from stylish_tts_amd import synth

    w = (synth.normal(f"g16ref.w.{cin}.{k}", (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    b = synth.normal(f"g16ref.b.{cout}", (cout,))
    x = synth.normal(f"g16ref.x.{cin}", (sum(lengths), cin + 3))  # (three columns beyond cin: ignored)
    got = G.conv_epi64([(x, w, dil)], lengths, b, mode)
    O.OPERAND_ROUND = mode
    try:
        lo = 0
        for L in lengths:
            ref = O.conv1d(np.ascontiguousarray(x[lo : lo + L, :cin].T[None]), w, b, padding=(k - 1) // 2 * dil, dilation=dil)[0].T
            assert np.abs(got[lo : lo + L] - ref).max() <= 1e-6 * np.abs(ref).max()
            lo += L
    finally:
        O.OPERAND_ROUND = None


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_two_segments_equal_one_conv_over_the_concatenation(mode):
    from stylish_tts_amd import synth

    lengths, c0, c1, cout, k = [12, 1, 33], 40, 22, 24, 3
    w = (synth.normal("g16ref.w2", (cout, c0 + c1, k)) / np.sqrt((c0 + c1) * k)).astype(np.float32)
    b = synth.normal("g16ref.b2", (cout,))
    r = synth.normal("g16ref.r2", (sum(lengths), cout))
    x = synth.normal("g16ref.x2", (sum(lengths), c0 + c1))
    x0, x1 = np.ascontiguousarray(x[:, :c0]), np.ascontiguousarray(x[:, c0:])
    kw = dict(act=G.ACT_LRELU, alpha=0.5, r=r)
    one = G.conv_epi64([(x, w, 1)], lengths, b, mode, **kw)
    two = G.conv_epi64([(x0, np.ascontiguousarray(w[:, :c0]), 1), (x1, np.ascontiguousarray(w[:, c0:]), 1)], lengths, b, mode, **kw)
    assert np.abs(one - two).max() <= 1e-13 * np.abs(one).max()
    # and the segments really carry their own tap count: a k = 1 second segment equals the middle tap of a k = 3 one whose outer taps are zero
    wz = w.copy()
    wz[:, c0:, 0] = wz[:, c0:, 2] = 0
    mixed = G.conv_epi64([(x0, np.ascontiguousarray(w[:, :c0]), 1), (x1, np.ascontiguousarray(w[:, c0:, 1:2]), 1)], lengths, b, mode, **kw)
    assert np.abs(mixed - G.conv_epi64([(x, wz, 1)], lengths, b, mode, **kw)).max() <= 1e-13 * np.abs(one).max()
