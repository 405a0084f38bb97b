"""tests/block64.py on the CPU: the float64 restatement of the AdaptiveDecoderBlock against the oracle, the float32 F(6,3) model, and the bounds of
tests/test_hip_block_forms.py tried on numpy models of the engine's forms AT THAT TEST'S SHAPES: the models pass, and every mutant of MUTANTS (one wrong
formula, rounding point or statistics merge each) is rejected.  A mutant that survived would mean a shape or a bound lets that defect through."""
from functools import lru_cache

import numpy as np
import pytest

import block64 as B
from norm64 import F32, F64, U

LENS = tuple(B.LENGTHS)
MODES = (None, "bf16", "f16")


@lru_cache(maxsize=None)
def case(name, lengths=LENS):
    """weights, inputs, the float64 results per rounding mode and the bars of one block on one batch."""
    w, p = B.weights(name)
    wt = B.block_weights(w, p)
    x, style = B.inputs(name, lengths, B.WIDTHS[name][0])
    want = {m: B.block64(x, lengths, style, wt, m) for m in MODES}
    ref = {m: B.oracle32(x, lengths, style, w, p, m) for m in MODES}
    bars = {m: B.bar(ref[m], want[m], lengths) if m is None else B.seeded_bars16(name, tuple(lengths), m) for m in MODES}
    return dict(w=w, p=p, wt=wt, x=x, style=style, want=want, ref=ref, bar=bars, lengths=lengths)


def wino_bar(c):
    y, _, _ = B.model32(c["x"], c["lengths"], c["style"], c["wt"], conv="wino", chunk=24)
    return B.bar(y, c["want"][None], c["lengths"])


@lru_cache(maxsize=None)
def pair():
    """encode -> decode on the batch: block B's input is [model A's y | constant columns]; -> (case-like dict of B, const_from)."""
    a, cout = case("enc"), B.WIDTHS["enc"][1]
    w, p = B.weights("dec")
    wt = B.block_weights(w, p)
    cst, _ = B.inputs("cst", LENS, B.WIDTHS["dec"][0] - cout)
    ya, _, _ = B.model32(a["x"], LENS, a["style"], a["wt"], chunk=24)
    x = np.concatenate([ya, cst], 1).astype(F32)
    want = {None: B.block64(x, LENS, a["style"], wt)}
    return dict(w=w, p=p, wt=wt, x=x, style=a["style"], want=want, bar={None: B.bar(B.oracle32(x, LENS, a["style"], w, p), want[None], LENS)}, lengths=LENS), cout


def worst(y, c, mode):
    return float(B.utt_errors(y, c["want"][mode], c["lengths"]).max())


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", sorted(B.WIDTHS))
def test_block64_agrees_with_the_oracle_to_fp32_noise(name):
    """fp32 noise of a K-term fp32 accumulation: sqrt(K) u for random signs, K = 3 max(cin, cout) terms per output; a factor 8 for the two convs, the shortcut
    and the max over the batch.  (2e-5 at 578 channels; a wrong formula is off by 1e-2 or more.)"""
    c = case(name)
    e = worst(c["ref"][None], c, None)
    print(f"{name}: oracle fp32 vs block64 {e:.2e}")
    assert e <= 8 * np.sqrt(3 * max(B.WIDTHS[name])) * U


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(B.WIDTHS))
def test_block64_agrees_with_the_oracle_under_operand_round(name, mode):
    """Same rounding points: what is left is fp32 noise plus the rare operand that rounds the other way (a 16-bit ulp of one activation or weight out of the
    ~1 700 terms of an output; an fp32 difference of a few ulps flips about one operand in 10^4).  A rounding point that was missing or misplaced would shift EVERY
    term by up to half a 16-bit ulp, which is what separates block64 with and without round_to (`d`): the two references must agree several times better than that."""
    c = case(name)
    e, d = worst(c["ref"][mode], c, mode), worst(c["want"][None], c, mode)
    print(f"{name} {mode}: oracle vs block64 {e:.2e}; unrounded block64 is {d:.2e} away")
    assert e <= 0.25 * d
    assert d > 2.0 ** (-12 if mode == "bf16" else -15)  # (the rounding is visible at all: 1 / 16 of the mode's unit roundoff)


def test_wino_model_is_a_convolution():
    rng = np.random.default_rng(5)
    w, b = rng.standard_normal((40, 33, 3)) / 10, rng.standard_normal(40)
    for L in (1, 5, 6, 7, 13):
        a = rng.standard_normal((L, 33))
        y = B.conv3_wino32(a, w, b)
        ref = B.conv3(a.astype(F64), w, b)
        assert np.abs(y - ref).max() <= 1e-4 * np.abs(ref).max(), L
    At, G, Bt = B.wino_matrices()
    g, d = np.sin(1.0 + np.arange(3)), np.cos(0.3 + 1.7 * np.arange(8))
    assert np.allclose(At @ ((G @ g) * (Bt @ d)), [sum(g[k] * d[i + k] for k in range(3)) for i in range(6)], rtol=1e-12, atol=1e-12)


def test_bits16_round_trip_and_truncation():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -1.0 - 3 * 2.0 ** -9, 3.1415926, 65000.0, 1e-3], F32)
    for mode, eps in (("bf16", 2.0 ** -7), ("f16", 2.0 ** -10)):  # (the spacing of the format's numbers relative to their size)
        r, t = B.rnd(a, mode), B.rnd(a, mode, truncate=True)
        assert (np.abs(r - a) <= eps / 2 * np.abs(a) * 1.001).all() and (np.abs(t) <= np.abs(a)).all() and (np.abs(t - a) < eps * np.abs(a)).all()
        assert (B.to_bits16(r, mode) == B.to_bits16(a, mode)).all()
    assert B.rnd(np.array([1.0 + 2.0 ** -8], F32), "bf16")[0] == 1.0 and B.rnd(np.array([1.0 + 3 * 2.0 ** -8], F32), "bf16")[0] == F32(1.0 + 2.0 ** -6)  # ties to even


# ------------------------------------------------------------------------------------------------ the forms' models against the GPU tests' bars
# (block, operand mode, conv form, statistics chunk rows, 16-bit rows)
MODEL_CASES = ([(n, None, "direct", 128, False) for n in ("enc", "dec", "id")] + [(n, None, "wino", k, False) for n in ("enc", "dec", "id") for k in (128, 24)]
               + [(n, m, "direct", 128, r) for n in ("enc", "dec", "id") for m in ("bf16", "f16") for r in (False, True)])


def bar_of(c, mode, conv):
    return wino_bar(c) if conv == "wino" else c["bar"][mode]


@pytest.mark.parametrize("name,mode,conv,chunk,rows16", MODEL_CASES)
def test_models_of_the_forms_pass_the_bars(name, mode, conv, chunk, rows16):
    c = case(name)
    y, y16, _ = B.model32(c["x"], LENS, c["style"], c["wt"], prec=mode, conv=conv, chunk=chunk, rows16=rows16)
    r = B.ratios(y, c["want"][mode], LENS, bar_of(c, mode, conv))
    print(f"{name} {mode} {conv} chunk {chunk}: model / bar {r}, bar {bar_of(c, mode, conv)}")
    assert B.within(r) and (conv == "direct" or abs(r - 1 / B.FOUR) < 0.1)  # (the Winograd bar IS this model's error times four, at chunks of 24 rows)
    if mode:
        assert (y16 == B.to_bits16(y, mode)).all()


def test_model_of_the_pair_passes_the_bar():
    c, cf = pair()
    for conv, chunk in (("direct", 128), ("wino", 24)):
        y, _, _ = B.model32(c["x"], LENS, c["style"], c["wt"], conv=conv, chunk=chunk, const_from=cf)
        r = B.ratios(y, c["want"][None], LENS, bar_of(c, None, conv))
        print(f"pair B {conv}: model / bar {r:.2f}")
        assert B.within(r)


def test_one_row_batch():
    c = case("enc", (1,))
    y, _, _ = B.model32(c["x"], (1,), c["style"], c["wt"])
    assert B.within(B.ratios(y, c["want"][None], (1,), c["bar"][None]))


# ------------------------------------------------------------------------------------------------ the mutants
# mutant -> where it must be rejected: (block, operand mode, conv, chunk, 16-bit rows).  A formula mutant is tried in fp32 (direct and Winograd bars) and in both
# 16-bit modes; the rounding mutants exist in the 16-bit modes only; the identity residual in the identity block; chunk mutants on chunks of 128 and of 24 rows.
_ALL = [("enc", None, "direct", 128, False), ("enc", None, "wino", 24, False), ("enc", "bf16", "direct", 128, True), ("enc", "f16", "direct", 128, True)]
_HALF = [("enc", m, "direct", 128, True) for m in ("bf16", "f16")]

REJECT = {
    "unbiased_var": _ALL, "eps_outside": _ALL, "gamma_no_one": _ALL, "tap_crosses": _ALL, "no_sqrt2": _ALL, "slope_001": _ALL,
    "last_chunk_dropped": _ALL, "m2_equal_chunks": _ALL,
    "sc_unrounded": _HALF,
    "operand_unrounded": [(n, m, "direct", 128, True) for n in ("enc", "dec", "id") for m in ("bf16", "f16")],
    "residual_hbuf": [("id", None, "direct", 128, False), ("id", None, "wino", 24, False), ("id", "bf16", "direct", 128, True), ("id", "f16", "direct", 128, True)],
}


@pytest.mark.parametrize("mutant", sorted(REJECT))
def test_mutant_is_rejected(mutant):
    for name, mode, conv, chunk, rows16 in REJECT[mutant]:
        c = case(name)
        y, _, _ = B.model32(c["x"], LENS, c["style"], c["wt"], prec=mode, conv=conv, chunk=chunk, rows16=rows16, mutant=mutant)
        r = B.ratios(y, c["want"][mode], LENS, bar_of(c, mode, conv))
        print(f"{mutant} on {name} {mode} {conv}: error / bar {r}")
        assert not B.within(r), (mutant, name, mode, conv, r)


def test_mutant_const_stats_missing_is_rejected():
    c, cf = pair()
    for conv, chunk in (("direct", 128), ("wino", 24)):
        y, _, _ = B.model32(c["x"], LENS, c["style"], c["wt"], conv=conv, chunk=chunk, const_from=cf, mutant="const_stats_missing")
        assert not B.within(B.ratios(y, c["want"][None], LENS, bar_of(c, None, conv)))


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_mutant_y16_truncated_is_rejected(mode):
    """y16 is held bit for bit to round-to-nearest-even of the y the same run wrote (the GPU test's check): truncation differs wherever the dropped bits are
    above half an ulp."""
    c = case("enc")
    y, y16, _ = B.model32(c["x"], LENS, c["style"], c["wt"], prec=mode, rows16=True, mutant="y16_truncated")
    assert (y16 != B.to_bits16(y, mode)).mean() > 0.25


def test_every_mutant_is_tried():
    assert set(REJECT) | {"const_stats_missing", "y16_truncated"} == set(B.MUTANTS)
