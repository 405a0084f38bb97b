"""The 16-bit store contractions with their WHOLE epilogue, operator by operator, against float64 (tests/gemm16_ref.py): conv_gemm16_kernel
(csrc/gemm16.hip.h, force_tile 19) and the 16-bit-row tiles of conv_gemm_f32 (csrc/gemm.hip.h, tiles 6 / 15 / 17 / 18), through
stts_op_conv1d_epi.  Every buffer a launch may write is pre-filled with a sentinel bit pattern (fp32: the quiet NaN 0x7FC0BEEF, 16-bit: 0x7FC1)
and compared as bits, so "not written" is a testable statement.

Which epilogue feature is pinned by which case (all on tile 19 in bf16; [f16]: in fp16 too; [tiles]: on tiles 6, 15, 17, 18 too, without stat_part):
  E1 pwconv1 [f16][tiles]   SiLU -> Y16 only + GRN sums; cout 384 ends inside the second 256-channel tile (npad 512)
  E2 pwconv2 [f16][tiles]   + R through a window (ldr 320, rcol0 4) -> Y
  E3 conv1 [f16]            cin 130 (kc 192: pad columns hold garbage), k 3 -> Y + AdaIN statistics; E3c: the same on bias-dominated channels
  E4 conv2 + shortcut [f16] two segments (256, k 3) + (130, k 1), alpha 1/sqrt 2 -> Y + Y16 + statistics with ld_stat 320 != N
  E5 identity block         + R (ldr 320), alpha 1/sqrt 2 -> Y + statistics: the pwconv2 body with alpha != 1 and statistics
  E6 prior conv [tiles]     Y16 only into a column window (ldy16 256, ycol16 128)
  E7 generic [tiles]        dilation 3, LeakyReLU, + R, alpha 0.5 -> Y (ycol0 8, ldy 160) + Y16, cout 132
  E8 projector              two segments (64, k 1) + (192, k 7) -> Y only
  W1 directory walk         52 utterances x 5 channel tiles = 260 virtual tiles > 256 blocks: some blocks walk two tiles, + R prefetch restarts
  W2 no directory           n_utt 64 (directory), 65 and 300 (scan fallback) with a zero-row utterance; GRN sums + statistics
  W3 capacity               host offsets are capacities, device offsets the real ones; rows of the slack stay untouched

Assertions (per case and utterance):
  1 values      |Y - ref64|.max() <= 2e-5 |ref64|.max() (the bar of test_conv1d_16bit_matches_rounded_oracle, K up to 7 168 there); everything outside
                the column window and every row past the real row count keeps the sentinel.
  2 rounded     Y16 == round-to-nearest-even(Y) bit for bit; Y16-only launches are repeated with Y requested as well (the generic body on tile 19):
                same Y16 bits, and that launch's Y stands for "the stored fp32 values" below.
  3 bodies      tile 19: the launch repeated with tune | 0x4000 (generic store body) gives bit-identical Y, Y16 and GRN sums in every case, and
                bit-identical statistics wherever alpha == 1.  With alpha != 1 (E4: the conv2 + shortcut body, E5: the pwconv2 body) the MEAN / M2 rows
                differ between the bodies (E4 bf16: 837 of the written elements, the largest gaps 2.4e-7 in a mean and 9.2e-5 in an M2 - the last
                bits of sums of O(1) terms; on a mean near 0 that reads as up to 1 536 fp32 ulps), and the ISA of the two bodies shows why: `vv *= alpha; ...; su += vv` is
                one basic block in a specialised body, where hipcc contracts it to v_pk_fma_f32 su = alpha * (acc + bias [+ R]) + su - the sum of the
                UNROUNDED products - next to the v_pk_mul_f32 whose rounded result is stored and squared; in the generic body the run-time `if (HY)` /
                `if (HY16)` branches put the multiply and the add into different blocks, so it adds the rounded product (v_pk_add_f32).  A legitimate
                contraction of the same expression: Y and Y16 do not move by a single bit (the bar for a body that differs by such a contraction
                would be 1 fp32 ulp of Y and equal Y16 away from rounding boundaries: met with room to spare), and for the statistics the bar is assertion 5 on EACH body
                (the fused sum is at most u * sum |v| away from the sum of the stored values; a worst-case derivation for it would read
                (nc + 2) instead of (nc + 1) - the stated bound is kept and met by both).
  4 GRN sums    with v the stored fp32 values: the four slots of a 128-row group sum to sum v^2 over its rows, and all ceil(len / 32) slots to the
                utterance's total, within 129 * 2^-24 relative (any order of <= 128 non-negative fp32 terms: 127 additions, + 1 for each square's own
                rounding, + 1 for the test's fp32 -> float64 slot sum being exact: 129 is a safe count); slots < ceil(len / 32) are finite, slots from
                there to ss_stride - 1 and channels >= N keep the sentinel.
  5 statistics  per 128-row chunk (nc rows) and channel, u = 2^-24, S1 = sum v, S2 = sum v^2, A = sum |v|.  The kernel computes s1 = fl(sum v),
                s2 = fl(sum fl(v^2)), mean = fl(s1 * fl(1 / nc)), M2 = max(fl(s2 - fl(mean * s1)), 0).
                  mean: |s1 - S1| <= (nc - 1) u A; the reciprocal and the product add 2 u |S1| <= 2 u A   =>  |mean - mean64| <= (nc + 1) u A / nc.
                  M2:   |s2 - S2| <= nc u S2 (nc - 1 additions + the squares' own rounding).  mean * s1 = s1^2 / nc up to 3 roundings; since A^2 <= nc S2
                        (Cauchy-Schwarz) and |S1| <= A:  |s1^2 - S1^2| / nc <= 2 (nc - 1) u A^2 / nc <= 2 (nc - 1) u S2, the three roundings <= 3 u S1^2 / nc
                        <= 3 u S2, the final subtraction <= u S2.  Sum: (3 nc + 2) u S2 to first order; the bar is (3 nc + 4) u S2 (second-order terms).
                        The clamp at 0 only moves M2 towards M2_64 >= 0.
                chunks < ceil(len / 128) are finite with M2 >= 0; later chunks and columns N .. ld_stat - 1 keep the sentinel.
  6 ragged = solo  (E2, E4, W2 with 65 utterances) every utterance run alone gives the batch's bits for its rows, sums and statistics.

Measured on an MI355X (printed by the tests with -s; also in DESIGN.md section 5b):
  * max over utterances of |Y - ref64|.max() / |ref64|.max(), bar 2e-5, tile 19 bf16: E1 2.0e-7, E2 1.9e-7, E3 2.3e-7, E3c 1.4e-7, E4 3.1e-7, E5 2.5e-7,
    E6 2.5e-7, E7 1.2e-7, E8 5.2e-7, W1 1.2e-7, W2 1.1e-7 .. 1.3e-7, W3 1.3e-7 / 2.0e-7; tile 19 fp16: E1 1.7e-7, E2 2.1e-7, E3 2.4e-7, E4 2.9e-7;
    tiles 6 / 15 / 17 / 18 give the same figure as one another: E1 2.0e-7 (fp16 1.7e-7), E2 1.9e-7 (2.1e-7), E6 1.9e-7, E7 1.2e-7.
  * E3c, the one-pass formula on bias-dominated channels (mean 8, standard deviation ~0.05, mean^2 / var = 1.5e4 .. 4.3e4): |M2 - M2_64| / M2_64 =
    2.2e-3 .. 1.2e-2 on the eight channels, against 1.5e-6 on the ordinary channels of the same launch (mean^2 / var ~ 6).  The sound bound holds.
  * the decoder test: batched 8.9e-4 / 1.1e-3 / 8.2e-4 on utterances 0 / 64 / 109, the same utterances alone 9.2e-4 / 1.3e-3 / 8.7e-4, d0 = 4.0e-3.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import pytest

import gemm16_ref as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT32, SENT16 = np.uint32(0x7FC0BEEF), np.uint16(0x7FC1)
U = 2.0 ** -24
RSQRT2 = float(np.float32(0.70710678118654752440))


@dataclass(frozen=True)
class Case:
    name: str
    segs: Tuple[Tuple[int, int, int], ...]  # (cin, k, dil) per K segment
    cout: int
    lengths: Tuple[int, ...]  # real rows per utterance
    act: int = G.ACT_NONE
    alpha: float = 1.0
    r: Optional[Tuple[int, int]] = None  # (ldr, rcol0)
    y: Optional[Tuple[int, int]] = None  # (ldy, ycol0)
    y16: Optional[Tuple[int, int]] = None  # (ldy16, ycol16)
    ss: bool = False
    stat: Optional[int] = None  # ld_stat
    caps: Optional[Tuple[int, ...]] = None  # capacity layout: rows each utterance may have at most
    cancel: bool = False  # E3c: eight channels with bias + 8 and a standard deviation of ~0.05


L_A = (300, 129, 31, 256, 1)
L_B = (257, 128, 127, 385, 5)
CANCEL_CH = (0, 37, 63, 64, 129, 200, 254, 255)


def _w2_lengths(n):
    L = [(1, 2, 3, 130)[i % 4] for i in range(n)]
    L[7] = 0  # (the Segments plumbing, the launcher and both tile lookups admit an utterance of zero rows: it owns no tile)
    if n > 64:
        L[66 if n > 66 else 64] = 257
    return tuple(L)


def _w3(n):
    lens = [1, 300, 129, 256, 77] if n == 5 else [1 + (i * 37) % 300 for i in range(n)]
    extra = [0, 260, 256, 0, 130] if n == 5 else [(0, 260, 5, 256, 0, 131, 17)[i % 7] for i in range(n)]
    extra[-1] = max(extra[-1], 130)  # the last capacity is larger than its real length
    return tuple(lens), tuple(a + b for a, b in zip(lens, extra))


CASES = {
    c.name: c
    for c in [
        Case("E1", ((128, 1, 1),), 384, L_A, act=G.ACT_SILU, y16=(384, 0), ss=True),
        Case("E2", ((384, 1, 1),), 256, L_A, r=(320, 4), y=(256, 0)),
        Case("E3", ((130, 3, 1),), 256, L_B, y=(256, 0), stat=256),
        Case("E3c", ((130, 3, 1),), 256, L_B, y=(256, 0), stat=256, cancel=True),
        Case("E4", ((256, 3, 1), (130, 1, 1)), 256, L_B, alpha=RSQRT2, y=(256, 0), y16=(256, 0), stat=320),
        Case("E5", ((256, 3, 1),), 256, L_B, alpha=RSQRT2, r=(320, 0), y=(256, 0), stat=256),
        Case("E6", ((64, 7, 1),), 64, (77, 5, 260, 3), y16=(256, 128)),
        Case("E7", ((64, 3, 3),), 132, (77, 5, 260), act=G.ACT_LRELU, alpha=0.5, r=(288, 12), y=(160, 8), y16=(136, 4)),
        Case("E8", ((64, 1, 1), (192, 7, 1)), 256, (300, 2), y=(256, 0)),
        Case("W1", ((64, 1, 1),), 1280, tuple((1, 2, 3)[i % 3] for i in range(52)), r=(1280, 0), y=(1280, 0)),
        Case("W2-64", ((64, 1, 1),), 256, _w2_lengths(64), y=(256, 0), ss=True, stat=256),
        Case("W2-65", ((64, 1, 1),), 256, _w2_lengths(65), y=(256, 0), ss=True, stat=256),
        Case("W2-300", ((64, 1, 1),), 256, _w2_lengths(300), y=(256, 0), ss=True, stat=256),
        Case("W3-5", ((64, 3, 1),), 512, _w3(5)[0], y=(512, 0), y16=(512, 0), ss=True, caps=_w3(5)[1]),
        Case("W3-70", ((64, 3, 1),), 512, _w3(70)[0], y=(512, 0), y16=(512, 0), ss=True, caps=_w3(70)[1]),
    ]
}
F16_TOO = ("E1", "E2", "E3", "E4")
OTHER_TILES = ("E1", "E2", "E6", "E7")
RUNS = [(n, "bf16", 19) for n in CASES] + [(n, "f16", 19) for n in F16_TOO]
RUNS += [(n, p, t) for n in OTHER_TILES for p in (("bf16", "f16") if n in F16_TOO else ("bf16",)) for t in (6, 15, 17, 18)]


@pytest.fixture(scope="module")
def hip(cfg):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)  # (the operator packs for the precision it is given; the engine's own mode plays no part)
    yield m
    m.close()


def _round_up(a, b):
    return (a + b - 1) // b * b


@lru_cache(maxsize=None)
def inputs(name):
    """Host inputs of a case (shared by every launch of it, never modified) and their float64 reference per mode."""
    from stylish_tts_amd import synth

    c = CASES[name]
    caps = c.caps or c.lengths
    R, Rreal = sum(caps), sum(c.lengths)
    segs = []
    for i, (cin, k, dil) in enumerate(c.segs):
        ldx = _round_up(cin, 64)
        # pad columns and the rows of the capacity slack hold finite garbage (|.| < 40: finite in fp16 too); the pad columns meet zero weights
        x = (synth.normal(f"g16.{name}.pad{i}", (R, ldx)) * 9.0).astype(np.float32)
        x[:Rreal, :cin] = synth.normal(f"g16.{name}.x{i}", (Rreal, cin))
        w = (synth.normal(f"g16.{name}.w{i}", (c.cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
        if c.cancel:
            w[list(CANCEL_CH)] *= np.float32(0.05)
        segs.append((x, cin, w, dil))
    bias = synth.normal(f"g16.{name}.b", (c.cout,))
    if c.cancel:
        bias[list(CANCEL_CH)] += np.float32(8.0)
    r = None
    if c.r:
        r = synth.normal(f"g16.{name}.r", (R, c.r[0]))  # (O(1) everywhere: what lies outside the window must not be read into the result)
    for a in [bias, r] + [s[0] for s in segs] + [s[2] for s in segs]:
        if a is not None:
            a.setflags(write=False)
    return dict(segs=segs, bias=bias, r=r)


@lru_cache(maxsize=None)
def ref64(name, prec):
    c, inp = CASES[name], inputs(name)
    Rreal = sum(c.lengths)
    r = None if inp["r"] is None else inp["r"][:Rreal, c.r[1] : c.r[1] + c.cout]
    ref = G.conv_epi64([(x[:Rreal], w, dil) for x, _, w, dil in inp["segs"]], c.lengths, inp["bias"], prec, c.act, c.alpha, r)
    ref.setflags(write=False)
    return ref


def _sentinel(shape, dtype):
    if dtype == torch.float32:
        a = np.full(shape, SENT32, np.uint32).view(np.float32)
    else:
        a = np.full(shape, SENT16, np.uint16).view(np.int16)
    return torch.from_numpy(a).cuda()


def launch(hip, name, prec, tile, tune=0, with_y=False, only=None):
    """One launch of case `name` (only = u: utterance u alone) into sentinel-filled buffers -> dict of host arrays (bit patterns kept)."""
    from stylish_tts_amd.runtime import Segments

    c, inp = CASES[name], inputs(name)
    d0 = torch.device("cuda", 0)
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    if only is None:
        rows = slice(0, sum(c.caps or c.lengths))
        if c.caps:
            seg = Segments(c.caps, d0, dev=torch.from_numpy(off.astype(np.int32)).to(d0), capacity=True)
        else:
            seg = Segments(c.lengths, d0)
    else:
        assert not c.caps
        rows = slice(int(off[only]), int(off[only + 1]))
        seg = Segments([c.lengths[only]], d0)
    R, n = seg.rows, seg.n
    to = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731  (a copy: the shared inputs are read-only)
    segments = [(to(x[rows]), cin, w, dil) for x, cin, w, dil in inp["segs"]]
    ysp = c.y or ((_round_up(c.cout, 32), 0) if with_y else None)
    y = _sentinel((R, ysp[0]), torch.float32) if ysp else None
    y16 = _sentinel((R, c.y16[0]), torch.int16) if c.y16 else None
    ss = _sentinel((n, (seg.max_len + 31) // 32 + 2, _round_up(c.cout, 32) + 32), torch.float32) if c.ss else None
    st = _sentinel((n, (seg.max_len + 127) // 128 + 1, 2, c.stat), torch.float32) if (c.stat and tile == 19) else None
    hip.op_conv1d_epi(seg, segments, inp["bias"], prec, tile, act=c.act, alpha=c.alpha, r=None if inp["r"] is None else to(inp["r"][rows]),
                      rcol0=c.r[1] if c.r else 0, y=y, ycol0=ysp[1] if ysp else 0, y16=y16, ycol16=c.y16[1] if c.y16 else 0, sumsq=ss, stat=st, tune=tune)
    out = dict(ycol0=ysp[1] if ysp else 0)
    for k, t in (("y", y), ("y16", y16), ("ss", ss), ("stat", st)):
        out[k] = None if t is None else t.cpu().numpy()
    if out["y16"] is not None:
        out["y16"] = out["y16"].view(np.uint16)
    return out


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    v = np.uint32 if a.dtype == np.float32 else a.dtype
    return a.shape == b.shape and np.array_equal(a.view(v), b.view(v))


def kept32(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENT32).all())


def check_rows(c, prec, out, ref, ycol0):
    """Assertions 1 and 2 on one launch; -> (the worst |Y - ref| / |ref|.max() over the utterances, the stored fp32 values [real rows, cout])."""
    N, Rreal = c.cout, sum(c.lengths)
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    y, y16 = out["y"], out["y16"]
    worst, v = 0.0, None
    if y is not None:
        v = y[:Rreal, ycol0 : ycol0 + N]
        assert np.isfinite(v).all(), (c.name, "Y: a value inside the window is not finite (unwritten or wrong)", np.argwhere(~np.isfinite(v))[:4])
        assert kept32(y[:Rreal, :ycol0]) and kept32(y[:Rreal, ycol0 + N :]), (c.name, "Y: written outside the column window")
        assert kept32(y[Rreal:]), (c.name, "Y: rows past the real row count written")
        for u, L in enumerate(c.lengths):
            if L == 0:
                continue
            g, rf = v[off[u] : off[u + 1]], ref[off[u] : off[u + 1]]
            e = float(np.abs(g - rf).max() / np.abs(rf).max())
            worst = max(worst, e)
            assert e <= 2e-5, (c.name, prec, "utterance", u, "first wrong element", np.argwhere(np.abs(g - rf) > 2e-5 * np.abs(rf).max())[:1], e)
    if y16 is not None:
        c16 = c.y16[1]
        w16 = y16[:Rreal, c16 : c16 + N]
        assert (y16[:Rreal, :c16] == SENT16).all() and (y16[:Rreal, c16 + N :] == SENT16).all(), (c.name, "Y16: written outside the column window")
        assert (y16[Rreal:] == SENT16).all(), (c.name, "Y16: rows past the real row count written")
        if v is not None:
            want = G.round_bits(v, prec).reshape(v.shape)
            assert np.array_equal(w16, want), (c.name, prec, "Y16 != RNE(Y)", np.argwhere(w16 != want)[:4])
    return worst, v


def check_sums(c, out, v):
    """Assertion 4."""
    ss, N = out["ss"], c.cout
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    assert kept32(ss[:, :, N:]), (c.name, "sumsq_part: channels >= N written")
    for u, L in enumerate(c.lengths):
        ns = (L + 31) // 32
        assert kept32(ss[u, ns:]), (c.name, "sumsq_part: a slot past ceil(len / 32) written", u, L)
        got = ss[u, :ns, :N]
        assert np.isfinite(got).all(), (c.name, "sumsq_part: a slot below ceil(len / 32) not written", u, L, np.argwhere(~np.isfinite(got))[:4])
        sq = v[off[u] : off[u + 1]].astype(np.float64) ** 2
        for g in range((L + 127) // 128):
            want = sq[128 * g : 128 * g + 128].sum(0)
            have = got[4 * g : 4 * g + 4].astype(np.float64).sum(0)
            assert (np.abs(have - want) <= 129 * U * want).all(), (c.name, "sumsq_part group", u, g, float((np.abs(have - want) / want).max()))
        if L:
            want, have = sq.sum(0), got.astype(np.float64).sum(0)
            assert (np.abs(have - want) <= 129 * U * want).all(), (c.name, "sumsq_part total", u)


def check_stats(c, out, v):
    """Assertion 5; -> per channel the worst |M2 - M2_64| / M2_64 and the mean^2 / variance it occurred at, over whole 128-row chunks."""
    st, N = out["stat"], c.cout
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    assert kept32(st[:, :, :, N:]), (c.name, "stat_part: columns N .. ld_stat - 1 written")
    rel = np.zeros(N)
    ratio = np.zeros(N)
    for u, L in enumerate(c.lengths):
        nch = (L + 127) // 128
        assert kept32(st[u, nch:]), (c.name, "stat_part: a chunk past ceil(len / 128) written", u, L)
        for ch in range(nch):
            x = v[off[u] + 128 * ch : off[u] + min(L, 128 * ch + 128)].astype(np.float64)
            nc = x.shape[0]
            mean, m2 = st[u, ch, 0, :N].astype(np.float64), st[u, ch, 1, :N].astype(np.float64)
            assert np.isfinite(mean).all() and np.isfinite(m2).all(), (c.name, "stat_part: chunk not written", u, ch)
            mean64 = x.mean(0)
            m2_64 = ((x - mean64) ** 2).sum(0)
            A, S2 = np.abs(x).sum(0), (x ** 2).sum(0)
            assert (np.abs(mean - mean64) <= (nc + 1) * U * A / nc).all(), (c.name, "mean", u, ch, float((np.abs(mean - mean64) / (U * A / nc)).max()))
            assert (np.abs(m2 - m2_64) <= (3 * nc + 4) * U * S2).all(), (c.name, "M2", u, ch, float((np.abs(m2 - m2_64) / (U * S2)).max()))
            assert (m2 >= 0).all(), (c.name, "M2 < 0", u, ch)
            if nc == 128:
                e = np.abs(m2 - m2_64) / m2_64
                ratio = np.where(e > rel, mean64 ** 2 / (m2_64 / nc), ratio)
                rel = np.maximum(rel, e)
    return rel, ratio


@pytest.mark.parametrize("name,prec,tile", RUNS, ids=[f"{n}-{p}-t{t}" for n, p, t in RUNS])
def test_epilogue_against_float64(hip, name, prec, tile):
    """Assertions 1 - 5 of the module docstring on one (case, mode, tile)."""
    c, ref = CASES[name], ref64(name, prec)
    out = launch(hip, name, prec, tile)
    assert out["stat"] is not None or not c.stat or tile != 19
    twin = None
    if c.y is None:  # Y16 only: the same launch with Y as well stores the same 16-bit rows, and its Y is "the stored fp32 values"
        twin = launch(hip, name, prec, tile, with_y=True)
        assert same_bits(twin["y16"], out["y16"]), (name, "Y16 differs between the Y16-only body and the launch that also stores Y")
        assert same_bits(twin["ss"], out["ss"])
        check_rows(c, prec, out, ref, 0)
    src = twin or out
    worst, v = check_rows(c, prec, src, ref, src["ycol0"])
    print(f"\n[gemm16 epilogue] {name} {prec} tile {tile}: max |Y - ref64| / |ref64|.max() = {worst:.2e} (bar 2e-5)")
    if c.ss:
        check_sums(c, out, v)
    rel = ratio = None
    if c.stat and tile == 19:
        rel, ratio = check_stats(c, out, v)
    if tile == 19:  # assertion 3: the generic store body
        gen = launch(hip, name, prec, tile, tune=0x4000)
        for k in ("y", "y16", "ss") + (() if c.alpha != 1.0 else ("stat",)):
            if not same_bits(gen[k], out[k]):
                a, b = out[k], gen[k]
                where = np.argwhere(a.view(np.uint32 if a.dtype == np.float32 else a.dtype) != b.view(np.uint32 if b.dtype == np.float32 else b.dtype))
                ulps = None
                if a.dtype == np.float32:
                    ulps = int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())
                pytest.fail(f"{name} {prec}: the generic store body differs from the specialised one in {k}: {len(where)} elements, first at {where[0]}, up to {ulps} fp32 ulps")
        if c.stat and c.alpha != 1.0:  # (see the module docstring: s1 of the specialised bodies accumulates the unrounded v * alpha)
            check_stats(c, gen, v)
            a, b = out["stat"].astype(np.float64), gen["stat"].astype(np.float64)
            assert kept32(out["stat"]) == kept32(gen["stat"]) and np.array_equal(np.isnan(a), np.isnan(b))
            print(f"[gemm16 statistics] {name} {prec}: specialised vs generic body, largest difference of a mean {np.nanmax(np.abs(a[:, :, 0] - b[:, :, 0])):.2e}, "
                  f"of an M2 {np.nanmax(np.abs(a[:, :, 1] - b[:, :, 1])):.2e}")
    if c.stat and tile == 19:
        if c.cancel:
            ch = list(CANCEL_CH)
            other = np.setdiff1d(np.arange(c.cout), ch)
            print(f"[gemm16 statistics] {name} {prec}: bias-dominated channels {ch}: worst |M2 - M2_64| / M2_64 per channel = "
                  f"{', '.join(f'{e:.1e}' for e in rel[ch])} at mean^2 / var = {', '.join(f'{q:.0f}' for q in ratio[ch])}; "
                  f"the other channels: worst {rel[other].max():.1e} (mean^2 / var there {ratio[other][np.argmax(rel[other])]:.2f})")


@pytest.mark.parametrize("name", ["E2", "E4", "W2-65"])
def test_ragged_batch_equals_each_utterance_alone(hip, name):
    """Assertion 6: no utterance's rows, GRN sums or statistics depend on what else is in the batch."""
    c = CASES[name]
    batch = launch(hip, name, "bf16", 19)
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    for u, L in enumerate(c.lengths):
        if L == 0:
            continue
        solo = launch(hip, name, "bf16", 19, only=u)
        for k in ("y", "y16"):
            if batch[k] is not None:
                assert same_bits(np.ascontiguousarray(batch[k][off[u] : off[u + 1]]), solo[k]), (name, k, "utterance", u, L)
        for k, per in (("ss", 32), ("stat", 128)):
            if batch[k] is not None:
                n = (L + per - 1) // per
                assert same_bits(np.ascontiguousarray(batch[k][u, :n]), np.ascontiguousarray(solo[k][0, :n])), (name, k, "utterance", u, L)


def _decoder_batch(tag, lens):
    from stylish_tts_amd import synth

    per = [dict(asr=synth.normal(f"{tag}.asr{i}", (1, 128, L)), pitch=synth.pitch_curve(f"{tag}.p{i}", 1, L),
                energy=(synth.uniform(f"{tag}.e{i}", (1, L)) * 2 + 2).astype(np.float32), style=(synth.normal(f"{tag}.s{i}", (1, 64)) * 0.7).astype(np.float32))
           for i, L in enumerate(lens)]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = (to(np.concatenate([p["asr"][0].T for p in per])), to(np.concatenate([p["pitch"][0] for p in per])), to(np.concatenate([p["energy"][0] for p in per])),
           to(np.concatenate([p["style"] for p in per])))
    return per, dev


def test_decoder_production_wiring_bf16(cfg, weights):
    """The engine, not the operator: the bf16 decoder on a batch that switches every large-batch path on at once.  110 utterances of 30 .. 50 frames
    (4 400 rows): above 4 096 rows AdaIN is no longer folded into the contractions' staging, above rows16_threshold() = 3 840 the normalised
    activations are 16-bit rows, 110 row tiles x 2 channel tiles = 220 >= gemm16_min_tiles = 192 selects conv_gemm16_kernel, n_utt > 64 takes its
    scan fallback, and no utterance fills a 128-row statistics chunk.

    Launch counts, from run_adain_block / decoder_forward: every block's conv1 and conv2 run on conv_gemm16_kernel (10 launches; the two asr_res
    convs read fp32 rows and stay on conv_gemm_f32).  conv1's epilogue leaves norm2's statistics and conv2's those of the next block's norm1, so
    adain_partial_kernel runs twice only: block 0's norm1 (nothing produced its input on the matrix cores) and the constant columns
    [asr_res | F0 | N] once.  The 3 960-row batch of the same kind stays on the folded path (<= 4 096 rows): ten statistics passes, one per norm,
    and no conv_gemm16_kernel launch.

    Values: against the oracle with the same rounding points, max-abs over |ref|.max() on utterances 0, 64 (the first past the directory width) and
    109.  The yardstick d0 is the same distance between the fp32 oracle and the rounded oracle: the size of the rounding noise that a reordered
    fp32 sum can flip.  The bar in force is err <= d0: the same three utterances run alone (the small-batch path, which the suite already holds to
    the waveform bars) sit inside d0 themselves, so d0 is a fair yardstick and the fallback bar (twice the solo error) is not needed."""
    import ctypes as C
    import json

    from oracle import stylish_oracle as O
    from stylish_tts_amd import _lib
    from stylish_tts_amd.runtime import HipModel, Segments

    w = weights["speech_predictor"]
    d0_ = torch.device("cuda", 0)
    lens = [30 + i % 21 for i in range(110)]
    small = lens[:100]
    assert sum(lens) > 4096 and 3840 <= sum(small) <= 4096 and max(lens) < 128
    picks = (0, 64, 109)
    per, dev = _decoder_batch("g16dec", lens)
    refs, d0 = {}, 0.0
    try:
        for u in picks:
            p = per[u]
            O.OPERAND_ROUND = "bf16"
            refs[u] = O.decoder_forward(p["asr"], p["pitch"], p["energy"], p["style"], w)
            O.OPERAND_ROUND = None
            f32 = O.decoder_forward(p["asr"], p["pitch"], p["energy"], p["style"], w)
            d0 = max(d0, float(np.abs(f32 - refs[u]).max() / np.abs(refs[u]).max()))
    finally:
        O.OPERAND_ROUND = None
    hip = HipModel(cfg, 0, precision="bf16")
    hip.load_weights({"speech_predictor": w}, which=7)
    lib = _lib.load()

    def profiled(seg, args):
        lib.stts_profile_begin()
        x = hip.decoder(seg, *args).cpu().numpy()
        buf = C.create_string_buffer(1 << 17)
        _lib.check(lib.stts_profile_report(C.c_void_p(torch.cuda.current_stream().cuda_stream), buf, len(buf)))
        recs = {r["kernel"]: r["launches"] for r in json.loads(buf.value.decode())}
        return x, recs

    s = Segments(lens, d0_)
    x, recs = profiled(s, dev)
    _, recs_small = profiled(Segments(small, d0_), _decoder_batch("g16dec", small)[1])
    assert np.array_equal(hip.decoder(s, *dev).cpu().numpy(), x), "the profiled launch form differs from the plain one"
    errs, solos = [], []
    for u in picks:
        ref = refs[u][0].T
        sc = np.abs(ref).max()
        errs.append(float(np.abs(x[s.host[u] : s.host[u + 1], :512] - ref).max() / sc))
        du = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (per[u]["asr"][0].T, per[u]["pitch"][0], per[u]["energy"][0], per[u]["style"]))
        xs = hip.decoder(Segments([lens[u]], d0_), *du).cpu().numpy()
        solos.append(float(np.abs(xs[:, :512] - ref).max() / sc))
    hip.check_status()
    hip.close()
    print(f"\n[gemm16 decoder wiring] bf16, 110 utterances / {sum(lens)} rows: launches {recs.get('conv_gemm16_kernel', 0)} conv_gemm16_kernel, "
          f"{recs.get('adain_partial_kernel', 0)} adain_partial_kernel ({sum(small)} rows: {recs_small.get('conv_gemm16_kernel', 0)} and "
          f"{recs_small.get('adain_partial_kernel', 0)}); err vs rounded oracle on utterances {picks}: batched {['%.2e' % e for e in errs]}, "
          f"alone {['%.2e' % e for e in solos]}; d0 (fp32 oracle vs rounded oracle) = {d0:.2e}")
    assert recs.get("conv_gemm16_kernel", 0) == 10 and recs_small.get("conv_gemm16_kernel", 0) == 0, (recs, recs_small)
    assert (recs.get("adain_partial_kernel", 0), recs_small.get("adain_partial_kernel", 0)) == (2, 10), (recs, recs_small)
    assert np.isfinite(x).all()
    assert max(errs) <= d0, (errs, solos, d0)


def test_operator_refuses_what_it_cannot_launch(hip):
    """A bad combination is an error status, never a launch: statistics off tile 19, a window outside its buffer, offsets that disagree."""
    from stylish_tts_amd.runtime import Segments

    c, inp = CASES["E3"], inputs("E3")
    d0 = torch.device("cuda", 0)
    seg = Segments(c.lengths, d0)
    to = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731
    segments = [(to(x), cin, w, dil) for x, cin, w, dil in inp["segs"]]
    y = _sentinel((seg.rows, 256), torch.float32)
    st = _sentinel((seg.n, 5, 2, 256), torch.float32)
    with pytest.raises(RuntimeError, match="tile 19"):
        hip.op_conv1d_epi(seg, segments, inp["bias"], "bf16", 15, y=y, stat=st)
    with pytest.raises(RuntimeError, match="window"):
        hip.op_conv1d_epi(seg, segments, inp["bias"], "bf16", 19, y=y, ycol0=4)
    with pytest.raises(RuntimeError, match="stat_nchunk"):
        hip.op_conv1d_epi(seg, segments, inp["bias"], "bf16", 19, y=y, stat=st[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="capacity flag"):
        hip.op_conv1d_epi(Segments(c.lengths, d0, dev=torch.zeros(seg.n + 1, dtype=torch.int32, device=d0)), segments, inp["bias"], "bf16", 19, y=y)
    with pytest.raises(RuntimeError, match="precision"):
        hip.op_conv1d_epi(seg, segments, inp["bias"], "f32", 19, y=y)
    torch.cuda.synchronize()
    assert kept32(y.cpu().numpy()) and kept32(st.cpu().numpy())
