"""The 2-D implicit-GEMM convolution (csrc/conv2d.hip.h: conv2d_kernel's four instances, conv2d_reduce_kernel) against float64, launch by launch, through
stts_op_conv2d: every tile (256 x 16, 128 x 32, 64 x 64 with and without the LeakyReLU operand) on ragged batches whose blocks end ragged and hold
utterance boundaries and empty utterances; K in chunks summed in the kernel and as grid slices; two segments; the 5 x 5 valid row map, the one-tap
contraction over frames, a level shift, the four sub-pixel parities of a stride-2 transposed conv; every step of the epilogue.

The reference, the bound (a count of roundings, in any summation order) and the cases are tests/conv2d64.py's; tests/test_conv2d64_cpu.py shows that a
numpy-fp32 emulation meets the bound and that seven defects exceed it 1e4 times and more.  Every output and residual buffer has guard rows before and
after and is pre-filled with the quiet NaN 0x7FC0BEEF: whatever is not an output position of the launch keeps its bits (the other parities of an up = 2
grid included), the columns cout .. ldy - 1 of written rows are exactly 0, and the residual is read at the launch's own positions only (every other one
holds the NaN).  The odd utterances are 1e3 times the even ones and the inputs' pad channels hold finite 1e3-scale values.

Beyond the bound: grid slices + reduce give the bits of the in-kernel chunk sums; every utterance alone gives the bits it has in its batch; a refused call
(a row stride of 8, ldy > npad, cout > ldy, a short input / output / residual buffer, offsets off the level's grid, up = 3, a parity not below up)
raises and leaves every sentinel in place.

Measured on an MI355X (-s prints them), largest error as a fraction of the bound:
  tiles on (5, 0, 9, 1) x 6     npad 16 / cout 3 / ldy 4: 0.048; 16 / 16: 0.038; 32 / 17: 0.066; 64 / 33: 0.053; 128 / 70 / ldy 80: 0.066; 64, LeakyReLU: 0.081
  tiles on (7, 12, 0, 30) x 8   256 x 16: 0.036; 128 x 32: 0.040; 64 x 64: 0.056; 64 x 64 with LeakyReLU in chunks of 64: 0.056; empty ends: 0.035; no rows: nothing launched
  K = 144                       chunks of 64: 0.039, of 144 and of 256: 0.053 - the same as grid slices; two segments (K = 432, chunks of 64): 0.030; LeakyReLU: 0.076
  row maps                      5 x 5 valid: 0.025; one tap over frames: 0.052; sh = 2: 0.049; parities 00 / 01 / 10 / 11: 0.217 / 0.129 / 0.249 / 0.172
  epilogue                      bias 0.059, ReLU 0.114, sigmoid 0.189, residual 0.061, residual and sqrt 2: 0.067
  cout 16 on the three tiles    the same bits (printed, not asserted)
With one in-bounds mutation of a scratch copy of conv2d_kernel at a time: the `kc == g.chunk` flush removed fails
test_grid_slices_give_the_bits_of_the_kernels_own_chunk_sums (the four pairs with more than one chunk) and nothing else - one chain for three is inside
the bound; dt and df swapped in the load fails 34 cases of test_launch_against_float64 and test_four_parities_fill_the_transposed_conv; `+ g.pt` dropped
from orow fails test_launch_against_float64[up2_10] and [up2_11], their batch-independence cases and test_four_parities_fill_the_transposed_conv.
"""
import numpy as np
import pytest

import conv2d64 as V

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT32 = np.uint32(0x7FC0BEEF)
F32, F64 = np.float32, np.float64
GUARD = 3  # rows before and after every output and residual buffer


@pytest.fixture(scope="module")
def hip(cfg):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)
    yield m
    m.close()


def seg_of(lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments(lengths, torch.device("cuda", 0))


def sentinel(shape):
    return np.full(shape, SENT32, np.uint32).view(F32)


def kept(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENT32).all())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def window(t, first_row, elems):
    """(pointer, element count) of `elems` floats from row `first_row` of a 2-D device tensor (an empty window still has an address)."""
    return t.data_ptr() + first_row * t.shape[1] * 4, elems


def launch(hip, c, d, ybuf=None, short=None, seg_lens=None):
    """One stts_op_conv2d launch of case c on data d -> the output buffer as numpy, [GUARD + out_rows + GUARD][ldy], pre-filled with the sentinel
    (or the given buffer, for a second launch into it); the residual buffer holds its values at the launch's positions and the sentinel everywhere else.
    short: the name of a buffer passed one element short; seg_lens: other full-rate lengths than lens << sh for both offset arrays.  Raises what the
    operator raises, after putting the buffers into launch.last."""
    seg_in, seg_out = seg_of(seg_lens or [L << c.sh for L in c.lens]), seg_of(seg_lens or [L << c.sh for L in c.lens_out])
    x0 = torch.from_numpy(np.concatenate([V.pack_rows(d["x0"], c.ld0, 1), sentinel((1, c.ld0))])).cuda()
    x1 = torch.from_numpy(np.concatenate([V.pack_rows(d["x1"], c.ld1, 2), sentinel((1, c.ld1))])).cuda() if c.cin1 else None
    in_rows = sum(c.lens) * c.Fin
    Tg, Fg = sum(c.lens_out) * c.up, c.F * c.up
    written = np.zeros((Tg, Fg), bool)
    written[c.pt :: c.up, c.pf :: c.up] = True
    # what the operator must be given: rows up to the last base position's output row
    need = 0 if c.rows == 0 else ((Tg // c.up - 1) * c.up + c.pt) * Fg + (c.F - 1) * c.up + c.pf + 1
    y = torch.from_numpy(sentinel((2 * GUARD + c.out_rows, c.ldy)) if ybuf is None else ybuf).cuda()
    r = None
    if d["res"] is not None:
        rg = sentinel((Tg, Fg, c.ldy))
        rg[written, : c.cout] = np.concatenate(d["res"]).reshape(Tg, Fg, c.cout)[written]
        r = torch.from_numpy(np.concatenate([sentinel((GUARD, c.ldy)), rg.reshape(-1, c.ldy), sentinel((GUARD, c.ldy))])).cuda()
    less = {k: (1 if short == k else 0) for k in ("x0", "x1", "y", "r")}
    fields = dict(w_host=d["w"], bias_host=d["bias"], cout=c.cout, cin0=c.cin0, cin1=c.cin1, ld0=c.ld0, ld1=c.ld1, npad=c.npad, lrelu=c.lrelu, chunk=c.chunk, sliced=c.sliced,
                  sh=c.sh, Fin=c.Fin, F=c.F, up=c.up, pt=c.pt, pf=c.pf, act=c.act, div=c.div, ldy=c.ldy)
    fields["x0"], fields["x0_elems"] = window(x0, 0, in_rows * c.ld0 - less["x0"])
    if x1 is not None:
        fields["x1"], fields["x1_elems"] = window(x1, 0, in_rows * c.ld1 - less["x1"])
    fields["y"], fields["y_elems"] = window(y, GUARD, need * c.ldy - less["y"])
    if r is not None:
        fields["r"], fields["r_elems"] = window(r, GUARD, need * c.ldy - less["r"])
    try:
        hip.op_conv2d(seg_in, seg_out, c.dt, c.df, **fields)
    finally:
        torch.cuda.synchronize()
        launch.last = (y.cpu().numpy(), None if r is None else r.cpu().numpy())
    if r is not None:  # the residual is an input
        assert same_bits(launch.last[1][GUARD : GUARD + c.out_rows].reshape(Tg, Fg, c.ldy), rg) and kept(launch.last[1][:GUARD]) and kept(launch.last[1][GUARD + c.out_rows :])
    return launch.last[0]


def grid_of(c, ybuf):
    return ybuf[GUARD : GUARD + c.out_rows].reshape(sum(c.lens_out) * c.up, c.F * c.up, c.ldy)


def check_untouched(c, ybuf, written, what):
    g = grid_of(c, ybuf)
    assert kept(ybuf[:GUARD]) and kept(ybuf[GUARD + c.out_rows :]), (what, "a guard row was written")
    assert kept(g[~written]), (what, "a position that is no output of the launch was written")
    assert (g[written][:, c.cout :].view(np.uint32) == 0).all(), (what, "columns cout .. ldy - 1 of a written row are not +0")


_BATCH = {}


def batch(hip, name):
    """The launch of case `name`, once per session -> its output grid [sum T_b up][F up][ldy] (checked: guards, unwritten positions, zero columns)."""
    if name not in _BATCH:
        c = V.CASES[name]
        ybuf = launch(hip, c, V.data(name))
        check_untouched(c, ybuf, V.expected(name)[2], name)
        _BATCH[name] = grid_of(c, ybuf)
    return _BATCH[name]


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_launch_against_float64(hip, name):
    c = V.CASES[name]
    want, bound, written = V.expected(name)
    g = batch(hip, name)
    got = g[written][:, : c.cout]
    assert np.isfinite(got).all(), name
    e = V.worst(got, want[written], bound[written])
    print(f"\n[conv2d] {name}: {c.rows} base rows, K {c.K} in chunks of {c.chunk}{' as slices' if c.sliced else ''}: {e:.3f} of the bound")
    assert e <= 1.0, (name, e, np.argwhere(np.abs(got - want[written]) > bound[written])[:3])


@pytest.mark.parametrize("kernel,slices", V.SLICED_PAIRS)
def test_grid_slices_give_the_bits_of_the_kernels_own_chunk_sums(hip, kernel, slices):
    a, b = batch(hip, kernel), batch(hip, slices)
    assert V.CASES[slices].sliced == 1 and V.CASES[kernel].sliced == 0 and V.CASES[slices].chunk == V.CASES[kernel].chunk
    assert same_bits(a, b), (kernel, float(np.nanmax(np.abs(a.astype(F64) - b))))


@pytest.mark.parametrize("name", sorted(n for n, c in V.CASES.items() if sum(1 for L in c.lens_out if L) > 1))
def test_an_utterance_alone_has_the_bits_of_its_batch(hip, name):
    c = V.CASES[name]
    g = batch(hip, name)
    off = V.offsets(c.lens_out) * c.up
    for u, L in enumerate(c.lens_out):
        if L:
            s, d = V.solo(name, u)
            alone = grid_of(s, launch(hip, s, d))
            assert same_bits(alone, g[off[u] : off[u + 1]]), (name, u)


def test_four_parities_fill_the_transposed_conv(hip):
    """After the first launch only its parity is written; after all four every position is, with the float64 transposed conv's values."""
    c0 = V.CASES[V.UP2[0]]
    ybuf = None
    seen = np.zeros(V.expected(V.UP2[0])[2].shape, bool)
    for name in V.UP2:
        c = V.CASES[name]
        ybuf = launch(hip, c, V.data(name), ybuf)
        seen |= V.expected(name)[2]
        check_untouched(c, ybuf, seen, name)
    assert seen.all()
    g = grid_of(c0, ybuf)
    for name in V.UP2:
        want, bound, written = V.expected(name)
        e = V.worst(g[written][:, : c0.cout], want[written], bound[written])
        print(f"\n[conv2d] {name} in the shared grid: {e:.3f} of the bound")
        assert e <= 1.0 and same_bits(g[written], batch(hip, name)[written]), name


def test_tiles_compared(hip):
    """The same convolution (cout 16) on the 256 x 16, 128 x 32 and 64 x 64 tiles: printed, not asserted (the header promises nothing across tiles)."""
    g = [batch(hip, f"tile_{t}_A")[:, :, :16] for t in ("n16c16", "n32c16", "n64c16")]
    _, bound, _ = V.expected("tile_n16c16_A")
    for t, h in zip(("128 x 32", "64 x 64"), g[1:]):
        d = np.abs(h.astype(F64) - g[0])
        print(f"\n[conv2d] tile {t} against 256 x 16: {'the same bits' if same_bits(h, g[0]) else f'{int((d > 0).sum())} of {d.size} elements differ, at most {float((d / bound).max()):.3f} of the bound'}")


REFUSALS = {
    "a row stride of 8": ("two_segments_s0", dict(cin0=5, cin1=5, ld0=8, ld1=8, K=144, chunk=144), None, "does not pack"),
    "ldy above npad": ("tile_n16c16_A", dict(ldy=20), None, "N <= ldy <= npad"),
    "cout above ldy": ("tile_n32c17_A", dict(ldy=16), None, "N <= ldy <= npad"),
    "a short input": ("tile_n16c16_A", {}, "x0", "x0 .* outside"),
    "a short second input": ("two_segments_s0", {}, "x1", "x1 .* outside"),
    "a short output": ("tile_n16c16_A", {}, "y", "y .* outside"),
    "a short output at parity 0": ("up2_00", {}, "y", "y .* outside"),
    "a short residual": ("epi_res", {}, "r", "r .* outside"),
    "offsets off the level's grid": ("shift2", dict(seg_lens=(12, 0, 6, 20)), None, "no multiples of 4"),  # 0, 12, 12, 18, 38 at a shift of 2, inside the buffers of 0, 12, 12, 20, 40
    "up of 3": ("up2_11", dict(up=3), None, "up 3"),
    "a parity not below up": ("tile_n16c16_A", dict(pt=1), None, "pt 1"),
    "a chunk that is no multiple of 16": ("tile_n16c16_A", dict(chunk=24), None, "chunk 24"),
    "the LeakyReLU operand off the 64 x 64 tile": ("tile_n32c17_A", dict(lrelu=1), None, "LeakyReLU operand"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refused_before_anything_is_written(hip, what):
    name, attrs, short, message = REFUSALS[what]
    c, d = V.CASES[name].replace(**attrs), dict(V.data(name))
    if "cin1" in attrs:  # the second segment cut to the narrower stride
        d["x1"] = [x[:, :, : attrs["cin1"]] for x in d["x1"]]
        d["w"] = np.ascontiguousarray(d["w"][:, : c.cin0 + c.cin1])
    with pytest.raises(RuntimeError, match="stylish_hip: .*" + message):
        launch(hip, c, d, short=short, seg_lens=attrs.get("seg_lens"))
    assert kept(launch.last[0]), (what, "a refused call wrote")

