"""The small kernels between the stages, one launch at a time against tests/glue64.py: frame_offsets, frame_token_map + gather_rows (stts_length_regulate),
frame_token_map + local_token, alignment_matrix, duration_decode, embed, broadcast_style, row_utt, the two transposes, single_channel_conv, decoder_front,
style_fc / style_fc_batch (through run_style), mean_rows and upsample4.  The entry points of the C-ABI where one exists, stts_op_glue / stts_op_chan_conv
otherwise - which launch through the functions the stages call (model.hip.h: launch_* / run_style), so grids and arguments are the product's.

Index and copy kernels are compared for equality; every output buffer is pre-filled with a canary (the quiet NaN 0x7FC0BEEF, glue64.SENTI for ints) and everything
outside what the operation owns must still hold it.  Arithmetic kernels are compared with float64 under glue64's bounds ((n + 4) 2^-24 sum|a b| + one output
rounding); -s prints the largest error as a fraction of the bound per case.  tests/test_glue64_cpu.py shows that these shapes and bounds reject sixteen kinds
of defect.

Measured on an MI355X, largest error / bound: single_channel_conv 0.001 - 0.015 with one tap, at most 0.003 with 3 and 7 (fp32, bf16 and f16
rows alike); decoder_front F0 0.15, N 0.10; run_style 0.003 - 0.021 (style_fc_kernel), 0.011 - 0.032 (style_fc_batch_kernel); mean_rows 0.093; upsample4 0.41.
"""
import ctypes as C

import numpy as np
import pytest

import glue64 as M
from oracle import stylish_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
TORCH16 = {1: "bfloat16", 2: "float16"}


@pytest.fixture(scope="module")
def hip(cfg):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)
    yield m
    m.close()


def seg_of(lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments(lengths, torch.device("cuda", 0))


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def sent(shape):
    return torch.from_numpy(M.sent(shape).copy()).cuda()


def isent(n):
    return torch.full((n,), M.SENTI, dtype=torch.int32, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def call(hip, name, *args):
    from stylish_tts_amd import _lib
    from stylish_tts_amd.runtime import _ptr, _stream

    conv = [_ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    if name in ("stts_frame_offsets", "stts_length_regulate", "stts_upsample4"):
        conv = [hip.ctx, _stream(), *conv]
    else:
        conv = [_stream(), *conv]
    _lib.check(getattr(hip.lib, name)(*conv))


def show(what, r):
    print(f"[glue] {what}: error / bound {r:.4f}")
    assert r < 1.0, (what, r)


def refused(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ frame offsets
@pytest.mark.parametrize("n_utt", M.OFFSETS_N_UTT)
def test_frame_offsets_against_int64(hip, n_utt):
    """exact capacities, several utterances over capacity at once, a capacity of 0: need, off_T and off_T4 equal the int64 sums; nothing behind them is written."""
    c = M.offsets_case(n_utt)
    tok_off, dur = dev(c["tok_off"], I32), dev(c["dur"])
    for k, caps in c["caps"].items():
        cap_off = dev(M.offsets(caps), I32)
        off_T, off_T4, need = isent(n_utt + 3), isent(n_utt + 3), isent(n_utt + 2)
        call(hip, "stts_frame_offsets", n_utt, tok_off, dur, cap_off, off_T, off_T4, need)
        off_T, off_T4, need = host(off_T), host(off_T4), host(need)
        assert M.offsets_equal(c["ref"][k], need[:n_utt], off_T[:n_utt + 1], off_T4[:n_utt + 1]), k
        assert (need[n_utt:] == M.SENTI).all() and (off_T[n_utt + 1:] == M.SENTI).all() and (off_T4[n_utt + 1:] == M.SENTI).all(), k


# ------------------------------------------------------------------------------------------------ length regulator, frame -> token map
@pytest.mark.parametrize("name", M.REGULATE_CASES)
def test_length_regulate_against_int64(hip, name):
    """ragged batches of 1 .. 1500 tokens, durations 0 .. 46, frame offsets consistent / short / long in turn, n_frames a capacity above frm_off[n_utt],
    ld_enc = C + 4, ld_out = C + 8: the gathered rows bit for bit, the canary in pad columns, in the rows past the frames and behind the map."""
    c = M.regulate_case(name)
    C_, n_buf = c["C"], c["n_frames"] + 3
    out, src = sent((n_buf, C_ + 8)), isent(n_buf)
    call(hip, "stts_length_regulate", len(c["P"]), dev(c["dur"]), dev(c["tok_off"], I32), dev(c["frm_off"], I32), C.c_int64(c["n_frames"]), c["rep"], dev(c["enc"]), C_ + 4, C_, out,
         C_ + 8, src)
    assert M.token_map_equal(c, host(src)), "frame -> token map"
    assert M.regulate_equal(c, host(out)), "gathered rows"


def test_length_regulate_refuses_a_width_that_is_no_multiple_of_4(hip):
    c = M.regulate_case("rep1_c4")
    out, src = sent((c["n_frames"], 136)), isent(c["n_frames"])
    refused("multiples of 4", call, hip, "stts_length_regulate", len(c["P"]), dev(c["dur"]), dev(c["tok_off"], I32), dev(c["frm_off"], I32), C.c_int64(c["n_frames"]), 1,
            dev(np.zeros((int(c["tok_off"][-1]), 132), F32)), 132, 130, out, 136, src)
    assert (host(src) == M.SENTI).all() and M.window_equal(host(out), np.zeros((0, 0), F32), 0, 0, 0)


@pytest.mark.parametrize("name", M.REGULATE_CASES)
def test_token_map_and_local_token_against_int64(hip, name):
    """the same grids through the pitch / energy predictor's chain: the map, and centre = the token-local index."""
    c = M.regulate_case(name)
    n_buf = c["n"] + 3
    src, centre = isent(n_buf), isent(n_buf)
    hip.op_glue(seg_of(np.diff(c["frm_off"])), tok=seg_of(c["P"]), kind=6, rep=c["rep"], dur=dev(c["dur"]), iy=src, iy2=centre)
    assert M.token_map_equal(c, host(src)) and M.local_token_equal(c, host(centre))


@pytest.mark.parametrize("P", M.ALIGN_P)
def test_alignment_matrix_against_reference(hip, P):
    c = M.alignment_case(P)
    out = sent(c["P"] * c["T"] + 5)
    call(hip, "stts_duration_to_alignment", dev(c["dur"]), c["P"], c["T"], out)
    assert M.alignment_equal(c, host(out))


def test_alignment_refuses_1025_tokens(hip):
    out = sent(1025 * 4)
    refused("at most 1024", call, hip, "stts_duration_to_alignment", dev(np.ones(1025, I32)), 1025, 4, out)
    assert (M.bits(host(out)) == M.SENT32).all()


# ------------------------------------------------------------------------------------------------ duration decode
def decode(hip, logits, ld, n_rows):
    wide = np.full((len(logits), ld), 1e4, F32)
    wide[:, :16] = logits
    out = isent(len(logits) + 2)
    call(hip, "stts_duration_decode", dev(wide), ld, n_rows, out)
    out = host(out)
    assert (out[n_rows:] == M.SENTI).all(), "written past n_rows"
    return out[:n_rows]


@pytest.mark.parametrize("scale", M.DECODE_SCALES)
def test_duration_decode_random_rows(hip, scale):
    """4096 rows; ld 16 and 32 (1e4 in the pad columns); n_rows on both sides of the 256-thread block."""
    lg = M.decode_case()["rand"][scale]
    dur, sure, _ = M.decode_ref(lg)
    assert (~sure).mean() <= 0.01
    for ld in (16, 32):
        assert M.decode_equal(dur, sure, decode(hip, lg, ld, len(lg))), ld
        for n in M.DECODE_N_ROWS:
            assert M.decode_equal(dur[:n], sure[:n], decode(hip, lg, ld, n)), (ld, n)


def test_duration_decode_ties_and_large_logits(hip):
    c = M.decode_case()
    want = O.prediction_to_duration(c["ties"]).astype(I64)
    assert tuple(want[:4]) == M.TIE_EXPECT
    got = decode(hip, c["ties"], 32, len(want))
    assert np.array_equal(got, want), (got, want)
    dur, sure, _ = M.decode_ref(c["large"])
    assert M.decode_equal(dur, sure, decode(hip, c["large"], 16, len(dur)))


# ------------------------------------------------------------------------------------------------ embed, broadcast_style, row_utt, transposes
@pytest.mark.parametrize("vocab,C_,rows", M.EMBED_CASES)
def test_embed_bit_exact(hip, vocab, C_, rows):
    c = M.embed_case(vocab, C_, rows)
    emb = dev(c["emb"])
    for key, bit in (("tokens", 0), ("bad", 2)):
        want, err = M.embed_ref(c["emb"], c[key])
        assert err == bit
        y, e = sent((rows + 1, C_ + 4)), torch.zeros(1, dtype=torch.int32, device="cuda")
        hip.op_glue(None, kind=2, n_rows=rows, C=C_, J=vocab, ldy=C_ + 4, x=emb, tokens=dev(c[key]), y=y, err=e)
        assert M.window_equal(host(y), want, rows, 0, C_), key
        assert int(host(e)[0]) == bit, key


def test_broadcast_style_bit_exact(hip):
    L, sd, col0, ldy = M.BROADCAST_LENGTHS, 64, 128, 200
    style = M.synth.normal("glue.broadcast", (len(L), sd + 4))
    R = sum(L)
    y = sent((R + 1, ldy))
    hip.op_glue(seg_of(L), kind=4, C=sd, ldx=sd + 4, ldy=ldy, col0=col0, x=dev(style), y=y)
    assert M.window_equal(host(y), style[M.row_utt_ref(L), :sd], R, col0, sd)


def test_row_utt_exact(hip):
    L = M.ROW_UTT_LENGTHS
    out = isent(sum(L) + 3)
    hip.op_glue(seg_of(L), kind=5, iy=out)
    out = host(out)
    assert np.array_equal(out[:sum(L)], M.row_utt_ref(L)) and (out[sum(L):] == M.SENTI).all()


@pytest.mark.parametrize("B,C_,T", M.TRANSPOSE_SHAPES)
def test_transposes_bit_exact(hip, B, C_, T):
    x = M.synth.normal(f"glue.transpose.{B}.{C_}.{T}", (B, C_, T))
    ld = (C_ + 31) // 32 * 32 + 32
    y = sent((B * T + 1, ld))
    call(hip, "stts_to_time_major", dev(x), B, C_, T, y, ld)
    want = np.zeros((B * T, ld), F32)  # the pad columns are written as zeros
    want[:, :C_] = x.transpose(0, 2, 1).reshape(B * T, C_)
    assert M.window_equal(host(y), want, B * T, 0, ld)
    rows = M.sent((B * T, ld)).copy()  # back: pad columns hold NaNs that must not be read
    rows[:, :C_] = want[:, :C_]
    z = sent(B * C_ * T + 3)
    call(hip, "stts_to_channel_major", dev(rows), ld, B, C_, T, z)
    z = host(z)
    assert np.array_equal(M.bits(z[:x.size]), M.bits(x.ravel())) and (M.bits(z[x.size:]) == M.SENT32).all()


# ------------------------------------------------------------------------------------------------ one-channel conv
def rows16(a, prec):
    t = dev(a)
    return t if prec == 0 else t.to(getattr(torch, TORCH16[prec]))


@pytest.mark.parametrize("prec", M.CHAN_PREC)
@pytest.mark.parametrize("ntaps", M.CHAN_NTAPS)
def test_single_channel_conv_against_float64(hip, prec, ntaps):
    """fp32, bf16 and f16 rows; one set and two sets in a launch; lengths 1 .. 100 around the wave's 8 rows and the block's 32; C = 260 gives lane 0 a second
    pass; the output is column 7 of an ldy of 12."""
    seg = seg_of(M.CHAN_LENGTHS)
    print()
    for C_ in M.CHAN_C:
        c = M.chan_case(prec, ntaps, C_)
        R = c["R"]
        xs = [rows16(s["x"], prec) for s in c["sets"]]
        if prec:
            assert all(np.array_equal(host(x.float()), s["x"]) for x, s in zip(xs, c["sets"]))  # the 16-bit rows hold the reference's values
        ws = [dev(s["w"]) for s in c["sets"]]
        common = dict(prec16=prec, ntaps=ntaps, C=C_, ldx=c["ldx"], ldy=M.CHAN_LDY, ycol=M.CHAN_YCOL)
        for nsets in (1, 2):
            ys = [sent((R + 1, M.CHAN_LDY)) for _ in range(2)]
            if nsets == 1:  # the second set alone, as set 0 of its launch
                hip.op_chan_conv(seg, nsets=1, x0=xs[1], w0=ws[1], bias0=c["sets"][1]["bias"], y0=ys[1], **common)
            else:
                hip.op_chan_conv(seg, nsets=2, x0=xs[0], w0=ws[0], bias0=c["sets"][0]["bias"], y0=ys[0], x1=xs[1], w1=ws[1], bias1=c["sets"][1]["bias"], y1=ys[1], **common)
            for i in range(2 - nsets, 2):
                y = host(ys[i])
                assert (M.bits(np.delete(y, M.CHAN_YCOL, axis=1)) == M.SENT32).all() and (M.bits(y[R:]) == M.SENT32).all(), "written outside the output column"
                show(f"single_channel_conv prec {prec} taps {ntaps} C {C_} sets {nsets} set {i}", M.chan_ratio(c, i, y[:R, M.CHAN_YCOL]))
            if nsets == 1:
                assert (M.bits(host(ys[0])) == M.SENT32).all()


def test_single_channel_conv_refusals(hip):
    c = M.chan_case(0, 3, 64)
    seg, R = seg_of(M.CHAN_LENGTHS), c["R"]
    s = c["sets"][0]
    y = sent((R, M.CHAN_LDY))
    ok = dict(nsets=1, prec16=0, ntaps=3, C=64, ldx=c["ldx"], ldy=M.CHAN_LDY, ycol=M.CHAN_YCOL, x0=dev(s["x"]), w0=dev(s["w"]), y0=y)
    refused("kernel size", hip.op_chan_conv, seg, **{**ok, "ntaps": 9, "w0": dev(np.zeros((9, 64), F32))})
    refused("kernel size", hip.op_chan_conv, seg, **{**ok, "ntaps": 2})
    refused("multiples of 4", hip.op_chan_conv, seg, **{**ok, "C": 62})
    refused("set 0", hip.op_chan_conv, seg, **{**ok, "x0": dev(s["x"][:-1])})
    refused("set 0", hip.op_chan_conv, seg, **{**ok, "y0": y[:-1]})
    refused("set 1", hip.op_chan_conv, seg, **{**ok, "nsets": 2})
    refused("ycol", hip.op_chan_conv, seg, **{**ok, "ycol": M.CHAN_LDY})
    assert (M.bits(host(y)) == M.SENT32).all()


# ------------------------------------------------------------------------------------------------ decoder front
def test_decoder_front_against_float64(hip):
    """lengths 1, 2, 3, 64, 257; distinct F0 / N filters: the encoding copied bit for bit, F0 / N within the 3-term bound at every row (both edges of every
    utterance included), zeros behind them, the first 576 columns of the concat buffers and the rows past the batch untouched."""
    c, f = M.front_case(), M.FRONT
    R = c["R"]
    enc_in, xa, xb = sent((R + 1, f["ld_enc"])), sent((R + 1, f["ld_x"])), sent((R + 1, f["ld_x"]))
    hip.op_glue(seg_of(M.FRONT_LENGTHS), kind=0, wf=M.FRONT_WF, wn=M.FRONT_WN, bf=M.FRONT_BF, bn=M.FRONT_BN, C=f["C"], ldx=f["ld_asr"], ldy=f["ld_enc"], ld2=f["ld_x"],
                c_hidden=f["c_hidden"], c_res=f["c_res"], x=dev(c["asr"]), x2=dev(c["pitch"]), x3=dev(c["energy"]), y=enc_in, y2=xa, y3=xb)
    r = M.front_check(c, host(enc_in), host(xa), host(xb))
    assert r["exact"], "copied columns, zeros or untouched regions"
    print()
    show("decoder_front F0", r["f0"])
    show("decoder_front N", r["n"])


# ------------------------------------------------------------------------------------------------ style projection
@pytest.mark.parametrize("K", M.STYLE_K)
@pytest.mark.parametrize("J", M.STYLE_J)
def test_run_style_against_float64(hip, K, J):
    """n_utt 1 .. 130: style_fc_kernel below 16 utterances, style_fc_batch_kernel from 16 on (one, two and three 64-lane passes)."""
    c = M.style_case(K, J)
    worst = {}
    for n_utt in M.STYLE_N_UTT:
        y = sent((n_utt + 1, c["ld"]))
        hip.op_glue(None, kind=1, n_utt=n_utt, J=J, K=K, ldy=c["ld"], w_host=c["W"], b_host=c["b"], x=dev(c["s"][:n_utt]), y=y)
        exact, r = M.style_check(c, n_utt, host(y))
        assert exact, ("pad columns or the row behind", n_utt)
        assert r < 1.0, (n_utt, r)
        k = "style_fc_kernel" if n_utt < 16 else "style_fc_batch_kernel"
        worst[k] = max(worst.get(k, 0.0), r)
    print()
    for k, r in worst.items():
        show(f"run_style K {K} J {J} {k}", r)


def test_run_style_refuses_a_table_wider_than_128(hip):
    """both style kernels cover K <= 128: a wider table is an error, not a projection of its first 128 columns."""
    for K, n_utt in ((132, 2), (256, 17)):
        y = sent((n_utt, 8))
        refused("style table of K", hip.op_glue, None, kind=1, n_utt=n_utt, J=8, K=K, ldy=8, w_host=np.ones((8, K), F32), b_host=np.zeros(8, F32),
                x=dev(np.ones((n_utt, K), F32)), y=y)
        assert (M.bits(host(y)) == M.SENT32).all()


# ------------------------------------------------------------------------------------------------ mean over rows, upsample
@pytest.mark.parametrize("C_", M.MEAN_C)
def test_mean_rows_against_float64(hip, C_):
    c = M.mean_case(C_)
    n = len(M.MEAN_LENGTHS)
    y = sent((n + 1, C_ + 2))
    hip.op_glue(seg_of(M.MEAN_LENGTHS), kind=3, C=C_, ldx=C_ + 6, ldy=C_ + 2, x=dev(c["x"]), y=y)
    y = host(y)
    assert (M.bits(y[n:]) == M.SENT32).all() and (M.bits(y[:, C_:]) == M.SENT32).all()
    print()
    show(f"mean_rows C {C_}", M.mean_ratio(c, y[:n, :C_]))


def test_upsample4_against_float64(hip):
    """T = 1, 2, 3, 255, 256, 257 and a zero-length utterance between two others."""
    c = M.upsample_case()
    L = M.UPSAMPLE_LENGTHS
    seg, seg4 = seg_of(L), seg_of([4 * t for t in L])
    y = sent(4 * c["R"] + 3)
    call(hip, "stts_upsample4", len(L), seg.host_ptr, seg.dev, seg4.dev, dev(c["x"]), y)
    y = host(y)
    assert (M.bits(y[4 * c["R"]:]) == M.SENT32).all()
    print()
    show("upsample4", M.upsample_ratio(c, y[:4 * c["R"]]))
