"""Every form the AdaptiveDecoderBlock plan can take (csrc/adain_block.hip.h plan_adain_block / plan_adain_chain), one at a time through stts_op_adain_chain with the
plan's thresholds brought down to a ~620-row batch, against tests/block64.py: the float64 restatement of the reference block with the engine's rounding
points.  Every test first asserts that the form it names is the form that ran (the plan the operator returns), then holds every utterance of every block's
output to block64's bars (FOUR x the error of a plain fp32 / rounded evaluation on the same inputs; block64.py BOUNDS), and checks that pad columns stay
zero, that the rows behind y and y16 are untouched and that the result is finite.  Forms that must agree bit for bit are compared with torch.equal.

A pair A -> B is checked block by block: B against block64 of the input B actually read (the y of A that this run wrote, next to the constant columns), so
A's error does not count twice.  The thresholds themselves (3 840 / 4 096 / 4 097 rows in the 16-bit modes) are run through stts_decoder_forward at the end.

Widths: 130 -> 512 (kcin 160 / 192), 578 -> 512 (the decoder's 66 constant columns), identity 512 -> 512 (block64.WIDTHS says why not narrower).
Measured ratios (worst error / bar): DESIGN.md 4, "The forms against float64"."""
from functools import lru_cache

import numpy as np
import pytest

import block64 as B

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FOLD, APPLY, WINO, BRIDGED = range(4)            # BlockConv
PASS, EPILOGUE, STAT_WINO, STAT_BRIDGE = range(4)  # StatFrom
IDENTITY, SEGMENT, STREAM, SIDE = range(4)       # ShortcutAt
Y16_NONE, Y16_EPILOGUE, Y16_CAST = range(3)      # Y16By
LENS = tuple(B.LENGTHS)
# conv_gemm16_kernel (the statistics epilogue) takes a launch of at least 192 tiles of 256 rows x 256 channels, i.e. 96 utterances at 512 channels however short
MANY = tuple(B.LENGTHS[i % 7] for i in range(100))
SMALL = (1, 5, 6, 7, 23, 24)  # 66 rows: a launch-bound batch, where the folded contractions split K
CANARY, CANARY16, GUARD = 12345.0, 0x7B7B, 8
PRECS = {"f32": None, "f32_native": None, "bf16": "bf16", "f16": "f16"}
RATIOS = []  # (test, precision, block, ratio) of everything this module compared; printed at the end of the module


@pytest.fixture(scope="module")
def models(cfg, weights):
    from stylish_tts_amd.runtime import HipModel

    made = {}

    def get(prec):
        if prec not in made:
            m = HipModel(cfg, 0, precision=prec)
            m.load_weights({"speech_predictor": weights["speech_predictor"]}, which=7)
            for name in B.WIDTHS:
                m.load_state_dict("", B.weights(name)[0])
            made[prec] = m
        return made[prec]

    yield get
    for m in made.values():
        m.close()
    for r in RATIOS:
        print("ratio", *r)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def segs(lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments(list(lengths), torch.device("cuda", 0))


@lru_cache(maxsize=None)
def data(name, lengths):
    return B.inputs(name, lengths, B.WIDTHS[name][0])


@lru_cache(maxsize=None)
def ref_of(name, lengths, mode, conv):
    x, style = data(name, lengths)
    w, p = B.weights(name)
    return B.reference(x, lengths, style, w, p, mode, conv, name=name)


_REF_B = {}


def ref_of_input(name, x, lengths, style, mode, conv):
    """reference of a block on an input that a run produced (cached by its bytes: forms that agree bit for bit share it)."""
    key = (name, mode, conv, hash(x.tobytes()))
    if key not in _REF_B:
        w, p = B.weights(name)
        _REF_B[key] = B.reference(x, lengths, style, w, p, mode, conv)
    return _REF_B[key]


def run(hip, prec, names, lengths, y16=False, ldx_extra=0, prefixes=None, **kw):
    """One block or a pair through the operator.  -> dict(plan, blocks = [plan], y = [numpy [rows, cout]], y16 = [bits or None], raw tensors for torch.equal)."""
    mode = PRECS[prec]
    al = 64 if mode else 32
    rows = int(sum(lengths))
    s = segs(lengths)
    x, style = data(names[0], lengths)
    cin0 = B.WIDTHS[names[0]][0]
    ldx = (cin0 + al - 1) // al * al + ldx_extra
    xp = np.zeros((rows, ldx), np.float32)
    xp[:, :cin0] = x
    blocks, bufs = [], []
    for i, n in enumerate(names):
        cin, cout = B.WIDTHS[n]
        last = i == len(names) - 1
        ldy = cout + 32 if last else (B.WIDTHS[names[i + 1]][0] + al - 1) // al * al
        full = torch.full((rows + GUARD, ldy), CANARY, dtype=torch.float32, device="cuda")
        full[:rows] = 0
        if not last:  # the constant columns of the next block's input
            cst, _ = B.inputs("cst", lengths, B.WIDTHS[names[i + 1]][0] - cout)
            full[:rows, cout : cout + cst.shape[1]] = dev(cst)
        b = dict(prefix=prefixes[i] if prefixes else B.weights(n)[1], cin=cin, cout=cout, y=full[:rows])
        f16 = None
        if y16 and mode:
            f16 = torch.full((rows + GUARD, ldy), CANARY16, dtype=torch.int16, device="cuda")
            b["y16"] = f16[:rows]
        blocks.append(b)
        bufs.append((full, f16, cout))
    chain, plans = hip.op_adain_chain(s, dev(xp), dev(style), blocks, **kw)
    torch.cuda.synchronize()
    out = dict(plan=chain, blocks=plans, y=[], y16=[], raw=[f[0] for f in bufs], x=[x], style=style, lengths=lengths, mode=mode)
    for i, (full, f16, cout) in enumerate(bufs):
        a = full.cpu().numpy()
        assert (a[rows:] == np.float32(CANARY)).all(), (names[i], "rows behind y were written")
        last = i == len(names) - 1
        if last:
            assert (a[:rows, cout:] == 0).all(), (names[i], "pad columns of y are not zero")
        else:
            cst, _ = B.inputs("cst", lengths, B.WIDTHS[names[i + 1]][0] - cout)
            assert np.array_equal(a[:rows, cout : cout + cst.shape[1]], cst) and (a[:rows, cout + cst.shape[1] :] == 0).all(), (names[i], "constant / pad columns of y changed")
            out["x"].append(np.ascontiguousarray(a[:rows, : B.WIDTHS[names[i + 1]][0]]))
        assert np.isfinite(a[:rows]).all(), (names[i], "non-finite output")
        out["y"].append(a[:rows, :cout])
        if f16 is not None:
            h = f16.cpu().numpy().view(np.uint16)
            assert (h[rows:] == CANARY16).all(), (names[i], "rows behind y16 were written")
            out["y16"].append(h[:rows, :cout])
        else:
            out["y16"].append(None)
    return out


def hold(test, prec, names, r, conv="direct"):
    """every block of a run against block64; records the ratios."""
    for i, n in enumerate(names):
        if i == 0:
            want, bars = ref_of(n, r["lengths"], r["mode"], conv)
        else:
            want, bars = ref_of_input(n, r["x"][i], r["lengths"], r["style"], r["mode"], conv)
        ratio = B.ratios(r["y"][i], want, r["lengths"], bars)
        RATIOS.append((test, prec, n, ratio))
        print(f"{test} {prec} {n}: error / bar {ratio}")
        assert B.within(ratio), (test, prec, n, ratio)
        if r["y16"][i] is not None:  # the rounded copy: round-to-nearest-even of the y this run wrote, bit for bit
            assert np.array_equal(r["y16"][i], B.to_bits16(r["y"][i], r["mode"])), (test, prec, n, "y16 is not round(y)")


def planned(r, i, **want):
    got = {k: r["blocks"][i][k] for k in want}
    assert got == want, (i, r["blocks"][i], r["plan"])


def same(a, b):
    for ta, tb in zip(a["raw"], b["raw"]):
        assert torch.equal(ta, tb)


F32 = ["f32", "f32_native"]
H16 = ["bf16", "f16"]
BIG = 1 << 20


# ------------------------------------------------------------------------------------------------ fp32 forms
@pytest.mark.parametrize("name", ["enc", "dec", "id"])
@pytest.mark.parametrize("prec", F32)
def test_fold_fold(models, prec, name):
    r = run(models(prec), prec, [name], LENS, fold_rows=BIG, wino=True, stats=True)
    planned(r, 0, conv1=FOLD, conv2=FOLD, norm1=PASS, norm2=PASS, rows16=0, shortcut=IDENTITY if name == "id" else SEGMENT, take_pending=1, affine_serial=0)
    hold("fold", prec, [name], r)


@pytest.mark.parametrize("prec", F32)
def test_one_row_batch(models, prec):
    r = run(models(prec), prec, ["enc"], (1,), fold_rows=BIG)
    planned(r, 0, conv1=FOLD, conv2=FOLD)
    hold("fold, 1 row", prec, ["enc"], r)
    r = run(models(prec), prec, ["enc"], (1,), fold_rows=0, wino=True)
    planned(r, 0, conv1=WINO, conv2=WINO)
    hold("winograd, 1 row", prec, ["enc"], r, "wino")


@pytest.mark.parametrize("prec", F32)
def test_fold_deferred_reduce_equals_own_reduce(models, prec):
    """conv1's split-K reduce is always finished by norm2's statistics launch; with `defer` conv2's is finished by the next block's norm1 statistics launch
    (block A) or by the chain at its end (block B)."""
    hip = models(prec)
    for lens in (SMALL, LENS):
        a = run(hip, prec, ["enc", "dec"], lens, fold_rows=BIG, defer=True)
        b = run(hip, prec, ["enc", "dec"], lens, fold_rows=BIG, defer=False)
        for i in (0, 1):
            planned(a, i, conv1=FOLD, conv2=FOLD, defer_conv2=1, take_pending=1)
            planned(b, i, conv1=FOLD, conv2=FOLD, defer_conv2=0, take_pending=1, pending=0)
        print(f"deferred reduce {prec} {sum(lens)} rows: split-K factors left pending", [p["pending"] for p in a["blocks"]])
        # the folded contractions split K at both sizes: a reduce really was left to the next block's statistics launch and to the chain's end
        assert a["blocks"][0]["pending"] >= 2 and a["blocks"][1]["pending"] >= 2, a["blocks"]
        same(a, b)
        hold(f"fold, deferred reduce, {sum(lens)} rows", prec, ["enc", "dec"], a)


@pytest.mark.parametrize("how", ["force_tile", "no_scratch"])
@pytest.mark.parametrize("prec", F32)
def test_apply_apply(models, prec, how):
    kw = dict(force_tile=4, wino=True) if how == "force_tile" else dict(wino=False)
    for name in ("enc", "id"):
        r = run(models(prec), prec, [name], LENS, fold_rows=0, **kw)
        planned(r, 0, conv1=APPLY, conv2=APPLY, norm1=PASS, norm2=PASS, rows16=0, shortcut=IDENTITY if name == "id" else SEGMENT, force_tile=kw.get("force_tile", 0))
        hold(f"apply ({how})", prec, [name], r)


@pytest.mark.parametrize("name", ["enc", "dec", "id"])
@pytest.mark.parametrize("prec", F32)
def test_winograd_own_statistics(models, prec, name):
    r = run(models(prec), prec, [name], LENS, fold_rows=0, wino=True, stats=False)
    planned(r, 0, conv1=WINO, conv2=WINO, norm1=PASS, norm2=PASS, next_norm1=PASS, shortcut=IDENTITY if name == "id" else STREAM, bridge_w=0)
    hold("winograd, own statistics", prec, [name], r, "wino")


@pytest.mark.parametrize("prec", F32)
def test_winograd_chain_statistics_and_bridge(models, prec):
    """STAT_WINO through two blocks (block B's norm1 merges the statistics block A's output transform left with those of the constant columns), and the same
    pair bridged: equal bit for bit."""
    hip = models(prec)
    a = run(hip, prec, ["enc", "dec"], LENS, fold_rows=0, wino=True, stats=True, bridge=0)
    assert a["plan"]["wino_stats"] == 1 and a["plan"]["bridge_w"] == 0, a["plan"]
    planned(a, 0, conv1=WINO, conv2=WINO, norm1=PASS, norm2=STAT_WINO, next_norm1=STAT_WINO, shortcut=STREAM)
    planned(a, 1, conv1=WINO, conv2=WINO, norm1=STAT_WINO, norm2=STAT_WINO, next_norm1=PASS, shortcut=STREAM)
    hold("winograd, chain statistics", prec, ["enc", "dec"], a, "wino")
    b = run(hip, prec, ["enc", "dec"], LENS, fold_rows=0, wino=True, stats=True, bridge=1)
    assert b["plan"]["bridge_w"] == 16, b["plan"]
    planned(b, 0, conv1=WINO, conv2=BRIDGED, norm2=STAT_BRIDGE, next_norm1=STAT_BRIDGE, bridge_w=16)
    planned(b, 1, conv1=BRIDGED, conv2=BRIDGED, norm1=STAT_BRIDGE, norm2=STAT_BRIDGE, next_norm1=PASS, bridge_w=16)
    hold("bridged", prec, ["enc", "dec"], b, "wino")
    same(a, b)


@pytest.mark.parametrize("prec", F32)
def test_conv2_direct_with_the_shortcut_as_a_segment(models, prec):
    r = run(models(prec), prec, ["enc"], LENS, fold_rows=0, wino=True, no_wino_conv2sc=True)
    planned(r, 0, conv1=WINO, conv2=APPLY, shortcut=SEGMENT)
    hold("winograd conv1, direct conv2 + segment", prec, ["enc"], r, "wino")


@pytest.mark.parametrize("prec", F32)
def test_shortcut_on_the_stream_equals_the_side_lane(models, prec):
    hip = models(prec)
    a = run(hip, prec, ["enc", "dec"], LENS, fold_rows=0, wino=True, side=True, sc_side_min_rows=BIG)
    b = run(hip, prec, ["enc", "dec"], LENS, fold_rows=0, wino=True, side=True, sc_side_min_rows=0)
    assert a["plan"]["side"] == 0 and b["plan"]["side"] == 1
    for i in (0, 1):
        planned(a, i, conv1=WINO, conv2=WINO, shortcut=STREAM)
        planned(b, i, conv1=WINO, conv2=WINO, shortcut=SIDE)
    same(a, b)
    hold("shortcut on the side lane", prec, ["enc", "dec"], b, "wino")


@pytest.mark.parametrize("prec", F32)
def test_affine_serial_against_the_lane_merge(models, prec):
    hip = models(prec)
    for kw, conv in ((dict(fold_rows=BIG), "direct"), (dict(fold_rows=0, wino=True), "wino")):
        r = run(hip, prec, ["enc"], LENS, affine_serial=True, **kw)
        planned(r, 0, affine_serial=1, conv1=FOLD if conv == "direct" else WINO)
        hold(f"affine_serial ({conv})", prec, ["enc"], r, conv)


# ------------------------------------------------------------------------------------------------ 16-bit forms
@pytest.mark.parametrize("name", ["enc", "dec", "id"])
@pytest.mark.parametrize("prec", H16)
def test_fold_on_fp32_rows_in_the_window(models, prec, name):
    """rows16 <= rows <= the 16-bit fold limit, 16-bit scratch offered: the window that used to plan 16-bit rows under folded contractions.  fp32 rows, the
    learned shortcut a segment on x, the rounded y from a cast pass."""
    r = run(models(prec), prec, [name], LENS, y16=True, rows16=100, fold16_rows=BIG, xs16=True, stats=True, wino=True)
    assert r["plan"]["rows16"] == 0, r["plan"]
    planned(r, 0, conv1=FOLD, conv2=FOLD, rows16=0, cast_x16=0, shortcut=IDENTITY if name == "id" else SEGMENT, y16=Y16_CAST, norm1=PASS, norm2=PASS)
    hold("fold, fp32 rows (window)", prec, [name], r)


@pytest.mark.parametrize("name", ["enc", "dec", "id"])
@pytest.mark.parametrize("prec", H16)
def test_rows16_own_statistics(models, prec, name):
    code = 1 if prec == "bf16" else 2
    r = run(models(prec), prec, [name], LENS, y16=True, rows16=100, fold16_rows=0, xs16=True, stats=True, no_stat_fuse=True)
    planned(r, 0, conv1=APPLY, conv2=APPLY, rows16=code, norm1=PASS, norm2=PASS, next_norm1=PASS, cast_x16=0 if name == "id" else 1,
            shortcut=IDENTITY if name == "id" else SEGMENT, y16=Y16_EPILOGUE)
    hold("16-bit rows, own statistics", prec, [name], r)


@pytest.mark.parametrize("prec", H16)
def test_rows16_statistics_from_the_epilogues(models, prec):
    code = 1 if prec == "bf16" else 2
    r = run(models(prec), prec, ["enc", "dec"], MANY, y16=True, rows16=100, fold16_rows=0, xs16=True, stats=True)
    assert r["plan"]["rows16"] == 1 and r["plan"]["stats"] == 1, r["plan"]
    planned(r, 0, conv1=APPLY, conv2=APPLY, rows16=code, norm1=PASS, norm2=EPILOGUE, next_norm1=EPILOGUE, cast_x16=1, y16=Y16_EPILOGUE, shortcut=SEGMENT)
    planned(r, 1, conv1=APPLY, conv2=APPLY, rows16=code, norm1=EPILOGUE, norm2=EPILOGUE, cast_x16=0, shortcut=SEGMENT)
    hold("16-bit rows, epilogue statistics", prec, ["enc", "dec"], r)


@pytest.mark.parametrize("why", ["ldx", "no_xs16"])
@pytest.mark.parametrize("prec", H16)
def test_refusals_fall_back_to_fp32_rows(models, prec, why):
    kw = dict(ldx_extra=4, xs16=True) if why == "ldx" else dict(xs16=False)
    r = run(models(prec), prec, ["enc"], LENS, rows16=100, fold16_rows=0, **kw)
    planned(r, 0, conv1=APPLY, conv2=APPLY, rows16=0, cast_x16=0, shortcut=SEGMENT)
    hold(f"refusal ({why})", prec, ["enc"], r)


# ------------------------------------------------------------------------------------------------ the real thresholds, through stts_decoder_forward
def decoder_case(rows, ragged):
    from stylish_tts_amd import synth

    lens = [rows - 3 * (rows // 4)] + [rows // 4] * 3 if not ragged else [rows - 3071, 1531, 1100, 440]
    assert sum(lens) == rows and min(lens) > 0
    per = [dict(asr=synth.normal(f"thr.asr{i}", (1, 128, L)), pitch=synth.pitch_curve(f"thr.p{i}", 1, L), energy=(synth.uniform(f"thr.e{i}", (1, L)) * 2 + 2).astype(np.float32),
                style=(synth.normal(f"thr.s{i}", (1, 64)) * 0.7).astype(np.float32)) for i, L in enumerate(lens)]
    return lens, per


_DEC = {}


def decoder_bar(i, p, w, mode):
    """cached by utterance (index and length name its data)"""
    key = (i, p["asr"].shape[2], mode)
    if key not in _DEC:
        _DEC[key] = _decoder_bar(p, w, mode)
    return _DEC[key]


def _decoder_bar(p, w, mode):
    return B.decoder_reference(p["asr"], p["pitch"], p["energy"], p["style"], w, mode)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("rows", [3840, 4096, 4097])
@pytest.mark.parametrize("prec", H16)
def test_decoder_at_the_16bit_thresholds(models, weights, prec, rows, ragged):
    """3 840 and 4 096 rows are the two edges of the window (folded: fp32 rows, no 16-bit copies), 4 097 the first 16-bit-row form.  The plan is read through the
    operator on the same Seg with no thresholds given (the engine's own); the decoder's output is held per utterance (first, middle, last) to decoder64."""
    hip, mode = models(prec), PRECS[prec]
    w = weights["speech_predictor"]
    lens, per = decoder_case(rows, ragged)
    s = segs(lens)
    # (no threshold given: the operator takes block_switches(); the blocks are the decoder's own first two)
    r = run(hip, prec, ["enc", "dec"], tuple(lens), y16=True, wino=True, stats=True, xs16=True, side=True, defer=True, bridge=-1,
            prefixes=["speech_predictor.decoder.encode", "speech_predictor.decoder.decode.0"])
    code = 1 if prec == "bf16" else 2
    for i in (0, 1):
        if rows <= 4096:
            planned(r, i, conv1=FOLD, conv2=FOLD, rows16=0, cast_x16=0, shortcut=SEGMENT)
        else:
            planned(r, i, conv1=APPLY, conv2=APPLY, rows16=code, shortcut=SEGMENT)
    assert r["plan"]["rows16"] == (0 if rows <= 4096 else 1), r["plan"]
    cat = lambda k: np.concatenate([p[k][0].T if p[k].ndim == 3 else p[k][0] for p in per])  # noqa: E731
    x = hip.decoder(s, dev(cat("asr")), dev(cat("pitch")), dev(cat("energy")), dev(np.concatenate([p["style"] for p in per]))).cpu().numpy()
    assert np.isfinite(x).all()
    for i in (0, len(lens) // 2, len(lens) - 1):
        want, bars, ref, e = decoder_bar(i, per[i], w, mode)
        got = x[s.host[i] : s.host[i + 1], :512]
        ratio = B.ratios(got, want, [lens[i]], bars)
        ex = float(B.utt_errors(got, ref, [lens[i]]).max())
        print(f"decoder {prec} {rows} rows utterance {i}: against the rounded oracle {ex:.2e}, (FOUR + 1) x the oracle's own error {(B.FOUR + 1) * e:.2e}")
        assert ex <= (B.FOUR + 1) * e, (prec, rows, i, ex, e)
        RATIOS.append((f"decoder {rows} rows{' ragged' if ragged else ''}", prec, f"utt {i}", ratio))
        print(f"decoder {prec} {rows} rows utterance {i}: error / bar {ratio}")
        assert B.within(ratio), (prec, rows, i, ratio)
