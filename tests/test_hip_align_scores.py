"""The alignment, duration and CFM validation scores on the engine (csrc/aligner.hip.h: ctc_forward_kernel and the two reductions beside it;
csrc/val_scores.hip.h: the duration and difference sums) against the float64 oracle of tests/ctc64.py, which tests/test_ctc64_cpu.py pins against
torch's float64 ctc_loss and the recorded reference run of DurationLoss.

ctc_nll's bound is derived, not tuned: log-sum-exp is 1-Lipschitz, so the per-step roundings of |alpha| <= |nll| add at most linearly, in the kernel
and in the oracle alike: |nll - nll64| <= 16 T 2^-53 max(1, |nll64|), and the fp32 roundings of the two are equal or adjacent.  The other sums are
held to the project's standing bar: the engine's error against float64 is at most 4 x the error of torch's fp32 run (or the reference's recorded
fp32 run) on the same inputs; where that fp32 run has no error, the fp32 roundings must agree.  Every test prints the ratio it measured."""
import os

import numpy as np
import pytest

import ctc64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
V, LD, TOKENS = 179, 192, 178
BAR = 4.0
CANARY = 777.0

_STATE = {}


def engine():
    from stylish_tts_amd.runtime import HipModel

    if "eng" not in _STATE:
        _STATE["eng"] = HipModel(None, 0)
    return _STATE["eng"]


def seg_of(lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments([int(n) for n in lengths], engine().device)


def padded_rows(lps):
    """[sum T, LD] on the device: the utterances' [T, V] rows one after the other, NaN in the pad columns."""
    x = np.full((sum(lp.shape[0] for lp in lps), LD), np.nan, np.float32)
    x[:, :V] = np.concatenate(lps)
    return torch.from_numpy(x).to(engine().device)


def run_nll(cases, blank, priors=None, scale=0.0):
    """cases: [(lp [T, V] float32, tokens)] -> the engine's [B] float64 values on the host."""
    lps, tks = [c[0] for c in cases], [c[1] for c in cases]
    tg = torch.tensor([v for tk in tks for v in tk], dtype=torch.int32)
    pr = None if priors is None else torch.from_numpy(priors)
    out = engine().ctc_nll(seg_of([lp.shape[0] for lp in lps]), padded_rows(lps), seg_of([len(tk) for tk in tks]), tg, blank, log_priors=pr, prior_scale=scale, classes=V)
    assert out.dtype == torch.float64 and out.shape == (len(cases),)
    return out.cpu().numpy()


def adjacent_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, np.float32(np.inf)) == b or np.nextafter(a, np.float32(-np.inf)) == b


def check_nll(name, got, lp, tk, blank, priors=None, scale=0.0):
    ref = ctc64.ctc_nll(lp, tk, blank, priors, scale)
    T = lp.shape[0]
    bound = 16 * T * 2.0**-53 * max(1.0, abs(ref))
    print(f"{name}: T {T} P {len(tk)} engine {got!r} float64 {ref!r} |diff| {abs(got - ref):.3e} = {abs(got - ref) / bound:.4f} of the bound {bound:.3e}")
    assert np.isfinite(ref) and abs(got - ref) <= bound and adjacent_f32(got, ref), (name, got, ref)
    return abs(got - ref) / bound


def against_fp32(name, mine, f64, f32):
    """The standing bar, element by element: |mine - f64| <= 4 |f32 - f64|, or equal fp32 roundings where the fp32 run has no error."""
    mine, f64, f32 = np.atleast_1d(np.asarray(mine, np.float64)), np.atleast_1d(np.asarray(f64, np.float64)), np.atleast_1d(np.asarray(f32, np.float64))
    err, ref = np.abs(mine - f64), np.abs(f32 - f64)
    ok = (err <= BAR * ref) | ((ref == 0) & (mine.astype(np.float32) == f64.astype(np.float32)))
    ratio = (err[ref > 0] / ref[ref > 0]).max() if (ref > 0).any() else 0.0
    print(f"{name}: engine max err {err.max():.3e}, fp32 run max err {ref.max():.3e}, worst ratio {ratio:.3e} (bar {BAR}), {int((ref == 0).sum())} of {ref.size} held to equal fp32 roundings")
    assert ok.all(), (name, mine[~ok], f64[~ok], f32[~ok])


def aligner_fixture(name):
    g = np.load(os.path.join(GOLD, f"aligner_{name}.npz"))
    return g[f"{name}_lp32"][0].astype(np.float32), [int(v) for v in g[f"{name}_targets"]]


def small_cases(blank=TOKENS):
    """(name, lp, tokens): the small shapes, with adjacent equal tokens; token ids avoid the blank."""
    lo = 1 if blank == 0 else 0
    mk = lambda seed, P, pairs=0: [t + lo for t in ctc64.make_tokens(seed, P, symbols=TOKENS - lo, equal_pairs=pairs)]  # noqa: E731
    out = [("T1 P1", ctc64.make_log_probs(11, 1), mk(21, 1)), ("T3 P1", ctc64.make_log_probs(12, 3), mk(22, 1)), ("T3 P2 equal", ctc64.make_log_probs(13, 3), mk(23, 2, 1)),
           ("T40 P14 three pairs", ctc64.make_log_probs(14, 40), mk(24, 14, 3))]
    assert out[2][2][0] == out[2][2][1] and ctc64.min_frames(out[3][2]) == 17
    return out


# ------------------------------------------------------------------------------------------------ ctc_nll
@pytest.mark.parametrize("blank", [TOKENS, 0])
def test_ctc_nll_small_shapes_ragged_equals_solo(blank):
    cases = small_cases(blank)
    batch = run_nll([(lp, tk) for _, lp, tk in cases], blank)
    again = run_nll([(lp, tk) for _, lp, tk in cases], blank)
    assert batch.tobytes() == again.tobytes()
    worst = 0.0
    for i, (name, lp, tk) in enumerate(cases):
        solo = run_nll([(lp, tk)], blank)
        assert solo.tobytes() == batch[i : i + 1].tobytes(), name
        worst = max(worst, check_nll(f"blank {blank} {name}", batch[i], lp, tk, blank))
    print(f"worst ratio to the bound: {worst:.4f}")


def test_ctc_nll_aligner_fixtures():
    cases = [aligner_fixture("t40"), aligner_fixture("t100")]
    got = run_nll(cases, TOKENS)
    for name, (lp, tk), v in zip(("t40", "t100"), cases, got):
        check_nll(name, v, lp, tk, TOKENS)
        assert run_nll([(lp, tk)], TOKENS)[0] == v


def test_ctc_nll_one_path_is_its_sum_and_one_frame_fewer_is_inf():
    tk = ctc64.make_tokens(31, 14, equal_pairs=3)
    need = ctc64.min_frames(tk)
    lp = ctc64.make_log_probs(32, need)
    got = run_nll([(lp, tk), (lp[:-1], tk), (lp, tk[:5])], TOKENS)
    assert got[0] == ctc64.single_path_nll(lp, tk, TOKENS) == ctc64.ctc_nll(lp, tk, TOKENS)
    assert got[1] == np.inf and ctc64.ctc_nll(lp[:-1], tk, TOKENS) == np.inf
    assert not np.isnan(got).any()
    check_nll("neighbour of the infeasible utterance", got[2], lp, tk[:5], TOKENS)


@pytest.mark.parametrize("P", [510, 509])
def test_ctc_nll_every_state(P):
    tk = ctc64.make_tokens(40 + P, P)
    lp = ctc64.make_log_probs(41 + P, 520)
    short = (ctc64.make_log_probs(43, 5), [3, 3])
    got = run_nll([short, (lp, tk)], TOKENS)  # the long utterance second: its offsets are not zero
    check_nll(f"P {P}", got[1], lp, tk, TOKENS)
    check_nll("its neighbour", got[0], short[0], short[1], TOKENS)
    assert run_nll([(lp, tk)], TOKENS)[0] == got[1]


def test_ctc_nll_rows_with_minus_inf_and_huge_negatives():
    T, tk = 40, ctc64.make_tokens(51, 12, equal_pairs=2)
    lp = ctc64.make_log_probs(52, T)
    rng = np.random.default_rng(53)
    keep = np.zeros((T, V), bool)  # one protected path: token k for frames [3 k, 3 k + 3), blanks at the end
    for t in range(T):
        keep[t, tk[t // 3] if t // 3 < len(tk) else TOKENS] = True
    for t in range(1, len(tk)):  # (a blank between equal neighbours)
        if tk[t] == tk[t - 1]:
            keep[3 * t, :] = False
            keep[3 * t, TOKENS] = True
    r = rng.random((T, V))
    lp[(r < 0.15) & ~keep] = -np.inf
    lp[(r > 0.85) & ~keep] = -3e38
    labels = sorted(set(tk) | {TOKENS})
    assert np.isneginf(lp[:, labels]).any() and (lp[:, labels] == np.float32(-3e38)).any()
    got = run_nll([(lp, tk)], TOKENS)
    check_nll("-inf and -3e38 off the path", got[0], lp, tk, TOKENS)
    dead = lp.copy()
    dead[7, :] = -np.inf  # no path survives a frame of zeros
    assert run_nll([(dead, tk)], TOKENS)[0] == np.inf == ctc64.ctc_nll(dead, tk, TOKENS)


def test_ctc_nll_label_priors():
    pri = np.random.default_rng(61).uniform(-12.0, 0.0, V)
    cases = small_cases()[1:] + [("t40", *aligner_fixture("t40"))]
    got = run_nll([(lp, tk) for _, lp, tk in cases], TOKENS, pri, 0.3)
    plain = run_nll([(lp, tk) for _, lp, tk in cases], TOKENS)
    for (name, lp, tk), v, p in zip(cases, got, plain):
        check_nll(f"priors {name}", v, lp, tk, TOKENS, pri, 0.3)
        assert v != p
    assert run_nll([(lp, tk) for _, lp, tk in cases], TOKENS, pri, 0.0).tobytes() == plain.tobytes()


# ------------------------------------------------------------------------------------------------ the two reductions beside it
def test_confidence_sums():
    eng = engine()
    L = [1, 7, 300, 257]
    rng = np.random.default_rng(71)
    sc = [(-rng.exponential(1.5, n)).astype(np.float32) for n in L]
    sc[1][3] = -np.inf  # a frame of probability zero
    flat = torch.from_numpy(np.concatenate(sc)).to(eng.device)
    got = eng.ctc_confidence_sums(seg_of(L), flat).cpu().numpy()
    assert eng.ctc_confidence_sums(seg_of(L), flat).cpu().numpy().tobytes() == got.tobytes()
    for i, s in enumerate(sc):
        assert eng.ctc_confidence_sums(seg_of([L[i]]), torch.from_numpy(s).to(eng.device)).cpu().numpy()[0] == got[i]
    against_fp32("confidence", got, [ctc64.confidence_sum(s) for s in sc], [float(torch.from_numpy(s).exp().sum()) for s in sc])


def test_prior_sums():
    eng = engine()
    L = [1, 63, 64, 65, 130]  # chunk edges of 64 rows inside and across utterances
    lps = [ctc64.make_log_probs(80 + i, n) for i, n in enumerate(L)]
    lps[2][:, 5] = -np.inf   # a class no frame ever emits
    lps[0][:, 5] = lps[1][:, 5] = lps[3][:, 5] = lps[4][:, 5] = -np.inf
    lps[3][:, 9] = -np.inf   # a class with whole chunks of zeros
    rows = padded_rows(lps)
    got = eng.ctc_prior_sums(seg_of(L), rows, classes=V).cpu().numpy()
    assert got.shape == (V,) and eng.ctc_prior_sums(seg_of(L), rows, classes=V).cpu().numpy().tobytes() == got.tobytes()
    assert eng.ctc_prior_sums(seg_of([sum(L)]), rows, classes=V).cpu().numpy().tobytes() == got.tobytes()  # all frames of the batch: the cut into utterances plays no part
    allrows = np.concatenate(lps)
    ref, f32 = ctc64.prior_sums(allrows, V), torch.logsumexp(torch.from_numpy(allrows), dim=0).double().numpy()
    assert got[5] == -np.inf and ref[5] == -np.inf and not np.isnan(got).any()
    ok = np.isfinite(ref)
    against_fp32("prior sums", got[ok], ref[ok], f32[ok])
    one = eng.ctc_prior_sums(seg_of([1]), padded_rows(lps[:1]), classes=V).cpu().numpy()
    assert (one == lps[0][0].astype(np.float64)).all()


# ------------------------------------------------------------------------------------------------ duration sums
@pytest.mark.parametrize("Cn", [16, 64])
def test_duration_sums_and_loss_against_the_reference(Cn):
    from stylish_tts_amd import modules as M
    from stylish_tts_amd import pipeline

    eng = engine()
    g = np.load(os.path.join(GOLD, "duration_loss.npz"))
    logits, gt, L, w = g[f"c{Cn}_logits"], g[f"c{Cn}_gt"], [int(n) for n in g[f"c{Cn}_lengths"]], g[f"c{Cn}_weight"]
    assert min(L) == 1 and gt[0, 0] == Cn - 1 and gt[2, 0] == 0 and gt[2, 1] == Cn - 1
    loss = M.DurationLoss(class_count=Cn, weight=torch.from_numpy(w), engine=eng)
    sums, _ = loss.sums(torch.from_numpy(logits), torch.from_numpy(gt), torch.tensor(L))
    s = sums.cpu().numpy()
    assert s.shape == (len(L), 3) and loss.sums(torch.from_numpy(logits), torch.from_numpy(gt), torch.tensor(L))[0].cpu().numpy().tobytes() == s.tobytes()
    ld = 80  # rows wider than the classes, NaN behind them; every utterance alone
    for b, n in enumerate(L):
        rows = np.full((n, ld), np.nan, np.float32)
        rows[:, :Cn] = logits[b, :n]
        solo = eng.duration_sums(seg_of([n]), torch.from_numpy(rows), torch.from_numpy(gt[b, :n]), torch.from_numpy(w), classes=Cn).cpu().numpy()
        assert solo.tobytes() == s[b : b + 1].tobytes(), b
    ce, cdw, ce_u, cdw_u = M.duration_score(s.tolist(), L)
    against_fp32(f"C {Cn} duration_ce_utt", ce_u, g[f"c{Cn}_ce_utt_f64"], g[f"c{Cn}_ce_utt_f32"])
    against_fp32(f"C {Cn} duration_utt", cdw_u, g[f"c{Cn}_cdw_utt_f64"], g[f"c{Cn}_cdw_utt_f32"])
    against_fp32(f"C {Cn} duration_ce", ce, g[f"c{Cn}_ce_f64"], g[f"c{Cn}_ce_f32"])
    against_fp32(f"C {Cn} duration", cdw, g[f"c{Cn}_cdw_f64"], g[f"c{Cn}_cdw_f32"])
    oracle = np.array([ctc64.duration_sums(logits[b, :n], gt[b, :n], w) for b, n in enumerate(L)])
    # against the oracle's own sums: s0 and s1 are sums of one sign over at most 30 rows (a few hundred fp64 roundings, 64 ulp); s2 takes
    # log(1 - sm + 1e-9), whose argument inherits the <= C 2^-53 rounding of the softmax's denominator over at least 1e-9: C 2^-53 / 1e-9 a row
    assert np.abs(s[:, :2] / oracle[:, :2] - 1).max() <= 64 * 2.0**-52
    assert (np.abs(s[:, 2] - oracle[:, 2]) <= np.array(L) * Cn * 2.0**-53 / 1e-9 + 64 * 2.0**-52 * np.abs(oracle[:, 2])).all()
    f_ce, f_cdw = loss(torch.from_numpy(logits), torch.from_numpy(gt), torch.tensor(L))
    assert f_ce.dtype == torch.float32 and adjacent_f32(float(f_ce), ce) and adjacent_f32(float(f_cdw), cdw)
    one = M.CDW_CCELoss(Cn, alpha=2, weight=torch.from_numpy(w), engine=eng)(torch.from_numpy(logits[1, : L[1]]), torch.from_numpy(gt[1, : L[1]]))
    assert float(one[0]) == np.float32(ce_u[1]) and float(one[1]) == np.float32(cdw_u[1])
    if Cn == 16:  # pipeline.duration_scores from durations and from the 0/1 alignment they describe
        dur_of = np.array([1, 2, 3, 4, 5, 6, 7, 9, 12, 15, 18, 22, 27, 32, 38, 46])
        durs = torch.from_numpy(dur_of[gt])
        out = pipeline.duration_scores(eng, torch.from_numpy(logits), durs, L, torch.from_numpy(w))
        assert out["duration_ce"] == ce and out["duration"] == cdw and out["duration_ce_utt"] == ce_u and out["duration_utt"] == cdw_u
        al = torch.zeros(len(L), gt.shape[1], int(durs.sum(1).max()))
        for b in range(len(L)):
            at = 0
            for p in range(gt.shape[1]):
                al[b, p, at : at + int(durs[b, p])] = 1
                at += int(durs[b, p])
        assert pipeline.duration_scores(eng, torch.from_numpy(logits), al, L, torch.from_numpy(w)) == out


# ------------------------------------------------------------------------------------------------ difference sums
@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_diff_sums(kind):
    eng = engine()
    L = [1, 255, 257, 4000]
    rng = np.random.default_rng(91)
    a = [rng.standard_normal(n).astype(np.float32) * 3 for n in L]
    b = [rng.standard_normal(n).astype(np.float32) for n in L]
    b[1] = a[1].copy()  # an identical pair sums to exactly 0
    fa, fb = torch.from_numpy(np.concatenate(a)).to(eng.device), torch.from_numpy(np.concatenate(b)).to(eng.device)
    got = eng.diff_sums(seg_of(L), fa, fb, kind).cpu().numpy()
    assert eng.diff_sums(seg_of(L), fa, fb, kind).cpu().numpy().tobytes() == got.tobytes() and got[1] == 0.0
    for i in range(len(L)):
        assert eng.diff_sums(seg_of([L[i]]), torch.from_numpy(a[i]), torch.from_numpy(b[i]), kind).cpu().numpy()[0] == got[i]
    d = [torch.from_numpy(x) - torch.from_numpy(y) for x, y in zip(a, b)]
    f32 = [float(v.abs().sum() if kind == "l1" else (v * v).sum()) for v in d]
    against_fp32(f"diff sums {kind}", got, [ctc64.diff_sum(x, y, kind) for x, y in zip(a, b)], f32)
    with pytest.raises(ValueError):
        eng.diff_sums(seg_of(L), fa, fb, "huber")


# ------------------------------------------------------------------------------------------------ canaries behind every output
def test_outputs_end_where_they_should():
    from stylish_tts_amd import _lib
    from stylish_tts_amd.runtime import _ptr, _stream

    eng = engine()
    dev = eng.device
    cases = small_cases()
    TL, PL = [c[1].shape[0] for c in cases], [len(c[2]) for c in cases]
    st, sp, B = seg_of(TL), seg_of(PL), len(cases)
    rows = padded_rows([c[1] for c in cases])
    tg = torch.tensor([v for c in cases for v in c[2]], dtype=torch.int32, device=dev)
    full = lambda n: torch.full((n,), CANARY, dtype=torch.float64, device=dev)  # noqa: E731

    out = full(B + 8)
    _lib.check(eng.lib.stts_ctc_nll(_stream(), B, st.host_ptr, _ptr(st.dev), sp.host_ptr, _ptr(sp.dev), _ptr(rows), LD, V, TOKENS, _ptr(tg), None, 0.0, _ptr(out)))
    assert (out[B:] == CANARY).all() and (out[:B] != CANARY).all()
    out = full(B + 8)
    col = rows[:, 0].contiguous()
    _lib.check(eng.lib.stts_ctc_confidence_sums(_stream(), B, st.host_ptr, _ptr(st.dev), _ptr(col), _ptr(out)))
    assert (out[B:] == CANARY).all() and (out[:B] != CANARY).all()
    out, need = full(V + 8), int(eng.lib.stts_ctc_prior_sums_workspace_bytes(B, st.host_ptr, V))
    ws = full(need // 8 + 8)
    _lib.check(eng.lib.stts_ctc_prior_sums(_stream(), B, st.host_ptr, _ptr(st.dev), _ptr(rows), LD, V, _ptr(out), _ptr(ws), need))
    assert (out[V:] == CANARY).all() and (ws[need // 8 :] == CANARY).all() and (out[:V] != CANARY).all()
    out = full(3 * B + 8)
    lg = torch.randn(sum(PL), 16, device=dev)
    w, tg16, c0, c1 = torch.ones(16, device=dev), (tg % 16).contiguous(), lg[:, 0].contiguous(), lg[:, 1].contiguous()
    _lib.check(eng.lib.stts_val_duration_sums(eng.ctx, _stream(), B, sp.host_ptr, _ptr(sp.dev), _ptr(lg), 16, 16, _ptr(tg16), _ptr(w), _ptr(out)))
    assert (out[3 * B :] == CANARY).all() and (out[: 3 * B] != CANARY).all()
    for kind in (0, 1):
        out = full(B + 8)
        _lib.check(eng.lib.stts_val_diff_sums(eng.ctx, _stream(), B, sp.host_ptr, _ptr(sp.dev), _ptr(c0), _ptr(c1), kind, _ptr(out)))
        assert (out[B:] == CANARY).all() and (out[:B] != CANARY).all()


# ------------------------------------------------------------------------------------------------ the shims
def batch_tnc(cases, pad_tokens):
    """[(lp, tokens)] -> CTCLossWithLabelPriors.forward's arguments: log_probs [T, N, C], padded targets, the two length tensors."""
    Tm, Pm = max(lp.shape[0] for lp, _ in cases), max(len(tk) for _, tk in cases)
    x = torch.zeros(Tm, len(cases), V)
    tg = torch.full((len(cases), Pm), pad_tokens, dtype=torch.long)
    for b, (lp, tk) in enumerate(cases):
        x[: lp.shape[0], b] = torch.from_numpy(lp)
        tg[b, : len(tk)] = torch.tensor(tk)
    return x, tg, torch.tensor([lp.shape[0] for lp, _ in cases]), torch.tensor([len(tk) for _, tk in cases])


def test_ctc_loss_shim_eval_and_both_pairings():
    from stylish_tts_amd import modules as M

    cases = [(lp, tk) for _, lp, tk in small_cases()[1:]] + [aligner_fixture("t100")]  # frame counts 3, 3, 40, 100: not sorted, with a tie
    args = batch_tnc(cases, 0)
    ref = np.array([ctc64.ctc_nll(lp, tk, TOKENS) for lp, tk in cases])
    TL, PL = [lp.shape[0] for lp, _ in cases], [len(tk) for _, tk in cases]
    loss = M.CTCLossWithLabelPriors(blank=TOKENS, engine=engine())
    nll = loss.nll(*args, step_type="eval").cpu().numpy()
    for v, r, T in zip(nll, ref, TL):
        assert abs(v - r) <= 16 * T * 2.0**-53 * max(1.0, abs(r))
    assert loss.log_priors_sum is None and loss.num_samples == 0
    r32 = nll.astype(np.float32)
    own = float((torch.from_numpy(r32) / torch.tensor(PL, dtype=torch.float32)).mean())
    assert adjacent_f32(float(loss(*args, step_type="eval")), own) and own == M.align_loss_value(nll, TL, PL, loss)
    order = [3, 2, 0, 1]  # frames 100, 40, 3, 3: the stable descending sort
    paired = M.CTCLossWithLabelPriors(blank=TOKENS, engine=engine(), reference_pairing=True)
    want = float((torch.from_numpy(r32[order]) / torch.tensor(PL, dtype=torch.float32)).mean())
    assert adjacent_f32(float(paired(*args, step_type="eval")), want) and want == M.align_loss_value(nll, TL, PL, paired) and abs(want - own) > 1e-3 * own
    assert adjacent_f32(float(M.CTCLossWithLabelPriors(blank=TOKENS, reduction="sum", engine=engine())(*args, step_type="eval")), float(torch.from_numpy(r32).sum()))
    none = M.CTCLossWithLabelPriors(blank=TOKENS, reduction="none", engine=engine(), reference_pairing=True)(*args, step_type="eval")
    assert none.dtype == torch.float32 and none.cpu().numpy().tolist() == r32[order].tolist()


def test_ctc_loss_shim_train_accumulates_and_applies_the_priors():
    from stylish_tts_amd import modules as M

    b1 = [(lp, tk) for _, lp, tk in small_cases()[1:]]
    b2 = [aligner_fixture("t40"), (ctc64.make_log_probs(99, 70), ctc64.make_tokens(98, 9, equal_pairs=1))]
    for lp, _ in b1 + b2:
        lp[:, 100] = -30.0  # a class so rare that its prior meets the floor
    loss = M.CTCLossWithLabelPriors(prior_scaling_factor=0.3, blank=TOKENS, engine=engine())
    first = [loss.nll(*batch_tnc(b, 0), step_type="train").cpu().numpy() for b in (b1, b2)]
    for b, got in zip((b1, b2), first):  # no priors yet: the plain likelihood
        for (lp, tk), v in zip(b, got):
            r = ctc64.ctc_nll(lp, tk, TOKENS)
            assert abs(v - r) <= 16 * lp.shape[0] * 2.0**-53 * max(1.0, abs(r))
    rows = np.concatenate([lp for lp, _ in b1 + b2])
    assert loss.num_samples == rows.shape[0]
    # two batches merged by one more logsumexp = the logsumexp of all their frames
    s1, s2 = ctc64.prior_sums(np.concatenate([lp for lp, _ in b1]), V), ctc64.prior_sums(np.concatenate([lp for lp, _ in b2]), V)
    want_sum = np.logaddexp(s1, s2)
    got_sum = loss.log_priors_sum.cpu().numpy().reshape(-1)
    assert np.abs(got_sum - want_sum).max() <= 1e-12
    loss.on_train_epoch_end()
    want = np.maximum(want_sum - np.log(rows.shape[0] + 1e-9), -12.0)
    got = loss.log_priors.cpu().numpy().reshape(-1)
    assert loss.log_priors_sum is None and loss.num_samples == 0 and got.min() >= -12.0 and (got == -12.0).any() and np.abs(got - want).max() <= 1e-12
    applied = loss.nll(*batch_tnc(b2, 0), step_type="train").cpu().numpy()
    for (lp, tk), v in zip(b2, applied):
        r = ctc64.ctc_nll(lp, tk, TOKENS, got, 0.3)
        assert abs(v - r) <= 16 * lp.shape[0] * 2.0**-53 * max(1.0, abs(r))
    assert (applied != first[1]).all()
    assert loss.nll(*batch_tnc(b2, 0), step_type="eval").cpu().numpy().tobytes() == first[1].tobytes()  # "eval" applies none


def test_alignment_scores_equals_the_pieces():
    from stylish_tts_amd import modules as M
    from stylish_tts_amd import synth

    eng = engine()
    m = M.TextAligner(80, TOKENS, engine=eng).load_synthetic(0)
    L, PL = [33, 60, 17], [5, 12, 4]
    mel = torch.from_numpy(synth.normal("align_scores.mel", (3, 60, 80)).astype(np.float32))
    texts = torch.zeros(3, 12, dtype=torch.long)
    toks = [ctc64.make_tokens(70 + b, PL[b], equal_pairs=1) for b in range(3)]
    for b in range(3):
        texts[b, : PL[b]] = torch.tensor(toks[b])
    out = m.alignment_scores(mel, L, texts, PL)
    lp, seg = m.packed(mel, L)
    sp = seg_of(PL)
    tg = torch.tensor([v for tk in toks for v in tk], dtype=torch.int32)
    r = eng.ctc_align(seg, lp, sp, tg, TOKENS)
    nll = eng.ctc_nll(seg, lp, sp, tg, TOKENS).cpu().tolist()
    conf = eng.ctc_confidence_sums(seg, r["scores"]).cpu().tolist()
    assert out["nll_utt"] == nll and out["confidence_utt"] == [c / n for c, n in zip(conf, L)] and out["confidence"] == sum(conf) / sum(L)
    assert out["align_loss"] == M.align_loss_value(nll, L, PL) and 0.0 < out["confidence"] <= 1.0
    lph = lp.cpu().numpy()
    for b in range(3):  # against the oracle on the engine's own log-probs, and torch's fp32 confidence
        rows = lph[seg.host[b] : seg.host[b + 1]]
        ref = ctc64.ctc_nll(rows, toks[b], TOKENS)
        assert abs(nll[b] - ref) <= 16 * L[b] * 2.0**-53 * max(1.0, abs(ref))
    paired = M.CTCLossWithLabelPriors(blank=TOKENS, engine=eng, reference_pairing=True)
    assert m.alignment_scores(mel, L, texts, PL, loss=paired)["align_loss"] == M.align_loss_value(nll, L, PL, paired) != out["align_loss"]


def test_validation_scores_cfm_terms():
    from stylish_tts_amd import pipeline

    eng = engine()
    rng = np.random.default_rng(111)
    audio, gt = torch.from_numpy(rng.standard_normal((2, 4800)).astype(np.float32) * 0.1), torch.from_numpy(rng.standard_normal((2, 4800)).astype(np.float32) * 0.1)
    base = pipeline.validation_scores(eng, audio, gt)
    assert sorted(base) == ["mel", "mel_r", "mel_utt"]
    pm, tm = rng.standard_normal((2, 80, 37)).astype(np.float32), rng.standard_normal((2, 80, 37)).astype(np.float32)
    pp, tp = [rng.standard_normal(n).astype(np.float32) for n in (37, 20)], [rng.standard_normal(n).astype(np.float32) for n in (37, 20)]
    hz_p, hz_t = [200 + 50 * v for v in pp], [210 + 40 * v for v in tp]
    out = pipeline.validation_scores(eng, audio, gt, mel_l2=(torch.from_numpy(pm), torch.from_numpy(tm)), normed_pitch_l2=([torch.from_numpy(v) for v in pp], [torch.from_numpy(v) for v in tp]),
                                     linear_pitch=([torch.from_numpy(v) for v in hz_p], [torch.from_numpy(v) for v in hz_t]))
    assert {k: out[k] for k in base} == base
    assert sorted(set(out) - set(base)) == ["linear_pitch", "linear_pitch_utt", "mel_l2", "mel_l2_utt", "normed_pitch_l2", "normed_pitch_l2_utt"]
    F = torch.nn.functional
    cat = lambda xs: torch.from_numpy(np.concatenate([np.ravel(x) for x in xs]))  # noqa: E731
    for name, a, b, fn, kind in (("mel_l2", pm, tm, F.mse_loss, "l2"), ("normed_pitch_l2", pp, tp, F.mse_loss, "l2"), ("linear_pitch", hz_p, hz_t, F.l1_loss, "l1")):
        n = sum(np.size(x) for x in a)
        f64 = sum(ctc64.diff_sum(x, y, kind) for x, y in zip(a, b)) / n
        against_fp32(name, out[name], f64, float(fn(cat(a), cat(b))))
        assert out[name + "_utt"] == pytest.approx([ctc64.diff_sum(x, y, kind) / np.size(x) for x, y in zip(a, b)], rel=1e-12)
    with pytest.raises(ValueError, match="mel_l2"):
        pipeline.validation_scores(eng, audio, gt, mel_l2=(torch.from_numpy(pm), torch.from_numpy(tm[:, :, :30])))
