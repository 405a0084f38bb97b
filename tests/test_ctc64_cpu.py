"""tests/ctc64.py, the float64 oracle of the alignment and duration scores, pinned without a GPU: its CTC recurrence against
torch.nn.functional.ctc_loss in float64, its duration sums against the recorded reference run (tests/golden/duration_loss.npz: the reference's
CDW_CCELoss / DurationLoss on fp32 and float64 copies of the same inputs), the host halves of the shims (tables, reductions, pairings), and the
new entry points' refusals, which return before anything touches a device.

The bound between the oracle and torch's float64 run is the one the kernel is held to: both add one rounding of |alpha| <= |nll| per frame and
log-sum-exp is 1-Lipschitz, so the roundings add at most linearly - 16 T 2^-53 max(1, |nll|), the 16 covering the few roundings of one step."""
import ctypes as C
import os

import numpy as np
import pytest

import ctc64

torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BLANK, V = 178, 179

# (T, P, adjacent equal pairs)
CASES = [(1, 1, 0), (3, 1, 0), (3, 2, 1), (17, 5, 1), (40, 14, 3), (100, 30, 2), (300, 120, 5)]


def torch_ctc(lp, targets, blank, dtype):
    x = torch.from_numpy(np.asarray(lp)).to(dtype)[:, None, :]
    return float(torch.nn.functional.ctc_loss(x, torch.tensor([targets]), torch.tensor([x.shape[0]]), torch.tensor([len(targets)]), blank=blank, reduction="none",
                                              zero_infinity=False)[0])


@pytest.mark.parametrize("T,P,pairs", CASES)
def test_recurrence_against_torch_float64(T, P, pairs):
    lp, tk = ctc64.make_log_probs(100 + T, T), ctc64.make_tokens(200 + T, P, equal_pairs=pairs)
    assert ctc64.min_frames(tk) <= T
    mine, ref, ref32 = ctc64.ctc_nll(lp, tk, BLANK), torch_ctc(lp, tk, BLANK, torch.float64), torch_ctc(lp, tk, BLANK, torch.float32)
    bound = 16 * T * 2.0**-53 * max(1.0, abs(ref))
    print(f"T {T} P {P}: oracle {mine!r} torch float64 {ref!r} |diff| {abs(mine - ref):.2e} (bound {bound:.2e}); torch fp32 is {abs(ref32 - ref):.2e} away")
    assert abs(mine - ref) <= bound


def test_blank_zero_and_priors_against_torch_float64():
    lp, tk = ctc64.make_log_probs(7, 33), [t + 1 for t in ctc64.make_tokens(8, 9, symbols=178, equal_pairs=1)]
    assert abs(ctc64.ctc_nll(lp, tk, 0) - torch_ctc(lp, tk, 0, torch.float64)) <= 16 * 33 * 2.0**-53 * 200
    pri = np.random.default_rng(9).uniform(-12, 0, V)
    shifted = lp.astype(np.float64) - 0.3 * pri  # what the reference hands to the loss in a "train" step
    assert abs(ctc64.ctc_nll(lp, tk, 0, pri, 0.3) - torch_ctc(shifted, tk, 0, torch.float64)) <= 16 * 33 * 2.0**-53 * 200


def test_infeasible_is_inf_in_both_and_one_path_is_its_sum():
    tk = ctc64.make_tokens(3, 14, equal_pairs=3)
    need = ctc64.min_frames(tk)
    assert need == 17
    lp = ctc64.make_log_probs(4, need)
    assert ctc64.ctc_nll(lp[:-1], tk, BLANK) == np.inf and torch_ctc(lp[:-1], tk, BLANK, torch.float64) == np.inf
    assert ctc64.ctc_nll(lp, tk, BLANK) == ctc64.single_path_nll(lp, tk, BLANK)
    assert abs(ctc64.ctc_nll(lp, tk, BLANK) - torch_ctc(lp, tk, BLANK, torch.float64)) <= 16 * need * 2.0**-53 * 200


def test_prior_sums_against_torch_float64():
    lp = ctc64.make_log_probs(5, 150)
    lp[:, 7] = -np.inf
    ref = torch.logsumexp(torch.from_numpy(lp).double(), dim=0).numpy()
    mine = ctc64.prior_sums(lp, V)
    assert mine[7] == -np.inf and ref[7] == -np.inf
    ok = np.isfinite(ref)
    assert np.abs(mine[ok] - ref[ok]).max() <= 150 * 2.0**-52 * 8


@pytest.mark.parametrize("Cn", [16, 64])
def test_duration_oracle_against_the_reference_float64(Cn):
    g = np.load(os.path.join(GOLD, "duration_loss.npz"))
    logits, gt, L, w = g[f"c{Cn}_logits"], g[f"c{Cn}_gt"], g[f"c{Cn}_lengths"], g[f"c{Cn}_weight"]
    sums = [ctc64.duration_sums(logits[b, :n], gt[b, :n], w) for b, n in enumerate(L)]
    ce, cdw, ce_u, cdw_u = ctc64.duration_scores(sums, L)
    for mine, ref in ((ce, g[f"c{Cn}_ce_f64"]), (cdw, g[f"c{Cn}_cdw_f64"])):
        assert abs(mine - float(ref)) <= 1e-13 * abs(float(ref))
    assert np.abs(np.array(ce_u) / g[f"c{Cn}_ce_utt_f64"] - 1).max() <= 1e-13 and np.abs(np.array(cdw_u) / g[f"c{Cn}_cdw_utt_f64"] - 1).max() <= 1e-13


def test_duration_tables():
    from stylish_tts_amd.modules import DurationProcessor

    p = DurationProcessor(16, 50)
    durs = torch.tensor([0, 1, 2, 7, 8, 10, 11, 19, 20, 34, 35, 41, 42, 50, 80])
    assert p.dur_to_class(durs).tolist() == [0, 0, 1, 6, 7, 7, 8, 10, 11, 13, 14, 14, 15, 15, 15]
    al = torch.zeros(2, 3, 60)
    al[0, 0, :5], al[0, 1, 5:17], al[1, 2, :] = 1, 1, 1  # 5, 12, 0 frames / 0, 0, 60 frames
    assert p.align_to_class(al).tolist() == [[4, 8, 0], [0, 0, 15]]
    assert p.class_to_dur_table.tolist() == [1, 2, 3, 4, 5, 6, 7, 9, 12, 15, 18, 22, 27, 32, 38, 46]
    for c, d in enumerate(p.class_to_dur_table.tolist()):  # a class' own duration maps back to it
        assert int(p.dur_to_class(torch.tensor([int(d)]))[0]) == c
    assert list(p.state_dict()) == []


def test_align_loss_reductions_and_pairings():
    from stylish_tts_amd import modules as M

    nll, TL, PL = [10.0, 40.0, 25.0], [50, 80, 80], [5, 20, 10]  # not sorted by frame count; a tie that keeps batch order
    assert M.align_loss_value(nll, TL, PL) == pytest.approx((10 / 5 + 40 / 20 + 25 / 10) / 3, rel=1e-6)
    ref = M.CTCLossWithLabelPriors(blank=BLANK, reference_pairing=True, engine=object())
    assert M.align_loss_value(nll, TL, PL, ref) == pytest.approx((40 / 5 + 25 / 20 + 10 / 10) / 3, rel=1e-6)
    assert M.align_loss_value(nll, TL, PL, M.CTCLossWithLabelPriors(reduction="sum", engine=object())) == 75.0
    assert M.align_loss_value(nll, TL, PL, M.CTCLossWithLabelPriors(reduction="none", reference_pairing=True, engine=object())) == [40.0, 25.0, 10.0]
    with pytest.raises(ValueError):
        M.CTCLossWithLabelPriors(reduction="batchmean")
    with pytest.raises(ValueError, match="class weights"):
        M.CDW_CCELoss(16, alpha=2, weight=None, engine=object())(torch.zeros(3, 16), torch.zeros(3, dtype=torch.long))
    ce, cdw, ce_u, cdw_u = M.duration_score([[-6.0, 3.0, -0.5], [-1.0, 1.0, -0.25]], [5, 1])
    assert ce_u == pytest.approx([2.0, 1.0]) and cdw_u == pytest.approx([10.0, 25.0]) and ce == pytest.approx(1.5) and cdw == pytest.approx(17.5)


def test_entry_points_refuse_before_any_launch():
    from stylish_tts_amd import _lib

    lib = _lib.load()
    off = lambda lens: (C.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens)]).tolist())  # noqa: E731
    buf = (C.c_double * 64)()
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    d = p(buf)

    def nll(T, P, out=d):
        return lib.stts_ctc_nll(None, len(T), p(off(T)), d, p(off(P)), d, d, 192, V, BLANK, d, None, 0.0, out)

    for T, P, needle in (([5, 4], [2, 0], "tokens"), ([600], [511], "tokens"), ([5, 0], [2, 2], "no frames")):
        assert nll(T, P) != 0 and needle in lib.stts_last_error().decode(), (T, P)
    assert nll([5], [2], None) != 0 and "null" in lib.stts_last_error().decode()
    assert lib.stts_ctc_nll(None, 1, p(off([5])), d, p(off([2])), d, d, 100, V, BLANK, d, None, 0.0, d) != 0
    assert lib.stts_ctc_confidence_sums(None, 2, p(off([5, 0])), d, d, d) != 0 and "no frames" in lib.stts_last_error().decode()
    assert lib.stts_ctc_confidence_sums(None, 1, p(off([5])), d, d, None) != 0
    assert lib.stts_ctc_prior_sums_workspace_bytes(2, p(off([5, 0])), V) == 0
    assert lib.stts_ctc_prior_sums_workspace_bytes(2, p(off([64, 1])), V) == 2 * V * 16
    assert lib.stts_ctc_prior_sums(None, 1, p(off([65])), d, d, 192, V, d, d, 2 * V * 16 - 1) != 0 and "workspace" in lib.stts_last_error().decode()
    assert lib.stts_ctc_prior_sums(None, 1, p(off([65])), d, d, 192, V, None, d, 2 * V * 16) != 0
    assert lib.stts_val_duration_sums(d, None, 1, p(off([5])), d, d, 80, 65, d, d, d) != 0 and "64" in lib.stts_last_error().decode()
    assert lib.stts_val_duration_sums(d, None, 2, p(off([5, 0])), d, d, 16, 16, d, d, d) != 0 and "no tokens" in lib.stts_last_error().decode()
    assert lib.stts_val_duration_sums(d, None, 1, p(off([5])), d, d, 16, 16, d, d, None) != 0
    assert lib.stts_val_diff_sums(d, None, 1, p(off([5])), d, d, d, 2, d) != 0 and "kind" in lib.stts_last_error().decode()
    assert lib.stts_val_diff_sums(d, None, 2, p(off([5, 0])), d, d, d, 1, d) != 0 and "no values" in lib.stts_last_error().decode()
    assert lib.stts_val_diff_sums(d, None, 1, p(off([5])), d, d, d, 1, None) != 0
