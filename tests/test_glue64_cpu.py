"""tests/glue64.py on the CPU: the references agree with oracle/stylish_oracle.py on the inputs tests/test_hip_glue_kernels.py uses, a small fp32 / int32 model of
every kernel passes its comparison function at those shapes and tolerances, and every mutated model - one defect each - is rejected by them."""
import numpy as np
import pytest

import glue64 as M
from oracle import stylish_oracle as O

F32, F64, I64 = np.float32, np.float64, np.int64


# ------------------------------------------------------------------------------------------------ the references against the oracle
def test_duration_reference_agrees_with_the_oracle_and_the_generator_keeps_the_cap():
    c = M.decode_case()
    for s, lg in c["rand"].items():
        dur, sure, _ = M.decode_ref(lg)
        assert (~sure).mean() <= 0.01, (s, (~sure).mean())  # at most 1 % of the random rows may be left out
        assert M.decode_equal(dur, sure, O.prediction_to_duration(lg)), s
    dur, sure, exp = M.decode_ref(c["ties"])
    assert np.array_equal(dur, O.prediction_to_duration(c["ties"]).astype(I64))  # exact half-integers: both round half to even
    assert np.array_equal(exp[:4], [10.5, 26.5, 16.5, 13.5]) and tuple(dur[:4]) == M.TIE_EXPECT
    dur, sure, _ = M.decode_ref(c["large"])
    assert sure.mean() > 0.5 and M.decode_equal(dur, sure, O.prediction_to_duration(c["large"]))


@pytest.mark.parametrize("P", M.ALIGN_P)
def test_alignment_reference_is_the_oracles(P):
    c = M.alignment_case(P)
    assert c["T"] > 0 and np.array_equal(c["ref"], O.duration_to_alignment(c["dur"]))


def test_token_map_reference_is_the_alignments_argmax():
    """consistent offsets: frame f's token is the row of the oracle's alignment matrix that holds its 1 (repeat_interleave(rep) along time)."""
    for name in M.REGULATE_CASES:
        c = M.regulate_case(name)
        for u in range(0, len(c["P"]), 3):  # the utterances with consistent offsets
            t0, t1, f0, f1 = c["tok_off"][u], c["tok_off"][u + 1], c["frm_off"][u], c["frm_off"][u + 1]
            if t1 - t0 > 600 or f1 == f0:
                continue  # (the matrix of the 1500-token utterance is not built)
            a = np.repeat(O.duration_to_alignment(c["dur"][t0:t1]), c["rep"], axis=1)
            assert np.array_equal(c["src"][f0:f1] - t0, a.argmax(0)), (name, u)
            assert np.array_equal(c["centre"][f0:f1], a.argmax(0))


def test_upsample_reference_agrees_with_the_oracle():
    c = M.upsample_case()
    off = M.offsets(M.UPSAMPLE_LENGTHS)
    got = np.concatenate([O.upsample_linear4(c["x"][None, off[u]:off[u + 1]])[0] if L else np.zeros(0, F32) for u, L in enumerate(M.UPSAMPLE_LENGTHS)])
    assert M.upsample_ratio(c, got) < 1.0


@pytest.mark.parametrize("ntaps", M.CHAN_NTAPS)
def test_conv_reference_agrees_with_the_oracle(ntaps):
    c = M.chan_case(0, ntaps, 260)
    off = M.offsets(M.CHAN_LENGTHS)
    for i, s in enumerate(c["sets"]):
        wt = np.ascontiguousarray(s["w"].T[None])  # [1, C, k]
        got = np.concatenate([O.conv1d(np.ascontiguousarray(s["x"][off[u]:off[u + 1], :c["C"]].T[None]), wt, np.array([s["bias"]], F32), padding=(ntaps - 1) // 2)[0, 0]
                              for u in range(len(M.CHAN_LENGTHS))])
        assert M.chan_ratio(c, i, got) < 1.0
    f = M.front_case()
    w3 = np.array(M.FRONT_WF, F32)[None, None]
    off = M.offsets(M.FRONT_LENGTHS)
    got = np.concatenate([O.conv1d(f["pitch"][None, None, off[u]:off[u + 1]], w3, np.array([M.FRONT_BF], F32), padding=1)[0, 0] for u in range(len(M.FRONT_LENGTHS))])
    assert M.ratio(got, f["f0"], M.dot_bound(3, f["f0_abs"], f["f0"])) < 1.0


# ------------------------------------------------------------------------------------------------ index kernels: model passes, mutants rejected
@pytest.mark.parametrize("n_utt", M.OFFSETS_N_UTT)
def test_frame_offsets_model_and_mutants(n_utt):
    c = M.offsets_case(n_utt)
    assert (c["dur"] < 0).any() and c["dur"].max() == 46 and (c["dur"] == 0).any()
    for k, caps in c["caps"].items():
        assert M.offsets_equal(c["ref"][k], *M.offsets_model(c["dur"], c["tok_off"], caps)), k
    if n_utt > 1:
        assert (c["caps"]["over"] < c["ref"]["over"][0]).sum() > 1 or n_utt < 4  # several utterances over capacity at once
    assert not M.offsets_equal(c["ref"]["exact"], *M.offsets_model(c["dur"], c["tok_off"], c["caps"]["exact"], "tok64"))
    assert not M.offsets_equal(c["ref"]["over"], *M.offsets_model(c["dur"], c["tok_off"], c["caps"]["over"], "noclamp"))
    assert not M.offsets_equal(c["ref"]["zero"], *M.offsets_model(c["dur"], c["tok_off"], c["caps"]["zero"], "noclamp"))
    if n_utt > 16:
        assert not M.offsets_equal(c["ref"]["exact"], *M.offsets_model(c["dur"], c["tok_off"], c["caps"]["exact"], "utt16"))


@pytest.mark.parametrize("name", M.REGULATE_CASES)
def test_token_map_model_and_mutants(name):
    c = M.regulate_case(name)
    assert c["dur"].min() == 0 and c["dur"].max() == 46
    n_buf = c["n_frames"] + 3
    src = M.token_map_model(c, n_buf)
    assert M.token_map_equal(c, src)
    out = M.sent((n_buf, c["C"] + 8)).copy()
    out[:c["n"], :c["C"]] = c["enc"][src[:c["n"]], :c["C"]]
    assert M.regulate_equal(c, out)
    off = out.copy()
    off[c["n"], 0] = 0.0  # a row written past frm_off[n_utt]
    assert not M.regulate_equal(c, off)
    assert not M.token_map_equal(c, M.token_map_model(c, n_buf, "carry"))
    assert not M.token_map_equal(c, M.token_map_model(c, n_buf, "tail0"))
    if c["rep"] > 1:
        assert not M.token_map_equal(c, M.token_map_model(c, n_buf, "rep_first"))
    utt = np.repeat(np.arange(len(c["P"])), np.diff(c["frm_off"]))
    centre = np.full(n_buf, M.SENTI, np.int32)
    centre[:c["n"]] = src[:c["n"]] - c["tok_off"][utt]
    assert M.local_token_equal(c, centre)
    centre[:c["n"]] = src[:c["n"]]  # the packed row where the token-local index belongs
    assert not M.local_token_equal(c, centre)


def test_duration_decode_model_and_mutants():
    c = M.decode_case()
    groups = list(c["rand"].values()) + [c["ties"], c["large"]]
    for lg in groups:
        dur, sure, _ = M.decode_ref(lg)
        assert M.decode_equal(dur, sure, M.decode_model(lg))
    tdur = O.prediction_to_duration(c["ties"]).astype(I64)
    all_sure = np.ones(len(tdur), bool)
    assert M.decode_equal(tdur, all_sure, M.decode_model(c["ties"]))
    for mutant in ("half_away", "argmax_last", "no_max"):
        assert not M.decode_equal(tdur, all_sure, M.decode_model(c["ties"], mutant)), mutant
    # the widest random rows alone reject the softmax that overflows
    lg = c["rand"][40.0]
    dur, sure, _ = M.decode_ref(lg)
    assert not M.decode_equal(dur, sure, M.decode_model(lg, "no_max"))


@pytest.mark.parametrize("P", M.ALIGN_P)
def test_alignment_comparison(P):
    c = M.alignment_case(P)
    out = M.sent(c["P"] * c["T"] + 7).copy()
    out[:c["P"] * c["T"]] = c["ref"].ravel()
    assert M.alignment_equal(c, out)
    out[c["T"] - 1] = 1 - out[c["T"] - 1]
    assert not M.alignment_equal(c, out)


def test_exact_comparisons():
    for shape in M.EMBED_CASES[:2]:
        c = M.embed_case(*shape)
        rows, C = shape[2], shape[1]
        want, err = M.embed_ref(c["emb"], c["tokens"])
        assert err == 0 and c["tokens"].max() == shape[0] - 1 and c["tokens"].min() == 0
        wb, errb = M.embed_ref(c["emb"], c["bad"])
        assert errb == 2 and np.array_equal(wb[rows // 2], want[0]) and np.array_equal(wb[rows // 3], want[0])  # (tokens[0] is id 0)
        out = M.sent((rows + 1, C + 4)).copy()
        out[:rows, :C] = want
        assert M.window_equal(out, want, rows, 0, C)
        out[0, C] = 0
        assert not M.window_equal(out, want, rows, 0, C)
    assert np.array_equal(M.row_utt_ref((2, 0, 1)), [0, 0, 2])


# ------------------------------------------------------------------------------------------------ arithmetic kernels: model passes, mutants rejected
@pytest.mark.parametrize("prec", M.CHAN_PREC)
@pytest.mark.parametrize("ntaps", M.CHAN_NTAPS)
def test_chan_conv_model_and_mutants(prec, ntaps):
    for C in M.CHAN_C:
        c = M.chan_case(prec, ntaps, C)
        xs = [s["x"][:, :C] for s in c["sets"]]
        assert all(np.array_equal(M.round_to(s["x"], prec), s["x"]) for s in c["sets"])  # the rows hold values of their type
        for i, s in enumerate(c["sets"]):
            assert M.chan_ratio(c, i, M.chan_model(xs[i], s["w"], s["bias"], M.CHAN_LENGTHS)) < 1.0
            assert M.chan_ratio(c, i, M.chan_model(xs[i], s["w"], s["bias"], M.CHAN_LENGTHS, "no_bias")) > 1.0
            if ntaps > 1:
                assert M.chan_ratio(c, i, M.chan_model(xs[i], s["w"], s["bias"], M.CHAN_LENGTHS, "halo")) > 1.0
                assert M.chan_ratio(c, i, M.chan_model(xs[i], s["w"], s["bias"], M.CHAN_LENGTHS, "taps_reversed")) > 1.0
        s0, s1 = c["sets"]
        assert M.chan_ratio(c, 1, M.chan_model(xs[1], s0["w"], s1["bias"], M.CHAN_LENGTHS)) > 1.0  # the second set reading the first set's weights
        assert M.chan_ratio(c, 1, M.chan_model(xs[0], s1["w"], s1["bias"], M.CHAN_LENGTHS)) > 1.0  # ... or its input


def test_decoder_front_model_and_mutants():
    c = M.front_case()
    r = M.front_check(c, *M.front_model(c))
    assert r["exact"] and r["f0"] < 1.0 and r["n"] < 1.0, r
    r = M.front_check(c, *M.front_model(c, "f0_on_energy"))
    assert r["n"] > 1.0
    enc_in, xa, xb = M.front_model(c)
    xa[0, 575] = 0.0  # a write into the hidden / residual columns
    assert not M.front_check(c, enc_in, xa, xb)["exact"]
    enc_in, xa, xb = M.front_model(c)
    enc_in[3, M.FRONT["ld_enc"] - 1] = 1.0  # a tail column that is not zero
    assert not M.front_check(c, enc_in, xa, xb)["exact"]


@pytest.mark.parametrize("K", M.STYLE_K)
@pytest.mark.parametrize("J", M.STYLE_J)
def test_style_model_and_mutants(K, J):
    c = M.style_case(K, J)
    for n_utt in M.STYLE_N_UTT:
        exact, r = M.style_check(c, n_utt, M.style_model(c, n_utt))
        assert exact and r < 1.0
        if K > 64:
            assert M.style_check(c, n_utt, M.style_model(c, n_utt, "cols64"))[1] > 1.0


@pytest.mark.parametrize("C", M.MEAN_C)
def test_mean_rows_model_and_mutants(C):
    c = M.mean_case(C)
    assert M.mean_ratio(c, M.mean_model(c)) < 1.0
    assert M.mean_ratio(c, M.mean_model(c, "div_max")) > 1.0
    assert M.mean_ratio(c, M.mean_model(c, "drop_last")) > 1.0


def test_upsample_model_and_mutants():
    c = M.upsample_case()
    assert M.upsample_ratio(c, M.upsample_model(c)) < 1.0
    assert M.upsample_ratio(c, M.upsample_model(c, "align_corners")) > 1.0
