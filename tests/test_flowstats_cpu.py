"""The flow statistics' surface that needs no GPU: the float64 restatement (tests/flowstats64.py) against the reference fixtures, the library's new
entries, the SpeechPredictor / NormalizingFlowLoss shims, and the mutants of flowstats64 - each moves a tap past the bar of
tests/test_hip_flow_stats.py at that test's shapes, so the GPU tests would catch it."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import flowstats64 as S  # noqa: E402
import flowstats_cases as C  # noqa: E402

from stylish_tts_amd import modules  # noqa: E402


def test_fixture_is_the_reference_inventory_and_well_conditioned(cfg):
    g = C.fixture()
    w, _ = C.weights(cfg)
    assert all("flow." + str(k) in w for k in g["keys"]) and len(g["keys"]) == sum(k.startswith("flow.") for k in w)
    assert list(np.diff(g["off"])) == [1, 2, 17, 33, 68]
    for name in ("fwd", "rev", "prior", "t2m"):
        for k in C.STREAMS:
            a = g[f"{name}_{k}"]
            assert a.dtype == np.float64 and np.isfinite(a).all() and np.abs(a).max() < 100
            assert 0 < g[f"err_{name}_{k}"][1] <= g[f"err_{name}_{k}"][0] < 1e-5


def test_flowstats64_reproduces_the_float64_fixtures(cfg):
    g = C.fixture()
    w, fws = C.weights(cfg)
    lengths = list(np.diff(g["off"]))
    got = {}
    got.update(zip(("fwd_z", "fwd_mean", "fwd_logstd"), S.flow(fws, g["z"], g["mean"], g["logstd"], g["style"], lengths, False)))
    got.update(zip(("rev_z", "rev_mean", "rev_logstd"), S.flow(fws, g["z"], g["mean"], g["logstd"], g["style"], lengths, True)))
    got.update(zip(("prior_z", "prior_mean", "prior_logstd"), S.prior(w, g["x"], g["noise"])))
    got.update(zip(("t2m_z", "t2m_mean", "t2m_logstd"), S.flow(fws, got["prior_z"], got["prior_mean"], got["prior_logstd"], g["style"], lengths, True)))
    for k, v in got.items():
        assert S.err(v, g[k])[0] <= 1e-12 * max(1.0, np.abs(g[k]).max()), k
    kl_text = S.kl_score(0, g["fwd_z"], g["fwd_logstd"], g["prior_mean"], g["prior_logstd"])
    kl_audio = S.kl_score(1, g["t2m_mean"], g["t2m_logstd"], g["mean"], g["logstd"])
    assert abs(kl_text - g["kl_text"][0]) <= 1e-12 * abs(kl_text) and abs(kl_audio - g["kl_audio"][0]) <= 1e-12 * abs(kl_audio)
    # the reference's own fp32 scores sit at fp32 distance
    assert abs(g["kl_text"][1] - kl_text) < 1e-5 * abs(kl_text) and abs(g["kl_audio"][1] - kl_audio) < 1e-5 * abs(kl_audio)
    # per-utterance sums add up to the score
    sums = S.kl_sums(0, g["fwd_z"], g["fwd_logstd"], g["prior_mean"], g["prior_logstd"], g["off"])
    assert abs(sums.sum() / g["off"][-1] - kl_text) <= 1e-12 * abs(kl_text)


def test_a_layer_chain_is_the_stage_and_untouched_halves_stay(cfg):
    g = C.fixture()
    _, fws = C.weights(cfg)
    lengths = list(np.diff(g["off"]))
    for reverse, name in ((False, "fwd"), (True, "rev")):
        three = tuple(g[k].astype(np.float64) for k in C.STREAMS)
        f = 7 if reverse else 0
        while f is not None:
            before = three
            *three, h0 = S.layer_with_next(fws, f, *three, g["style"], lengths, reverse)
            p = f & 1
            for a, b in zip(three, before):
                assert np.array_equal(a[:, p * 64 : (p + 1) * 64], b[:, p * 64 : (p + 1) * 64])
            n = S.next_layer(f, reverse)
            assert (h0 is None) == (n is None)
            f = n
        for a, k in zip(three, C.STREAMS):
            assert S.err(a, g[f"{name}_{k}"])[0] <= 1e-12 * np.abs(g[f"{name}_{k}"]).max()


def test_library_declares_and_exports_the_entries():
    from stylish_tts_amd import _lib

    lib = _lib.load()
    for name in ("stts_flow_stats_forward", "stts_flow_stats_workspace_bytes", "stts_prior_stats_forward", "stts_val_kl_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "stts_op_flow_stats_layer" in _lib.TEST_SIGNATURES and hasattr(lib, "stts_op_flow_stats_layer")
    assert len(_lib.SIGNATURES["stts_flow_stats_forward"][1]) == 16 and len(_lib.SIGNATURES["stts_val_kl_sums"][1]) == 15
    assert lib.stts_flow_stats_workspace_bytes(None, 16, 1, 16) == 0
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "stylish_hip.h")).read()
    for name in ("stts_flow_stats_forward", "stts_flow_stats_workspace_bytes", "stts_prior_stats_forward", "stts_val_kl_sums", "stts_op_flow_stats_layer"):
        assert name + "(" in hdr
    assert "STTS_W_FLOW_STATS = 524288" in hdr and "STTS_W_ALL = 255" in hdr
    assert modules.W_FLOW_STATS == 524288


def test_forward_signature_and_refusals(cfg):
    sig = inspect.signature(modules.SpeechPredictor.forward)
    assert sig.parameters["flow_stats"].default is False and sig.parameters["audio_gt"].default is None
    sp = modules.SpeechPredictor(cfg)
    with pytest.raises(NotImplementedError, match="flow_stats"):
        sp(None, None, None, None, None, flow_stats=True)
    with pytest.raises(NotImplementedError, match="posterior"):
        sp(None, None, None, None, None, audio_gt=torch.zeros(1, 300), flow_stats=True)
    pred = modules.DecoderPrediction(audio=None, magnitude=None, phase=None)
    assert not modules.has_flow_stats(pred)
    with pytest.raises(ValueError, match="flow statistics"):
        modules.NormalizingFlowLoss(cfg).scores(pred)
    # the score divides by the rows, not by rows x channels
    assert modules.flow_kl_score([6.0, 4.0], [2, 3]) == (2.0, [3.0, 4.0 / 3.0])


LAYER_MUTANTS = ("forward_on_reverse", "mean_no_exp", "logstd_sign", "halves_swapped", "neighbour_rows", "halo_1", "cond_next_layer", "pre_wrong_next")


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_moves_a_tap_past_the_gpu_bar(cfg, mutant):
    _, fws = C.weights(cfg)
    g = C.fixture()
    if mutant in LAYER_MUTANTS:  # the layer-alone test's shapes and its bar: BAR x the error of torch fp32
        c = C.layer_case(cfg, "ragged", 3, True)
        got = S.layer_with_next(fws, 3, c["z"], c["mean"], c["logstd"], c["style"], c["lengths"], True, mut=mutant)
        if mutant == "halves_swapped":  # (it writes the half the layer must leave alone)
            assert not np.array_equal(got[0][:, 64:], np.asarray(c["z"], np.float64)[:, 64:])
            return
        worst = C.layer_worst_ratio(c, got)
    elif mutant == "layer_order":  # the stage test's shapes and its bar: BAR x the reference fp32 run's recorded error
        lengths = list(np.diff(g["off"]))
        got = S.flow(fws, g["z"], g["mean"], g["logstd"], g["style"], lengths, True, mut=mutant)
        worst = max(S.err(a, g[f"rev_{k}"])[j] / g[f"err_rev_{k}"][j] for a, k in zip(got, C.STREAMS) for j in range(2))
    else:  # kl_mask_per_channel: the reduction's bar, on the score
        a, b, c_, d = g["fwd_z"], g["fwd_logstd"], g["prior_mean"], g["prior_logstd"]
        p0, p1 = S.kl_pieces(0, a, b, c_, d)
        bound = (p0.size + 16) * 2.0 ** -53 * (np.abs(p0) + np.abs(p1)).sum() / a.shape[0]
        assert abs(S.kl_score(0, a, b, c_, d, mut=mutant) - S.kl_score(0, a, b, c_, d)) > bound
        return
    assert worst > C.BAR, f"{mutant}: worst ratio {worst:.3g} stays inside the bar"
