"""RMVPE's Viterbi decoding without a GPU: the float64 oracle of tests/viterbi64.py on hand-computable cases, the premises of the GPU tests
(tests/test_hip_rmvpe_viterbi.py: every fixture's decision margin, the jump across the band, the tie rule), the transition table the library is
handed, and the shims' argument checks."""
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import viterbi64 as V  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NARROW = dict(n_blocks=1, inter_layers=1, en_out_channels=8)
LOG_EPS = math.log(2.0**-126)


def fixtures():
    """{name: salience [T, 360]}: the inputs whose paths the GPU tests compare."""
    return {"decode_sal0": np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"][0],
            "hidden32": np.load(os.path.join(GOLD, "resample_rmvpe.npz"))["hidden32"][0],
            "pitch_like": V.pitch_like()}


def test_transition_by_hand():
    L = V.lt()
    assert L.shape == (360, 360) and L.dtype == np.float64
    assert L[100, 100] == math.log(30 / 900) and L[100, 129] == math.log(1 / 900) and L[129, 100] == L[100, 129]  # inner rows sum to 900
    assert abs(L[0, 0] - math.log(30 / 465)) < 1e-15 and abs(L[0, 29] - math.log(1 / 465)) < 1e-15  # row 0: 30 + 29 + .. + 1 = 465
    out = np.abs(np.arange(360)[:, None] - np.arange(360)[None, :]) > 29
    assert (L[out] == L[0, 359]).all() and abs(L[0, 359] - LOG_EPS) < 1e-13 and np.isfinite(L).all()  # a jump is allowed, at one finite cost


def test_one_frame_and_two_frames_by_hand():
    s = np.zeros((1, 360), np.float32)
    s[0, 7], s[0, 200] = 0.25, 0.75
    r = V.viterbi(s)
    assert r["path"].tolist() == [200] and abs(r["logp"] - (math.log(0.75) + math.log(1 / 360))) < 1e-15
    # two frames, two candidates each: stay at 200 (0.75 * 0.25 * A[200][200]) against move to 205 (0.75 * 0.75 * A[200][205])
    s2 = np.zeros((2, 360), np.float32)
    s2[0, 7], s2[0, 200] = 0.25, 0.75
    s2[1, 200], s2[1, 205] = 0.25, 0.75
    r = V.viterbi(s2)
    want = math.log(0.75) + math.log(1 / 360) + math.log(25 / 900) + math.log(0.75)
    assert r["path"].tolist() == [200, 205] and abs(r["logp"] - want) < 1e-14
    assert abs(V.score(s2, [200, 200]) - (math.log(0.75) + math.log(1 / 360) + math.log(30 / 900) + math.log(0.25))) < 1e-14
    assert V.score(s2, r["path"]) == r["logp"]


def test_the_optimum_jumps_across_the_band():
    r = V.viterbi(V.jump_case())
    assert r["path"].tolist() == [10] * 10 + [300] * 10 and r["logp"] == -152.31003351232144 and r["ties"] == []
    # the best path that never leaves the band is far worse: walking 29 bins a frame costs log(eps) emissions on the way
    band_only = [10] * 10 + [min(300, 10 + 29 * k) for k in range(1, 11)]
    assert V.score(V.jump_case(), band_only) < r["logp"] - 500
    for sw in (1, 18):
        r = V.viterbi(V.jump_case(switch=sw))
        assert r["path"].tolist() == [10] * sw + [300] * (20 - sw) and r["ties"] == []


def test_constant_salience_takes_the_lowest_index():
    r = V.viterbi(np.full((5, 360), 0.5, np.float32))
    assert r["path"].tolist() == [0] * 5 and r["margin"] == 0.0


def test_every_fixture_has_a_margin_and_differs_from_the_argmax():
    for name, s in fixtures().items():
        r = V.viterbi(s)
        differ = int((r["path"] != s.argmax(1)).sum())
        print(f"{name}: T {len(s)} logp {r['logp']:.6f} margin {r['margin']:.2e} path differs from the per-frame argmax on {differ} frames")
        assert r["margin"] > 1e-9 and differ > 0 and r["ties"] == []
        assert abs(V.score(s, r["path"]) - r["logp"]) <= V.logp_bound(len(s), r["logp"])


def test_degenerate_rows_follow_the_stated_rules():
    s = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"][1].copy()
    assert (s.sum(1) == 0).any()  # the fixture's zero-sum row
    s[5] = np.nan
    s[9, 100] = -0.5
    e = V.emissions(s)
    zero = int(np.nonzero(np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"][1].sum(1) == 0)[0][0])
    assert np.isfinite(e).all() and (e[5] == e[5, 0]).all() and abs(e[5, 0] - LOG_EPS) < 1e-13 and (e[zero] == e[5, 0]).all() and e[9, 100] == e[5, 0]
    r = V.viterbi(s)
    assert np.isfinite(r["logp"]) and np.isfinite(V.local_average_f0(s, r["path"])).all()


def test_local_average_around_the_argmax_is_the_default_decode():
    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))
    for k, th in enumerate(g["decode_thred"]):
        got = np.stack([V.local_average_f0(s, s.argmax(1), float(th)) for s in g["decode_sal"]])
        assert np.array_equal(got > 0, g[f"decode_f64_{k}"] > 0) and np.abs(got - g[f"decode_f64_{k}"]).max() <= 1e-9


def test_viterbi_tables_equal_the_oracle_bit_for_bit():
    from stylish_tts_amd import rmvpe

    band, lt_out, eps = rmvpe.viterbi_tables()
    L = V.lt()
    assert band.shape == (360, 59) and band.dtype == np.float64 and eps == V.EPS == 2.0**-126 and lt_out == L[0, 359]
    for j in range(360):
        for k in range(59):
            i = j - 29 + k
            assert band[j, k] == (L[i, j] if 0 <= i < 360 else -np.inf), (j, k)
    assert np.array_equal(rmvpe.viterbi_transition(), L)
    assert rmvpe.viterbi_tables()[0] is band  # built once


def test_library_entry_points_and_workspace_query():
    from stylish_tts_amd import _lib

    lib = _lib.load()
    for name in ("stts_rmvpe_viterbi", "stts_rmvpe_viterbi_workspace_bytes", "stts_rmvpe_decode_at"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    off = (C.c_int32 * 4)(0, 1, 3, 260)
    need = lib.stts_rmvpe_viterbi_workspace_bytes(3, off)
    assert need >= 260 * 360 * 2 + 260 * 8 + 260 * 4  # back pointers, frame sums, the path
    assert need <= 260 * 360 * 2 + 260 * 8 + 260 * 4 + 3 * 256 + 4096
    assert lib.stts_rmvpe_viterbi_workspace_bytes(2, (C.c_int32 * 3)(0, 5, 5)) == 0  # an utterance without frames
    assert lib.stts_rmvpe_viterbi_workspace_bytes(0, off) == 0 and lib.stts_rmvpe_viterbi_workspace_bytes(1, None) == 0


def test_the_shims_take_the_decoder_keyword_and_refuse_bad_shapes_without_a_gpu():
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import modules
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    m = modules.RmvpePitchExtractor(config=NARROW).load_synthetic(0)
    for fn in (m.decode, m.packed, m.forward, m.packed_from_audio, m.infer_from_audio, VoiceConverter.convert_audio):
        assert inspect.signature(fn).parameters["decoder"].default == "argmax"
    sig = inspect.signature(m.decode)
    assert sig.parameters["lengths"].default is None and sig.parameters["return_path"].default is False
    sig = inspect.signature(HipModel.rmvpe_viterbi)
    assert list(sig.parameters) == ["self", "seg", "salience", "thred", "path", "logp"] and sig.parameters["thred"].default == 0.03
    for bad in (torch.zeros(360), torch.zeros(2, 20, 359), torch.zeros(1, 2, 20, 360), torch.zeros(0, 360)):
        with pytest.raises(ValueError, match="salience"):
            m.decode(bad, decoder="viterbi")
    for lengths in ([20, 20], [21], [0]):
        with pytest.raises(ValueError, match="lengths"):
            m.decode(torch.zeros(1, 20, 360), decoder="viterbi", lengths=lengths)
    with pytest.raises(ValueError, match="viterbi"):
        m.decode(torch.zeros(1, 20, 360), lengths=[20])
    for fn, arg in ((m.decode, torch.zeros(1, 20, 360)), (m.forward, torch.zeros(1, 128, 40)), (m.packed, torch.zeros(1, 128, 40)),
                    (m.packed_from_audio, torch.zeros(1, 16000)), (m.infer_from_audio, torch.zeros(1, 16000))):
        with pytest.raises(ValueError, match="decoder must be one of"):
            fn(arg, decoder="librosa")
    # the reference's own flag keeps raising, and names the keyword that is built
    with pytest.raises(NotImplementedError, match='decoder="viterbi"'):
        m.decode(torch.zeros(1, 20, 360), use_viterbi=True)
    with pytest.raises(NotImplementedError, match='decoder="viterbi"'):
        m.infer_from_audio(torch.zeros(1, 16000), use_viterbi=True, decoder="viterbi")
    # the length rules of the audio entry hold in front of the new keyword too
    with pytest.raises(ValueError, match="512"):
        m.infer_from_audio(torch.zeros(1, 512), decoder="viterbi")
    with pytest.raises(ValueError, match="16000"):
        m.infer_from_audio(torch.zeros(1, 24000), sample_rate=24000, decoder="viterbi")
    with pytest.raises(ValueError, match="lengths"):
        m(torch.zeros(2, 128, 40), lengths=[40, 41], decoder="viterbi")
