"""No GPU: the host side of the validation scores (csrc/val_scores.hip.h) - tests/valscores64.py against the float64 arrays of the fixtures
(tests/golden/gen_golden_valscores.py: the reference's MultiSpectrogram / MultiResolutionSTFTLoss / MagPhaseLoss run in float64), the modules'
constructor and forward signatures against the reference's (listed here by name), the ValueError paths that need no device, the library's
host-only size helper against what the Python side allocates, and the filter table every run sums."""
import ctypes as C
import inspect

import numpy as np
import pytest

import valscores64 as V
from conftest import load_golden

KEYS = sorted(V.BATCHES)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.fixture(scope="module", params=KEYS)
def case(request):
    g = load_golden("valscores_" + request.param)
    assert int(g["seed"]) == V.SEED, "the fixtures were made under another seed than tests/valscores64.py SEED"
    tg, pr = V.batch(request.param)
    assert [w.size for w in tg] == list(g["lengths"]) == list(V.BATCHES[request.param])
    assert np.array_equal(np.concatenate(tg).view(np.uint32), g["target"].view(np.uint32)), "the recipes no longer give the fixtures' recordings"
    assert np.array_equal(np.concatenate(pr).view(np.uint32), g["pred"].view(np.uint32))
    return request.param, g, tg, pr


def test_signals_have_what_the_kernels_can_get_wrong(case):
    key, g, tg, pr = case
    for u, (t, p) in enumerate(zip(tg, pr)):
        assert (t == 0).sum() >= 200 and ((np.abs(t) > 0) & (np.abs(t) < 3e-4)).sum() >= 200  # exact zeros, and a stretch around 1e-4
        assert np.array_equal(t, p) == (u == V.IDENTICAL[key])
        for res in V.RESOLUTIONS:
            m = V.multi_spectrogram(t, res)[2]
            assert (m > V.MASK).any() and ((m > 0) & (m <= V.MASK)).any()  # bins on both sides of the mask
    assert (V.multi_spectrogram(tg[0], V.RESOLUTIONS[0])[2] == 0).all(axis=1).any()  # a frame of exact zeros
    fb = V.filters(512)
    assert ((fb > 0).sum(axis=1) == 0).any() and ((fb > 0).sum(axis=1) == 1).any()  # at fft 512 the lowest filters are empty or one bin wide


def test_valscores64_reproduces_the_float64_tensors(case):
    key, g, tg, pr = case
    for r, res in enumerate(V.RESOLUTIONS):
        mine = [V.multi_spectrogram(w, res) for w in tg + pr]
        assert list(g[f"rows_r{r}"]) == [len(m[0][::6]) for m in mine]
        for q, name in enumerate(("mag", "phase", "fft_mag")):
            got, want = np.concatenate([m[q][::6] for m in mine]), g[f"{name}64_r{r}"]
            assert got.shape == want.shape
            if name == "phase":  # masked phases, compared as the anti-wrapping distance: the same angle on the other side of the cut is no error
                assert V.anti_wrap(got - want).max() < 1e-12 * np.pi
                on = np.concatenate([m[2][::6] for m in mine]) > V.MASK
                assert (want[~on] == 0).all() and (got[~on] == 0).all()
                assert np.array_equal(got == 0, want == 0) and not ((want != 0) & (np.abs(want) < 1e-9)).any()  # the generator's condition (c)
            else:
                assert rel(got, want) < 1e-12, (key, r, name)


def test_valscores64_reproduces_the_float64_scores(case):
    key, g, tg, pr = case
    sums = V.mel_sums(tg, pr)
    mel, mel_r, mel_utt = V.mel_score(sums)
    assert rel(sums, g["sums64"]) < 1e-12 and rel(mel, g["mel64"]) < 1e-12 and rel(mel_r, g["mel_r64"]) < 1e-12 and rel(mel_utt, g["mel_utt64"]) < 1e-12
    if V.IDENTICAL[key] is not None:
        assert (sums[:, V.IDENTICAL[key], 0] == 0).all() and mel_utt[V.IDENTICAL[key]] == 0
    n_fft, _, hop = V.MAGPHASE
    sp = [V.pred_spectra(key, u, w.size // hop + 1, n_fft // 2 + 1) for u, w in enumerate(tg)]
    ms = V.magphase_sums(tg, [s[0] for s in sp], [s[1] for s in sp])
    mag, phase, terms = V.magphase_score(ms, sum(w.size // hop + 1 for w in tg), n_fft // 2 + 1)
    assert rel(ms, g["mp_sums64"]) < 1e-12 and rel(mag, g["mag64"]) < 1e-12 and rel(phase, g["phase64"]) < 1e-12 and rel(terms, g["terms64"]) < 1e-12
    assert rel(V.smooth_l1_sum(*V.curves(key)), g["pitch64"]) < 1e-12
    if "mel_batch64" in g.files:  # the reference's modules on the equal-length batch as it is
        assert rel(mel, g["mel_batch64"]) < 1e-12 and rel(mag, g["mag_batch64"]) < 1e-12 and rel(phase, g["phase_batch64"]) < 1e-12


def test_fixture_conditions(case):
    """What the generator asserted, read back: every scalar's fp32-run error is at least 1e-10 of it (an exact 0 aside), so no bar is empty."""
    _, g, _, _ = case
    for k in ("sums", "mel_utt", "mel_r", "mel", "mag", "phase", "terms", "pitch"):
        a, e = np.asarray(g[k + "64"]), np.asarray(g[k + "_err"])
        assert ((a == 0) | (e >= 1e-10 * np.abs(a))).all(), k
    a, e = g["mp_sums64"], g["mp_err"]
    assert (e >= 1e-10 * np.abs(a)).all()
    for r in range(len(V.RESOLUTIONS)):
        for name in ("mag", "phase", "fft_mag"):
            assert (g[f"{name}_err_r{r}"] > 0).all()


def test_host_scores_are_valscores64s(case):
    """modules.mel_score / magphase_score: the plain float64 arithmetic between the device sums and the reported numbers."""
    from stylish_tts_amd import modules

    _, g, tg, _ = case
    mel, mel_r, mel_utt = modules.mel_score(g["sums64"].tolist())
    want = V.mel_score(g["sums64"])
    assert rel(mel, want[0]) < 1e-15 and rel(mel_r, want[1]) < 1e-15 and rel(mel_utt, want[2]) < 1e-15
    n_fft, _, hop = V.MAGPHASE
    rows = sum(w.size // hop + 1 for w in tg)
    mag, phase, terms = modules.magphase_score(g["mp_sums64"].tolist(), rows, n_fft // 2 + 1)
    want = V.magphase_score(g["mp_sums64"], rows, n_fft // 2 + 1)
    assert rel(mag, want[0]) < 1e-15 and rel(phase, want[1]) < 1e-15 and rel(terms, want[2]) < 1e-15


@pytest.mark.parametrize("r", range(len(V.RESOLUTIONS)))
def test_the_filter_table_is_the_one_the_fixtures_were_made_with(r):
    """The fixtures record the filter values the reference's two runs summed (its restated MelScale); the library's host-side table - what
    log_mel_tables uploads for the kernels, and what tests/valscores64.py sums - must be those values bit for bit, or filter rounding would enter
    every comparison.  Beside it the formula: torchaudio's triangles in float64, rounded once."""
    from stylish_tts_amd import log_mel

    n_fft = V.RESOLUTIONS[r][0]
    table, band = log_mel.filter_table(n_fft, V.N_MELS, V.SR)
    for key in KEYS:
        g = load_golden("valscores_" + key)
        assert np.array_equal(np.flatnonzero(table), g[f"fb_idx_r{r}"])
        assert np.array_equal(table.ravel()[g[f"fb_idx_r{r}"]].view(np.uint32), g[f"fb_val_r{r}"].view(np.uint32))
    ref = V.formula_filters(n_fft).astype(np.float64)
    assert (np.abs(table.astype(np.float64) - ref) <= np.maximum(np.abs(ref) * 2.0**-23, 1e-30)).all()
    assert ((table > 0).sum(axis=1) == band[:, 1] - band[:, 0]).all()


# the reference's constructors and forwards, by parameter name and kind (train/multi_spectrogram.py:25-57, train/losses.py:14-27, :85-108)
P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
SIGNATURES = {
    ("MultiSpectrogram", "__init__"): [("resolutions", P), ("window", P), ("sample_rate", K)],
    ("MultiSpectrogram", "calculate_single"): [("audio", P), ("index", P), ("item", P)],
    ("MultiSpectrogram", "forward"): [("target", K), ("pred", K)],
    ("MultiResolutionSTFTLoss", "__init__"): [("sample_rate", K)],
    ("MultiResolutionSTFTLoss", "forward"): [("target_list", K), ("pred_list", K), ("log", K)],
    ("MagPhaseLoss", "__init__"): [("n_fft", K), ("hop_length", K), ("win_length", K)],
    ("MagPhaseLoss", "forward"): [("pred", P), ("gt", P), ("log", P)],
}


@pytest.mark.parametrize("cls,fn", sorted(SIGNATURES))
def test_module_signatures_are_the_references(cls, fn):
    from stylish_tts_amd import modules

    ps = [(p.name, p.kind) for p in inspect.signature(getattr(getattr(modules, cls), fn)).parameters.values()][1:]
    want = SIGNATURES[(cls, fn)]
    assert ps[: len(want)] == want
    assert all(n in ("engine", "cfg") and k == K for n, k in ps[len(want) :])  # what the port adds: keyword-only, optional


def test_modules_and_resolutions_follow_the_reference():
    from stylish_tts_amd import modules, val_scores

    assert [val_scores.as_tuple(r) for r in val_scores.resolutions] == list(V.RESOLUTIONS) and val_scores.multi_spectrogram_count == 3
    ms = modules.MultiSpectrogram(sample_rate=V.SR)
    assert ms.resolutions == list(V.RESOLUTIONS) and ms.n_mels == V.N_MELS
    mp = modules.MagPhaseLoss(n_fft=2048, hop_length=300, win_length=1200)
    assert (mp.n_fft, mp.win_length, mp.hop_length) == V.MAGPHASE
    assert rel(val_scores.phase_weights(1025), V.phase_weights(1025)) < 1e-15
    with pytest.raises(NotImplementedError):
        modules.MultiSpectrogram(window=np.hanning, sample_rate=V.SR)


def test_geometry_and_length_errors_name_the_rule():
    from stylish_tts_amd import modules, val_scores

    for bad, word in [((1000, 240, 50), "power of two"), ((128, 100, 50), r"outside \[256, 4096\]"), ((512, 600, 50), "win_length"),
                      ((512, 240, 0), "hop_length")]:
        with pytest.raises(ValueError, match=word):
            val_scores.check_geometry(*bad)
        with pytest.raises(ValueError, match=word):
            modules.MultiSpectrogram(resolutions=[(bad[0], bad[2], bad[1])], sample_rate=V.SR)
    with pytest.raises(ValueError, match="n_mels"):
        val_scores.check_geometry(512, 240, 50, 257, V.SR)
    with pytest.raises(ValueError, match=r"utterance 1 has 1024 samples.*n_fft / 2 = 1024"):
        val_scores.frame_counts([4800, 1024], 2048, 240)
    assert val_scores.frame_counts([4800, 3300, 1025], 2048, 240) == [21, 14, 5]
    with pytest.raises(ValueError, match=r"utterance 2: the target has 1025 samples, the prediction 1026"):
        val_scores.check_pair([4800, 3300, 1025], [4800, 3300, 1026])
    with pytest.raises(ValueError, match=r"utterance 1 has 44 prediction rows.*45 frames"):
        val_scores.check_rows([4800, 3300], [65, 44], 75)
    val_scores.check_rows([4800, 3300, 1025], [65, 45, 14], 75)
    with pytest.raises(ValueError, match="hop_length"):
        modules.MagPhaseLoss(n_fft=2048, hop_length=3, win_length=1200)  # hop_length // 4 = 0


@pytest.mark.parametrize("key", KEYS)
def test_val_sizes_equal_what_python_allocates(key):
    from stylish_tts_amd import val_scores

    L = V.BATCHES[key]
    for fft, hop, _ in V.RESOLUTIONS + ((2048, 75, 1200),):
        mine, lib = val_scores.sizes(L, fft, hop), val_scores.lib_sizes(L, fft, hop)
        assert mine == lib and mine["rows"] == sum(n // hop + 1 for n in L)
        assert mine["mel_partials"] == 2 * mine["rows"] and mine["magphase_scratch"] == mine["rows"] * (fft // 2 + 1)
    with pytest.raises(ValueError, match="utterance 2 has 1025 samples"):
        val_scores.lib_sizes([4800, 3300, 1025], 4096, 50)
    with pytest.raises(ValueError, match="power of two"):
        val_scores.lib_sizes([4800], 1000, 50)


def test_the_entry_points_name_the_utterance_before_they_need_a_context():
    """The interface conditions read host arrays only: a null context still gets the status that names the utterance."""
    from stylish_tts_amd import _lib

    lib = _lib.load()
    off = lambda L: np.concatenate([[0], np.cumsum(L)]).astype(np.int32)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    err = lambda: lib.stts_last_error().decode()  # noqa: E731
    s, sp, rows = off([4800, 3300]), off([4800, 3301]), off([97, 67])
    assert lib.stts_val_mel_sums(None, None, 2, p(s), p(sp), None, p(rows), None, None, None, 512, 240, 50, 128, V.SR, None, None) != 0
    assert "utterance 1: the target has 3300 samples, the prediction 3301" in err()
    rows = off([65, 44])
    assert lib.stts_val_magphase_sums(None, None, 2, p(s), None, p(rows), None, None, None, None, 1056, 2048, 1200, 75, None, None, None) != 0
    assert "utterance 1 has 44 rows" in err() and "45 frames" in err()
    rows = off([97, 66])
    assert lib.stts_multi_spectrogram_forward(None, None, 2, p(s), None, p(rows), None, None, 512, 240, 50, 128, V.SR, None, 128, None, None, 257) != 0
    assert "no output" in err()
    assert lib.stts_val_smooth_l1_sums(None, None, 2, p(off([5, 0])), None, None, None, None) != 0
    assert "utterance 1 has no values" in err()
