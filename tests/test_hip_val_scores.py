"""GPU: the validation scores (csrc/val_scores.hip.h; HipModel.multi_spectrogram / mel_sums / magphase_sums / smooth_l1_sums, modules.MultiSpectrogram /
MultiResolutionSTFTLoss / MagPhaseLoss, pipeline.validation_scores) against the fixtures of tests/golden/gen_golden_valscores.py - the reference's
modules run in fp32 and in float64 - and against tests/valscores64.py, the float64 run restated (the fixtures hold a sample of the tensors only;
tests/test_val_scores_cpu.py pins the restatement on it to 1e-12).  The bar, for every tensor and every sum and score: error against the float64 run
at most 4x the fp32 run's own error on the same input (the bar of the log-mel, HuBERT, RMVPE and aligner ports); since the arithmetic is fp64 the
ratios are expected far below 1 (`pytest -m gpu tests/test_hip_val_scores.py -s` prints them; DESIGN.md section 5n has the measured worst one).  Then
what no fixture holds: ragged = solo, run-to-run and reordering bit equality, the padding columns and the optional outputs of the materialised
rows, the fused sums against the materialised rows, smooth-L1 against numpy float64, the wiring into SpeechPredictor / validation_scores, and bit
stability beside the split-fp32 frame path on another stream.

The zero pattern of the masked phase equals the float64 run's exactly, with no bin exempt.  The generator's condition (a) keeps every magnitude clear
of the mask; its condition (c) requires every kept angle to be an exact 0 (the DC and Nyquist bins with a positive real part, whose imaginary part
is exactly 0 in any transform) or farther than 1e-9 from 0 - which a frame centred on a reflected edge would break, its spectrum being real, so the
signals keep such frames wholly below the mask (tests/valscores64.py, signal)."""
import math
import types

import numpy as np
import pytest

import valscores64 as V
from conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_FFT, WIN, HOP = V.MAGPHASE
BINS = N_FFT // 2 + 1
RATIOS = {}


@pytest.fixture(scope="module")
def eng(cfg):
    from stylish_tts_amd.runtime import HipModel

    e = HipModel(cfg, 0, precision="f32")  # the scores need no weights
    yield e
    e.close()
    if RATIOS:
        print("\n[val_scores] worst ratio of the HIP error to the fp32 run's own error:", {k: f"{v:.2e}" for k, v in sorted(RATIOS.items())})


@pytest.fixture(scope="module")
def ref():
    """Per batch: the fixture, the signals, and the float64 restatement of every tensor - computed once, shared, left unchanged."""
    out = {}
    for key in V.BATCHES:
        tg, pr = V.batch(key)
        tens = [[V.multi_spectrogram(w, res) for w in tg + pr] for res in V.RESOLUTIONS]
        sp = [V.pred_spectra(key, u, w.size // HOP + 1, BINS) for u, w in enumerate(tg)]
        out[key] = types.SimpleNamespace(g=load_golden("valscores_" + key), tg=tg, pr=pr, tens=tens, sp=sp, L=[w.size for w in tg])
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seg_of(eng, L):
    from stylish_tts_amd.runtime import Segments

    return Segments(L, eng.device)


def note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


def within_bar(name, mine, ref64, err, phase=False, factor=4.0):
    e = np.asarray(mine, np.float64).reshape(ref64.shape) - ref64
    if phase:
        e = V.anti_wrap(e)
    mx, rms = np.abs(e).max(), np.sqrt((e * e).mean())
    print(f"  {name}: HIP vs f64 max {mx:.3e} rms {rms:.3e}; fp32 run vs f64 max {err[0]:.3e} rms {err[1]:.3e}; ratios {mx / err[0]:.3f} {rms / err[1]:.3f}")
    note("tensors", max(mx / err[0], rms / err[1]))
    assert mx <= factor * err[0] and rms <= factor * err[1], (name, mx, rms, tuple(err))


def scalar_bar(name, mine, ref64, err, factor=4.0, key="scores"):
    mine, ref64, err = np.asarray(mine, np.float64), np.asarray(ref64, np.float64), np.asarray(err, np.float64)
    e = np.abs(mine.reshape(ref64.shape) - ref64)
    ratio = np.where(err > 0, e / np.where(err > 0, err, 1.0), np.where(e == 0, 0.0, np.inf))
    print(f"  {name}: |HIP - f64| / |fp32 run - f64| = {np.array2string(np.atleast_1d(ratio).ravel(), precision=2)}")
    note(key, ratio.max())
    assert (e <= factor * err).all(), (name, mine, ref64, err)


def zero_pattern(name, phase, ref_phase, ref_mag):
    """Exactly the float64 run's: 0 at every bin it masks off, and among the bins it keeps 0 where its own angle is an exact 0 (the DC and Nyquist
    bins with a positive real part) and nowhere else.  Nothing is exempt: the generator's conditions (a) and (c) keep every bin clear of the mask
    and every kept angle either exactly 0 or far from it."""
    kept = ref_mag > V.MASK
    assert not ((ref_phase != 0) & (np.abs(ref_phase) < 1e-9)).any(), name  # (c), read back on the whole tensors
    assert np.array_equal(phase == 0, ref_phase == 0), (name, int(((phase == 0) != (ref_phase == 0)).sum()))
    assert (ref_phase[~kept] == 0).all() and (ref_phase[kept] == 0).sum() < kept.sum() // 10, name


def packed_spectra(eng, sp, ld=1056):
    la = torch.zeros(sum(s[0].shape[0] for s in sp), ld, device=eng.device)
    ph = torch.zeros_like(la)
    la[:, :BINS], ph[:, :BINS] = dev(np.concatenate([s[0] for s in sp])), dev(np.concatenate([s[1] for s in sp]))
    return la, ph


# ------------------------------------------------------------------------------------------------ 1. MultiSpectrogram tensors
@pytest.mark.parametrize("key", sorted(V.BATCHES))
def test_multi_spectrogram_tensors(eng, ref, key):
    from stylish_tts_amd import modules

    c = ref[key]
    B = len(c.L)
    if key == "B":  # the module's channel-major lists on the equal-length batch
        ms = modules.MultiSpectrogram(sample_rate=V.SR, engine=eng)
        lists = ms(target=torch.from_numpy(np.stack(c.tg)), pred=torch.from_numpy(np.stack(c.pr)))
        assert len(lists) == 6 and all(len(x) == len(V.RESOLUTIONS) for x in lists)
    for r, (fft, hop, win) in enumerate(V.RESOLUTIONS):
        nb, F = fft // 2 + 1, [n // hop + 1 for n in c.L]
        got = {}
        if key == "B":
            for side, q in (("t", 0), ("p", 1)):
                mag, phase, fm = lists[q][r], lists[2 + q][r], lists[4 + q][r]
                assert mag.shape == (B, 1, V.N_MELS, F[0]) and phase.shape == (B, nb, F[0]) and fm.shape == (B, 1, nb, F[0])
                tmaj = lambda x: x.reshape(B, -1, F[0]).permute(0, 2, 1).reshape(B * F[0], -1).cpu().numpy()  # noqa: E731
                got[side] = (tmaj(mag), tmaj(phase), tmaj(fm))
        else:  # packed ragged rows
            for side, ws in (("t", c.tg), ("p", c.pr)):
                seg_m, mag, phase, fm = eng.multi_spectrogram(seg_of(eng, c.L), dev(np.concatenate(ws)), fft, win, hop, V.N_MELS, V.SR, mag=True, phase=True,
                                                              fft_mag=True)
                assert seg_m.lengths == F and mag.shape == (sum(F), V.N_MELS) and phase.shape == fm.shape == (sum(F), nb)
                got[side] = (mag.cpu().numpy(), phase.cpu().numpy(), fm.cpu().numpy())
        want = [np.concatenate([t[q] for t in c.tens[r]]) for q in range(3)]  # targets, then predictions
        for q, name in enumerate(("mag", "phase", "fft_mag")):
            mine = np.concatenate([got["t"][q], got["p"][q]])
            within_bar(f"{key} r{r} {name}", mine, want[q], c.g[f"{name}_err_r{r}"], phase=name == "phase")
        zero_pattern(f"{key} r{r}", np.concatenate([got["t"][1], got["p"][1]]), want[1], want[2])


# ------------------------------------------------------------------------------------------------ 2. sums and scores
@pytest.mark.parametrize("key", sorted(V.BATCHES))
def test_sums_and_scores_against_the_float64_run(eng, ref, key):
    from stylish_tts_amd import modules

    c, g = ref[key], ref[key].g
    seg = seg_of(eng, c.L)
    sums = eng.mel_sums(seg, dev(np.concatenate(c.tg)), dev(np.concatenate(c.pr)), sample_rate=V.SR)
    assert sums.shape == (3, len(c.L), 2) and sums.dtype == torch.float64
    s = sums.cpu().numpy()
    scalar_bar(f"{key} mel sums", s, g["sums64"], g["sums_err"])
    if V.IDENTICAL[key] is not None:
        assert (s[:, V.IDENTICAL[key], 0] == 0.0).all()  # the identical pair: a numerator of exactly 0
    mel, mel_r, mel_utt = modules.mel_score(s.tolist())
    scalar_bar(f"{key} mel", mel, g["mel64"], g["mel_err"])
    scalar_bar(f"{key} mel_r", mel_r, g["mel_r64"], g["mel_r_err"])
    scalar_bar(f"{key} mel_utt", mel_utt, g["mel_utt64"], g["mel_utt_err"])
    rows = [n // HOP + 1 for n in c.L]
    la, ph = packed_spectra(eng, c.sp)
    ph0 = ph.clone()
    mp = eng.magphase_sums(seg, dev(np.concatenate(c.tg)), seg_of(eng, rows), la, ph, la.shape[1], N_FFT, WIN, HOP)
    assert mp.shape == (len(c.L), 4) and mp.dtype == torch.float64 and torch.equal(ph, ph0)
    scalar_bar(f"{key} mag/phase sums", mp.cpu().numpy(), g["mp_sums64"], g["mp_err"])
    mag, phase, terms = modules.magphase_score(mp.cpu().tolist(), sum(rows), BINS)
    scalar_bar(f"{key} mag", mag, g["mag64"], g["mag_err"])
    scalar_bar(f"{key} phase terms", terms, g["terms64"], g["terms_err"])
    scalar_bar(f"{key} phase", phase, g["phase64"], g["phase_err"])
    if key == "B":  # the modules on the batch as it is, against the reference's modules on it
        log = types.SimpleNamespace(v={})
        log.add_loss = lambda k, v: log.v.__setitem__(k, float(v))
        ms = modules.MultiSpectrogram(sample_rate=V.SR, engine=eng)
        lists = ms(target=torch.from_numpy(np.stack(c.tg)), pred=torch.from_numpy(np.stack(c.pr)))
        modules.MultiResolutionSTFTLoss(sample_rate=V.SR)(target_list=lists[0], pred_list=lists[1], log=log)
        pred = types.SimpleNamespace(magnitude=torch.from_numpy(np.stack([x[0].T for x in c.sp])), phase=torch.from_numpy(np.stack([x[1].T for x in c.sp])))
        keep = pred.phase.clone()
        modules.MagPhaseLoss(n_fft=N_FFT, hop_length=4 * HOP, win_length=WIN, engine=eng)(pred, torch.from_numpy(np.stack(c.tg)), log)
        assert torch.equal(pred.phase, keep)  # the reference overwrites pred.phase with its masked copy; the port does not
        for k in ("mel", "mag", "phase"):
            scalar_bar(f"B modules {k}", log.v[k], g[f"{k}_batch64"], g[f"{k}_batch_err"])
        assert log.v["mel"] == mel and log.v["mag"] == mag and log.v["phase"] == phase
        # lists that are not the untouched pair of one forward call - copied here, then edited in place - are scored from their own tensors
        loss = modules.MultiResolutionSTFTLoss(sample_rate=V.SR)
        assert loss(target_list=lists[0], pred_list=lists[1], log=log) == mel and loss.last_path == "fused"
        on_tensors = float(loss(target_list=list(lists[0]), pred_list=list(lists[1]), log=log))
        assert loss.last_path == "tensors"
        scalar_bar("B mel from the fp32 tensors", on_tensors, g["mel_batch64"], g["mel_batch_err"], key="mel from the fp32 tensors")
        want = float(np.mean([float((t.double() - p.double()).abs().sum() / (t.double().abs().sum() + 1e-6)) for t, p in zip(lists[0], lists[1])]))
        assert abs(on_tensors - want) <= 1e-15 * want
        lists[1][0].mul_(2.0)
        edited = float(loss(target_list=lists[0], pred_list=lists[1], log=log))
        assert loss.last_path == "tensors" and edited > 2 * mel


@pytest.mark.parametrize("fft,hop,win", [(256, 64, 256), (4096, 600, 2400)])
def test_the_other_transform_sizes_against_valscores64(eng, ref, fft, hop, win):
    """The two transform sizes the reference's geometries do not use (another kernel instantiation each), against the float64 restatement: fp64 on
    both sides, a few thousand roundings per value, so 1e-9 relative leaves orders of margin over either side's rounding."""
    c = ref["A"]
    L, tg, pr = c.L[:2], c.tg[:2], c.pr[:2]  # 1025 samples are too few for n_fft 4096
    seg = seg_of(eng, L)
    got = eng.mel_sums(seg, dev(np.concatenate(tg)), dev(np.concatenate(pr)), resolutions=[(fft, hop, win)], sample_rate=V.SR).cpu().numpy()
    want = V.mel_sums(tg, pr, [(fft, hop, win)])
    assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all() and (got[0, 1, 0] == 0.0)
    nb, rows = fft // 2 + 1, [n // hop + 1 for n in L]
    sp = [V.pred_spectra("other", u, r, nb) for u, r in enumerate(rows)]
    la, ph = dev(np.concatenate([s[0] for s in sp])), dev(np.concatenate([s[1] for s in sp]))
    mp = eng.magphase_sums(seg, dev(np.concatenate(tg)), seg_of(eng, rows), la, ph, nb, fft, win, hop).cpu().numpy()
    want = V.magphase_sums(tg, [s[0] for s in sp], [s[1] for s in sp], (fft, win, hop))
    assert (np.abs(mp - want) <= 1e-9 * np.abs(want)).all(), (mp, want)
    seg_m, mag, phase, fm = eng.multi_spectrogram(seg, dev(np.concatenate(pr)), fft, win, hop, V.N_MELS, V.SR, mag=True, phase=True, fft_mag=True)
    full = [V.multi_spectrogram(w, (fft, hop, win)) for w in pr]
    for q, mine in enumerate((mag, phase, fm)):
        want = np.concatenate([t[q] for t in full])
        e = mine.double().cpu().numpy() - want
        e = V.anti_wrap(e) if q == 1 else e
        assert np.abs(e).max() <= 2.0**-23 * max(1.0, np.abs(want).max()), (fft, q)  # one rounding to fp32


# ------------------------------------------------------------------------------------------------ 3. bit equality
def test_ragged_equals_solo_repeats_and_reorders_bit_for_bit(eng, ref):
    c = ref["A"]
    B = len(c.L)
    flat = lambda ws: dev(np.concatenate(ws))  # noqa: E731

    def run(order):
        L = [c.L[u] for u in order]
        tg, pr, sp = [c.tg[u] for u in order], [c.pr[u] for u in order], [c.sp[u] for u in order]
        seg = seg_of(eng, L)
        sums = eng.mel_sums(seg, flat(tg), flat(pr), sample_rate=V.SR)
        la, ph = packed_spectra(eng, sp)
        mp = eng.magphase_sums(seg, flat(tg), seg_of(eng, [n // HOP + 1 for n in L]), la, ph, la.shape[1], N_FFT, WIN, HOP)
        rows = [eng.multi_spectrogram(seg, flat(pr), fft, win, hop, V.N_MELS, V.SR, mag=True, phase=True, fft_mag=True) for fft, hop, win in V.RESOLUTIONS]
        return sums, mp, rows

    sums, mp, rows = run(range(B))
    again = run(range(B))
    assert torch.equal(sums, again[0]) and torch.equal(mp, again[1])
    assert all(torch.equal(a, b) for x, y in zip(rows, again[2]) for a, b in zip(x[1:], y[1:]))
    for u in range(B):  # every utterance alone
        s1, m1, r1 = run([u])
        assert torch.equal(s1[:, 0], sums[:, u]) and torch.equal(m1[0], mp[u]), u
        for (seg_m, *full), (_, *solo) in zip(rows, r1):
            lo, hi = seg_m.host[u], seg_m.host[u + 1]
            assert all(torch.equal(a[lo:hi], b) for a, b in zip(full, solo)), u
    order = [2, 0, 1]
    s2, m2, _ = run(order)
    assert torch.equal(s2, sums[:, order]) and torch.equal(m2, mp[order])


def test_refusals_name_the_utterance(eng, ref):
    c = ref["A"]
    seg = seg_of(eng, c.L)
    flat = dev(np.concatenate(c.tg))
    with pytest.raises(ValueError, match="utterance 2: the target has 1025 samples, the prediction 1030"):
        eng.mel_sums(seg, flat, torch.zeros(4800 + 3300 + 1030, device=eng.device), sample_rate=V.SR, seg_pred=seg_of(eng, [4800, 3300, 1030]))
    with pytest.raises(ValueError, match="utterance 2 has 1024 samples"):
        eng.mel_sums(seg_of(eng, [4800, 3300, 1024]), flat[:-1], flat[:-1], sample_rate=V.SR)
    la, ph = packed_spectra(eng, c.sp)
    with pytest.raises(ValueError, match="utterance 1 has 44 prediction rows"):
        eng.magphase_sums(seg, flat, seg_of(eng, [65, 44, 14]), la[:-1], ph[:-1], la.shape[1], N_FFT, WIN, HOP)
    with pytest.raises(ValueError, match="win_length"):
        eng.multi_spectrogram(seg, flat, 512, 600, 50)


# ------------------------------------------------------------------------------------------------ 4. materialised rows
def test_padding_columns_and_optional_outputs(eng, ref):
    c = ref["A"]
    seg, flat = seg_of(eng, c.L), dev(np.concatenate(c.pr))
    for fft, hop, win in V.RESOLUTIONS:
        nb = fft // 2 + 1
        seg_m, mag, phase, fm = eng.multi_spectrogram(seg, flat, fft, win, hop, V.N_MELS, V.SR, mag=True, phase=True, fft_mag=True)
        fill = dict(mag=torch.full((seg_m.rows, 160), 7.5, device=eng.device), phase=torch.full((seg_m.rows, nb + 31), 7.5, device=eng.device),
                    fft_mag=torch.full((seg_m.rows, nb + 31), 7.5, device=eng.device))
        eng.multi_spectrogram(seg, flat, fft, win, hop, V.N_MELS, V.SR, out=fill)
        for k, full, width in (("mag", mag, V.N_MELS), ("phase", phase, nb), ("fft_mag", fm, nb)):
            assert torch.equal(fill[k][:, :width], full) and (fill[k][:, width:] == 7.5).all(), (fft, k)
            alone = eng.multi_spectrogram(seg, flat, fft, win, hop, V.N_MELS, V.SR, mag=k == "mag", phase=k == "phase", fft_mag=k == "fft_mag")
            assert [x is None for x in alone[1:]] == [k != "mag", k != "phase", k != "fft_mag"]
            assert torch.equal(alone[1 + ("mag", "phase", "fft_mag").index(k)], full), (fft, k)


# ------------------------------------------------------------------------------------------------ 5. fused against materialised
@pytest.mark.parametrize("key", sorted(V.BATCHES))
def test_fused_sums_against_the_materialised_rows(eng, ref, key):
    """The fused sums never round to fp32; the materialised mag rows do, once, each value by at most 2^-24 of itself: the sums formed on the host in
    float64 from those rows lie within 2^-24 (sum |t| + sum |p|) of the fused numerator and 2^-24 sum |t| of the denominator."""
    c = ref[key]
    seg = seg_of(eng, c.L)
    sums = eng.mel_sums(seg, dev(np.concatenate(c.tg)), dev(np.concatenate(c.pr)), sample_rate=V.SR).cpu().numpy()
    for r, (fft, hop, win) in enumerate(V.RESOLUTIONS):
        seg_m, mt, _, _ = eng.multi_spectrogram(seg, dev(np.concatenate(c.tg)), fft, win, hop, V.N_MELS, V.SR)
        _, mp, _, _ = eng.multi_spectrogram(seg, dev(np.concatenate(c.pr)), fft, win, hop, V.N_MELS, V.SR)
        mt, mp = mt.double().cpu().numpy(), mp.double().cpu().numpy()
        for u in range(len(c.L)):
            t, p = mt[seg_m.host[u] : seg_m.host[u + 1]], mp[seg_m.host[u] : seg_m.host[u + 1]]
            num, den, sp = np.abs(t - p).sum(), np.abs(t).sum(), np.abs(p).sum()
            assert abs(num - sums[r, u, 0]) <= 2.0**-24 * (den + sp) and abs(den - sums[r, u, 1]) <= 2.0**-24 * den, (key, r, u)


# ------------------------------------------------------------------------------------------------ 6. smooth-L1
def test_smooth_l1_sums_against_numpy_float64(eng):
    a, b = V.curves("A")
    d = np.abs(a[:4].astype(np.float64) - b[:4].astype(np.float64))
    assert list(d) == [0.0, 1.0, 1.0, 0.0] and (np.abs(a.astype(np.float64) - b) > 1).any() and (np.abs(a.astype(np.float64) - b) < 1).any()
    L = [300, 1, 476]
    got = eng.smooth_l1_sums(seg_of(eng, L), dev(a), dev(b))
    assert got.shape == (3,) and got.dtype == torch.float64
    lo = 0
    for u, n in enumerate(L):
        dd = np.abs(a[lo : lo + n].astype(np.float64) - b[lo : lo + n].astype(np.float64))
        want = math.fsum(np.where(dd < 1.0, 0.5 * dd * dd, dd - 0.5).tolist())
        assert abs(float(got[u]) - want) <= 1e-14 * abs(want), (u, float(got[u]), want)
        lo += n
    assert float(eng.smooth_l1_sums(seg_of(eng, [4]), dev(a[:4]), dev(b[:4]))[0]) == 1.0  # 0 + 0.5 + 0.5 + 0
    again = eng.smooth_l1_sums(seg_of(eng, L), dev(a), dev(b))
    assert torch.equal(got, again)


# ------------------------------------------------------------------------------------------------ 7. wiring
def test_validation_scores_of_a_speech_predictor_prediction():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.pipeline import validation_scores
    from stylish_tts_amd.runtime import HipModel
    from test_oracle_golden import narrow_cfg

    cfg, _ = narrow_cfg()
    eng = HipModel(cfg, 0)
    try:
        sp = modules.SpeechPredictor(cfg, engine=eng).load_synthetic(0)
        P, T = 6, 16
        texts = torch.from_numpy(synth.tokens("vs.tokens", 1, P, 178).astype(np.int64))
        align = torch.from_numpy(synth.alignment_from_durations(synth.durations_for("vs.dur", P, T))[None].astype(np.float32))
        pitch = torch.from_numpy(synth.pitch_curve("vs.pitch", 1, T))
        energy = torch.from_numpy((synth.uniform("vs.energy", (1, T)) * 2.0 + 2.0).astype(np.float32))
        nz = {k: torch.from_numpy(v) for k, v in synth.path_noise("vs", 1, 4 * T, flow_dim=cfg.decoder.hidden_dim // 4).items()}
        pred = sp(texts, torch.tensor([P]), align, pitch, energy, noise=nz)
        audio = pred.audio.reshape(1, -1)
        assert audio.shape[1] == 4 * T * 75 and pred.phase.shape == (1, BINS, 4 * T + 1)
        keep = pred.phase.clone()
        own = validation_scores(eng, audio, audio, prediction=pred)
        assert own["mel"] == 0.0 and own["mel_r"] == [0.0] * 3 and own["mel_utt"] == [0.0] and torch.equal(pred.phase, keep)
        gt = torch.from_numpy(V.perturbed(audio.cpu().numpy(), "narrow"))
        pe = (pitch * 1.05, pitch), (energy + 0.7, energy)
        got = validation_scores(eng, audio, gt, prediction=pred, pitch=pe[0], energy=pe[1])
        assert set(got) == {"mel", "mel_r", "mel_utt", "mag", "phase", "phase_terms", "pitch", "energy"} and torch.equal(pred.phase, keep)
        # the host reads the device once per call: every sum travels in one buffer
        reads, orig = [], {n: getattr(torch.Tensor, n) for n in ("cpu", "tolist", "item", "numpy", "__bool__", "__float__")}

        def spy(n):
            def f(self, *a, **k):
                if self.is_cuda:
                    reads.append(n)
                return orig[n](self, *a, **k)
            return f

        try:
            for n in orig:
                setattr(torch.Tensor, n, spy(n))
            again = validation_scores(eng, audio, gt, prediction=pred, pitch=pe[0], energy=pe[1])
        finally:
            for n, fn in orig.items():
                setattr(torch.Tensor, n, fn)
        assert reads == ["cpu"] and again == got, reads
        # the three modules by hand: the same numbers, bit for bit
        log = types.SimpleNamespace(v={})
        log.add_loss = lambda k, v: log.v.__setitem__(k, float(v))
        lists = modules.MultiSpectrogram(sample_rate=cfg.sample_rate, engine=eng)(target=gt, pred=audio)
        loss = modules.MultiResolutionSTFTLoss(sample_rate=cfg.sample_rate)(target_list=lists[0], pred_list=lists[1], log=log)
        modules.MagPhaseLoss(n_fft=cfg.n_fft, hop_length=cfg.hop_length, win_length=cfg.win_length, engine=eng)(pred, gt, log)
        assert float(loss) == log.v["mel"] == got["mel"] and log.v["mag"] == got["mag"] and log.v["phase"] == got["phase"]
        assert torch.equal(pred.phase, keep)
        # the vocoder's time-major rows in place of the DecoderPrediction (the last row repeated, as the reference pads)
        la, ph = eng.to_time_major(pred.magnitude[:, :, :-1].contiguous()), eng.to_time_major(pred.phase[:, :, :-1].contiguous())
        rows = validation_scores(eng, audio, gt, prediction=(la, ph))
        assert rows["mag"] == got["mag"] and rows["phase"] == got["phase"] and rows["mel"] == got["mel"]
        # and the float64 restatement on the host: fp64 on both sides, a few thousand roundings each
        a64, g64 = audio.cpu().numpy()[0], gt.numpy()[0]
        want = V.mel_score(V.mel_sums([g64], [a64]))
        assert abs(got["mel"] - want[0]) <= 1e-9 * want[0] and got["mel"] > 0
        ms = V.magphase_sums([g64], [pred.magnitude[0].cpu().numpy().T], [pred.phase[0].cpu().numpy().T])
        mag, phase, _ = V.magphase_score(ms, 4 * T + 1, BINS)
        assert abs(got["mag"] - mag) <= 1e-9 * mag and abs(got["phase"] - phase) <= 1e-9 * phase
        assert abs(got["pitch"] - V.smooth_l1_sum(pe[0][0].numpy(), pe[0][1].numpy()) / T) <= 1e-12 * got["pitch"]
        assert abs(got["energy"] - V.smooth_l1_sum(pe[1][0].numpy(), pe[1][1].numpy()) / T) <= 1e-12 * got["energy"]
        with pytest.raises(ValueError, match="utterance 0: the target has 4801 samples, the prediction 4800"):
            validation_scores(eng, audio, torch.zeros(1, 4801))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 8. beside other streams
def test_fused_mel_bit_stable_beside_split_fp32_frame_path(cfg, ref):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    devid = eng.device
    c = ref["A"]
    tg, pr = dev(np.concatenate(c.tg)), dev(np.concatenate(c.pr))
    seg_s = Segments(c.L, devid)
    L = [240] * 4
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("vsc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("vsc.f0", (R,))) * 60 + 120), energy=dev(synth.normal("vsc.en", (R,))),
              style=dev(synth.normal("vsc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("vsc.pn", (R, 128))), sn=dev(synth.normal("vsc.sn", (R * 75,))),
              ph=dev(synth.uniform("vsc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    def run():
        return eng.mel_sums(seg_s, tg, pr, sample_rate=V.SR)

    solo = run().clone()
    torch.cuda.synchronize()
    scalar_bar("A mel sums (solo)", solo.cpu().numpy(), c.g["sums64"], c.g["sums_err"])
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(4):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def mels():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [run() for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    with ThreadPoolExecutor(2) as ex:
        f = ex.submit(frames)
        got = ex.submit(mels).result()
        f.result()
    for j, out in enumerate(got):
        assert torch.equal(out, solo), j
    eng.close()
