"""The flow statistics on the engine (csrc/flow_stats.hip.h) against tests/flowstats64.py (numpy float64) and the reference fixtures of
tests/golden/gen_golden_flowstats.py.

Bars.  A coupling layer alone: the engine's error of each stream (and of the next layer's h_0 where the form hands it back) against float64 over
the error of the same layer computed in fp32 by torch on the CPU from the same inputs - max-abs and rms ratios each <= BAR = 4, the project's
standing margin over the reference's own rounding.  The stage: every stream within BAR x the fixture's recorded fp32-reference error, in every form
and the planned one.  The KL reduction: within (N + 16) 2^-53 sum |piece| of the float64 numpy sum over the same fp32 inputs - N roundings of a
fixed-order fp64 sum plus a few ulp per piece for exp; N = the utterance's rows x 128, a piece = each of the two summands of the per-element term
(flowstats64.kl_pieces), whose magnitudes bound the rounding of the term even where they cancel.  Run with -s to see the figures (DESIGN.md 5q
quotes them)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
import flowstats64 as S  # noqa: E402
import flowstats_cases as C  # noqa: E402

BAR = C.BAR
FORMS = (0, 16, 32, 64)
W_POSTERIOR, W_FLOW_STATS = 262144, 524288

_S = {}


def env(cfg):
    """One fp32 engine with the speech predictor and the posterior encoder (synthetic weights, seed 0), everything finalized."""
    if not _S:
        from stylish_tts_amd import params
        from stylish_tts_amd.runtime import HipModel

        w, fws = C.weights(cfg)
        sd = params.synth_state_dict(params.posterior_encoder_spec(cfg, ""), 0, prefix="speech_predictor.posterior_encoder.")
        m = HipModel(cfg, 0)
        m.load_state_dict("speech_predictor", w)
        m.load_state_dict("speech_predictor", sd, prefix="posterior_encoder.")
        m.finalize(15 | W_POSTERIOR | W_FLOW_STATS)
        _S.update(m=m, w=w, fws=fws, g=C.fixture())
    return _S


class forced:
    """STTS_FSTAT_WN for the calls inside (the library reads it on every call); None = the plan's own choice."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.get("STTS_FSTAT_WN")
        if self.form is None:
            os.environ.pop("STTS_FSTAT_WN", None)
        else:
            os.environ["STTS_FSTAT_WN"] = str(self.form)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STTS_FSTAT_WN", None)
        else:
            os.environ["STTS_FSTAT_WN"] = self.old


def dev(m, a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C", copy=True)).to(m.device)


def seg_of(m, lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments([int(n) for n in lengths], m.device)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("f", (0, 3, 7))
@pytest.mark.parametrize("batch", ("ragged", "ones"))
def test_layer_alone(cfg, batch, f, reverse, form):
    s = env(cfg)
    m = s["m"]
    c = C.layer_case(cfg, batch, f, reverse)
    R = sum(c["lengths"])
    outs = m.op_flow_stats_layer(seg_of(m, c["lengths"]), f, dev(m, c["z"]), dev(m, c["mean"]), dev(m, c["logstd"]), dev(m, c["style"]), reverse, form=form, pad_rows=8)
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    assert all(np.isnan(o[R:]).all() for o in outs), "rows behind the last utterance were written"
    p = f & 1
    for o, k in zip(outs, C.STREAMS):  # the half the layer reads leaves it bit-identical
        assert np.array_equal(o[:R, p * 64 : (p + 1) * 64], c[k][:, p * 64 : (p + 1) * 64]), f"{k}: the untouched half changed"
    has_h0 = form != 0 and c["ref"][3] is not None
    if not has_h0:
        assert np.isnan(outs[3]).all(), "h0 was written by a form / layer that has none"
    print(f"layer {f} {'reverse' if reverse else 'forward'} {batch} form {form}")
    worst = C.layer_worst_ratio(c, [o[:R] for o in outs[:3]] + ([outs[3][:R]] if has_h0 else []))
    assert worst <= BAR


def run_stage(s, form, reverse, three=None, lengths=None, style=None, m=None):
    m, g = m or s["m"], s["g"]
    three = three if three is not None else tuple(g[k] for k in C.STREAMS)
    lengths = lengths if lengths is not None else np.diff(g["off"])
    with forced(form):
        o = m.flow_stats(seg_of(m, lengths), *(dev(m, a) for a in three), dev(m, g["style"] if style is None else style), reverse)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_streams(g, o, name, label):
    worst = 0.0
    for k in C.STREAMS:
        emax, erms = S.err(o[k], g[f"{name}_{k}"])
        rmax, rrms = g[f"err_{name}_{k}"]
        print(f"{label} {k:7s}: engine max {emax:.2e} rms {erms:.2e} | reference fp32 max {rmax:.2e} rms {rrms:.2e} | ratio {emax / rmax:.2f} {erms / rrms:.2f}")
        worst = max(worst, emax / rmax, erms / rrms)
    assert worst <= BAR, f"{label}: worst ratio {worst:.2f}"


@pytest.mark.parametrize("form", FORMS + (None,))
@pytest.mark.parametrize("reverse", (False, True))
def test_stage_against_the_fixtures(cfg, reverse, form):
    s = env(cfg)
    check_streams(s["g"], run_stage(s, form, reverse), "rev" if reverse else "fwd", f"{'reverse' if reverse else 'forward'} form {form}")


def test_prior_stats_against_the_fixture(cfg):
    s = env(cfg)
    m, g = s["m"], s["g"]
    o = m.prior_stats(seg_of(m, np.diff(g["off"])), dev(m, g["x"]), dev(m, g["noise"]))
    torch.cuda.synchronize()
    check_streams(g, {k: v.cpu().numpy() for k, v in o.items()}, "prior", "prior")


def test_kl_sums_alone(cfg):
    s = env(cfg)
    m, g = s["m"], s["g"]
    off = g["off"]
    seg = seg_of(m, np.diff(off))
    f32 = lambda k: g[k].astype(np.float32)  # noqa: E731
    for kind, names in ((0, ("fwd_z", "fwd_logstd", "prior_mean", "prior_logstd")), (1, ("t2m_mean", "t2m_logstd", "mean", "logstd"))):
        a, b, c, d = (f32(k) for k in names)
        got = m.kl_sums(seg, kind, dev(m, a), dev(m, b), dev(m, c), dev(m, d)).cpu().numpy()
        want = S.kl_sums(kind, a, b, c, d, off)
        p0, p1 = S.kl_pieces(kind, a, b, c, d)
        mag = (np.abs(p0) + np.abs(p1)).sum(1)
        for u in range(len(off) - 1):
            n = (off[u + 1] - off[u]) * a.shape[1]
            bound = (n + 16) * 2.0 ** -53 * mag[off[u] : off[u + 1]].sum()
            print(f"kl kind {kind} utterance {u}: engine {got[u]:.17g} numpy {want[u]:.17g} diff {abs(got[u] - want[u]):.3g} bound {bound:.3g}")
            assert abs(got[u] - want[u]) <= bound
        again = m.kl_sums(seg, kind, dev(m, a), dev(m, b), dev(m, c), dev(m, d)).cpu().numpy()
        assert np.array_equal(got, again), "two calls differ: the reduction has no fixed order"


def test_end_to_end_kl_scores_are_reported(cfg):
    """kl_text / kl_audio from the engine's own statistics against the fixture's float64 scores: printed, not a bar - the bars sit on
    the taps and on the reduction."""
    s = env(cfg)
    m, g = s["m"], s["g"]
    seg = seg_of(m, np.diff(g["off"]))
    style = dev(m, g["style"])
    text = m.prior_stats(seg, dev(m, g["x"]), dev(m, g["noise"]))
    t2m = m.flow_stats(seg, text["z"], text["mean"], text["logstd"], style, True)
    mel = {k: dev(m, g[k]) for k in C.STREAMS}
    m2t = m.flow_stats(seg, mel["z"], mel["mean"], mel["logstd"], style, False)
    R = seg.rows
    kl_text = float(m.kl_sums(seg, 0, m2t["z"], m2t["logstd"], text["mean"], text["logstd"]).sum().item()) / R
    kl_audio = float(m.kl_sums(seg, 1, t2m["mean"], t2m["logstd"], mel["mean"], mel["logstd"]).sum().item()) / R
    for name, v in (("kl_text", kl_text), ("kl_audio", kl_audio)):
        print(f"{name}: engine {v:.10g} float64 {g[name][0]:.10g} diff {abs(v - g[name][0]):.3g} | reference fp32 diff {abs(g[name][1] - g[name][0]):.3g}")
        assert np.isfinite(v)


def test_ragged_equals_solo_and_repeats(cfg):
    s = env(cfg)
    g = s["g"]
    off = g["off"]
    for form in FORMS:
        for reverse in (False, True):
            full, twice = run_stage(s, form, reverse), run_stage(s, form, reverse)
            for k in C.STREAMS:
                assert np.array_equal(full[k], twice[k]), f"form {form}: two calls differ in {k}"
            for u in range(len(off) - 1):
                rows = slice(int(off[u]), int(off[u + 1]))
                solo = run_stage(s, form, reverse, three=tuple(g[k][rows] for k in C.STREAMS), lengths=[rows.stop - rows.start], style=g["style"][u : u + 1])
                for k in C.STREAMS:
                    assert np.array_equal(full[k][rows], solo[k]), f"form {form}: utterance {u} alone differs in {k}"


def test_finalized_alone_and_on_a_bf16_engine_give_the_same_bits(cfg):
    from stylish_tts_amd.runtime import HipModel

    s = env(cfg)
    g = s["g"]
    ref = {rev: run_stage(s, None, rev) for rev in (False, True)}
    seg_lens = np.diff(g["off"])
    pr = s["m"].prior_stats(seg_of(s["m"], seg_lens), dev(s["m"], g["x"]), dev(s["m"], g["noise"]))
    for precision, which in (("f32", (W_FLOW_STATS,)), ("f32", (W_FLOW_STATS, 7)), ("bf16", (7, W_FLOW_STATS))):
        m2 = HipModel(cfg, 0, precision=precision)
        m2.load_state_dict("speech_predictor", s["w"])
        for bits in which:  # alone, before the frame path's components, after them on a 16-bit engine
            m2.finalize(bits)
        for rev in (False, True):
            o = run_stage(s, None, rev, m=m2)
            for k in C.STREAMS:
                assert np.array_equal(o[k], ref[rev][k]), f"{precision} {which}: {k} differs"
        p2 = m2.prior_stats(seg_of(m2, seg_lens), dev(m2, g["x"]), dev(m2, g["noise"]))
        for k in C.STREAMS:
            assert torch.equal(p2[k].cpu(), pr[k].cpu()), f"{precision} {which}: prior {k} differs"
        m2.close()


def test_concurrent_streams_stay_bit_identical(cfg):
    """Three stage calls in flight on their own streams, a split-fp32 frame path beside them: every one equals the call alone."""
    import threading

    from stylish_tts_amd import synth

    s = env(cfg)
    m = s["m"]
    alone = {rev: run_stage(s, None, rev) for rev in (False, True)}
    seg4 = seg_of(m, [64, 96])
    R4 = seg4.rows
    fp_in = dict(asr=dev(m, synth.normal("fst.asr", (R4, cfg.inter_dim))), pitch=dev(m, np.abs(synth.normal("fst.f0", (R4,))) * 60 + 120),
                 energy=dev(m, synth.normal("fst.en", (R4,))), style=dev(m, synth.normal("fst.sty", (2, cfg.style_dim))),
                 prior_noise=dev(m, synth.normal("fst.pn", (R4, 128))), src_noise=dev(m, synth.normal("fst.sn", (R4 * 75,))), init_phase=dev(m, synth.uniform("fst.ph", (1,))))
    results, errors = [None] * 3, []

    def work(j):
        try:
            torch.cuda.set_device(m.device)
            st = torch.cuda.Stream(device=m.device)
            with torch.cuda.stream(st):
                for _ in range(3):
                    results[j] = {rev: run_stage(s, None, rev) for rev in (False, True)}
                    if j == 0:
                        m.frame_path(seg4, fp_in["asr"], fp_in["pitch"], fp_in["energy"], fp_in["style"], fp_in["prior_noise"], fp_in["src_noise"], fp_in["init_phase"],
                                     batch_scope=False)
            st.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(j,)) for j in range(3)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for r in results:
        for rev in (False, True):
            for k in C.STREAMS:
                assert np.array_equal(r[rev][k], alone[rev][k])


def test_refusals_and_the_exact_workspace(cfg):
    from stylish_tts_amd.runtime import HipModel, Segments, _ptr, _stream

    s = env(cfg)
    m, g = s["m"], s["g"]
    seg = seg_of(m, [16, 5])
    R = seg.rows
    three = [dev(m, g[k][:R]) for k in C.STREAMS]
    style = dev(m, g["style"][:2])
    outs = [torch.full((R, 128), 7.0, device=m.device) for _ in range(3)]
    need = m.flow_stats_workspace_bytes(seg)
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)

    def call(nbytes, flags=0, ins=three, o=outs):
        return m.lib.stts_flow_stats_forward(m.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), 1, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(style), _ptr(o[0]),
                                             _ptr(o[1]), _ptr(o[2]), _ptr(ws), nbytes, flags)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == 7.0).all()) for o in outs)

    assert call(need - 1) != 0 and b"workspace too small" in m.lib.stts_last_error() and untouched()
    assert call(need, flags=1) != 0 and b"plain segments" in m.lib.stts_last_error() and untouched()
    assert call(need, o=[three[0], outs[1], outs[2]]) != 0 and b"other buffers" in m.lib.stts_last_error() and untouched()
    x = dev(m, g["x"][:R])
    nz = dev(m, g["noise"][:R])
    assert m.lib.stts_prior_stats_forward(m.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(x), 256, _ptr(nz), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                          None, 0, 0) != 0
    assert b"ld_x" in m.lib.stts_last_error() and untouched()
    with pytest.raises(RuntimeError, match="plain segments"):
        m.prior_stats(Segments.capacity([16, 5], m.device), x, nz)
    assert call(need) == 0  # exactly what the stage carves is accepted
    torch.cuda.synchronize()
    assert not any(bool((o == 7.0).any()) for o in outs)
    # a missing component: an engine with the frame path only
    m2 = HipModel(cfg, 0)
    m2.load_state_dict("speech_predictor", s["w"])
    m2.finalize(7)
    assert m2.flow_stats_workspace_bytes(seg_of(m2, [16])) == 0
    with pytest.raises(RuntimeError, match="not finalized"):
        m2.flow_stats(seg_of(m2, [16]), *(dev(m2, g[k][:16]) for k in C.STREAMS), dev(m2, g["style"][:1]), True)
    with pytest.raises(RuntimeError, match="not finalized"):
        m2.prior_stats(seg_of(m2, [16]), dev(m2, g["x"][:16]), dev(m2, g["noise"][:16]))
    m2.close()


def test_module_level(cfg):
    import posterior64 as P64

    from stylish_tts_amd import modules, pipeline
    from stylish_tts_amd.runtime import Segments

    s = env(cfg)
    m = s["m"]
    pe = modules.PosteriorEncoder.from_config(cfg, engine=m).load_synthetic(0)
    sp = modules.SpeechPredictor(cfg, engine=m).load_synthetic(0)
    sp.attach_posterior(pe)
    T, P = 6, 5
    texts = torch.tensor([[3, 9, 4, 17, 8]])
    lens = torch.tensor([P])
    al = torch.zeros(1, P, T)
    t0 = 0
    for p_, d in enumerate([1, 2, 1, 1, 1]):
        al[0, p_, t0 : t0 + d] = 1
        t0 += d
    pitch, energy = torch.full((1, T), 150.0), 0.3 * torch.randn(1, T, generator=torch.Generator().manual_seed(9))
    wave = torch.from_numpy(P64.recording(77, 300 * T))[None]
    gen = lambda seed, *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))  # noqa: E731
    nzd = dict(posterior_noise=gen(1, 1, 128, 4 * T), prior_noise=gen(3, 1, 128, 4 * T), src_noise=gen(2, 1, 1, 300 * T), init_phase=torch.tensor([[0.25]]))
    plain = sp(texts, lens, al, pitch, energy, audio_gt=wave, noise=nzd)
    assert plain.text_stats is None and plain.text2mel_stats is None and plain.mel2text_stats is None
    pred = sp(texts, lens, al, pitch, energy, audio_gt=wave, noise=nzd, flow_stats=True)
    assert modules.has_flow_stats(pred) and all(t.shape == (1, 128, 4 * T) for st_ in (pred.text_stats, pred.text2mel_stats, pred.mel2text_stats) for t in st_)
    assert torch.equal(pred.audio, plain.audio) and torch.equal(pred.magnitude, plain.magnitude) and torch.equal(pred.phase, plain.phase)
    for a, b in zip(pred.mel_stats, plain.mel_stats):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="prior_noise"):
        sp(texts, lens, al, pitch, energy, audio_gt=wave, noise={k: v for k, v in nzd.items() if k != "prior_noise"}, flow_stats=True)
    # the four statistics are the stages' own outputs, bit for bit
    sp_seg, st, st4 = Segments([P], m.device), Segments([T], m.device), Segments([4 * T], m.device)
    enc = m.text_encoder(1, sp_seg, texts[0].to(m.device))
    sty = m.text_style(1, sp_seg, enc)
    dur = al.sum(2).round().to(torch.int32)[0].to(m.device)
    asr = m.length_regulate(sp_seg, st4, dur, 4, enc, cfg.inter_dim)
    x = m.decoder(st4, asr, m.upsample4(st, st4, pitch[0].to(m.device)), m.upsample4(st, st4, energy[0].to(m.device)), sty)
    tm = lambda t: t[0].T.contiguous().to(m.device)  # noqa: E731
    text = m.prior_stats(st4, x, tm(nzd["prior_noise"]))
    t2m = m.flow_stats(st4, text["z"], text["mean"], text["logstd"], sty, True)
    m2t = m.flow_stats(st4, *(tm(t) for t in pred.mel_stats), sty, False)
    for got, want in ((pred.text_stats, text), (pred.text2mel_stats, t2m), (pred.mel2text_stats, m2t)):
        for a, k in zip(got, C.STREAMS):
            assert torch.equal(tm(a), want[k]), k
    # scores: NormalizingFlowLoss, its forward(pred, log), validation_scores
    nf = modules.NormalizingFlowLoss(cfg, engine=m)
    sc = nf.scores(pred)
    assert set(sc) == {"kl_text", "kl_audio", "kl_text_utt", "kl_audio_utt"} and all(np.isfinite(sc[k]) for k in ("kl_text", "kl_audio"))
    want = S.kl_score(0, *(tm(t).cpu().numpy() for t in (pred.mel2text_stats.z, pred.mel2text_stats.logstd, pred.text_stats.mean, pred.text_stats.logstd)))
    assert abs(sc["kl_text"] - want) <= 1e-12 * abs(want)

    class Log:
        def __init__(self):
            self.got = {}

        def add_loss(self, k, v):
            self.got[k] = float(v)

    log = Log()
    nf(pred, log)
    assert log.got == {"kl_text": sc["kl_text"], "kl_audio": sc["kl_audio"]}
    vs = pipeline.validation_scores(m, pred.audio, wave.to(m.device), prediction=pred)
    assert all(vs[k] == sc[k] for k in sc) and np.isfinite(vs["mag"])
    assert "kl_text" not in pipeline.validation_scores(m, plain.audio, wave.to(m.device), prediction=plain)
    # a ragged batch: lists per utterance, each equal to that utterance's own call
    T2 = 5
    texts2 = torch.tensor([[3, 9, 4, 17, 8], [5, 6, 7, 0, 0]])
    lens2 = torch.tensor([5, 3])
    al2 = torch.zeros(2, P, T)
    al2[0] = al[0]
    for p_, (a0, a1) in enumerate(((0, 2), (2, 3), (3, 5))):
        al2[1, p_, a0:a1] = 1
    wave2 = torch.from_numpy(P64.recording(80, 300 * T2))
    pitch2, energy2 = torch.full((2, T), 150.0), 0.3 * gen(10, 2, T)
    nz_r = dict(posterior_noise=gen(5, 2, 128, 4 * T), prior_noise=gen(7, 2, 128, 4 * T), src_noise=gen(6, 2, 1, 300 * T), init_phase=torch.tensor([[0.25]]))
    rag = sp(texts2, lens2, al2, pitch2, energy2, audio_gt=[wave[0], wave2], noise=nz_r, flow_stats=True)
    assert isinstance(rag.text_stats, list) and [t.z.shape for t in rag.mel2text_stats] == [(1, 128, 4 * T), (1, 128, 4 * T2)]
    for u, (tx, ln, Tu, wv) in enumerate(((texts2[:1], lens2[:1], T, wave), (texts2[1:, :3], lens2[1:], T2, wave2[None]))):
        nz_u = {k: (v if k == "init_phase" else v[u : u + 1, :, : (300 if k == "src_noise" else 4) * Tu]) for k, v in nz_r.items()}
        solo = sp(tx, ln, al2[u : u + 1, : int(ln[0]), :Tu], pitch2[u : u + 1, :Tu], energy2[u : u + 1, :Tu], audio_gt=wv, noise=nz_u, flow_stats=True)
        for name in ("text_stats", "text2mel_stats", "mel_stats", "mel2text_stats"):
            for a, b in zip(getattr(rag, name)[u], getattr(solo, name)):
                assert torch.equal(a, b), f"ragged utterance {u}: {name} differs from its own call"
    rs = nf.scores(rag)
    assert len(rs["kl_text_utt"]) == 2 and np.isfinite(rs["kl_audio"])
