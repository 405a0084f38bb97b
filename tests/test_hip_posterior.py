"""The posterior encoder on the engine (csrc/posterior.hip.h) against tests/posterior64.py (numpy float64) and the reference fixtures of
tests/golden/gen_golden_posterior.py.

Bars.  A layer alone: the engine's error of h and out against float64 over the error of the same layer computed in fp32 by torch on the CPU from the
same inputs - max-abs and rms ratios each <= BAR = 4, the project's standing margin over the reference's own rounding.  The stage: every tap within
BAR x the fixture's recorded fp32-reference error of that tap (max-abs and rms).  Run with -s to see the ratios (DESIGN.md 5p quotes them)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
import posterior64 as P64  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
FORMS = (0, 16, 32, 64)
W_POSTERIOR = 262144
RAGGED = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]  # crosses every block height and its halo
TAPS = ("x0", "wn", "mean", "logstd", "z", "mel")

_S = {}


def env(cfg):
    """One fp32 engine with the speech predictor and the posterior encoder (synthetic weights, seed 0), the float64 weights, the fixtures."""
    if not _S:
        from stylish_tts_amd import params
        from stylish_tts_amd.runtime import HipModel

        sd = params.synth_state_dict(params.posterior_encoder_spec(cfg, ""), 0, prefix="speech_predictor.posterior_encoder.")
        sp = params.synth_state_dict(params.speech_predictor_spec(cfg), 0, prefix="speech_predictor.")
        m = HipModel(cfg, 0)
        m.load_state_dict("speech_predictor", sp)
        m.load_state_dict("speech_predictor", sd, prefix="posterior_encoder.")
        m.finalize(15 | W_POSTERIOR)
        _S.update(m=m, sd=sd, sp=sp, W=P64.Weights(sd), post_flow=(sp["post_flow.weight"], sp["post_flow.bias"]))
        g = dict(np.load(os.path.join(GOLD, "posterior_narrow.npz")))
        g["har_spec"] = np.load(os.path.join(GOLD, "posterior_narrow_spec.npz"))["har_spec"]
        g["har_phase"] = np.load(os.path.join(GOLD, "posterior_narrow_phase.npz"))["har_phase"]
        misc = dict(np.load(os.path.join(GOLD, "posterior_misc.npz")))
        _S["narrow"], _S["misc"] = g, {k: v for k, v in misc.items() if not k.startswith("g1024_")}
        # one 240-frame utterance: the taps of all rows, the spectra of the first SPEC_ROWS_3S rows
        _S["3s"] = {k: v for f in ("posterior_3s", "posterior_3s_stats", "posterior_3s_spectra") for k, v in np.load(os.path.join(GOLD, f + ".npz")).items()}
        # the second geometry (1024 / 1024 / 256): an engine of its own, built from that config with its own weight inventory
        from stylish_tts_amd.config import load_model_config

        g2 = {k[len("g1024_"):]: v for k, v in misc.items() if k.startswith("g1024_")}
        base = dict(cfg)
        base.update(n_fft=int(g2["geom"][0]), win_length=int(g2["geom"][1]), hop_length=int(g2["geom"][2]))
        cfg2 = load_model_config(base)
        sd2 = params.synth_state_dict(params.posterior_encoder_spec(cfg2, ""), 0, prefix="speech_predictor.posterior_encoder.")
        sp2 = params.synth_state_dict(params.speech_predictor_spec(cfg2), 0, prefix="speech_predictor.")
        m2 = HipModel(cfg2, 0)
        m2.load_state_dict("speech_predictor", sp2)
        m2.load_state_dict("speech_predictor", sd2, prefix="posterior_encoder.")
        m2.finalize(15 | W_POSTERIOR)
        g2["_m"] = m2
        _S["g1024"] = g2
        for g, w in ((_S["narrow"], sp), (_S["misc"], sp), (_S["3s"], sp), (g2, sp2)):
            g["mel"] = g["z"] @ np.asarray(w["post_flow.weight"], np.float64).T + np.asarray(w["post_flow.bias"], np.float64)
    return _S


SPEC_ROWS_3S = 64   # rows of the 240-frame fixture whose spectra are stored
FIELD = 12          # rows a tap looks to either side: 12 layers of k = 3


class forced:
    """STTS_POST_WN for the calls inside (the library reads it on every call)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.get("STTS_POST_WN")
        if self.form is None:
            os.environ.pop("STTS_POST_WN", None)
        else:
            os.environ["STTS_POST_WN"] = str(self.form)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STTS_POST_WN", None)
        else:
            os.environ["STTS_POST_WN"] = self.old


def dev(m, a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C", copy=True)).to(m.device)


def seg_of(m, lengths):
    from stylish_tts_amd.runtime import Segments

    return Segments(lengths, m.device)


def layer_torch32(sd, i, n_layers, h, out, cond, off, acc):
    """The layer in fp32 by torch on the CPU: weight_norm folded in fp32 as torch does, conv1d / linear per utterance."""
    F = torch.nn.functional
    t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float32))  # noqa: E731
    wn = lambda p: torch._weight_norm(t(p + ".weight_v"), t(p + ".weight_g"), 0)  # noqa: E731
    H = h.shape[1]
    win, wrs = wn(f"enc.in_layers.{i}"), wn(f"enc.res_skip_layers.{i}")
    h2, out2 = torch.from_numpy(h.copy()), torch.from_numpy(out.copy()) if acc else torch.zeros(out.shape)
    hin = torch.from_numpy(h)
    for u in range(len(off) - 1):
        lo, hi = int(off[u]), int(off[u + 1])
        xin = F.conv1d(hin[lo:hi].T[None], win, t(f"enc.in_layers.{i}.bias"), padding=1)
        xin = xin + torch.from_numpy(cond[u, i * 2 * H : (i + 1) * 2 * H])[None, :, None]
        acts = torch.tanh(xin[:, :H]) * torch.sigmoid(xin[:, H:])
        rs = F.linear(acts.mT, wrs, t(f"enc.res_skip_layers.{i}.bias"))[0]
        if i < n_layers - 1:
            h2[lo:hi] = hin[lo:hi] + rs[:, :H]
            out2[lo:hi] = out2[lo:hi] + rs[:, H:]
        else:
            out2[lo:hi] = out2[lo:hi] + rs
    return h2.numpy(), out2.numpy()


_LAYER_REF = {}


def layer_case(s, lengths, i):
    """Inputs and the two references of one (batch, layer), computed once and shared by the forms."""
    key = (tuple(lengths), i)
    if key not in _LAYER_REF:
        rng = np.random.default_rng(1000 + 17 * i + len(lengths))
        off = np.concatenate([[0], np.cumsum(lengths)])
        R, H = int(off[-1]), s["W"].hidden
        h, out = rng.standard_normal((R, H)).astype(np.float32), rng.standard_normal((R, H)).astype(np.float32)
        style = (0.5 * rng.standard_normal((len(lengths), 64))).astype(np.float32)
        cond = P64.cond_rows(s["W"], style.astype(np.float64)).astype(np.float32)
        acc = i > 0
        h64, o64 = P64.layer(s["W"], i, h.astype(np.float64), out.astype(np.float64), cond.astype(np.float64), off)
        h32, o32 = layer_torch32(s["sd"], i, s["W"].n_layers, h, out, cond, off, acc)
        _LAYER_REF[key] = dict(off=off, h=h, out=out, cond=cond, h64=h64, o64=o64, eh=P64.err(h32, h64), eo=P64.err(o32, o64))
        for v in _LAYER_REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _LAYER_REF[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", (0, 5, 11))
@pytest.mark.parametrize("batch", ("ragged", "ones"))
def test_layer_alone(cfg, batch, i, form):
    s = env(cfg)
    m = s["m"]
    lengths = RAGGED if batch == "ragged" else [1] * 40
    c = layer_case(s, lengths, i)
    R = int(c["off"][-1])
    h_out, o_out = m.op_posterior_layer(seg_of(m, lengths), i, dev(m, c["h"]), dev(m, c["out"]), dev(m, c["cond"]), form=form, pad_rows=8)
    torch.cuda.synchronize()
    h_out, o_out = h_out.cpu().numpy(), o_out.cpu().numpy()
    assert np.isnan(h_out[R:]).all() and np.isnan(o_out[R:]).all(), "rows behind the last utterance were written"
    worst = 0.0
    pairs = [("out", o_out[:R], c["o64"], c["eo"])]
    if i < s["W"].n_layers - 1:
        pairs.append(("h", h_out[:R], c["h64"], c["eh"]))
    else:
        assert np.array_equal(h_out[:R], c["h"]), "the last layer must leave h alone"
    for name, got, ref, (rmax, rrms) in pairs:
        emax, erms = P64.err(got, ref)
        print(f"layer {i:2d} {batch:6s} form {form:2d} {name:3s}: engine max {emax:.2e} rms {erms:.2e} | torch fp32 max {rmax:.2e} rms {rrms:.2e} | ratio {emax / rmax:.2f} {erms / rrms:.2f}")
        worst = max(worst, emax / rmax, erms / rrms)
    assert worst <= BAR
    if form:  # the fused forms agree with the generic form within the same bar
        g_h, g_o = m.op_posterior_layer(seg_of(m, lengths), i, dev(m, c["h"]), dev(m, c["out"]), dev(m, c["cond"]), form=0)
        assert P64.err(o_out[:R], g_o.cpu().numpy())[0] <= BAR * c["eo"][0]
        if i < s["W"].n_layers - 1:
            assert P64.err(h_out[:R], g_h.cpu().numpy())[0] <= BAR * c["eh"][0]


def run_stage(s, g, form, audio=False, spectra=None, lengths=None, rows=None, taps=True):
    m = g.get("_m", s["m"])
    off = g["off"]
    lengths = [int(off[u + 1] - off[u]) for u in range(len(off) - 1)] if lengths is None else lengths
    sl = slice(None) if rows is None else rows
    style = dev(m, g["style"]) if "style" in g else None
    kw = dict(audio=dev(m, g["audio"])) if audio else dict(spectra=tuple(dev(m, a[sl]) for a in (spectra or (g["har_spec"], g["har_phase"]))))
    with forced(form):
        o = m.posterior(seg_of(m, lengths), style=style, noise=dev(m, g["noise"][sl]), taps=taps, mel=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_taps(g, o, label, rows=slice(None)):
    worst = 0.0
    for k in TAPS:
        emax, erms = P64.err(o[k][rows], g[k][rows])
        rmax, rrms = g["err_" + k]
        print(f"{label} {k:7s}: engine max {emax:.2e} rms {erms:.2e} | reference fp32 max {rmax:.2e} rms {rrms:.2e} | ratio {emax / rmax:.2f} {erms / rrms:.2f}")
        worst = max(worst, emax / rmax, erms / rrms)
    assert worst <= BAR, f"{label}: worst ratio {worst:.2f}"


@pytest.mark.parametrize("form", FORMS + (None,))
@pytest.mark.parametrize("case", ("narrow", "misc", "g1024", "3s"))
def test_stage_from_spectra(cfg, case, form):
    """The float64 fixtures' spectra (fp32) in, every tap and z with the recorded noise; misc is g=None, g1024 the geometry 1024 / 1024 / 256.  Of the
    240-frame utterance the spectra of the first 64 rows are stored: they run as an utterance of 64 rows, whose rows 0 .. 51 see nothing else."""
    s = env(cfg)
    g = s[case]
    if case == "3s":
        n = SPEC_ROWS_3S
        check_taps(g, run_stage(s, g, form, lengths=[n], rows=slice(0, n)), f"{case} form {form}", rows=slice(0, n - FIELD))
    else:
        check_taps(g, run_stage(s, g, form), f"{case} form {form}")


@pytest.mark.parametrize("case", ("narrow", "misc", "g1024", "3s"))
def test_stage_from_audio(cfg, case):
    """3s: all 240 rows from the recording (four 64-row blocks, the halo chain of twelve layers across them); the branch of the stored 64 rows is
    adopted, the rest is the engine's own fp64 transform."""
    from oracle import stylish_oracle as O

    s = env(cfg)
    g = s[case]
    o = run_stage(s, g, None, audio=True)
    nb, n = g["har_spec"].shape[1], g["har_spec"].shape[0]
    emax, erms = P64.err(o["har_spec"][:n, :nb], g["har_spec"])
    print(f"{case} har_spec: engine max {emax:.2e} rms {erms:.2e} | reference fp32 STFT max {g['err_spec'][0]:.2e} rms {g['err_spec'][1]:.2e}")
    assert emax <= BAR * g["err_spec"][0] and erms <= BAR * g["err_spec"][1]
    assert not o["har_spec"][:, nb:].any() and not o["har_phase"][:, nb:].any()
    phase = o["har_phase"][:, :nb].copy()
    phase[:n], bad = O.align_branch(phase[:n], g["har_phase"], o["har_spec"][:n, :nb], return_bad=True)
    assert bad == 0
    for form in (FORMS if case == "3s" else (None,)):
        check_taps(g, run_stage(s, g, form, spectra=(o["har_spec"][:, :nb], phase)), f"{case} adopted form {form}")
    again = run_stage(s, g, None, spectra=(o["har_spec"], o["har_phase"]))
    for k in TAPS + ("mean", "logstd"):
        assert np.array_equal(o[k], again[k]), f"from audio != from the spectra it wrote: {k}"


def test_ragged_equals_solo_and_repeats(cfg):
    s = env(cfg)
    g = s["narrow"]
    off = g["off"]
    for form in FORMS:
        full = run_stage(s, g, form)
        twice = run_stage(s, g, form)
        for k in TAPS:
            assert np.array_equal(full[k], twice[k]), f"form {form}: two calls differ in {k}"
        for u in range(len(off) - 1):
            rows = slice(int(off[u]), int(off[u + 1]))
            gu = dict(g, style=g["style"][u : u + 1])
            solo = run_stage(s, gu, form, lengths=[rows.stop - rows.start], rows=rows)
            for k in TAPS:
                assert np.array_equal(full[k][rows], solo[k]), f"form {form}: utterance {u} alone differs in {k}"


def test_concurrent_streams_stay_bit_identical(cfg):
    """Three stage calls in flight on their own streams, a frame path beside them: every one equals the call alone."""
    import threading

    from stylish_tts_amd import synth

    s = env(cfg)
    m, g = s["m"], s["narrow"]
    alone = run_stage(s, g, None, taps=False)
    seg4 = seg_of(m, [64, 96])
    R4 = seg4.rows
    fp_in = dict(asr=dev(m, synth.normal("post.asr", (R4, cfg.inter_dim))), pitch=dev(m, np.abs(synth.normal("post.f0", (R4,))) * 60 + 120),
                 energy=dev(m, synth.normal("post.en", (R4,))), style=dev(m, synth.normal("post.sty", (2, cfg.style_dim))),
                 prior_noise=dev(m, synth.normal("post.pn", (R4, 128))), src_noise=dev(m, synth.normal("post.sn", (R4 * 75,))), init_phase=dev(m, synth.uniform("post.ph", (1,))))
    results, errors = [None] * 3, []

    def work(j):
        try:
            torch.cuda.set_device(m.device)
            st = torch.cuda.Stream(device=m.device)
            with torch.cuda.stream(st):
                for _ in range(3):
                    results[j] = run_stage(s, g, None, taps=False)
                    if j == 0:  # (split fp32 contractions of a frame path on the chip beside the posterior calls)
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
        for k in ("z", "mean", "logstd", "mel"):
            assert np.array_equal(r[k], alone[k])


def test_refusals(cfg):
    from stylish_tts_amd import _lib, params
    from stylish_tts_amd.runtime import HipModel, Segments, _ptr, _stream

    s = env(cfg)
    m, g = s["m"], s["misc"]
    nz = dev(m, g["noise"])
    with pytest.raises(RuntimeError, match="too short"):
        m.posterior(seg_of(m, [13]), audio=dev(m, g["audio"][: 13 * 75]), noise=nz[:13])
    cap = Segments.capacity([16], m.device)
    with pytest.raises(RuntimeError, match="plain segments"):
        m.posterior(cap, audio=dev(m, g["audio"]), noise=nz)
    # an undersized workspace: one 256-byte unit below the least accepted size (found by bisection over refusals, nothing is launched by a refused call)
    seg = seg_of(m, [16])
    spec, phase = (torch.zeros(16, m.har_ld, device=m.device) for _ in range(2))
    z = torch.full((16, 128), 7.0, device=m.device)
    need = int(m.lib.stts_posterior_workspace_bytes(m.ctx, 16, 1, 16))
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)

    def call(nbytes, ld=None):
        return m.lib.stts_posterior_forward(m.ctx, _stream(), 1, seg.host_ptr, _ptr(seg.dev), None, _ptr(spec), _ptr(phase), ld or m.har_ld, None, _ptr(nz), _ptr(z),
                                            None, None, None, 0, None, None, _ptr(ws), nbytes, 0)

    assert call(need) == 0
    lo, hi = 0, need // 256  # units: hi accepted
    while hi - lo > 1:
        mid = (lo + hi) // 2
        z.fill_(7.0)
        if call(mid * 256) == 0:
            hi = mid
        else:
            assert b"workspace too small" in m.lib.stts_last_error()
            torch.cuda.synchronize()
            assert bool((z == 7.0).all()), "a refused call wrote its output"
            lo = mid
    assert hi * 256 <= need
    assert call(need, ld=1024) != 0 and b"ld_har" in m.lib.stts_last_error()
    # mel_out without the flow weights: an engine that finalized the posterior alone
    m2 = HipModel(cfg, 0)
    m2.load_state_dict("speech_predictor", s["sd"], prefix="posterior_encoder.")
    m2.finalize(W_POSTERIOR)
    o = m2.posterior(seg_of(m2, [16]), spectra=(dev(m2, g["har_spec"]), dev(m2, g["har_phase"])), noise=dev(m2, g["noise"]))
    ref = run_stage(s, g, None)
    assert np.array_equal(o["z"].cpu().numpy(), ref["z"]), "finalized alone and after the frame path must give the same bits"
    with pytest.raises(RuntimeError, match="STTS_W_FLOW"):
        m2.posterior(seg_of(m2, [16]), spectra=(dev(m2, g["har_spec"]), dev(m2, g["har_phase"])), noise=dev(m2, g["noise"]), mel=True)
    m2.close()
    del params, _lib


def test_module_level(cfg):
    from stylish_tts_amd import modules, pipeline

    s = env(cfg)
    m, g = s["m"], s["narrow"]
    pe = modules.PosteriorEncoder.from_config(cfg, engine=m).load_synthetic(0)
    off = g["off"]
    rows = slice(int(off[0]), int(off[1]))
    n = rows.stop
    x = torch.from_numpy(g["audio"][: 75 * n])[None, None]
    style = torch.from_numpy(g["style"][:1])
    noise = torch.from_numpy(g["noise"][rows].T.copy())[None]
    z, mean, logstd = pe(x, style[:, :, None], noise=noise)
    st = m.posterior(seg_of(m, [n]), audio=dev(m, g["audio"][: 75 * n]), style=dev(m, g["style"][:1]), noise=dev(m, g["noise"][rows]))
    for a, k in ((z, "z"), (mean, "mean"), (logstd, "logstd")):
        assert a.shape == (1, 128, n) and torch.equal(a[0].T.contiguous(), st[k]), k
    # SpeechPredictor.forward(audio_gt=...)
    sp = modules.SpeechPredictor(cfg, engine=m).load_synthetic(0)
    T = 6
    P = 5
    texts = torch.tensor([[3, 9, 4, 17, 8]])
    lens = torch.tensor([P])
    dur = [1, 2, 1, 1, 1]
    al = torch.zeros(1, P, T)
    t0 = 0
    for p_, d in enumerate(dur):
        al[0, p_, t0 : t0 + d] = 1
        t0 += d
    pitch = torch.full((1, T), 150.0)
    energy = torch.zeros(1, T)
    wave = torch.from_numpy(P64.recording(77, 300 * T))[None]
    nzd = dict(posterior_noise=torch.randn(1, 128, 4 * T, generator=torch.Generator().manual_seed(1)),
               src_noise=torch.randn(1, 1, 300 * T, generator=torch.Generator().manual_seed(2)), init_phase=torch.tensor([[0.25]]))
    assert not sp.has_posterior
    with pytest.raises(NotImplementedError):
        sp(texts, lens, al, pitch, energy, audio_gt=wave, noise=nzd)
    keys_before = list(sp.state_dict().keys())
    sp.attach_posterior(pe)
    assert sp.has_posterior and list(sp.state_dict().keys()) == keys_before
    pred = sp(texts, lens, al, pitch, energy, audio_gt=wave, noise=nzd)
    assert pred.text_stats is None and pred.text2mel_stats is None and pred.mel2text_stats is None
    zz, mm, ll = pred.mel_stats
    assert zz.shape == (1, 128, 4 * T) and bool(torch.isfinite(pred.audio).all())
    assert torch.allclose(zz, mm + nzd["posterior_noise"].to(zz.device) * torch.exp(ll), atol=1e-4)
    # the audio is the vocoder's on post_flow(z): Generator.forward fed that mel and the same noise gives the same bits
    toks = texts[0].to(m.device)
    from stylish_tts_amd.runtime import Segments

    sp_seg = Segments([P], m.device)
    sty = m.text_style(1, sp_seg, m.text_encoder(1, sp_seg, toks))
    st2 = m.posterior(seg_of(m, [4 * T]), audio=dev(m, wave[0].numpy()), style=sty, noise=nzd["posterior_noise"][0].T.contiguous().to(m.device), mel=True)
    # mel_stats are the stage's own outputs for that style, bit for bit (the stage's bars are the tests above)
    for got, k in ((zz, "z"), (mm, "mean"), (ll, "logstd")):
        assert torch.equal(got[0].T.contiguous(), st2[k]), k
    gen = modules.Generator(style_dim=64, n_fft=cfg.n_fft, win_length=cfg.win_length, hop_length=cfg.hop_length, config=cfg.generator, cfg=cfg, engine=m).load_synthetic(0)
    up = m.upsample4(Segments([T], m.device), Segments([4 * T], m.device), pitch[0].to(m.device))[None]
    ref = gen(mel=st2["mel"].T[None].contiguous(), style=sty, pitch=up, noise=nzd)
    assert torch.equal(ref.audio, pred.audio)
    # a ragged batch passes lists: audio and mel_stats come back per utterance, each equal to that utterance's own call
    T2 = 5
    texts2 = torch.tensor([[3, 9, 4, 17, 8], [5, 6, 7, 0, 0]])
    lens2 = torch.tensor([5, 3])
    al2 = torch.zeros(2, P, T)
    al2[0] = al[0]
    for p_, (a0, a1) in enumerate(((0, 2), (2, 3), (3, 5))):
        al2[1, p_, a0:a1] = 1
    wave2 = torch.from_numpy(P64.recording(80, 300 * T2))
    nz_r = dict(posterior_noise=torch.randn(2, 128, 4 * T, generator=torch.Generator().manual_seed(5)),
                src_noise=torch.randn(2, 1, 300 * T, generator=torch.Generator().manual_seed(6)), init_phase=torch.tensor([[0.25]]))
    rag = sp(texts2, lens2, al2, torch.full((2, T), 150.0), torch.zeros(2, T), audio_gt=[wave[0], wave2], noise=nz_r)
    assert isinstance(rag.audio, list) and rag.magnitude is None and rag.phase is None and rag.text_stats is None
    assert [a.numel() for a in rag.audio] == [300 * T, 300 * T2] and [st_.z.shape for st_ in rag.mel_stats] == [(1, 128, 4 * T), (1, 128, 4 * T2)]
    for u, (tx, ln, Tu, wv) in enumerate(((texts2[:1], lens2[:1], T, wave), (texts2[1:, :3], lens2[1:], T2, wave2[None]))):
        nz_u = dict(posterior_noise=nz_r["posterior_noise"][u : u + 1, :, : 4 * Tu], src_noise=nz_r["src_noise"][u : u + 1, :, : 300 * Tu], init_phase=nz_r["init_phase"])
        solo = sp(tx, ln, al2[u : u + 1, : int(ln[0]), :Tu], torch.full((1, Tu), 150.0), torch.zeros(1, Tu), audio_gt=wv, noise=nz_u)
        for a, b in zip(rag.mel_stats[u], solo.mel_stats):
            assert torch.equal(a, b), f"ragged utterance {u}: mel_stats differ from its own call"
    # an attached posterior on another engine is refused with a clear error
    from stylish_tts_amd.runtime import HipModel

    other = HipModel(cfg, 0)
    sp.attach_posterior(modules.PosteriorEncoder.from_config(cfg, engine=other).load_synthetic(0))
    with pytest.raises(RuntimeError, match="another engine"):
        sp(texts, lens, al, pitch, energy, audio_gt=wave, noise=nzd)
    other.close()
    sp.attach_posterior(pe)
    # Synthesizer.resynthesize: a ragged batch of two equals the calls one by one; validation scores
    syn = pipeline.Synthesizer(m)
    tl = [[3, 9, 4, 17, 8], [5, 6, 7]]
    durs = [[1, 2, 1, 1, 1], [2, 1, 2]]
    recs = [torch.from_numpy(P64.recording(78, 300 * 6)), torch.from_numpy(P64.recording(79, 300 * 5))]
    f0 = [torch.full((6,), 140.0), torch.full((5,), 180.0)]
    R = 4 * 11
    nz2 = dict(posterior_noise=torch.randn(R, 128, generator=torch.Generator().manual_seed(3)).to(m.device),
               src_noise=torch.randn(R * 75, generator=torch.Generator().manual_seed(4)).to(m.device), init_phase=torch.tensor([0.5], device=m.device))
    both = syn.resynthesize(tl, recs, durs, f0, noise=nz2)
    r0 = 4 * 6
    parts = [dict(posterior_noise=nz2["posterior_noise"][:r0], src_noise=nz2["src_noise"][: r0 * 75], init_phase=nz2["init_phase"]),
             dict(posterior_noise=nz2["posterior_noise"][r0:], src_noise=nz2["src_noise"][r0 * 75 :], init_phase=nz2["init_phase"])]
    for u in range(2):
        one = syn.resynthesize([tl[u]], [recs[u]], [durs[u]], [f0[u]], noise=parts[u])[0]
        assert torch.equal(one, both[u]), f"utterance {u}: alone != in the ragged batch"
    same = pipeline.validation_scores(m, [recs[0].to(m.device)], [recs[0].to(m.device)])
    assert same["mel"] == 0
    sc = pipeline.validation_scores(m, [w.reshape(-1) for w in both], [r.to(m.device) for r in recs])
    assert np.isfinite(sc["mel"])
