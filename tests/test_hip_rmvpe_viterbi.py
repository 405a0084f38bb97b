"""RMVPE's Viterbi pitch decoding on the engine (csrc/rmvpe_viterbi.hip.h) against the float64 oracle of tests/viterbi64.py:
the full 360 x 360 recursion of the stated objective, with no band shortcut.

Bounds.  path: identical wherever the oracle's decision margin exceeds 1e-9 (the kernel's fp64 accumulation error at these lengths is ~1e-10: a
disagreement above the margin is a bug, not rounding); logp within 8 T 2^-53 max(1, |logp|) (T two-add steps of fp64 rounding, a factor 4 for the
device logarithm); the kernel's path re-scored by the oracle within the same bound of the optimum, whatever the ties; f0 within 1 fp32 ulp of the
float64 value (one rounding plus the double-rounding edge).  The entry point is called through ctypes with sentinels around every output and after
the workspace."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
import viterbi64 as V  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NARROW = dict(n_blocks=1, inter_layers=1, en_out_channels=8)
NARROW_HUBERT = {"hidden_dim": 128, "sr": 16000, "arch": {"hidden_size": 128, "num_attention_heads": 2, "num_hidden_layers": 2, "intermediate_size": 256,
                                                          "conv_dim": [64] * 7, "num_conv_pos_embeddings": 32, "num_conv_pos_embedding_groups": 4}}
CHUNK = 64  # kRvVitChunk: back-pointer rows per backtracking round; T - 1 = 64 fills one round exactly
GUARD = 32
THRED = 0.03


@pytest.fixture(scope="module")
def eng():
    from stylish_tts_amd.runtime import HipModel

    e = HipModel(None, 0)
    yield e
    e.close()


_ORACLE = {}


def oracle(name, sal):
    """The oracle's result for a named input, computed once and left alone."""
    if name not in _ORACLE:
        r = V.viterbi(sal)
        r["f0"] = V.local_average_f0(sal, r["path"], THRED)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[name] = r
    return _ORACLE[name]


def inputs():
    g = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"]
    return {"decode_sal0": g[0], "hidden32": np.load(os.path.join(GOLD, "resample_rmvpe.npz"))["hidden32"][0], "pitch_like": V.pitch_like()}


def raw_viterbi(eng, sals, thred=THRED, ld=360):
    """stts_rmvpe_viterbi on a ragged batch through ctypes: every output between GUARD sentinels, the workspace exactly as long as its query says
    plus a sentinel tail.  Returns per-utterance (path, logp, f0) and asserts that no sentinel changed."""
    from stylish_tts_amd import rmvpe
    from stylish_tts_amd.runtime import Segments, _ptr, _stream

    dev = eng.device
    seg = Segments([len(s) for s in sals], dev)
    rows = torch.full((seg.rows, ld), 7.0, dtype=torch.float32)
    rows[:, :360] = torch.from_numpy(np.concatenate(sals).astype(np.float32))
    rows = rows.to(dev)
    band, lt_out, eps = rmvpe.viterbi_tables()
    lt = torch.from_numpy(band.copy()).to(dev)
    need = int(eng.lib.stts_rmvpe_viterbi_workspace_bytes(seg.n, seg.host_ptr))
    assert need > 0
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    path = torch.full((seg.rows + 2 * GUARD,), -77, dtype=torch.int32, device=dev)
    f0 = torch.full((seg.rows + 2 * GUARD,), -5.0, dtype=torch.float32, device=dev)
    logp = torch.full((seg.n + 2 * GUARD,), 123.0, dtype=torch.float64, device=dev)
    rc = eng.lib.stts_rmvpe_viterbi(eng.ctx, _stream(), seg.n, seg.host_ptr, _ptr(seg.dev), _ptr(rows), ld, _ptr(lt), C.c_double(lt_out), C.c_double(eps), C.c_float(thred),
                                    _ptr(path[GUARD:]), _ptr(logp[GUARD:]), _ptr(f0[GUARD:]), _ptr(ws), need)
    assert rc == 0, eng.lib.stts_last_error()
    torch.cuda.synchronize()
    path, f0, logp, tail = path.cpu().numpy(), f0.cpu().numpy(), logp.cpu().numpy(), ws[need:].cpu().numpy()
    for a, fill in ((path, -77), (f0, -5.0), (logp, 123.0)):
        assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), "a sentinel around an output changed"
    assert (tail == 0xA5).all(), "the workspace tail changed"
    o = seg.host
    return [(path[GUARD + o[u] : GUARD + o[u + 1]].astype(np.int64), float(logp[GUARD + u]), f0[GUARD + o[u] : GUARD + o[u + 1]]) for u in range(seg.n)]


def check(name, sal, got, exact_path=None):
    """One utterance against the oracle.  exact_path: demanded whatever the margin (the cases whose path follows from the tie rule alone); None: where margin > 1e-9."""
    path, logp, f0 = got
    r = oracle(name, sal)
    T = len(sal)
    bound = V.logp_bound(T, r["logp"])
    rescored = V.score(sal, path)
    f64 = V.local_average_f0(sal, path, THRED)
    f0_err = np.abs(f0.astype(np.float64) - f64) / np.maximum(V.ulp32(f64), 2.0**-149)
    print(f"{name}: T {T} margin {r['margin']:.2e} | logp {logp:.12f} oracle {r['logp']:.12f} diff {abs(logp - r['logp']):.2e} bound {bound:.2e} | re-scored path "
          f"{r['logp'] - rescored:.2e} below the optimum | f0 {f0_err.max():.2f} ulp | path equal {np.array_equal(path, r['path'])}")
    assert path.shape == (T,) and path.min() >= 0 and path.max() < 360
    assert np.isfinite(logp) and abs(logp - r["logp"]) <= bound
    assert abs(rescored - r["logp"]) <= bound  # optimal, whatever the ties
    if exact_path is not None:
        assert path.tolist() == list(exact_path)
    if r["margin"] > 1e-9:
        assert np.array_equal(path, r["path"])
    assert np.isfinite(f0).all() and f0_err.max() <= 1.0
    if np.array_equal(path, r["path"]):
        assert np.array_equal(f64, r["f0"])


def test_path_logp_and_f0_against_the_oracle(eng):
    ins = inputs()
    got = raw_viterbi(eng, list(ins.values()))
    for (name, s), g in zip(ins.items(), got):
        assert (g[0] != s.argmax(1)).any()  # not the per-frame argmax
        check(name, s, g)
    # ragged: no recursion, one step, either side of the backtracking round (T - 1 = 63, 64, 65), odd lengths; each a prefix of one input
    p = ins["pitch_like"]
    lengths = [1, 2, 17, CHUNK, CHUNK + 1, CHUNK + 2, 257]
    got = raw_viterbi(eng, [p[:n] for n in lengths])
    for n, g in zip(lengths, got):
        check(f"pitch_like[:{n}]", p[:n], g)
    # rows wider than 360: the stride is honoured
    wide = raw_viterbi(eng, [p[:17], ins["hidden32"]], ld=368)
    assert np.array_equal(wide[0][0], got[2][0]) and wide[0][1] == got[2][1] and np.array_equal(wide[0][2], got[2][2])


def test_the_guard_lets_the_path_jump_across_the_band(eng):
    cases = {f"jump{sw}": V.jump_case(switch=sw) for sw in (10, 1, 18)}
    got = raw_viterbi(eng, list(cases.values()))
    for (name, s), g, sw in zip(cases.items(), got, (10, 1, 18)):
        check(name, s, g, exact_path=[10] * sw + [300] * (20 - sw))
    assert oracle("jump10", cases["jump10"])["logp"] == -152.31003351232144


def test_ties_take_the_lowest_index(eng):
    const = np.full((5, 360), 0.5, np.float32)
    s = inputs()["decode_sal0"]
    mirrored = np.ascontiguousarray(s[:, ::-1])
    got = raw_viterbi(eng, [const, s, mirrored])
    check("const", const, got[0], exact_path=[0] * 5)
    check("mirrored", mirrored, got[2])
    a, b = oracle("decode_sal0", s), oracle("mirrored", mirrored)
    tied = sorted(set(a["ties"]) | set(b["ties"]))
    keep = np.ones(len(s), bool)
    if tied:
        keep[: max(tied) + 1] = False  # a tie at frame t may change the path up to t
    assert np.array_equal(got[2][0][keep], 359 - got[1][0][keep]) and keep.any()


def test_degenerate_rows(eng):
    s = np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"][1].copy()
    assert (s.sum(1) == 0).any()
    plain = s.copy()
    s[5] = np.nan
    s[9, 100] = -0.5
    first_nan = np.full((3, 360), np.nan, np.float32)
    first_nan[1:] = inputs()["decode_sal0"][:2]
    got = raw_viterbi(eng, [plain, s, first_nan, first_nan[:1]])
    check("zero_row", plain, got[0])
    check("nan_negative", s, got[1])
    check("first_nan", first_nan, got[2])
    check("only_nan", first_nan[:1], got[3], exact_path=[0])
    assert got[1][2][5] == 0.0 and got[3][2][0] == 0.0  # a row of NaNs has no maximum above any threshold


def test_ragged_equals_solo_and_the_tail_equals_the_default_decode(eng):
    from stylish_tts_amd.runtime import Segments

    ins = inputs()
    p = ins["pitch_like"]
    sals = [p[:1], ins["hidden32"], p[: CHUNK + 1], ins["decode_sal0"], p]
    batch = raw_viterbi(eng, sals)
    for s, b in zip(sals, batch):
        (solo,) = raw_viterbi(eng, [s])
        assert np.array_equal(solo[0], b[0]) and solo[1] == b[1] and np.array_equal(solo[2].view(np.uint32), b[2].view(np.uint32))
    # HipModel.rmvpe_viterbi: the same bits through the runtime's own buffers
    rows = torch.from_numpy(np.concatenate(sals))
    f0, path, logp = eng.rmvpe_viterbi(Segments([len(s) for s in sals], eng.device), rows, THRED, path=True, logp=True)
    assert torch.equal(f0.cpu(), torch.from_numpy(np.concatenate([b[2] for b in batch]))) and path.dtype == torch.int32 and logp.dtype == torch.float64
    assert np.array_equal(path.cpu().numpy(), np.concatenate([b[0] for b in batch])) and logp.cpu().tolist() == [b[1] for b in batch]
    assert torch.equal(eng.rmvpe_viterbi(Segments([len(s) for s in sals], eng.device), rows, THRED), f0)
    # the decode tail around the argmax is the default decode, bit for bit (one shared local average)
    sal = torch.from_numpy(np.load(os.path.join(GOLD, "rmvpe_misc.npz"))["decode_sal"]).reshape(-1, 360)
    for th in (0.03, 0.5):
        want = eng.rmvpe_decode(sal, th)
        assert torch.equal(eng.rmvpe_decode(sal, th, center=sal.argmax(1)), want)
    moved = eng.rmvpe_decode(sal, 0.03, center=(sal.argmax(1) + 3).clamp(max=359))
    assert not torch.equal(moved, eng.rmvpe_decode(sal, 0.03))
    for bad in (-5, 400):  # clamped, in bounds
        assert bool(torch.isfinite(eng.rmvpe_decode(sal, 0.03, center=torch.full((sal.shape[0],), bad))).all())


def test_refusals(eng):
    from stylish_tts_amd.runtime import Segments, _ptr, _stream

    dev = eng.device
    seg = Segments([3], dev)
    rows, lt = torch.zeros(3, 360, device=dev), torch.zeros(360, 59, dtype=torch.float64, device=dev)
    ws, f0 = torch.zeros(1 << 16, dtype=torch.uint8, device=dev), torch.zeros(3, device=dev)
    call = lambda n, host, ldd, table, out, nbytes: eng.lib.stts_rmvpe_viterbi(eng.ctx, _stream(), n, host, _ptr(seg.dev), _ptr(rows), ldd, table, C.c_double(-87.0),  # noqa: E731
                                                                               C.c_double(2.0**-126), C.c_float(0.03), None, None, out, _ptr(ws), nbytes)
    empty = np.array([0, 2, 2], np.int32)
    assert call(2, empty.ctypes.data_as(C.c_void_p), 360, _ptr(lt), _ptr(f0), ws.numel()) != 0 and b"no frames" in eng.lib.stts_last_error()
    assert call(1, seg.host_ptr, 360, None, _ptr(f0), ws.numel()) != 0 and b"table" in eng.lib.stts_last_error()
    assert call(1, seg.host_ptr, 359, _ptr(lt), _ptr(f0), ws.numel()) != 0 and b"360" in eng.lib.stts_last_error()
    assert call(1, seg.host_ptr, 360, _ptr(lt), None, ws.numel()) != 0
    assert call(1, seg.host_ptr, 360, _ptr(lt), _ptr(f0), 256) != 0 and b"workspace" in eng.lib.stts_last_error()
    assert call(1, seg.host_ptr, 360, _ptr(lt), _ptr(f0), ws.numel()) == 0
    torch.cuda.synchronize()


def test_the_extractor_end_to_end(eng):
    """infer_from_audio(decoder="viterbi") is decode(mel2hidden(mel), decoder="viterbi"): the path is searched at 100 frames / s, resampling comes after."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import Segments

    g = np.load(os.path.join(GOLD, "resample_rmvpe.npz"))
    px = modules.RmvpePitchExtractor(config=NARROW, engine=eng).load_synthetic(0)
    w = torch.from_numpy(g["audio"])[None]
    hid = px.mel2hidden(px.mel(w, sample_rate=24000, resample=True))
    px.thred = th = float(hid.max(dim=-1)[0].median())  # voiced and unvoiced frames from the synthetic network
    want, path = px.decode(hid, th, decoder="viterbi", return_path=True)
    got = px.infer_from_audio(w, thred=th, sample_rate=24000, resample=True, decoder="viterbi")
    assert got.shape == (1, 51) and torch.equal(got, want) and path.shape == (1, 51) and bool((want == 0).any()) and bool((want > 0).any())
    r = V.viterbi(hid[0].cpu().numpy())
    if r["margin"] > 1e-9:
        assert np.array_equal(path[0].cpu().numpy(), r["path"])
    assert not torch.equal(got, px.infer_from_audio(w, thred=th, sample_rate=24000, resample=True))  # not the argmax decode
    assert torch.equal(px(px.mel(w, sample_rate=24000, resample=True), thred=th, decoder="viterbi"), want)
    # [T, 360] and ragged lengths: every utterance as alone, zeros past its length
    assert torch.equal(px.decode(hid[0], th, decoder="viterbi"), want[0])
    two = torch.cat([hid, hid.flip(1)])
    rg, rp = px.decode(two, th, decoder="viterbi", lengths=[51, 20], return_path=True)
    assert torch.equal(rg[0], want[0]) and torch.equal(rg[1, :20], px.decode(two[1, :20], th, decoder="viterbi")) and not bool(rg[1, 20:].any()) and not bool(rp[1, 20:].any())
    # frames=: the 100 frames / s curve, then the linear resampling
    fr = px.infer_from_audio(w, frames=[40], thred=th, sample_rate=24000, resample=True, decoder="viterbi")
    assert torch.equal(fr[0], eng.rmvpe_resample(Segments([51], eng.device), want[0].contiguous(), Segments([40], eng.device)))


def test_convert_audio_with_the_viterbi_curve():
    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.config import DEFAULT_MODEL, load_model_config
    from stylish_tts_amd.pipeline import VoiceConverter
    from stylish_tts_amd.runtime import HipModel

    raw = copy.deepcopy(DEFAULT_MODEL)
    raw["hubert"] = copy.deepcopy(NARROW_HUBERT)
    cfg = load_model_config(raw)
    e = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=e, synthetic_seed=0, hubert=True, ssl=True, cfm_pitch=True)
    px = modules.RmvpePitchExtractor(config=NARROW, engine=e).load_synthetic(0)
    vc = VoiceConverter(e, [mods["hubert_speech_predictor"], mods["hubert_pitch_energy_predictor"], mods["cfm_pitch_predictor"], mods["hubert"]])
    S, T = [16000, 8000], [80, 40]
    w = torch.zeros(2, 16000)
    for b, n in enumerate(S):
        w[b, :n] = torch.from_numpy((synth.normal(f"rvc.wave{b}", (n,)) * 0.1).astype(np.float32))
    spk = torch.from_numpy(synth.normal("rvc.spk", (2, vc.spk_dim)) * 0.5)
    R4 = 4 * sum(T)
    noise = dict(prior_noise=torch.from_numpy(synth.normal("rvc.vpn", (R4, 128))).cuda(), src_noise=torch.from_numpy(synth.normal("rvc.vsn", (R4 * e.hop4,))).cuda(),
                 init_phase=torch.zeros(1).cuda())
    hid = px.mel2hidden(px.mel(w[:1]))
    px.thred = float(hid.max(dim=-1)[0].median())
    own = px.packed_from_audio(w, S, T, decoder="viterbi").clone()
    plain = px.packed_from_audio(w, S, T).clone()
    assert own.shape == (sum(T),) and not torch.equal(own, plain)
    waves, det = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px, decoder="viterbi")
    assert torch.equal(det["pitch"], own) and all(bool(torch.isfinite(x).all()) for x in waves)
    _, det0 = vc.convert_audio(w, S, T, spk, noise=noise, return_details=True, pitch_extractor=px)
    assert torch.equal(det0["pitch"], plain)  # the default stays the argmax decode
    e.close()
