"""GPU: CfmPitchPredictor (speaker branch and frame-rate network) gives the bits of a solo run while the fp32 frame path (split-fp32
contractions, packed-fp32 instructions) runs on another stream of the same engine (DESIGN.md sections 5d, 5h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_cfm_pitch_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    cp = modules.CfmPitchPredictor(768, 80, cfg=cfg, engine=eng).load_synthetic(0)
    cp.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def batch(j, La, Lm):
        a = torch.zeros(len(La), 768, max(La))
        m = torch.zeros(len(La), 80, max(Lm))
        for b, (t, tm) in enumerate(zip(La, Lm)):
            a[b, :, :t] = torch.from_numpy(synth.normal(f"cpc.asr{j}.{b}", (768, t)))
            m[b, :, :tm] = torch.from_numpy(synth.normal(f"cpc.mel{j}.{b}", (80, tm)))
        return a.cuda(), m.cuda(), La, Lm

    calls = [batch(0, [240], [240]), batch(1, [803, 33], [300, 33]), batch(2, [47, 240, 511], [40, 240, 200])]
    stats = (7.4, 0.45)
    L = [240] * 8
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("cpc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("cpc.f0", (R,))) * 60 + 120),
              energy=dev(synth.normal("cpc.en", (R,))), style=dev(synth.normal("cpc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("cpc.pn", (R, 128))),
              sn=dev(synth.normal("cpc.sn", (R * 75,))), ph=dev(synth.uniform("cpc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    def run_all():
        return [tuple(t.clone() for t in cp.run(*c, f0_log2_stats=stats)[:2]) for c in calls]

    solo = run_all()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(8):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def pitches():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = run_all()
            torch.cuda.current_stream().synchronize()
        return out

    for _ in range(3):
        with ThreadPoolExecutor(2) as ex:
            f = ex.submit(frames)
            got = ex.submit(pitches).result()
            f.result()
        for j, (a, b) in enumerate(zip(got, solo)):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), j
