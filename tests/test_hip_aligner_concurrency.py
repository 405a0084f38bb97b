"""GPU: TextAligner.align on its own stream gives the bits of a solo run while the fp32 frame path (split-fp32 contractions) runs on another
stream of the same engine, as the mel-style, CFM-pitch and AdaptiveHubert stages do (DESIGN.md sections 5d, 5k)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_alignment_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, aligner=True)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    al = mods["text_aligner"]
    al.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    L, PL = [240, 100, 33], [50, 30, 9]
    mel = torch.zeros(3, 240, al.n_mels)
    text = torch.zeros(3, 50, dtype=torch.int64)
    for b, (n, p) in enumerate(zip(L, PL)):
        mel[b, :n] = torch.from_numpy(synth.normal(f"alc.mel.{b}", (n, al.n_mels)).astype(np.float32))
        text[b, :p] = torch.from_numpy(np.clip((synth.uniform(f"alc.tok.{b}", (p,)) * al.num_symbols).astype(np.int64), 0, al.num_symbols - 1))
    mel = mel.cuda()
    FL = [240] * 8
    seg = Segments([4 * n for n in FL], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("alc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("alc.f0", (R,))) * 60 + 120),
              energy=dev(synth.normal("alc.en", (R,))), style=dev(synth.normal("alc.sty", (len(FL), cfg.style_dim))), pn=dev(synth.normal("alc.pn", (R, 128))),
              sn=dev(synth.normal("alc.sn", (R * 75,))), ph=dev(synth.uniform("alc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    def run():
        stacks, scores = al.align(mel, L, text, PL)
        return [s.clone() for s in stacks] + [s.clone() for s in scores]

    solo = run()
    torch.cuda.synchronize()
    for b, n in enumerate(L):
        assert float(solo[b][0].sum()) == n and float(solo[b][0].min()) >= 1
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(6):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def aligns():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [run() for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    for _ in range(2):
        with ThreadPoolExecutor(2) as ex:
            f = ex.submit(frames)
            got = ex.submit(aligns).result()
            f.result()
        for j, a in enumerate(got):
            assert all(torch.equal(x, y) for x, y in zip(a, solo)), j
