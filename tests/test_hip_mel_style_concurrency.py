"""GPU: MelStyleEncoder gives the bits of a solo run while the fp32 frame path (split-fp32 contractions, packed-fp32 instructions) runs on
another stream of the same engine (DESIGN.md sections 5d, 5g)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_mel_style_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    enc = modules.MelStyleEncoder(80, 256, 1024, True, cfg=cfg, engine=eng, component="cfm_pitch_predictor.spk_emb").load_synthetic(0)
    enc.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    mels = [(torch.from_numpy(synth.normal(f"msc{j}", (len(L), 1, 80, max(L)))).cuda(), L) for j, L in enumerate([[240], [803, 33], [47, 240, 511]])]
    L = [240] * 8
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("msc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("msc.f0", (R,))) * 60 + 120),
              energy=dev(synth.normal("msc.en", (R,))), style=dev(synth.normal("msc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("msc.pn", (R, 128))),
              sn=dev(synth.normal("msc.sn", (R * 75,))), ph=dev(synth.uniform("msc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    solo = [enc(x, lengths=l).clone() for x, l in mels]  # noqa: E741
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(8):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def styles():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [enc(x, lengths=l) for x, l in mels]  # noqa: E741
            torch.cuda.current_stream().synchronize()
        return out

    for _ in range(3):
        with ThreadPoolExecutor(2) as ex:
            f = ex.submit(frames)
            got = ex.submit(styles).result()
            f.result()
        for j, (a, b) in enumerate(zip(got, solo)):
            assert torch.equal(a, b), j
