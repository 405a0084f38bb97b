"""GPU: AdaptiveHubert gives the bits of a solo run while the fp32 frame path (split-fp32 contractions, packed-fp32 instructions) runs on
another stream of the same engine (DESIGN.md sections 5d, 5i), and those bits are within the float64 bar of tests/test_hip_ssl.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_features_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0, ssl=True)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    enc = mods["hubert"]
    enc.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    w = torch.from_numpy((synth.normal("ssl.wave.b3s", (1, 48000)) * 0.3).astype(np.float32)).cuda()
    L = [240] * 8
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("sslc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("sslc.f0", (R,))) * 60 + 120),
              energy=dev(synth.normal("sslc.en", (R,))), style=dev(synth.normal("sslc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("sslc.pn", (R, 128))),
              sn=dev(synth.normal("sslc.sn", (R * 75,))), ph=dev(synth.uniform("sslc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    solo = enc(w, 240).clone()
    torch.cuda.synchronize()
    g = np.load(os.path.join(GOLD, "ssl_base_3s.npz"))
    idx, f32, f64 = g["b3s_out_idx"].astype(np.int64), g["b3s_out_f32"].astype(np.float64), g["b3s_out_f64"]
    mine = solo.cpu().double().numpy().ravel()[idx]
    assert np.abs(mine - f64).max() <= 4.0 * np.abs(f32 - f64).max()
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(6):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def feats():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [enc(w, 240) for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    for _ in range(2):
        with ThreadPoolExecutor(2) as ex:
            f = ex.submit(frames)
            got = ex.submit(feats).result()
            f.result()
        for j, a in enumerate(got):
            assert torch.equal(a, solo), j
