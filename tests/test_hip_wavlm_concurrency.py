"""GPU: the narrow WavLM gives the bits of a solo run while the fp32 frame path (split-fp32 contractions, packed-fp32 instructions) runs on
another stream of the same engine (DESIGN.md sections 5d, 5o), in the manner of tests/test_hip_ssl_concurrency.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NARROW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7, num_conv_pos_embeddings=32,
              num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40)


def test_states_bit_stable_beside_split_fp32_frame_path(cfg):
    from concurrent.futures import ThreadPoolExecutor

    from stylish_tts_amd import modules, synth
    from stylish_tts_amd.runtime import HipModel, Segments

    eng = HipModel(cfg, 0, precision="f32")
    mods = modules.build_inference_modules(cfg, engine=eng, synthetic_seed=0)
    mods["speech_predictor"].engine  # bind the frame path before any stream runs
    net = modules.WavLM(config=NARROW, engine=eng).load_synthetic(0)
    net.engine
    devid = eng.device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    w = torch.from_numpy((synth.normal("wavlm.wave.n1s", (1, 16000)) * 0.3).astype(np.float32)).cuda()
    L = [240] * 8
    seg = Segments([4 * n for n in L], devid)
    R = seg.rows
    fp = dict(asr=dev(synth.normal("wlc.asr", (R, cfg.inter_dim))), pitch=dev(np.abs(synth.normal("wlc.f0", (R,))) * 60 + 120),
              energy=dev(synth.normal("wlc.en", (R,))), style=dev(synth.normal("wlc.sty", (len(L), cfg.style_dim))), pn=dev(synth.normal("wlc.pn", (R, 128))),
              sn=dev(synth.normal("wlc.sn", (R * 75,))), ph=dev(synth.uniform("wlc.ph", (1,))))

    def frame_path():
        return eng.frame_path(seg, fp["asr"], fp["pitch"], fp["energy"], fp["style"], fp["pn"], fp["sn"], fp["ph"], batch_scope=False)

    solo = [s.clone() for s in net.hidden_states(w)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(s).all() for s in solo) and float(solo[-1].std()) > 0.5
    streams = [torch.cuda.Stream(device=devid) for _ in range(2)]

    def frames():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[0]):
            for _ in range(6):
                frame_path()
            torch.cuda.current_stream().synchronize()

    def states():
        torch.cuda.set_device(devid)
        with torch.cuda.stream(streams[1]):
            out = [[s.clone() for s in net.hidden_states(w)] for _ in range(3)]
            torch.cuda.current_stream().synchronize()
        return out

    for _ in range(2):
        with ThreadPoolExecutor(2) as ex:
            f = ex.submit(frames)
            got = ex.submit(states).result()
            f.result()
        for j, a in enumerate(got):
            assert all(torch.equal(x, y) for x, y in zip(a, solo)), j
