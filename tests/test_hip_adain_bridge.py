"""The decoder's fp32 Winograd branch with ONE launch between an AdaIN block's chained convs (winograd_bridge_kernel: output transform of conv A,
statistics, affine + LeakyReLU, input transform of conv B) against the three launches it replaces (winograd_output_kernel<8, true>,
adain_affine_lanes_kernel, winograd_input_kernel<8>).  Every value comes from the same expression in the same order, so `x_out` of
stts_decoder_forward must be equal BIT FOR BIT.  STTS_ADAIN_BRIDGE is read per call: 0 = the three launches, 1 = the bridge wherever it can run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# every edge of a group (6 rows) and of a statistics chunk (24 rows): one row, one short of / exactly / one past a group and a chunk, several
# iterations of a block (64 groups each) with a ragged tail; 2 531 rows, just above the Winograd branch's row threshold (model.hip.h fold_rows(): 2 500)
RAGGED = [1, 5, 6, 7, 23, 24, 25, 143, 960, 1337]
CASES = {"ragged": RAGGED, "cfg2": [960] * 8}


@pytest.fixture(scope="module")
def hip(cfg, weights):
    from stylish_tts_amd.runtime import HipModel

    m = HipModel(cfg, 0)
    m.load_weights({"speech_predictor": weights["speech_predictor"]}, which=7)
    yield m
    m.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_bridge_equals_the_three_launches_bit_for_bit(hip, monkeypatch, case):
    from stylish_tts_amd import synth
    from stylish_tts_amd.runtime import Segments

    lens = CASES[case]
    assert sum(lens) > 2500
    if case == "ragged":
        assert sum(lens) == 2531
    B = len(lens)
    s = Segments(lens, torch.device("cuda", 0))
    asr = dev(np.concatenate([synth.normal(f"bridge.asr{b}", (t, 128)) for b, t in enumerate(lens)]))
    pitch = dev(np.concatenate([synth.pitch_curve(f"bridge.pitch{b}", 1, t)[0] for b, t in enumerate(lens)]))
    energy = dev(np.concatenate([(synth.uniform(f"bridge.energy{b}", (t,)) * 2 + 2).astype(np.float32) for b, t in enumerate(lens)]))
    style = dev((synth.normal("bridge.style", (B, 64)) * 0.7).astype(np.float32))

    def run(mode):
        monkeypatch.setenv("STTS_ADAIN_BRIDGE", mode)
        x = hip.decoder(s, asr, pitch, energy, style).clone()
        hip.check_status()
        return x

    old, new, again = run("0"), run("1"), run("1")
    torch.cuda.synchronize()
    assert old.shape[0] == sum(lens)
    assert bool(torch.isfinite(old).all()) and float(old.abs().max()) > 0
    diff = int((old != new).sum())
    print(f"\n[adain bridge] {case}: {old.numel()} values, {diff} differ, max-abs difference {float((old - new).abs().max()):.3e}")
    assert torch.equal(new, old)
    assert torch.equal(again, new)

    # the switch really selects the path: of the ten affine-table launches of the three-launch form only block 0's first norm keeps its own, and the
    # profiled (event-timed) launch form of the bridge gives the same bits
    import ctypes as C
    import json

    from stylish_tts_amd import _lib

    lib = _lib.load()

    def affine_launches(mode):
        monkeypatch.setenv("STTS_ADAIN_BRIDGE", mode)
        lib.stts_profile_begin()
        x = hip.decoder(s, asr, pitch, energy, style).clone()
        buf = C.create_string_buffer(1 << 17)
        _lib.check(lib.stts_profile_report(C.c_void_p(torch.cuda.current_stream().cuda_stream), buf, len(buf)))
        recs = {r["kernel"]: r for r in json.loads(buf.value.decode())}
        assert all(r["kind"] == "contraction" for k, r in recs.items() if k.startswith("winograd_"))
        return recs["adain_affine_lanes_kernel"]["launches"], x

    n_old, x_old = affine_launches("0")
    n_new, x_new = affine_launches("1")
    assert (n_old, n_new) == (10, 1), (n_old, n_new)
    assert torch.equal(x_old, old) and torch.equal(x_new, old)
