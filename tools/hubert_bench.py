"""VoiceConverter.convert() throughput (HuBERT features + speaker embedding -> waveform) at B = 1 x 3 s, 8 x 3 s and 16 x 10 s in fp32
and 8 x 3 s in bf16, with the split of one call into speaker MLP, encoder at 4T, pitch predictor and frame path (CUDA events between
the stages on the caller's stream), and the text-to-speech frame path at B = 8 x 3 s in the same process as the yardstick.
Synthetic weights (params, seed 0) and random inputs.  Prints one JSON line per configuration.

    python tools/hubert_bench.py [--steps 20 --warmup 5]
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/hubert_bench.py
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("f32", 1, 3.0), ("f32", 8, 3.0), ("f32", 16, 10.0), ("bf16", 8, 3.0)]


def engine(precision):
    from stylish_tts_amd import modules
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.runtime import HipModel

    cfg = load_model_config()
    eng = HipModel(cfg, 0, precision=precision)
    m = modules.build_inference_modules(cfg, engine=eng, hubert=True)
    sp, pe = m["hubert_speech_predictor"].load_synthetic(0), m["hubert_pitch_energy_predictor"].load_synthetic(0)
    _, _ = sp.engine, pe.engine
    return eng, [sp, pe]


def stage_split(eng, vc, feats, L, spk, noise):
    """One call of convert()'s stages with events between them -> ms per stage."""
    import torch
    from stylish_tts_amd.modules import _f, _pack_rows
    from stylish_tts_amd.runtime import Segments

    dev = eng.device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    st = Segments(L, dev)
    st4 = st.scaled(4)
    ev[0].record()
    x = _pack_rows(eng, feats, L)
    ev[1].record()
    style, pe_style = eng.speaker_style(_f(spk, dev))
    ev[2].record()
    f0, en = eng.hubert_pitch_energy(st, x, pe_style)
    ev[3].record()
    asr = eng.hubert_encoder(st, x)
    ev[4].record()
    p4, e4 = eng.upsample4(st, st4, f0), eng.upsample4(st, st4, en)
    eng.frame_path(st4, asr, p4, e4, style, noise["prior_noise"], noise["src_noise"], noise["init_phase"], batch_scope=False)
    ev[5].record()
    torch.cuda.synchronize()
    eng.check_status()
    names = ["pack_features", "speaker_mlp", "pitch_predictor", "encoder_4T", "frame_path"]
    return {n: round(ev[i].elapsed_time(ev[i + 1]), 3) for i, n in enumerate(names)}


def bench(precision, B, seconds, steps, warmup, eng=None, mods=None):
    import torch
    from stylish_tts_amd.pipeline import VoiceConverter

    own = eng is None
    if own:
        eng, mods = engine(precision)
    dev = eng.device
    T = int(round(seconds * eng.cfg.sample_rate / eng.cfg.hop_length))
    g = torch.Generator(device="cpu").manual_seed(1)
    feats = torch.randn(B, 768, T, generator=g).to(dev)
    spk = torch.randn(B, 10240, generator=g).to(dev)
    R = 4 * T * B
    noise = dict(prior_noise=torch.randn(R, 128, generator=g).to(dev), src_noise=torch.randn(R * eng.hop4, generator=g).to(dev),
                 init_phase=torch.rand(1, generator=g).to(dev))
    vc = VoiceConverter(eng, modules=mods)
    L = [T] * B
    for _ in range(warmup):
        vc.convert(feats, L, spk, noise=noise)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vc.convert(feats, L, spk, noise=noise)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    split = [stage_split(eng, vc, feats, L, spk, noise) for _ in range(3)]
    med = {k: sorted(s[k] for s in split)[1] for k in split[0]}
    out = dict(config=f"convert_{precision}_B{B}_{seconds:g}s", B=B, T=T, T4=4 * T, ms_per_call=round(dt * 1e3, 3), utt_per_s=round(B / dt, 1),
               stage_ms=med, front_end_share=round((med["speaker_mlp"] + med["pitch_predictor"] + med["encoder_4T"]) / sum(med.values()), 3))
    print(json.dumps(out), flush=True)
    return eng, mods


def yardstick(steps, warmup):
    """The text-to-speech frame path (the benchmark's cfg2 unit) at B = 8 x 3 s, on its own engine in this process."""
    import torch
    from stylish_tts_amd import params
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.runtime import HipModel, Segments

    cfg = load_model_config()
    eng = HipModel(cfg, 0)
    eng.load_weights({"speech_predictor": params.synth_state_dict(params.module_spec("speech_predictor", cfg), 0, prefix="speech_predictor.")}, which=7)
    B, T4 = 8, 960
    seg = Segments([T4] * B, eng.device)
    R, dev = seg.rows, eng.device
    g = torch.Generator(device="cpu").manual_seed(1)
    args = [torch.randn(R, 128, generator=g).to(dev), (torch.rand(R, generator=g) * 100 + 120).to(dev), (torch.rand(R, generator=g) * 2 + 2).to(dev),
            (torch.randn(B, 64, generator=g) * 0.7).to(dev), torch.randn(R, 128, generator=g).to(dev), torch.randn(R * eng.hop4, generator=g).to(dev),
            torch.rand(1, generator=g).to(dev)]
    for _ in range(warmup):
        eng.frame_path(seg, *args, batch_scope=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.frame_path(seg, *args, batch_scope=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    eng.check_status()
    print(json.dumps(dict(config="tts_frame_path_B8_3s", B=B, T4=T4, ms_per_call=round(dt * 1e3, 3), utt_per_s=round(B / dt, 1))), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.steps < 1:
        sys.exit("--steps must be >= 1")
    yardstick(a.steps, a.warmup)
    eng = mods = None
    for prec, B, sec in CONFIGS:
        if eng is not None and eng.precision != prec:
            eng.close()
            eng = mods = None
        eng, mods = bench(prec, B, sec, a.steps, a.warmup, eng, mods)
    eng.close()
