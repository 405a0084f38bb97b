"""Frame path ms / step and utterances / s at B = 8 x 3 s for the STFT geometries of tests/golden/gen_golden_geometry.py and for the default
geometry, the latter with the specialised signal kernels and with the run-time-geometry ones forced (STTS_SIGNAL_GENERIC=1; read at context
creation, so each configuration runs in a child process of its own).  Prints one JSON line per configuration.

    python tools/geometry_bench.py                    # all
    python tools/geometry_bench.py geom_1024          # one (child mode)
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/geometry_bench.py <name>
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMS = {"default": (2048, 1200, 300), "default_generic": (2048, 1200, 300), "geom_1024": (1024, 1024, 256), "geom_512": (512, 400, 100),
         "geom_4096": (4096, 2400, 600)}
B, SECONDS, STEPS, WARMUP = 8, 3.0, 20, 5


def run(name):
    import torch
    from stylish_tts_amd import params
    from stylish_tts_amd.config import load_model_config
    from stylish_tts_amd.runtime import HipModel, Segments

    n_fft, win, hop = GEOMS[name]
    base = dict(load_model_config())
    base.update(n_fft=n_fft, win_length=win, hop_length=hop)
    cfg = load_model_config(base)
    eng = HipModel(cfg, 0)
    eng.load_weights({"speech_predictor": params.synth_state_dict(params.module_spec("speech_predictor", cfg), 0, prefix="speech_predictor.")}, which=7)
    T4 = int(SECONDS * 24000 / eng.hop4)  # rows of 3 s at 24 kHz (960 at the default hop)
    seg = Segments([T4] * B, eng.device)
    R, dev = seg.rows, eng.device
    g = torch.Generator(device="cpu").manual_seed(1)
    asr = torch.randn(R, 128, generator=g).to(dev)
    pitch = (torch.rand(R, generator=g) * 100 + 120).to(dev)
    energy = (torch.rand(R, generator=g) * 2 + 2).to(dev)
    style = (torch.randn(B, 64, generator=g) * 0.7).to(dev)
    pn = torch.randn(R, 128, generator=g).to(dev)
    sn = torch.randn(R * eng.hop4, generator=g).to(dev)
    ph = torch.rand(1, generator=g).to(dev)
    for _ in range(WARMUP):
        eng.frame_path(seg, asr, pitch, energy, style, pn, sn, ph, batch_scope=False)
    eng.check_status()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        eng.frame_path(seg, asr, pitch, energy, style, pn, sn, ph, batch_scope=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    eng.check_status()
    print(json.dumps(dict(config=name, n_fft=n_fft, win=win, hop=hop, B=B, T4=T4, audio_s=T4 * eng.hop4 / cfg.sample_rate,
                          ms_per_step=round(dt * 1e3, 3), utt_per_s=round(B / dt, 1), generic=os.environ.get("STTS_SIGNAL_GENERIC", "0"))), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for name in GEOMS:
            env = dict(os.environ, STTS_SIGNAL_GENERIC="1" if name == "default_generic" else "0")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, timeout=600)
            if r.returncode != 0:
                sys.exit(r.returncode)
