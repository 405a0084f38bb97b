#!/usr/bin/env python3
"""Build the library's HOST side with AddressSanitizer + UBSan against the HIP stub and run the sanitizer driver.

    python tests/asan/build_and_run.py [build_dir]

Steps: (1) hipcc --cuda-host-only -fsanitize=address,undefined -c for every translation unit of the library (no device code is generated or loaded),
(2) link it with hip_stub.cpp into libstylish_hip_asan.so (the fat-binary symbol the host code references is defined as an
empty blob), (3) dump the synthetic weights of every inference module, of the voice-conversion models, of the CFM estimator, of a narrow
AdaptiveHubert, of a narrow text aligner (with three TDNN layers and with one) and of a small RMVPE to a binary file, (4) run asan_driver on it.
(5) run `asan_driver <weights> gemm` (the contraction cases only) once per setting of GEMM_SETTINGS, and `asan_driver <weights> block` (the AdaptiveDecoderBlock
cases only) once per setting of BLOCK_SETTINGS, each line prefixed with `[setting]`.
Exit code 0 = no sanitizer report, every stage accepted its workspace for every shape, and the packed bytes did not depend on the order of the
finalizes.  The driver's `digest <precision> <what> <hex>` lines say what was packed: two builds of the library pack the same bytes exactly when
these lines are the same."""
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


# the process-wide switches of the contractions (csrc/gemm_plan.hip.h gemm_switches)
GEMM_SETTINGS = ["STTS_NO_X3=1", "STTS_X3_REM=1", "STTS_X3_TILE=5", "STTS_X3_TILE=6", "STTS_X3_TILE=22", "STTS_X3P_GLDS=0", "STTS_TILE16=14", "STTS_TILE16=16", "STTS_TILE16=18",
                 "STTS_SPLITK_MIN_ITERS=2", "STTS_GEMM16_MIN_TILES=1"]
# the process-wide switches of the AdaptiveDecoderBlock chains (csrc/adain_block.hip.h block_switches)
BLOCK_SETTINGS = ["STTS_NO_WINO_STATS=1", "STTS_NO_STAT_FUSE=1", "STTS_NO_WINO_CONV2SC=1", "STTS_AFFINE_SERIAL=1", "STTS_FOLD_ROWS=0", "STTS_SC_SIDE_MIN_ROWS=0"]


def write_tensors(f, m, spec, seen=None):
    from stylish_tts_amd import params

    for k, v in params.synth_state_dict(spec, 0, prefix=m + ".").items():
        if seen is not None:  # (two specs of one module that share tensors: a name is a tensor, written once)
            if k in seen:
                continue
            seen.add(k)
        name = (m + "." + k).encode()
        shape = v.shape if v.ndim else (1,)
        f.write(struct.pack("<i", len(name)) + name + struct.pack("<i", len(shape)) + struct.pack(f"<{len(shape)}q", *shape))
        f.write(v.astype("<f4").tobytes())


def main(build_dir):
    os.makedirs(build_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17", "-fPIC"]
    # every translation unit of the library (__graft_entry__.UNITS: api.hip + one unit per operand form of the contraction kernels), host side only, in parallel
    import __graft_entry__ as entry

    objs, procs = [], []
    for u in entry.UNITS:
        o = os.path.join(build_dir, u.replace(".hip", "_host.o"))
        objs.append(o)
        procs.append(subprocess.Popen([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-DSTTS_TEST_OPS", *san, "-c", os.path.join(ROOT, "stylish_tts_amd", "csrc", u), "-o", o]))
    if any(p.wait() != 0 for p in procs):
        raise subprocess.CalledProcessError(1, "hipcc --cuda-host-only")
    fatbin = sorted({s for o in objs for s in subprocess.check_output(["nm", "-u", o], text=True).split() if s.startswith("__hip_fatbin")})
    cxx = os.environ.get("CXX_ASAN", "/opt/rocm/lib/llvm/bin/clang++")  # the same clang, as a plain C++ compiler / linker driver
    stub = os.path.join(build_dir, "hip_stub.o")
    subprocess.check_call([cxx, *san, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", os.path.join(HERE, "hip_stub.cpp"), "-o", stub])
    lib = os.path.join(build_dir, "libstylish_hip_asan.so")
    defsym = [f"-Wl,--defsym={s}=stts_stub_fatbin" for s in fatbin]
    subprocess.check_call([cxx, "-shared", *san, *objs, stub, *defsym, "-o", lib])
    exe = os.path.join(build_dir, "asan_driver")
    subprocess.check_call([cxx, *san, "-DSTTS_TEST_OPS", os.path.join(HERE, "asan_driver.cpp"), lib, f"-Wl,-rpath,{build_dir}", "-o", exe])

    # weights: every module's synthetic state dict under the name modules.py loads it by (module + "." + key); the header is the three dims structs
    from stylish_tts_amd import _lib, aligner, hubert_ssl, params, rmvpe
    from stylish_tts_amd.config import load_model_config

    cfg = load_model_config()
    # the narrow AdaptiveHubert of tests/golden/gen_golden_ssl.py (NARROW)
    ssl_arch = hubert_ssl.arch(dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(64,) * 7,
                                    num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=4))
    specs = [(m, params.module_spec(m, cfg)) for t in (params.MODULE_SPECS, params.HUBERT_MODULE_SPECS, params.MEL_STYLE_MODULE_SPECS) for m in t]
    specs += [("cfm_mel_decoder", params.cfm_mel_decoder_spec()), ("hubert", params.hubert_ssl_spec(ssl_arch))]
    # a narrow text aligner, and the same with ONE tdnn layer (its Ffn is then encoder.layers.1: the driver finalizes both from one dump); a small RMVPE
    al_dims = aligner.dims(hidden_dim=128, tdnn_blstm_spec=(("tdnn", 5, 1, 1), ("tdnn", 3, 1, 1), ("tdnn", 3, 1, 1), ("ffn", 2)))
    al_one = aligner.dims(hidden_dim=128, tdnn_blstm_spec=(("tdnn", 5, 1, 1), ("ffn", 2)))
    rv_dims = rmvpe.dims(dict(n_blocks=1, inter_layers=1, en_out_channels=4))
    extra_dims = bytes(aligner.dims_struct(al_dims)) + bytes(rmvpe.dims_struct(rv_dims))
    wpath = os.path.join(build_dir, "weights.bin")
    with open(wpath, "wb") as f:
        f.write(bytes(_lib.dims_from_config(cfg)) + bytes(_lib.CfmDims(**params.CFM_DEFAULT_DIMS)) + bytes(hubert_ssl.dims_struct(ssl_arch)) + extra_dims)
        for m, spec in specs:
            write_tensors(f, m, spec)
        seen = set()
        write_tensors(f, "text_aligner", params.text_aligner_spec(al_dims), seen)
        write_tensors(f, "text_aligner", params.text_aligner_spec(al_one), seen)
        write_tensors(f, "rmvpe", params.rmvpe_spec(rv_dims))
    # ... and the text-to-speech weights of the narrow model of tests/golden/gen_golden.py (NARROW: decoder / generator width 384): its flow has 96 channels and runs
    # as plain contractions (gate / split-accumulate / couple epilogues)
    narrow = load_model_config(dict(dict(cfg), decoder=dict(cfg["decoder"], hidden_dim=384, residual_dim=32),
                                    generator=dict(cfg["generator"], input_dim=384, hidden_dim=384, conv_intermediate_dim=1152)))
    npath = os.path.join(build_dir, "weights_narrow.bin")
    with open(npath, "wb") as f:
        f.write(bytes(_lib.dims_from_config(narrow)) + bytes(_lib.CfmDims(**params.CFM_DEFAULT_DIMS)) + bytes(hubert_ssl.dims_struct(ssl_arch)) + extra_dims)
        write_tensors(f, "speech_predictor", params.module_spec("speech_predictor", narrow))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    # the block cases under each of the block's process-wide switches, one fresh process per setting, next to the whole run (they are independent of it)
    blocks = [(s, subprocess.Popen([exe, wpath, "block"], env=dict(env, **dict([s.split("=")])), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
              for s in BLOCK_SETTINGS]
    r = subprocess.run([exe, wpath, npath], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    # the contraction cases once more under each experiment switch, one fresh process per setting (gemm_switches() reads them once per process); printed first,
    # so that the output still ends with the whole run's last lines
    rc = r.returncode
    for setting in GEMM_SETTINGS:
        if rc != 0:
            break
        k, v = setting.split("=")
        g = subprocess.run([exe, wpath, "gemm"], env=dict(env, **{k: v}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print("".join(f"[{setting}] {line}\n" for line in g.stdout.splitlines()))
        rc = g.returncode
    for setting, p in blocks:
        out = p.communicate()[0]
        print("".join(f"[{setting}] {line}\n" for line in out.splitlines()))
        rc = rc or p.returncode
    print(r.stdout)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "/tmp/stts_asan_build"))
