#!/usr/bin/env python3
"""Build the library's HOST side with AddressSanitizer + UBSan against the HIP stub (the steps of build_and_run.py) and run rmvpe_viterbi_driver.cpp,
a stand-alone program, on the model config's dims.  Nothing is preloaded and nothing runs on a device.

    python tests/asan/rmvpe_viterbi_build_and_run.py [build_dir]

Exit code 0 = no sanitizer report and every case of the driver held (the query sizes the carving, ragged batches run, every refusal comes before any launch)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main(build_dir):
    os.makedirs(build_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17", "-fPIC"]
    import __graft_entry__ as entry

    objs, procs = [], []
    for u in entry.UNITS:
        o = os.path.join(build_dir, u.replace(".hip", "_host.o"))
        objs.append(o)
        procs.append(subprocess.Popen([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-DSTTS_TEST_OPS", *san, "-c", os.path.join(ROOT, "stylish_tts_amd", "csrc", u), "-o", o]))
    if any(p.wait() != 0 for p in procs):
        raise subprocess.CalledProcessError(1, "hipcc --cuda-host-only")
    fatbin = sorted({s for o in objs for s in subprocess.check_output(["nm", "-u", o], text=True).split() if s.startswith("__hip_fatbin")})
    cxx = os.environ.get("CXX_ASAN", "/opt/rocm/lib/llvm/bin/clang++")
    stub = os.path.join(build_dir, "hip_stub.o")
    subprocess.check_call([cxx, *san, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", os.path.join(HERE, "hip_stub.cpp"), "-o", stub])
    lib = os.path.join(build_dir, "libstylish_hip_asan.so")
    subprocess.check_call([cxx, "-shared", *san, *objs, stub, *[f"-Wl,--defsym={s}=stts_stub_fatbin" for s in fatbin], "-o", lib])
    exe = os.path.join(build_dir, "rmvpe_viterbi_driver")
    subprocess.check_call([cxx, *san, os.path.join(HERE, "rmvpe_viterbi_driver.cpp"), lib, f"-Wl,-rpath,{build_dir}", "-o", exe])

    from stylish_tts_amd import _lib
    from stylish_tts_amd.config import load_model_config

    dpath = os.path.join(build_dir, "rmvpe_viterbi_dims.bin")
    with open(dpath, "wb") as f:
        f.write(bytes(_lib.dims_from_config(load_model_config())))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, dpath], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "/tmp/stts_asan_rmvpe_viterbi_build"))
