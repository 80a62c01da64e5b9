"""Recipe for the reference-consumer binaries (TEST INFRASTRUCTURE): the reference's own benchmark, example and test
programs, compiled UNCHANGED from the reference tree against include/heongpu/heongpu.hpp + libhegpu.so (only the cuda*
runtime names they call themselves are mapped, include/heongpu/cuda_names.hpp).

Outputs go to oracle/_ref/ (git-ignored; built where the reference tree is available and carried with the working tree
to the machine that runs the GPU tests).  They find heongpu_amd/lib/libhegpu.so through their rpath, so a later build of
the library on that machine is the one they run against.  Programs whose source is absent are skipped.

The second product is oracle/_ref/libref_kernels.so: the reference's own RNS kernel files (REFERENCE_KERNEL_FILES),
compiled UNCHANGED and in place against the stand-in for the one GPU-NTT header they include (oracle/ref_shim/) and linked
with oracle/ref_kernels_driver.cpp, whose refk_* entries launch them next to this project's kernels
(tests/test_gpu_reference_kernels.py).  Skipped when the reference tree is absent, like the consumers.

The reference tree is HEONGPU_REFERENCE_DIR, default /root/reference."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")
HIPCC = "/opt/rocm/bin/hipcc"

REFERENCE_BENCHMARKS = ("ckks", "bfv", "tfhe")
# the reference's example programs that stay inside the built scope (example/basic/*.cpp)
REFERENCE_EXAMPLES = ("1_basic_bfv", "2_basic_ckks", "3_basic_memorypool_config", "4_switchkey_methods_bfv",
                      "5_switchkey_methods_ckks", "8_default_stream_usage", "9_multi_stream_usage_way1",
                      "6_ckks_coefficient_encoding", "10_multi_stream_usage_way2", "13_bfv_serialization",
                      "14_ckks_serialization", "15_basic_tfhe")
# the reference's own test programs (test/*.cpp, GoogleTest TEST/EXPECT_EQ through tests/cpp/gtest/gtest.h)
REFERENCE_TESTS = ("test_bfv_addition", "test_bfv_encoding", "test_bfv_encryption", "test_bfv_multiplication",
                   "test_bfv_relinearization", "test_bfv_rotation_method_1", "test_bfv_rotation_method_2",
                   "test_ckks_addition", "test_ckks_encoding", "test_ckks_encryption", "test_ckks_multiplication",
                   "test_ckks_relinearization", "test_ckks_rotation_method_1", "test_ckks_rotation_method_2",
                   "test_tfhe_gate_boot")
# src/lib/kernel/<name>.cu: every RNS kernel of the hot path; all they need of GPU-NTT is gpuntt/common/modular_arith.cuh
REFERENCE_KERNEL_FILES = ("switchkey", "multiplication", "addition")
KERNELS_LIB = os.path.join(OUT_DIR, "libref_kernels.so")


def reference_dir():
    return os.environ.get("HEONGPU_REFERENCE_DIR", "/root/reference")


def exe_path(name):
    """oracle/_ref/<name>: ref_benchmark_<b>, ref_example_<e>, ref_<test>"""
    return os.path.join(OUT_DIR, name)


def jobs(ref):
    out = [(os.path.join(ref, "benchmark", "benchmark_%s.cpp" % n), "ref_benchmark_" + n) for n in REFERENCE_BENCHMARKS]
    out += [(os.path.join(ref, "example", "basic", "%s.cpp" % n), "ref_example_" + n) for n in REFERENCE_EXAMPLES]
    out += [(os.path.join(ref, "test", "%s.cpp" % n), "ref_" + n) for n in REFERENCE_TESTS]
    return out


def build_kernels(ref):
    """oracle/_ref/libref_kernels.so from the three reference kernel files + the driver; no-op without the reference tree."""
    srcs = [os.path.join(ref, "src", "lib", "kernel", n + ".cu") for n in REFERENCE_KERNEL_FILES]
    if not any(os.path.exists(s) for s in srcs):
        return
    os.makedirs(OUT_DIR, exist_ok=True)
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-w", "-I" + shim,
             "-I" + os.path.join(shim, "compat"), "-I" + os.path.join(ref, "src", "include"), "-x", "hip"]
    srcs.append(os.path.join(ROOT, "oracle", "ref_kernels_driver.cpp"))
    with tempfile.TemporaryDirectory(prefix="ref_kernels_") as tmp:
        objs = [os.path.join(tmp, "%d.o" % i) for i in range(len(srcs))]
        procs = [subprocess.Popen(flags + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
        failed = [p for p in procs if p.wait() != 0]
        if failed:
            raise RuntimeError("a reference kernel file no longer compiles unchanged: %s" % " ".join(failed[0].args))
        link = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", KERNELS_LIB]
        if subprocess.call(link) != 0:
            raise RuntimeError("the reference kernel library does not link: %s" % " ".join(link))


def build():
    """Compile every reference consumer whose source exists (in parallel); needs heongpu_amd/lib/libhegpu.so built."""
    ref = reference_dir()
    build_kernels(ref)
    todo = [(src, out) for src, out in jobs(ref) if os.path.exists(src)]
    if not todo:
        return
    os.makedirs(OUT_DIR, exist_ok=True)
    lib = os.path.join(ROOT, "heongpu_amd", "lib")
    procs = []
    for src, out in todo:
        procs.append(subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fopenmp", "-DHEONGPU_CUDA_NAMES",
             "-DHEONGPU_WITH_ZLIB", "-w", "-I" + os.path.join(ROOT, "include"),
             "-I" + os.path.join(ROOT, "include", "heongpu", "consumer_compat"), "-I" + os.path.join(ref, "example"),
             "-I" + os.path.join(ROOT, "tests", "cpp"),
             "-x", "hip", src, "-o", exe_path(out), "-L" + lib, "-lhegpu", "-lz",
             "-Wl,-rpath,$ORIGIN/../../heongpu_amd/lib"]))
    failed = [p for p in procs if p.wait() != 0]
    if failed:
        raise RuntimeError("a reference consumer no longer compiles unchanged: %s" % " ".join(failed[0].args))
