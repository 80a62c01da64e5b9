"""The class layer of the CKKS refresh in include/heongpu/heongpu.hpp (EvalModConfig, EncodingMatrixConfig,
BootstrappingConfigV2, generate_bootstrapping_params_v2, bootstrapping_key_indexs, regular_bootstrapping_v2,
generate_secret_key_v2, PrecisionStats) through the project's own consumer tests/cpp/test_bootstrap.cpp: it compiles on a
host without a GPU, and on the GPU it runs the call sequence of the reference's example 5 at N = 4096, prints the
precision statistics, fails above 1e-4, checks the two exceptions of regular_bootstrapping_v2 and that the parameters
lock.  The reference's own example/bootstrapping/5_ckks_regular_bootstrapping_v2.cpp compiles unchanged where its tree is
available (compile only: its key generation at N = 2^16 alone takes longer than a suite test may)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB_DIR = os.path.join(ROOT, "heongpu_amd", "lib")
REFERENCE = os.environ.get("HEONGPU_REFERENCE_DIR", "/root/reference")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_cpp_bootstrap")
    assert os.path.exists(os.path.join(LIB_DIR, "libhegpu.so")), "build the library first (__graft_entry__.build())"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_bootstrap.cpp"),
                        "-o", exe, "-L" + LIB_DIR, "-lhegpu", "-Wl,-rpath," + LIB_DIR],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_bootstrap_consumer_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_reference_example_5_compiles_unchanged(tmp_path):
    """the flags of the other reference consumers (oracle/ref_build.py); nothing of the build is kept"""
    name = "5_ckks_regular_bootstrapping_v2"
    src = os.path.join(REFERENCE, "example", "bootstrapping", name + ".cpp")
    if not os.path.exists(src):
        pytest.skip("no reference tree on this machine")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fopenmp", "-DHEONGPU_CUDA_NAMES",
                        "-DHEONGPU_WITH_ZLIB", "-w", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "include", "heongpu", "consumer_compat"),
                        "-I" + os.path.join(REFERENCE, "example"), "-I" + os.path.join(ROOT, "tests", "cpp"),
                        "-x", "hip", src, "-o", os.path.join(str(tmp_path), name), "-L" + LIB_DIR, "-lhegpu", "-lz",
                        "-Wl,-rpath," + LIB_DIR], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_refresh_through_the_class_layer(tmp_path):
    import torch
    assert torch.cuda.is_available()
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "all bootstrap class-layer checks passed" in r.stdout
