"""The class layer of slim, bit and gate bootstrapping in include/heongpu/heongpu.hpp (BootstrappingConfig,
arithmetic_bootstrapping_type, logic_bootstrapping_type, HEArithmeticOperator<CKKS>::generate_bootstrapping_params /
slim_bootstrapping, HELogicOperator<CKKS>::generate_bootstrapping_params / bootstrapping_key_indexs / bit_bootstrapping /
*_bootstrapping) through the project's own consumer tests/cpp/test_slim_bootstrap.cpp: it compiles on a host without a GPU,
and on the GPU it runs slim (0.2 in every slot), bit (the reference example's message) and AND / XOR with the reference's
call sequences at N = 4096 and secrets of weight 16, fails above 1e-4 and checks the reference's exceptions.  The
reference's own example/bootstrapping/2_..., 3_... and 4_... compile unchanged where its tree is available (compile only,
as example 5 in tests/test_bootstrap_class_layer.py: the consumer above runs their call sequences on shorter chains)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB_DIR = os.path.join(ROOT, "heongpu_amd", "lib")
REFERENCE = os.environ.get("HEONGPU_REFERENCE_DIR", "/root/reference")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_cpp_slim_bootstrap")
    assert os.path.exists(os.path.join(LIB_DIR, "libhegpu.so")), "build the library first (__graft_entry__.build())"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_slim_bootstrap.cpp"),
                        "-o", exe, "-L" + LIB_DIR, "-lhegpu", "-Wl,-rpath," + LIB_DIR],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_slim_bootstrap_consumer_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("name", ["2_ckks_slim_bootstrapping", "3_ckks_bit_bootstrapping", "4_ckks_gate_bootstrapping"])
def test_reference_example_compiles_unchanged(tmp_path, name):
    """the flags of the other reference consumers (oracle/ref_build.py); nothing of the build is kept"""
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
def test_slim_bit_and_gates_through_the_class_layer(tmp_path):
    import torch
    assert torch.cuda.is_available()
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-8000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-1000:]
    assert "all slim bootstrap class-layer checks passed" in r.stdout
