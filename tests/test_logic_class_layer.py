"""The logic-gate class layer of include/heongpu/heongpu.hpp (HELogicOperator<Scheme::BFV>, HELogicOperator<Scheme::CKKS>)
through the project's own consumer tests/cpp/test_logic.cpp: it compiles on a host without a GPU, and on the GPU it runs every
gate with a ciphertext and a plaintext second operand, out of place and in place, checks the values, the result's depth,
scale and flags, the exception type of every refusal, a HOST-stored operand and that an out-of-place NOT leaves its input
alone, and exits non-zero on a wrong result.  (`make -C heongpu_amd/csrc logictest` builds the same program by hand.)
The reference's own example/basic/11_basic_bfv_logic.cpp and 12_basic_ckks_logic.cpp compile unchanged where its tree is
available."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB_DIR = os.path.join(ROOT, "heongpu_amd", "lib")
REFERENCE = os.environ.get("HEONGPU_REFERENCE_DIR", "/root/reference")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_cpp_logic")
    assert os.path.exists(os.path.join(LIB_DIR, "libhegpu.so")), "build the library first (__graft_entry__.build())"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_logic.cpp"),
                        "-o", exe, "-L" + LIB_DIR, "-lhegpu", "-Wl,-rpath," + LIB_DIR],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_logic_consumer_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("name", ["11_basic_bfv_logic", "12_basic_ckks_logic"])
def test_reference_logic_example_compiles_unchanged(name, tmp_path):
    """the flags of the other reference consumers (oracle/ref_build.py); nothing of the build is kept"""
    src = os.path.join(REFERENCE, "example", "basic", name + ".cpp")
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
def test_logic_gates_through_the_class_layer(tmp_path):
    import torch
    assert torch.cuda.is_available()
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "all logic class-layer checks passed" in r.stdout
