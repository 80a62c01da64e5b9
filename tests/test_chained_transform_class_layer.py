"""Chained giant steps through the class layer of include/heongpu/heongpu.hpp (LinearTransform's chain_giant_steps,
HEArithmeticOperator::set_chained_giant_steps) by the project's own consumer tests/cpp/test_chained_transform.cpp: it
compiles on a host without a GPU, and on the GPU it runs a chained LinearTransform on a Galois key built from its reduced
required_shifts() against the dense product, generates the encoding-transform context with the switch on and off,
compares the two key_indexs_, carries coeff_to_slot -> slot_to_coeff on the reduced key, checks the exception type of a
missing key, and exits non-zero on a wrong result.
(`make -C heongpu_amd/csrc chainedtransformtest` builds the same program by hand.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB_DIR = os.path.join(ROOT, "heongpu_amd", "lib")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_cpp_chained_transform")
    assert os.path.exists(os.path.join(LIB_DIR, "libhegpu.so")), "build the library first (__graft_entry__.build())"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_chained_transform.cpp"),
                        "-o", exe, "-L" + LIB_DIR, "-lhegpu", "-Wl,-rpath," + LIB_DIR],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chained_transform_consumer_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_chained_transforms_through_the_class_layer(tmp_path):
    import torch
    assert torch.cuda.is_available()
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "all chained-transform class-layer checks passed" in r.stdout
