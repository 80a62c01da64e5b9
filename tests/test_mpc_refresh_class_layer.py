"""The collective refresh of the multiparty class layer (HEMultiPartyManager::distributed_bootstrapping_participant /
_coordinator, include/heongpu/heongpu.hpp) through the project's own consumer tests/cpp/test_mpc_refresh.cpp: it compiles
on a host without a GPU, and on the GPU three parties take a product down to the last level (CKKS) or through a
multiplication (BFV), refresh it, multiply again and open the result by collective decryption; the program exits
non-zero on a wrong result."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB_DIR = os.path.join(ROOT, "heongpu_amd", "lib")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_cpp_mpc_refresh")
    assert os.path.exists(os.path.join(LIB_DIR, "libhegpu.so")), "build the library first (__graft_entry__.build())"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_mpc_refresh.cpp"),
                        "-o", exe, "-L" + LIB_DIR, "-lhegpu", "-Wl,-rpath," + LIB_DIR],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refresh_consumer_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_three_parties_refresh_through_the_class_layer(tmp_path):
    import torch
    assert torch.cuda.is_available()
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert "all collective-refresh class-layer checks passed" in r.stdout
