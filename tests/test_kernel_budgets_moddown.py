"""Budgets of the key-switch kernels with the mod-down tail (ks_row_mac_fp_moddown / ks_row_mac_moddown, the Q slots of
a CKKS method-I key switch on the fused path): the same two waves per SIMD and no scratch as the kernels without it
(tests/test_kernel_budgets.py) -- the tail runs after the digit loop and must not add live values across it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# kernel (substring of the mangled name) -> (minimum waves per SIMD, maximum scratch bytes per lane)
BUDGETS = {
    "21ks_row_mac_fp_moddownE": (2, 0),
    "18ks_row_mac_moddownE": (2, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_moddown_tail_kernels_keep_their_register_budgets(tmp_path):
    src = os.path.join(ROOT, "heongpu_amd", "csrc", "ntt.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", src,
                        "-o", str(tmp_path / "ntt.s"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    for key, (min_waves, max_scratch) in BUDGETS.items():
        hits = [n for n in usage if key in n]
        assert len(hits) == 1, (key, hits)
        u = usage[hits[0]]
        assert u.get("Occupancy", 0) >= min_waves, (hits[0], u)
        assert u.get("ScratchSize", 0) <= max_scratch, (hits[0], u)
