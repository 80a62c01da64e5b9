"""Budgets of the kernels whose FP64 products take their quotient from the rounded product (fpmod.cuh fp_mul_nc:
ks_row_mac_fp, ks_row_mac_fp_moddown and the FP64 half of ks_row_mac_split): dropping the recomputed companions must
leave them at the two waves per SIMD and the scratch they had with them -- 0, 0 and 44 bytes per lane (the split
form's hold output addresses across the digit loop, not inside it).  In the style of tests/test_kernel_budgets_moddown.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# kernel (substring of the mangled name) -> (minimum waves per SIMD, maximum scratch bytes per lane)
BUDGETS = {
    "13ks_row_mac_fpILb0EE": (2, 0),
    "21ks_row_mac_fp_moddownE": (2, 0),
    "16ks_row_mac_split": (2, 44),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_quotient_from_product_kernels_keep_their_budgets(tmp_path):
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
        print(hits[0], u)
        assert u.get("Occupancy", 0) >= min_waves, (hits[0], u)
        assert u.get("ScratchSize", 0) <= max_scratch, (hits[0], u)
