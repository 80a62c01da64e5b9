"""Budgets of the wide row kernels (context option "wide_access": ks_pair_mac_fp / ks_pair_mac, with and without the
mod-down tail): each keeps the two waves per SIMD and the empty scratch of the natural kernel it stands beside
(ks_row_mac_fp, ks_row_mac_fp_moddown, ks_row_mac, ks_row_mac_moddown).  The 16-byte loads want their registers in
aligned groups of four, so the eight LDS read-back addresses and the store address of the pair ownership are formed
where they are used instead of being held across the digit loop (ntt.hip: ks_own_read).  In the style of
tests/test_kernel_budgets_quotient.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# kernel (substring of the mangled name) -> (minimum waves per SIMD, maximum scratch bytes per lane)
BUDGETS = {
    "14ks_pair_mac_fpILb0EE": (2, 0),
    "14ks_pair_mac_fpILb1EE": (2, 0),
    "11ks_pair_macILb0EE": (2, 0),
    "11ks_pair_macILb1EE": (2, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wide_row_kernels_keep_the_budgets_of_the_natural_ones(tmp_path):
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
