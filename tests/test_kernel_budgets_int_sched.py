"""Budgets of the integer transform kernels that carry the correction schedule of the correcting butterflies (ntt.hip
cs_sched) and are not pinned elsewhere: the column passes of N = 2^12 ... 2^15 (tests/test_kernel_budgets.py pins the
N = 2^16 ones, ntt_fwd_row and ks_row_mac; tests/test_kernel_budgets_moddown.py the mod-down forms).  A third body per
kernel (scheduled next to correction-free and correcting-every-stage) must not cost registers: the ceilings are the
counts of the commit before the schedule, and no kernel may use scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# kernel (substring of the mangled name) -> (maximum VGPRs, minimum waves per SIMD)
BUDGETS = {
    "11ntt_fwd_colILi4ELb1EE": (90, 5),
    "11ntt_fwd_colILi4ELb0EE": (114, 4),
    "11ntt_fwd_colILi5ELb1EE": (87, 4),
    "11ntt_fwd_colILi5ELb0EE": (109, 4),
    "11ntt_fwd_colILi6ELb1EE": (102, 4),
    "11ntt_fwd_colILi6ELb0EE": (109, 4),
    "11ntt_fwd_colILi7ELb1EE": (106, 4),
    "11ntt_fwd_colILi7ELb0EE": (109, 4),
}
# every kernel the schedule touches, pinned here or elsewhere: no scratch
NO_SCRATCH = list(BUDGETS) + ["11ntt_fwd_colILi8ELb0EE", "11ntt_fwd_colILi8ELb1EE", "11ntt_fwd_rowE", "10ks_row_macILb0EE",
                              "18ks_row_mac_moddownE", "21ks_row_mac_fp_moddownE"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_scheduled_integer_kernels_keep_their_registers(tmp_path):
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

    def one(key):
        hits = [n for n in usage if key in n]
        assert len(hits) == 1, (key, hits)
        return hits[0], usage[hits[0]]

    for key, (max_vgprs, min_waves) in BUDGETS.items():
        n, u = one(key)
        assert u.get("VGPRs", 1 << 30) + u.get("AGPRs", 0) <= max_vgprs, (n, u)
        assert u.get("Occupancy", 0) >= min_waves, (n, u)
    for key in NO_SCRATCH:
        n, u = one(key)
        assert u.get("ScratchSize", 1) == 0, (n, u)
