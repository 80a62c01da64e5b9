"""The two kernels at the real / imaginary boundary of CoeffToSlot / SlotToCoeff (rns.hip; CPU-only: hipcc
cross-compiles for gfx950 and reports every kernel's resource usage) compile without scratch memory.  They are streaming
kernels of a handful of live values per thread; their register counts are recorded (printed), not pinned: nobody has
measured where occupancy matters for these streams."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage

KERNELS = ["17k_ckks_conj_splitE", "17k_ckks_conj_mergeE"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_boundary_kernels_use_no_scratch(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    for tag in KERNELS:
        names = [n for n in usage if tag in n]
        assert len(names) == 1, (tag, names)
        u = usage[names[0]]
        print(names[0], {k: u[k] for k in sorted(u) if "GPR" in k or "Scratch" in k or "Occupancy" in k})
        assert u.get("ScratchSize", -1) == 0, (names[0], u)
        assert 0 < u.get("VGPRs", 0) <= 64, (names[0], u)  # a streaming kernel: far from any occupancy limit
