"""Resource budgets of the two polynomial-evaluation kernels of rns.hip (CPU-only: the hipcc resource report).  Both are
streams: no instance may spill, and the widest weighted sum -- 16 loads of 16 bytes in flight per part -- may take no more
registers than the widest k_ckks_diag_mac, which holds twice as many loaded values.  Nobody has measured where occupancy
matters for this kernel, so the register count is printed.  That comparison alone guards little (k_ckks_diag_mac<16> takes
all 256 registers), so the widest instance is also held to 128 registers, four waves per SIMD: its 16 loads of 16 bytes in
flight are 64 registers, and the accumulators, the modulus record and the addresses have to fit the other 64 -- beyond that
a compute unit has fewer wavefronts streaming than the narrower instances, which is the regression to catch."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_poly_eval_kernels_do_not_spill(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    wsum = {n: u for n, u in usage.items() if "k_ckks_weighted_sum" in n}
    dsub = {n: u for n, u in usage.items() if "k_ckks_double_sub" in n}
    assert len(wsum) == 5 and len(dsub) == 1, (sorted(wsum), sorted(dsub))
    for name, u in {**wsum, **dsub}.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
    widest = [u for n, u in wsum.items() if "ILi16EE" in n]
    diag = [u for n, u in usage.items() if "k_ckks_diag_macILi16EE" in n]
    assert len(widest) == 1 and len(diag) == 1
    print("k_ckks_weighted_sum<16> registers:", widest[0]["VGPRs"], " k_ckks_diag_mac<16>:", diag[0]["VGPRs"])
    assert widest[0]["VGPRs"] <= diag[0]["VGPRs"]
    assert widest[0]["VGPRs"] <= 128 and widest[0]["Occupancy"] >= 4, widest[0]
