"""Resource budgets of k_gate_combine (rns.hip), the one pass after the product of a BFV / CKKS logic gate (CPU-only: the
hipcc resource report).  It is a stream with at most three loads of 16 bytes in flight per thread (a, b and the product):
12 registers of loaded values, the modulus record, the addresses and the BFV plaintext scaling fit 64 registers many times
over, so no instance may spill and the widest is held to 64 VGPRs, eight waves per SIMD.  Nobody has measured whether
occupancy matters for this kernel, so the counts are printed."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gate_combine_does_not_spill(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    gate = {n: u for n, u in usage.items() if "k_gate_combine" in n}
    assert len(gate) == 2, sorted(gate)  # the CKKS and the BFV instance
    for name, u in gate.items():
        print(name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs"] <= 64, (name, u)
