"""Budget of the one kernel the slim, bit and gate refreshes add (CPU-only: hipcc's resource-usage remarks for gfx950, as
tests/test_kernel_budgets_bootstrap.py).

k_ckks_conj_real is the real half of k_ckks_conj_split: two 16-byte loads, two modular additions per word pair, one
16-byte store; no Barrett product, no psi_half.  One instance, no scratch, no LDS, at most 64 registers, eight waves per
SIMD.  The counts are printed and recorded in DESIGN.md 4.5g."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_ckks_conj_real_is_a_stream(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    hits = [n for n in usage if "k_ckks_conj_real" in n]
    assert len(hits) == 1, hits
    u = usage[hits[0]]
    print(hits[0], u)
    assert u["ScratchSize"] == 0 and u["LDS Size"] == 0, u
    assert u["VGPRs"] <= 64 and u["Occupancy"] == 8, u
    # the split next to it, for the comparison the design document makes
    split = [n for n in usage if "k_ckks_conj_split" in n]
    assert len(split) == 1, split
    print(split[0], usage[split[0]])
