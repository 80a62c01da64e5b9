"""Budget of the one kernel the CKKS refresh adds (CPU-only: hipcc's resource-usage remarks for gfx950, as
tests/test_kernel_budgets_mod_raise.py).

k_scale_q0 multiplies the two q_0 limbs by the refresh's integer pre-multiplier: one 16-byte load, two Barrett products,
one or two 16-byte stores.  One instance, no scratch, no LDS, few enough registers for eight waves per SIMD (128 at most)."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_scale_q0_is_a_stream(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    hits = [n for n in usage if "k_scale_q0" in n]
    assert len(hits) == 1, hits
    u = usage[hits[0]]
    print(hits[0], u)
    assert u["ScratchSize"] == 0 and u["LDS Size"] == 0, u
    assert u["VGPRs"] <= 128 and u["Occupancy"] == 8, u
