"""Budgets of the modulus raise (CPU-only: hipcc's resource-usage remarks for gfx950, as tests/test_kernel_budgets.py).

k_mod_raise is a stream like k_decompose -- one 16-byte load, `limbs` 16-byte stores: one instance, no scratch, no LDS, and
few enough registers for eight waves per SIMD (128 at most; it takes 22).

hegpu_ckks_mod_raise launches the decomposing forward transform that the rescale and the mod-down launch; it must not have
added a kernel to ntt.hip.  The families of forward kernels are counted (a new template instance would show here), none
of them may spill, and the budgets tests/test_kernel_budgets.py pins for the existing instances are asserted again on the
same report."""
import os
import re
from collections import Counter

import pytest

from test_kernel_budgets import BUDGETS, HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_mod_raise_is_a_stream(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    hits = [n for n in usage if "k_mod_raise" in n]
    assert len(hits) == 1, hits
    u = usage[hits[0]]
    print(hits[0], u)
    assert u["ScratchSize"] == 0 and u["LDS Size"] == 0, u
    assert u["VGPRs"] <= 128 and u["Occupancy"] == 8, u


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_new_transform_instance(tmp_path):
    usage = _usage("ntt.hip", tmp_path)
    families = Counter(re.sub(r"(IL|E?NS_).*", "", n.replace("_ZN5hegpu", "")) for n in usage)
    print(dict(families))
    # S1 = 4 .. 8, plain and decomposing; the single pass up to N = 2^14; the multi-modulus column pass; its 2^16 form
    assert families["11ntt_fwd_col"] == 10 and families["14ntt_fwd_single"] == 6
    assert families["17ntt_fwd_col_multi"] == 5 and families["22ntt_fwd_col_decomp_all"] == 1
    assert families["11ntt_fwd_row"] == 1 and families["11ntt_inv_row"] == 1 and families["11ntt_inv_col"] == 10
    for name, u in usage.items():
        if "ntt_fwd" in name:
            assert u["ScratchSize"] == 0, (name, u)
    for key, (min_waves, max_scratch) in BUDGETS.items():
        hits = [n for n in usage if key in n]
        assert len(hits) == 1, (key, hits)
        assert usage[hits[0]]["Occupancy"] >= min_waves and usage[hits[0]]["ScratchSize"] <= max_scratch, (hits[0], usage[hits[0]])
