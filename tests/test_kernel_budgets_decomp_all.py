"""Budget of the decomposing column pass that carries the integer targets (ntt_fwd_col_decomp_all<8>; CPU-only, hipcc's
resource-usage remarks for gfx950 as in tests/test_kernel_budgets.py).  The kernel replaces two launches only while three
of its workgroups share a CU: at most 168 registers (three waves per SIMD), no scratch, and static LDS of which three
copies fit the 160 KiB of a CU.  The two kernels it stands in for stay instantiated -- the launches it does not take
(S1 = 7, plans without integer targets, unknown integer slots, copy_src) still use them."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_decomp_all_keeps_three_workgroups_per_cu(tmp_path):
    usage = _usage("ntt.hip", tmp_path)
    hits = [n for n in usage if "22ntt_fwd_col_decomp_allILi8EE" in n]
    assert len(hits) == 1, hits
    u = usage[hits[0]]
    print(hits[0], u)
    assert u.get("Occupancy", 0) >= 3, (hits[0], u)
    assert u.get("ScratchSize", 1) == 0, (hits[0], u)
    assert u.get("LDS Size", 1 << 30) * 3 <= 160 * 1024, (hits[0], u)
    assert [n for n in usage if "ntt_fwd_col_decomp_all" in n] == hits, "instantiated for S1 = 8 only"
    for key in ("17ntt_fwd_col_multiILi8EE", "11ntt_fwd_colILi8ELb1EE"):
        assert len([n for n in usage if key in n]) == 1, key
