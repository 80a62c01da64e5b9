"""Budgets of every multi-modulus column kernel (CPU-only, hipcc's resource-usage remarks for gfx950 as in
tests/test_kernel_budgets.py): ntt_fwd_col_decomp_all<8> and ntt_fwd_col_multi<8> keep three waves per SIMD (at most 168
registers; 147 as built), ntt_fwd_col_multi<5..7> four (at most 128; 118), none of them uses scratch and the static LDS
stays at 40 KiB (tile + the two twiddle slots)."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage

# kernel (substring of the mangled name) -> (minimum waves per SIMD, maximum registers)
COL_AHEAD = {
    "22ntt_fwd_col_decomp_allILi8EE": (3, 168),
    "17ntt_fwd_col_multiILi8EE": (3, 168),
    "17ntt_fwd_col_multiILi7EE": (4, 128),
    "17ntt_fwd_col_multiILi6EE": (4, 128),
    "17ntt_fwd_col_multiILi5EE": (4, 128),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_multi_modulus_column_kernels_keep_their_waves(tmp_path):
    usage = _usage("ntt.hip", tmp_path)
    for key, (min_waves, max_regs) in COL_AHEAD.items():
        hits = [n for n in usage if key in n]
        assert len(hits) == 1, (key, hits)
        u = usage[hits[0]]
        print(hits[0], u)
        assert u.get("Occupancy", 0) >= min_waves, (hits[0], u)
        assert u.get("VGPRs", 1 << 30) + u.get("AGPRs", 0) <= max_regs, (hits[0], u)
        assert u.get("ScratchSize", 1) == 0, (hits[0], u)
        assert u.get("LDS Size", 0) == 40 * 1024, (hits[0], u)
