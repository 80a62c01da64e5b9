"""The linear-transform kernels of rns.hip (CPU-only: hipcc cross-compiles for gfx950 and reports every kernel's resource
usage) compile without scratch memory.  k_ckks_diag_mac keeps 2 n1 rotated values per coefficient in a register array;
an index into it that is not a compile-time constant would move the array to private memory, which is why the kernel is
instantiated on the row width.  No occupancy figure is pinned: nobody has measured where it matters for these streams."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage

WIDTHS = [1, 2, 4, 8, 16]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_linear_transform_kernels_use_no_scratch(tmp_path):
    usage = _usage("rns.hip", tmp_path)
    mac = sorted(n for n in usage if "15k_ckks_diag_macILi" in n)
    assert [n for w in WIDTHS for n in mac if "15k_ckks_diag_macILi%dEE" % w in n] == sorted(
        mac, key=lambda n: int(n.split("ILi")[1].split("E")[0])), mac
    assert len(mac) == len(WIDTHS), mac
    total = [n for n in usage if "16k_ckks_sum_termsE" in n]
    assert len(total) == 1, total
    for name in mac + total:
        assert usage[name].get("ScratchSize", -1) == 0, (name, usage[name])
