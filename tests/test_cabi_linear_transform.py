"""CPU: the linear-transform entries of include/hegpu.h are exported by libhegpu.so with the declared argument counts,
and without a device they fail loudly instead of falling back."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hegpu_ckks_diag_mac": 13, "hegpu_ckks_linear_transform_workspace_bytes": 5, "hegpu_ckks_linear_transform": 19}


def test_symbols_and_argument_counts(hg):
    from heongpu_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hegpu.h")).read(), flags=re.S)
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name, argc in ENTRIES.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, f"{name} is not declared in hegpu.h"
        assert len(m.group(1).split(",")) == argc, (name, m.group(1))
        assert len(bound[name][2]) == argc, (name, "ctypes signature")


def test_workspace_size_function(hg):
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [40, 30, 30], [40], sec=hg.SEC_NONE)
    n, Q = 4096, 3
    for n1, n2, depth, batch in ((4, 7, 0, 1), (1, 1, 1, 2), (16, 2, 0, 3)):
        ct = 2 * (Q - depth) * n * 8
        want = (max(n1, n2) + n2) * ct * batch + c.workspace_bytes(hg.OP_CKKS_ROTATE_HOISTED, depth, batch)
        assert c.linear_transform_workspace_bytes(n1, n2, depth, batch) == want
    assert c.linear_transform_workspace_bytes(17, 1, 0, 1) == 0
    assert c.linear_transform_workspace_bytes(1, 0, 0, 1) == 0
    # the existing rows are untouched
    assert c.workspace_bytes(hg.OP_CKKS_GALOIS, 0, 1) == (2 * 3 + 3 * 4 + 2 * 4) * n * 8


def test_no_device_means_loud_failure(hg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [36, 36], [37])
    lib = c._lib
    ix = (ctypes.c_int * 1)(0)
    assert lib.hegpu_ckks_diag_mac(c._h, 0, 0, 1, 0, 1, ix, 1, 0, 0, 0, 1, None) == hg.E_NODEVICE
    keys = (ctypes.c_void_p * 1)(None)
    elts = (ctypes.c_int * 1)(0)
    assert lib.hegpu_ckks_linear_transform(c._h, 0, 0, 0, 0, 0, 1, ix, 1, 1, keys, elts, keys, elts, 0, 1, None, 0,
                                           None) == hg.E_NODEVICE
