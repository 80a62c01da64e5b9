"""CPU: the encoding-transform entries of include/hegpu.h are exported by libhegpu.so with the declared argument counts,
the workspace size function adds up, and without a device the device entries fail loudly instead of falling back."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hegpu_encoding_transform_shape": 6, "hegpu_encoding_transform_fill": 7, "hegpu_ckks_conj_split": 12,
           "hegpu_ckks_conj_merge": 11, "hegpu_ckks_encoding_transform_workspace_bytes": 5, "hegpu_ckks_coeff_to_slot": 14,
           "hegpu_ckks_slot_to_coeff": 14}


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


def test_factor_struct_matches_the_header(hg):
    from heongpu_amd import _lib
    header = open(os.path.join(ROOT, "include", "hegpu.h")).read()
    body = re.search(r"typedef struct hegpu_linear_factor \{(.*?)\} hegpu_linear_factor;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.LinearFactor._fields_], names


def test_workspace_size_function(hg):
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [40, 30, 30, 30, 30], [40], sec=hg.SEC_NONE)
    n, Q = 4096, 5
    factors = [(0, 1, [[0] * 3] * 7, [None] * 3, [0] * 3, [None] * 7, [0] * 7),
               (0, 1, [[0] * 8] * 2, [None] * 8, [0] * 8, [None] * 2, [0] * 2)]
    for depth, batch in ((0, 1), (1, 3)):
        step = max(c.linear_transform_workspace_bytes(3, 7, depth, batch), c.linear_transform_workspace_bytes(8, 2, depth, batch))
        assert c.encoding_transform_workspace_bytes(factors, depth, batch) == 2 * 2 * (Q - depth) * n * 8 * batch + step
    assert c.encoding_transform_workspace_bytes(factors, Q, 1) == 0
    assert c.encoding_transform_workspace_bytes([], 0, 1) == 0


def test_no_device_means_loud_failure(hg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [36, 36, 36, 36], [37], sec=hg.SEC_NONE)
    lib = c._lib
    assert lib.hegpu_ckks_conj_split(c._h, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, None) == hg.E_NODEVICE
    assert lib.hegpu_ckks_conj_merge(c._h, 0, 0, 0, 0, 0, 0, 0, 0, 1, None) == hg.E_NODEVICE
    assert lib.hegpu_ckks_coeff_to_slot(c._h, 0, 0, 0, 0, 0, None, 0, 0, 0, 1, None, 0, None) == hg.E_NODEVICE
    assert lib.hegpu_ckks_slot_to_coeff(c._h, 0, 0, 0, 0, 0, 0, None, 0, 0, 1, None, 0, None) == hg.E_NODEVICE
    # the factorisation needs no device
    assert len(hg.encoding_transform_factors(4096, True, 3)) == 3
