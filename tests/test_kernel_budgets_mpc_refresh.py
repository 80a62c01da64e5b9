"""The kernels of the collective refresh (keygen.hip; CPU-only: hipcc cross-compiles for gfx950 and reports every
kernel's resource usage) compile without scratch memory, and the library exports the four entries.  The streaming
kernels carry the share pointers as a by-value array, like the other multiparty kernels; the lift composes up to 64 words
of a coefficient in registers, every word index static, and parks them in LDS before the loops that index them at run
time -- the form that spills first if that is got wrong.  No
occupancy figure is pinned: nobody has measured where it stops mattering for these kernels."""
import os
import subprocess

import pytest

from test_kernel_budgets import HIPCC, _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFRESH_KERNELS = ["k_kg_mpc_refresh_noiseE", "k_kg_mpc_shareE", "k_kg_mpc_refresh_bfv_noiseE",
                   "k_kg_mpc_sumE", "k_kg_mpc_refresh_finishE", "k_kg_mpc_bfv_roundE",
                   # one instance per bound on the word count, as the decoder's compose
                   "k_kg_mpc_refresh_liftILi8EE", "k_kg_mpc_refresh_liftILi16EE", "k_kg_mpc_refresh_liftILi32EE",
                   "k_kg_mpc_refresh_liftILi64EE"]
ENTRIES = ["hegpu_mpc_ckks_refresh_share", "hegpu_mpc_ckks_refresh_merge", "hegpu_mpc_bfv_refresh_share",
           "hegpu_mpc_bfv_refresh_merge"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refresh_kernels_use_no_scratch(tmp_path):
    usage = _usage("keygen.hip", tmp_path)
    for key in REFRESH_KERNELS:
        hits = [n for n in usage if key in n]
        assert len(hits) == 1, (key, hits)
        assert usage[hits[0]].get("ScratchSize", -1) == 0, (hits[0], usage[hits[0]])
    # the decoder's compose kernels share the lift's device function: moving it to a header must not have cost them theirs
    enc = _usage("encode.hip", tmp_path)
    for n, u in enc.items():
        if "compose" in n:
            assert u.get("ScratchSize", -1) == 0, (n, u)


def test_refresh_entries_are_exported():
    lib = os.path.join(ROOT, "heongpu_amd", "lib", "libhegpu.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for e in ENTRIES:
        assert e in names, e
    import heongpu_amd as hg
    for m in ("mpc_ckks_refresh_share", "mpc_ckks_refresh_merge", "mpc_bfv_refresh_share", "mpc_bfv_refresh_merge"):
        assert callable(getattr(hg.Context, m))
    assert (hg.OP_MPC_REFRESH_SHARE, hg.OP_MPC_REFRESH_MERGE) == (20, 21)
