"""The multiparty kernels of keygen.hip (CPU-only: hipcc cross-compiles for gfx950 and reports every kernel's resource
usage) compile without scratch memory.  They are HBM streams; a spill would add a second stream of private-memory traffic
to each.  The share pointers travel as a by-value array in the kernel arguments and are indexed in a loop -- the form
that would spill first if the compiler copied the array to private memory.  No occupancy figure is pinned: nobody has
measured where it stops mattering for these kernels."""
import os

import pytest

from test_kernel_budgets import HIPCC, _usage

MPC_KERNELS = ["k_kg_switchkey",            # widened: also the round-1 share of the relinearisation key
               "k_kg_mpc_relin_round2", "k_kg_mpc_accumulate", "k_kg_mpc_add_gaussian",
               "k_kg_mpc_share",            # the decrypt share; with a second half, the refresh share
               "k_kg_mpc_sum",              # the CKKS merge; with a share stride and offset, the refresh sums
               "k_kg_mpc_bfv_round",        # the BFV merge; with a share stride, the refresh's
               "k_kg_bfv_decryption"]       # shares its rounding stage with the BFV merge


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mpc_kernels_use_no_scratch(tmp_path):
    usage = _usage("keygen.hip", tmp_path)
    for key in MPC_KERNELS:
        hits = [n for n in usage if key + "E" in n]
        assert len(hits) == 1, (key, hits)
        assert usage[hits[0]].get("ScratchSize", -1) == 0, (hits[0], usage[hits[0]])
