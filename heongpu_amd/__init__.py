"""heongpu_amd -- MI355X-native RNS-polynomial backend behind HEonGPU's operator API.

The product is heongpu_amd/lib/libhegpu.so (hand-written HIP for gfx950 plus
a C ABI, see include/hegpu.h).  This package is the ctypes plumbing used by
tests/ and bench.py; importing it without the built library fails loudly.
"""
from . import _lib
from .api import (BFV, CKKS, SEC_NONE, SEC_128, SEC_192, SEC_256, TABLES_QP, TABLES_Q_BSK, OP_CKKS_RELIN, OP_CKKS_RESCALE,
                  OP_CKKS_GALOIS, OP_CKKS_ROTATE_HOISTED, OP_BFV_MULTIPLY, OP_BFV_RELIN, OP_BFV_GALOIS, E_INVALID, E_LOGIC, E_RUNTIME,
                  E_NODEVICE, Context, HEError, Rng, TfheContext, OP_KEYGEN_SECRET, OP_KEYGEN_PUBLIC,
                  OP_KEYGEN_SWITCH, OP_CKKS_ENCRYPT, OP_BFV_ENCRYPT, OP_BFV_DECRYPT, OP_BFV_DECODE, OP_CKKS_ENCODE,
                  OP_CKKS_DECODE, OP_BFV_MULTIPLY_PLAIN, OP_MPC_KEY_SHARE, OP_MPC_BFV_DECRYPT_MERGE, OP_MPC_REFRESH_SHARE, OP_MPC_REFRESH_MERGE,
                  MPC_PUBLIC_KEY,
                  MPC_GALOIS_KEY, MPC_RELIN_ROUND1, GATE_NAND, GATE_AND, GATE_AND_FIRST_NOT,
                  GATE_NOR, GATE_OR, GATE_XNOR, GATE_XOR, GATE_NOT, steps_to_galois_elt, ks_launch_forms, linear_transform_plan, giant_step_chain, chained_giant_steps, GiantStepChain, encoding_transform_factors, poly_eval_plan, eval_mod_plan, PolyEvalPlan, bootstrap_plan, BootstrapPlan, eval_trig_plan, slim_bootstrap_plan, SlimBootstrapPlan, SLIM_FUNCTIONS, OP_CKKS_MOD_RAISE, OP_CKKS_BOOTSTRAP, MONOMIAL, CHEBYSHEV, POLY_POWER, POLY_LEAF, POLY_COMBINE, POLY_TAIL_NONE, POLY_TAIL_ONE, to_device, to_host, default_options, broadcast_key, broadcast_bytes, broadcast_path_name,
                  BCAST_FLAT, BCAST_TREE, BCAST_STAGED, BCAST_SAME_DEVICE, OP_CKKS_LOGIC_GATE, OP_BFV_LOGIC_GATE, LOGIC_AND,
                  LOGIC_OR, LOGIC_XOR, LOGIC_NAND, LOGIC_NOR, LOGIC_XNOR, LOGIC_NOT, GATE_B_NONE, GATE_B_CIPHER, GATE_B_PLAIN)

_lib.load()

__all__ = ["BFV", "CKKS", "SEC_NONE", "SEC_128", "SEC_192", "SEC_256", "TABLES_QP", "TABLES_Q_BSK", "Context", "HEError", "Rng",
           "steps_to_galois_elt", "ks_launch_forms", "linear_transform_plan", "giant_step_chain", "chained_giant_steps", "GiantStepChain", "encoding_transform_factors", "poly_eval_plan", "eval_mod_plan", "PolyEvalPlan", "bootstrap_plan", "BootstrapPlan", "eval_trig_plan", "slim_bootstrap_plan", "SlimBootstrapPlan", "SLIM_FUNCTIONS", "MONOMIAL", "CHEBYSHEV", "POLY_POWER", "POLY_LEAF", "POLY_COMBINE", "POLY_TAIL_NONE", "POLY_TAIL_ONE", "to_device", "to_host", "default_options", "broadcast_key", "broadcast_bytes", "broadcast_path_name",
           "BCAST_FLAT", "BCAST_TREE", "BCAST_STAGED", "BCAST_SAME_DEVICE"]
