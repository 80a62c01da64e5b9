"""CPU: every workspace size the library reports, compared exactly with tests/golden/workspace_sizes.json.

The sizes are public ABI (callers allocate by them), so no row may change by a byte.  Host-only contexts answer the size
queries; nothing here needs a device.  The golden file is this module's own table, written once by running the module as
a script (python tests/test_workspace_sizes.py) at the commit before the workspace layouts became functions.

The contexts are the three-prime sets of the C ABI tests and the method II sets of test_gpu_parity.py::test_ckks_method_II
and ::test_bfv_method_II, all at N = 4096.  The degree-31 Chebyshev plan needs more levels than any of them has: it is
sized on the eight-prime chain of test_gpu_poly_eval.py, which contributes the polynomial rows only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
N = 4096
# name: (scheme, log_q, log_p, plain modulus)
CONTEXTS = {
    "ckks": ("CKKS", [40, 30, 30], [40], 0),
    "ckks_p2": ("CKKS", [40, 35, 35, 35, 35], [40, 40], 0),
    "ckks_p3": ("CKKS", [40, 35, 35, 35, 35], [40, 41, 40], 0),
    "bfv": ("BFV", [36, 36, 36], [37], 65537),
    "bfv_p2": ("BFV", [36, 36, 36], [37, 37], 65537),
}
LONG = ("CKKS", [60, 40, 40, 40, 40, 40, 40, 40], [60], 0)
OPS = range(25)  # 0 and 24 are no rows: they stay 0
BATCHES = (1, 3)
LINEAR_SHAPES = ((1, 1), (3, 7), (8, 2), (16, 16))
# (n1, n2) of the factor list of test_cabi_encoding_transform.py; the size depends on nothing else of a factor
FACTORS = [(0, 1, [[0] * 3] * 7, [None] * 3, [0] * 3, [None] * 7, [0] * 7),
           (0, 1, [[0] * 8] * 2, [None] * 8, [0] * 8, [None] * 2, [0] * 2)]


def make_context(hg, spec):
    scheme, log_q, log_p, t = spec
    return hg.Context.from_bit_sizes(getattr(hg, scheme), N, log_q, log_p, plain_modulus=t, sec=hg.SEC_NONE)


def poly_plans(hg, c):
    """name -> (plan, depth) for the plans the context has the levels for"""
    primes = [int(v) for v in c.table("modulus")][:c.Q_size]
    scale = float(primes[1])
    plans = {}
    if c.Q_size >= 5:
        coeffs = [(-1.0) ** i / (i + 1) for i in range(8)]
        plans["monomial7"] = hg.poly_eval_plan(hg.MONOMIAL, coeffs, c.Q_size - 1, scale, scale, primes)
    if c.Q_size >= 8:
        coeffs = [(-1.0) ** i / (i + 1) for i in range(32)]
        plans["chebyshev31"] = hg.poly_eval_plan(hg.CHEBYSHEV, coeffs, c.Q_size - 1, scale, scale, primes)
    return plans


def build_table(hg):
    table = {}
    for name, spec in CONTEXTS.items():
        c = make_context(hg, spec)
        for depth in range(c.Q_size):
            for batch in BATCHES:
                for op in OPS:
                    table[f"{name}/op{op}/d{depth}/b{batch}"] = c.workspace_bytes(op, depth, batch)
                if spec[0] != "CKKS":
                    continue
                for n1, n2 in LINEAR_SHAPES:
                    table[f"{name}/linear{n1}x{n2}/d{depth}/b{batch}"] = c.linear_transform_workspace_bytes(n1, n2, depth, batch)
                table[f"{name}/encoding/d{depth}/b{batch}"] = c.encoding_transform_workspace_bytes(FACTORS, depth, batch)
    for name, spec in (("ckks_p2", CONTEXTS["ckks_p2"]), ("ckks_long", LONG)):
        c = make_context(hg, spec)
        for plan_name, plan in poly_plans(hg, c).items():
            for batch in BATCHES:
                table[f"{name}/poly_{plan_name}/d0/b{batch}"] = c.poly_eval_workspace_bytes(plan, 0, batch)
    return table


def test_every_reported_size_is_the_recorded_one(hg):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = build_table(hg)
    assert sorted(got) == sorted(want), "the table's rows changed: regenerate only when a row is added on purpose"
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, f"(reported, recorded) differ: {wrong}"


def test_the_table_covers_what_it_should(hg):
    with open(GOLDEN) as f:
        want = json.load(f)
    for name in CONTEXTS:
        assert want[f"{name}/op0/d0/b1"] == 0 and want[f"{name}/op24/d0/b1"] == 0, "unknown op ids report 0"
    # every real row but the share of the refresh (sampled in place: 0 bytes) needs a workspace somewhere
    for op in range(1, 24):
        if op != 20:
            assert any(want[f"{name}/op{op}/d0/b1"] > 0 for name in CONTEXTS), op
    assert want["ckks_p2/poly_monomial7/d0/b1"] > 0 and want["ckks_long/poly_chebyshev31/d0/b3"] > 0
    assert want["ckks/linear3x7/d1/b3"] > 0 and want["ckks_p3/encoding/d0/b1"] > 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import heongpu_amd

    with open(GOLDEN, "w") as out:
        json.dump(build_table(heongpu_amd), out, indent=0, sort_keys=True)
        out.write("\n")
    print("wrote", GOLDEN)
