"""TEST INFRASTRUCTURE: the INSTRUMENTED build (see run_audit.py) through the mod-down tail of the fused key switch at its
extremes (tests/tail_inputs.py): relinearize and two rotations with config C4's chain and 16 digits, the fused large-launch
path forced at N = 2^14 so that the CPU oracle checks every output.  Writes per workload what the device recorded and
whether the outputs equal the oracle's.

Usage (GPU box, HEGPU_AUDIT_LIB = tests/audit/lib/libhegpu_audit.so in the environment -- tests/test_gpu_fp_tail.py sets
it for the child process it starts):  python tests/audit/run_tail_audit.py out.json"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import run_audit as ra  # noqa: E402  (binds the instrumented library; puts the repository and tests/ on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import heongpu_amd as hg  # noqa: E402
import tail_inputs as ti  # noqa: E402


def main():
    out_path = sys.argv[1]
    assert torch.cuda.is_available(), "needs a HIP device"
    n_power, depth = 14, 0
    n = 1 << n_power
    log_q, log_p = ti.C4_CHAIN
    c, o, primes = ra.ckks(n, log_q, log_p, HEGPU_FUSED_ROW_MAC=1, HEGPU_DIGIT_SPLIT=0, HEGPU_MODDOWN_IN_MAC=1)
    Q, Qp = len(log_q), len(log_q) + len(log_p)
    l = Q - depth
    key = ti.max_key(primes, Q, Qp, n)
    dkey = hg.to_device(key)
    results = {}
    ra.read_tables()  # clear

    cts = ti.cases(c, primes, l, n, 2)
    ra.read_tables()  # (the transforms that built the inputs are not the subject)
    batch = len(cts)
    d = hg.to_device(np.concatenate([x for _, x in cts]))
    c.ckks_relinearize_inplace(d, 3 * l * n, dkey, depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
    torch.cuda.synchronize()
    got = hg.to_host(d).reshape(batch, -1)
    detail = {}
    for b, (label, x) in enumerate(cts):
        want = o.ckks_relinearize(x.copy(), key, depth)
        detail[label] = bool(np.array_equal(got[b][:2 * l * n], want[:2 * l * n]))
    results["relinearize"] = dict(tables=ra.read_tables(), equal_to_oracle=all(detail.values()), detail=detail)
    print("relinearize oracle-equal:", detail, flush=True)

    cts = ti.cases(c, primes, l, n, 1)
    ra.read_tables()
    batch = len(cts)
    d = hg.to_device(np.concatenate([x for _, x in cts]))
    for steps in (1, -3):
        g = hg.steps_to_galois_elt(steps, n, 5)
        rot = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
        c.ckks_apply_galois(d, 2 * l * n, rot, 2 * l * n, dkey, g, depth, batch, c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
        torch.cuda.synchronize()
        got = hg.to_host(rot).reshape(batch, -1)
        detail = {}
        for b, (label, x) in enumerate(cts):
            detail[label] = bool(np.array_equal(got[b], o.ckks_apply_galois(x.copy(), key, g, depth)))
        results["rotate_%d" % steps] = dict(tables=ra.read_tables(), equal_to_oracle=all(detail.values()), detail=detail)
        print("rotate", steps, "oracle-equal:", detail, flush=True)

    with open(out_path, "w") as f:
        json.dump(results, f)
    bad = [k for k, v in results.items() if not v["equal_to_oracle"] or
           any(sum(t["violations"].values()) for t in v["tables"].values())]
    print("tail audit written to", out_path, "| failing:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
