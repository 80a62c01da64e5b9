"""Times the modulus raise: hegpu_ckks_mod_raise (inverse transform of the two q_0 limbs, one forward transform whose
first load is the lift, one copy of limb 0) against the chain of three entries it equals bit for bit -- hegpu_ntt (inverse),
hegpu_mod_raise, hegpu_ntt (forward) of all 2 L limbs -- and hegpu_mod_raise alone, on random residues.  It prints the
bytes each must move and the time that takes at the copy rate of profiles/r6_final/copy_bw.txt.  It asserts nothing.

    python tools/mod_raise_bench.py [--iters 20] [--log-n 16] [--limbs 16] [--batch 1]

With W = batch * N * 8 bytes (one limb of every item) and L limbs of the result, per ciphertext of two parts: the kernel
alone reads 2 W and writes 2 L W; the chain moves 4 W (inverse), (2 + 2 L) W (lift) and 8 L W (forward transform in two
passes, 4 L W in one); the fused sequence moves 4 W (inverse), 4 W (copy of limb 0) and 2 W + 2 (L - 1) W + 4 (L - 1) W for
the forward transform of the L - 1 lifted limbs.  Each timed call is bracketed by events on the stream; the median is
reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RW_TBPS = 5.31  # profiles/r6_final/copy_bw.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--limbs", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, L, batch = 1 << a.log_n, a.limbs, a.batch
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (L - 1), [60], sec=hg.SEC_NONE)
    c.upload()
    g = torch.Generator(device="cuda").manual_seed(1)
    ct = torch.randint(0, 1 << 59, (batch * 2 * n,), dtype=torch.int64, device="cuda", generator=g)
    coef = torch.empty_like(ct)
    raised = torch.empty(batch * 2 * L * n, dtype=torch.int64, device="cuda")
    out = torch.empty_like(raised)
    ws = c.workspace(hg.OP_CKKS_MOD_RAISE, 0, batch)

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}

    def chain():
        c.ntt(ct, coef, True, 2 * batch, 1)
        c.mod_raise(coef, 2 * n, raised, 2 * L * n, L, 2, batch)
        c.ntt(raised, raised, False, 2 * L * batch, L)

    W = batch * n * 8
    res = {"shape": {"n": n, "limbs": L, "batch": batch}}
    c.ntt(ct, coef, True, 2 * batch, 1)
    res["mod_raise_kernel_ms"] = dict(timed(lambda: c.mod_raise(coef, 2 * n, raised, 2 * L * n, L, 2, batch)), bytes=(2 + 2 * L) * W)
    res["chain_ms"] = dict(timed(chain), bytes=(4 + 2 + 2 * L + 8 * L) * W)
    res["ckks_mod_raise_ms"] = dict(timed(lambda: c.ckks_mod_raise(ct, 2 * n, out, 2 * L * n, 0, batch, ws)),
                                    bytes=(4 + 4 + 2 + 6 * (L - 1)) * W)
    chain()
    torch.cuda.synchronize()
    res["equal"] = bool(torch.equal(out, raised))
    for k in ("mod_raise_kernel_ms", "chain_ms", "ckks_mod_raise_ms"):
        res[k]["ms_at_copy_rate"] = res[k]["bytes"] / (COPY_RW_TBPS * 1e9)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
