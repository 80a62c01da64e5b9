"""Times the two launches-that-matter of collective decryption at the bench shape (CKKS N = 2^16, 16 limbs, batch 64,
k = 3 parties) and prints the bytes each must move and the resulting rate.

    python tools/mpc_decrypt_bench.py [--iters 20]

decrypt_share is timed as the whole entry a party pays for: the Gaussian sampler, its NTT and the fused
product-and-add; the bytes printed next to it are those of the fused kernel alone (read c1, s_i and the transformed
error, write h_i), so its rate is a lower bound of that kernel's.  decrypt_merge is one launch: it reads c0 and k shares
and writes m.  Each timed call is bracketed by events on the stream; the median of the timed calls is reported
(the working set, > 2 GiB, exceeds every cache, so calls do not warm each other)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--parties", type=int, default=3)
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, Q, k, batch = 1 << 16, 16, a.parties, a.batch
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    c.upload()
    words = 2 * Q * n
    g = torch.Generator(device="cuda").manual_seed(1)
    ct = torch.randint(0, 1 << 40, (batch * words,), dtype=torch.int64, device="cuda", generator=g)
    rngs = [hg.Rng(10 + i) for i in range(k)]
    sks = [c.generate_secret_key(r) for r in rngs]
    shares = [c.mpc_ckks_decrypt_share(rngs[i], ct, words, sks[i], 0, batch) for i in range(k)]

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
        return ms[len(ms) // 2], ms[0], ms[-1]

    lib, st = hg._lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.empty(batch * Q * n, dtype=torch.int64, device="cuda")
    arr = c._share_array(shares)
    poly = batch * Q * n * 8
    res = {"shape": {"n": n, "limbs": Q, "batch": batch, "parties": k}}
    t = timed(lambda: lib.hegpu_mpc_ckks_decrypt_share(c._h, rngs[0]._h, ct.data_ptr(), words, sks[0].data_ptr(), 0,
                                                       out.data_ptr(), batch, st))
    res["decrypt_share_entry_ms"] = {"median": t[0], "min": t[1], "max": t[2]}
    t = timed(lambda: lib.hegpu_mpc_ckks_decrypt_merge(c._h, ct.data_ptr(), words, arr, k, 0, out.data_ptr(), batch, st))
    merge_bytes = (k + 2) * poly
    res["decrypt_merge_ms"] = {"median": t[0], "min": t[1], "max": t[2], "bytes": merge_bytes,
                               "GBps": merge_bytes / t[0] / 1e6}
    res["decrypt_share_entry_ms"]["fused_kernel_bytes"] = 3 * poly + Q * n * 8
    print(json.dumps(res))


if __name__ == "__main__":
    main()
