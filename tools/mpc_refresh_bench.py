"""Times the two entries of the collective refresh at the bench shape (CKKS N = 2^16, 16 limbs, batch 64, k = 3 parties)
at depth 8 and depth 15 and prints, next to each time, the bytes the entry's streaming kernels must move (counted from
the layouts of include/hegpu.h) and the ratio to the copy rates of profiles/r6_final/copy_bw.txt.

    python tools/mpc_refresh_bench.py [--iters 20]

With W = batch * N * 8 bytes (one limb of every item), l = Q - depth:
  share   fused product-and-add: reads c1 (l W), the transformed noise (l + Q) W, writes the share (l + Q) W; s_i is
          (l + Q) N * 8 bytes read once per item from cache.  The sampler writes (l + Q) W and the NTT reads and writes
          (l + Q) W twice (two passes); both are reported as part of the entry's time only.
  merge   sum: reads c0 (l W) and k l W, writes l W; finish: reads Q W and k Q W, writes 2 Q W.  INTT over l limbs, the
          lift (reads l W, writes Q W) and the NTT over Q limbs are compute, not streams; the entry's time includes them.
Each timed call is bracketed by events on the stream; the median of the timed calls is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RW_TBPS, COPY_R_TBPS = 5.31, 6.40  # profiles/r6_final/copy_bw.txt


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
    g = torch.Generator(device="cuda").manual_seed(1)
    rngs = [hg.Rng(10 + i) for i in range(k)]
    sks = [c.generate_secret_key(r) for r in rngs]
    lib, st = hg._lib.load(), torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            assert fn() == 0
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

    res = {"shape": {"n": n, "limbs": Q, "batch": batch, "parties": k}}
    W = batch * n * 8
    for depth in (8, 15):
        l = Q - depth
        words = 2 * l * n
        ct = torch.randint(0, 1 << 40, (batch * words,), dtype=torch.int64, device="cuda", generator=g)
        mask_bits = min(126, 60 + 50 * (l - 1) - 8)
        crs = hg.Rng(1)
        shares = [c.mpc_ckks_refresh_share(crs, rngs[i], ct, words, sks[i], depth, mask_bits, batch) for i in range(k)]
        arr = c._share_array(shares)
        out = torch.empty(batch * 2 * Q * n, dtype=torch.int64, device="cuda")
        ws = c.workspace(hg.OP_MPC_REFRESH_MERGE, depth, batch)
        t = timed(lambda: lib.hegpu_mpc_ckks_refresh_share(c._h, crs._h, rngs[0]._h, ct.data_ptr(), words,
                                                            sks[0].data_ptr(), depth, mask_bits, shares[0].data_ptr(),
                                                            batch, None, 0, st))
        t["fused_kernel_bytes"] = (l + 2 * (l + Q)) * W
        t["fused_kernel_min_ms_at_copy_rate"] = t["fused_kernel_bytes"] / (COPY_RW_TBPS * 1e9)
        res[f"depth{depth}_share_entry_ms"] = t
        t = timed(lambda: lib.hegpu_mpc_ckks_refresh_merge(c._h, crs._h, ct.data_ptr(), words, arr, k, depth,
                                                            out.data_ptr(), 2 * Q * n, batch, ws.data_ptr(),
                                                            ws.numel() * 8, st))
        t["stream_bytes"] = ((k + 2) * l + (k + 3) * Q) * W
        t["stream_min_ms_at_read_rate"] = t["stream_bytes"] / (COPY_R_TBPS * 1e9)
        res[f"depth{depth}_merge_entry_ms"] = t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
