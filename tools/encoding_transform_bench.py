"""Times CoeffToSlot and SlotToCoeff at N = 2^16, 16 limbs, three pieces (hegpu_ckks_coeff_to_slot from depth 0,
hegpu_ckks_slot_to_coeff from depth 4; the plans of the real factorisation, random residues for data, diagonals and
keys), and the two passes at the real / imaginary boundary (hegpu_ckks_conj_split, hegpu_ckks_conj_merge) against their
compositions from hegpu_addition and hegpu_ckks_mult_i on the same inputs.  Next to the passes it prints the bytes they
must move and the time that takes at the copy rate of profiles/r6_final/copy_bw.txt.  It asserts nothing.

    python tools/encoding_transform_bench.py [--iters 10] [--batch 8] [--chained] [--pieces 3]

--chained: the factors' giant steps are chained (giant_step_chain; hegpu_linear_factor.giant_parent).  The line also
carries the distinct rotation keys of the mode and their bytes.

With W = batch * N * 8 bytes (one limb of every item) and l limbs: the split reads 4 l W and writes 4 l W; its composition
moves 4 + 2 (addition), 4 + 2 (subtraction) and 2 + 2 (mult_i) l W.  The merge reads 4 l W and writes 2 l W; its
composition moves 2 + 2 (mult_i) and 4 + 2 (addition) l W.  Each timed call is bracketed by events on the stream; the
median is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RW_TBPS = 5.31  # profiles/r6_final/copy_bw.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="items of the boundary passes")
    ap.add_argument("--seq-batch", type=int, default=1, help="items of the two sequences")
    ap.add_argument("--chained", action="store_true", help="chain the giant steps of every factor")
    ap.add_argument("--pieces", type=int, default=3)
    ap.add_argument("--only-sequences", action="store_true", help="skip the boundary passes")
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, Q, pieces = 1 << 16, 16, a.pieces
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    c.upload()
    g = torch.Generator(device="cuda").manual_seed(1)

    def rand(count):  # canonical residues of every modulus of the chain
        return torch.randint(0, 1 << 40, (count,), dtype=torch.int64, device="cuda", generator=g)

    def timed(fn):
        for _ in range(2):
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

    key_words = c.switch_key_digits() * 2 * c.Q_prime_size * n
    keys = {}

    def key(shift):
        if not shift:
            return None
        if shift not in keys:
            keys[shift] = rand(key_words)
        return keys[shift]

    def factors(inverse, first_depth):
        out, shape = [], []
        for f, grp in enumerate(hg.encoding_transform_factors(n, inverse, pieces)):
            plan = hg.linear_transform_plan(grp.offsets, n // 2, stride=grp.stride)
            l = Q - (first_depth + f)
            chain = hg.giant_step_chain(plan.giant_shifts, n // 2)
            giant = chain.link_shifts if a.chained else plan.giant_shifts
            out.append((rand(len(grp.offsets) * l * n), len(grp.offsets), plan.index, [key(s) for s in plan.baby_shifts],
                        [hg.steps_to_galois_elt(s, n, 5) if s else 0 for s in plan.baby_shifts],
                        [key(s) for s in giant], [hg.steps_to_galois_elt(s, n, 5) if s else 0 for s in giant])
                       + ((chain.parent,) if a.chained else ()))
            shape.append({"stages": grp.stages, "stride": grp.stride, "diagonals": len(grp.offsets), "n1": plan.n1, "n2": plan.n2})
        return out, shape

    res = {"shape": {"n": n, "limbs": Q, "pieces": pieces, "batch_sequences": a.seq_batch, "batch_passes": a.batch}}
    sb = a.seq_batch
    conj = rand(key_words)
    ctos, res["coeff_to_slot_factors"] = factors(True, 0)
    stoc, res["slot_to_coeff_factors"] = factors(False, pieces + 2)
    res["giant_steps"] = "chained" if a.chained else "direct"
    res["rotation_keys"] = {"count": len(keys), "bytes": len(keys) * key_words * 8}
    words0 = 2 * Q * n
    ct = rand(sb * words0)
    ow = 2 * (Q - pieces - 1) * n
    out0, out1 = torch.empty(sb * ow, dtype=torch.int64, device="cuda"), torch.empty(sb * ow, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(ctos, 0, sb) // 8, dtype=torch.int64, device="cuda")
    res["coeff_to_slot_ms"] = timed(lambda: c.ckks_coeff_to_slot(ct, words0, out0, out1, ow, ctos, conj, 0, sb, ws))
    del ws
    room = 2 * (Q - 2 * pieces - 1) * n
    back = torch.empty(sb * room, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(stoc, pieces + 1, sb) // 8, dtype=torch.int64,
                     device="cuda")
    res["slot_to_coeff_ms"] = timed(lambda: c.ckks_slot_to_coeff(out0, ow, out1, ow, back, room, stoc, pieces + 1, sb, ws))
    del ws, keys
    if a.only_sequences:
        print(json.dumps(res))
        return

    # the boundary passes at the depth CoeffToSlot reaches them (3) and SlotToCoeff starts (4), one limb dropped
    batch = a.batch
    for name, depth in (("conj_split", pieces), ("conj_merge", pieces + 1)):
        l, lo = Q - depth, Q - depth - 1
        wi, wo = 2 * l * n, 2 * lo * n
        x, y = rand(batch * wi), rand(batch * wi)
        o0, o1 = torch.empty(batch * wo, dtype=torch.int64, device="cuda"), torch.empty(batch * wo, dtype=torch.int64, device="cuda")
        # the composition works on ciphertexts of the kept limbs only (what a mod_drop would leave), packed
        xk, yk = rand(batch * wo), rand(batch * wo)
        t0, t1 = torch.empty_like(xk), torch.empty_like(xk)
        W = batch * n * 8
        if name == "conj_split":
            t = timed(lambda: c.ckks_conj_split(x, wi, y, wi, o0, o1, wo, depth, depth + 1, batch))
            t["bytes"] = 8 * lo * W

            def comp():
                c.addition(xk, yk, t0, lo, 2, batch, op=0)
                c.addition(xk, yk, t1, lo, 2, batch, op=1)
                for b in range(batch):  # mult_i takes one ciphertext
                    c.ckks_mult_i(t1[b * wo:(b + 1) * wo], lo, 2, divide=True, out=o1[b * wo:(b + 1) * wo])
            tc = timed(comp)
            tc["bytes"] = 16 * lo * W
        else:
            t = timed(lambda: c.ckks_conj_merge(x, wi, y, wi, o0, wo, depth, depth + 1, batch))
            t["bytes"] = 6 * lo * W

            def comp():
                for b in range(batch):
                    c.ckks_mult_i(yk[b * wo:(b + 1) * wo], lo, 2, divide=False, out=t1[b * wo:(b + 1) * wo])
                c.addition(xk, t1, t0, lo, 2, batch, op=0)
            tc = timed(comp)
            tc["bytes"] = 10 * lo * W
        for d in (t, tc):
            d["ms_at_copy_rate"] = d["bytes"] / (COPY_RW_TBPS * 1e9)
        res[name + "_ms"] = t
        res[name + "_composition_ms"] = tc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
