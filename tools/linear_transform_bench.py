"""Times the plaintext matrix x encrypted vector transform at N = 2^16, 16 limbs, batch 8, 32 diagonals (n1 = 8 baby
steps, n2 = 4 giant steps): the fused entry hegpu_ckks_linear_transform against the composition of the existing
entries on the same inputs (rotate_hoisted, cipherplain_multiplication + addition per diagonal and item, apply_galois
per giant step, addition), and the one-pass kernel hegpu_ckks_diag_mac against the multiply + add part of that
composition alone.  Next to the kernel's time it prints the bytes the kernel must move and the ratio to the copy rates
of profiles/r6_final/copy_bw.txt.  It asserts nothing.

    python tools/linear_transform_bench.py [--iters 10] [--chained] [--diagonals 32] [--period 8]

--chained: the fused entry runs with chained giant steps (hegpu_ckks_linear_transform_chained over giant_step_chain);
the composition stays the direct one.  The line also carries the distinct rotation keys of the mode and their bytes.

With W = batch * N * 8 bytes (one limb of every item), l = 16: the kernel reads the n1 rotated ciphertexts (2 l W each)
and writes the n2 inner sums (2 l W each); the diagonals are l N * 8 bytes each, shared by the items: read from HBM at
least once (diag_bytes_once) and at most once per item.  The composition moves 3 l W + 2 l W for every product and
4 l W + 2 l W for every addition.  Each timed call is bracketed by events on the stream; the median is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RW_TBPS, COPY_R_TBPS = 5.31, 6.40  # profiles/r6_final/copy_bw.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--chained", action="store_true", help="chain the giant steps of the fused entry")
    ap.add_argument("--diagonals", type=int, default=32)
    ap.add_argument("--period", type=int, default=8)
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, Q, batch, n_diag, period = 1 << 16, 16, a.batch, a.diagonals, a.period
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    c.upload()
    g = torch.Generator(device="cuda").manual_seed(1)
    lib, st = hg._lib.load(), torch.cuda.current_stream().cuda_stream
    plan = hg.linear_transform_plan(range(n_diag), n // 2, period)
    n1, n2, l = plan.n1, plan.n2, Q
    words = 2 * l * n

    def rand(count):  # canonical residues of every modulus of the chain
        return torch.randint(0, 1 << 40, (count,), dtype=torch.int64, device="cuda", generator=g)

    ct, diags = rand(batch * words), rand(n_diag * l * n).reshape(n_diag, l * n)
    key_words = c.switch_key_digits() * 2 * c.Q_prime_size * n
    chain = hg.giant_step_chain(plan.giant_shifts, n // 2)
    keys = {s: rand(key_words) for s in set(plan.baby_shifts + plan.giant_shifts + chain.link_shifts) if s}
    belts = [hg.steps_to_galois_elt(s, n, 5) if s else 0 for s in plan.baby_shifts]
    gelts = [hg.steps_to_galois_elt(s, n, 5) if s else 0 for s in plan.giant_shifts]
    bkeys, gkeys = [keys.get(s) for s in plan.baby_shifts], [keys.get(s) for s in plan.giant_shifts]
    lelts = [hg.steps_to_galois_elt(s, n, 5) if s else 0 for s in chain.link_shifts]
    lkeys = [keys.get(s) for s in chain.link_shifts]
    out = torch.empty(batch * words, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(n1, n2, 0, batch) // 8, dtype=torch.int64, device="cuda")
    rot = torch.empty(batch * n1 * words, dtype=torch.int64, device="cuda")
    inner = torch.empty(batch * n2 * words, dtype=torch.int64, device="cuda")
    kws = c.workspace(hg.OP_CKKS_ROTATE_HOISTED, 0, batch)
    prod, turned = torch.empty(batch * words, dtype=torch.int64, device="cuda"), torch.empty(batch * words, dtype=torch.int64, device="cuda")
    sums = [torch.empty(batch * words, dtype=torch.int64, device="cuda") for _ in range(n2)]

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

    def fused():
        if a.chained:
            c.ckks_linear_transform(ct, words, out, words, diags, n_diag, plan.index, bkeys, belts, lkeys, lelts, 0, batch, ws,
                                    giant_parent=chain.parent)
        else:
            c.ckks_linear_transform(ct, words, out, words, diags, n_diag, plan.index, bkeys, belts, gkeys, gelts, 0, batch, ws)

    def hoisted():
        c.ckks_rotate_hoisted(ct, words, rot, n1 * words, bkeys, belts, 0, batch, kws)

    def mul_add():  # the composition's inner sums from the rotations in `rot`
        r = rot.reshape(batch, n1, words)
        for j, row in enumerate(plan.index):
            first = True
            for i, at in enumerate(row):
                if at < 0:
                    continue
                dst = sums[j] if first else prod
                for b in range(batch):
                    lib.hegpu_cipherplain_multiplication(c._h, r[b, i].data_ptr(), diags[at].data_ptr(),
                                                         dst.data_ptr() + b * words * 8, l, st)
                if not first:
                    c.addition(sums[j], prod, sums[j], l, 2, batch)
                first = False

    def composition():
        hoisted()
        mul_add()
        total = None
        for j in range(n2):
            term = sums[j]
            if gelts[j]:
                c.ckks_apply_galois(sums[j], words, turned, words, gkeys[j], gelts[j], 0, batch, kws)
                term = turned
            if total is None:
                total = term
            else:
                c.addition(out if total is not sums[0] else total, term, out, l, 2, batch)
                total = out

    def one_pass():
        c.ckks_diag_mac(rot, n1 * words, n1, diags, n_diag, plan.index, n2, inner, n2 * words, 0, batch)

    W = batch * n * 8
    res = {"shape": {"n": n, "limbs": l, "batch": batch, "diagonals": n_diag, "n1": n1, "n2": n2}}
    used = {s for s in plan.baby_shifts + (chain.link_shifts if a.chained else plan.giant_shifts) if s}
    res["giant_steps"] = "chained" if a.chained else "direct"
    res["rotation_keys"] = {"count": len(used), "bytes": len(used) * key_words * 8}
    res["fused_entry_ms"] = timed(fused)
    res["composition_ms"] = timed(composition)
    res["rotate_hoisted_ms"] = timed(hoisted)
    t = timed(one_pass)
    t["bytes_rot_and_out"] = (n1 + n2) * 2 * l * W
    t["diag_bytes_once"] = n_diag * l * n * 8
    t["diag_bytes_per_item"] = n_diag * l * W
    t["min_ms_at_copy_rate"] = (t["bytes_rot_and_out"] + t["diag_bytes_once"]) / (COPY_RW_TBPS * 1e9)
    t["max_stream_ms_at_copy_rate"] = (t["bytes_rot_and_out"] + t["diag_bytes_per_item"]) / (COPY_RW_TBPS * 1e9)
    res["diag_mac_kernel_ms"] = t
    t = timed(mul_add)
    t["bytes"] = (n_diag * 5 + (n_diag - n2) * 6) * l * W
    t["min_ms_at_copy_rate"] = t["bytes"] / (COPY_RW_TBPS * 1e9)
    res["multiply_add_composition_ms"] = t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
