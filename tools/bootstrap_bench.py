"""Times one CKKS refresh (hegpu_ckks_bootstrap) and its five parts as single entries -- the pre-multiplication and the
modulus raise, the two key switches around it, CoeffToSlot, EvalMod over both halves, SlotToCoeff -- on random residues
(keys, diagonals and input: the time does not depend on the values), and checks that the entry equals the chain bit for
bit.  Degree 30, r = 3, K = 12, ratio 256, scale 2^40, three pieces each way.  It asserts nothing but that equality.

    python tools/bootstrap_bench.py [--iters 10] [--log-n 16] [--limbs 17] [--batch 1] [--no-switch-keys] [--chained]

--chained: the giant steps of every factor are chained (bootstrap_factors(chained=True)): the reduced Galois key set.

The chain {60, 50 x (limbs - 1)} | {60}; the plan spends 3 + 1 + 8 + 1 + 3 limbs and needs one left, so 17 is the
shortest chain that fits.  Each timed call is bracketed by events on the stream; the median is reported.  `bench.py`
runs none of this code."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--limbs", type=int, default=17)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--no-switch-keys", action="store_true")
    ap.add_argument("--chained", action="store_true", help="chain the giant steps of every factor")
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, Q, B, with_keys = 1 << a.log_n, a.limbs, a.batch, not a.no_switch_keys
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    plan = hg.bootstrap_plan(primes[:Q], 2.0 ** 40, Q - 1, K=12)
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda words: torch.randint(0, 1 << 48, (words,), dtype=torch.int64, device="cuda", generator=g)  # noqa: E731
    key_words = c.switch_key_digits() * 2 * c.Q_prime_size * n
    pool = [rand(key_words) for _ in range(3)]
    conj, relin, d2s, s2d = (rand(key_words) for _ in range(4))
    cts, stc, elts = c.bootstrap_factors(plan, lambda e: pool[e % 3], lambda values, scale, limbs: rand(limbs * n),
                                         chained=a.chained)
    ct = rand(B * 2 * n)
    room = 2 * (plan.out_level + 2) * n
    out, want = torch.zeros(B * room, dtype=torch.int64, device="cuda"), torch.zeros(B * room, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.bootstrap_workspace_bytes(plan, cts, stc, with_keys, B) // 8, dtype=torch.int64, device="cuda")
    sw = dict(swk_dense_to_sparse=d2s, swk_sparse_to_dense=s2d) if with_keys else {}

    rd = Q - 1 - plan.cts_level
    rs, hs, es = 2 * (plan.cts_level + 1) * n, 2 * (plan.eval_level + 1) * n, 2 * plan.eval_mod.out_limbs * n
    new = lambda words: torch.empty(words, dtype=torch.int64, device="cuda")  # noqa: E731
    scaled, sparse, raised, dense, halves, sines = new(B * 2 * n), new(B * 2 * n), new(B * rs), new(B * rs), new(2 * B * hs), new(2 * B * es)
    ws_gal = c.workspace(hg.OP_CKKS_ROTATE_HOISTED, 0, B)
    ws_raise = c.workspace(hg.OP_CKKS_MOD_RAISE, rd, B)
    ws_cts = new(c.encoding_transform_workspace_bytes(cts, rd, B) // 8)
    ws_em = new(c.poly_eval_workspace_bytes(plan.eval_mod, Q - 1 - plan.eval_level, 2 * B) // 8)
    ws_stc = new(c.encoding_transform_workspace_bytes(stc, Q - 1 - plan.stc_level, B) // 8)

    def part_raise():
        for b in range(B):
            c.ckks_constant_op(2, ct[b * 2 * n:(b + 1) * 2 * n], float(plan.k1), 1, out=scaled[b * 2 * n:(b + 1) * 2 * n])
        c.ckks_mod_raise(sparse if with_keys else scaled, 2 * n, raised, rs, rd, B, ws_raise)

    def part_switch_down():
        c.ckks_apply_galois(scaled, 2 * n, sparse, 2 * n, d2s, 1, Q - 1, B, ws_gal)

    def part_switch_up():
        c.ckks_apply_galois(raised, rs, dense, rs, s2d, 1, rd, B, ws_gal)

    def part_cts():
        c.ckks_coeff_to_slot(dense if with_keys else raised, rs, halves[:B * hs], halves[B * hs:], hs, cts, conj, rd, B, ws_cts)

    def part_eval_mod():
        c.ckks_poly_eval(halves, hs, sines, es, plan.eval_mod, relin, Q - 1 - plan.eval_level, 2 * B, ws_em)

    def part_stc():
        c.ckks_slot_to_coeff(sines[:B * es], es, sines[B * es:], es, want, room, stc, Q - 1 - plan.stc_level, B, ws_stc)

    def chain():
        for b in range(B):
            c.ckks_constant_op(2, ct[b * 2 * n:(b + 1) * 2 * n], float(plan.k1), 1, out=scaled[b * 2 * n:(b + 1) * 2 * n])
        if with_keys:
            part_switch_down()
        c.ckks_mod_raise(sparse if with_keys else scaled, 2 * n, raised, rs, rd, B, ws_raise)
        if with_keys:
            part_switch_up()
        part_cts()
        part_eval_mod()
        part_stc()

    def entry():
        c.ckks_bootstrap(ct, 2 * n, out, room, plan, cts, stc, conj, relin, B, ws, **sw)

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

    chain()  # every part's input is in place from here on
    entry()
    torch.cuda.synchronize()
    ow = 2 * (plan.out_level + 1) * n
    equal = bool(torch.equal(out.view(B, room)[:, :ow], want.view(B, room)[:, :ow]))
    res = {"shape": {"n": n, "limbs": Q, "batch": B, "switch_keys": with_keys, "k1": plan.k1,
                     "diagonals": [f[1] for f in cts + stc], "n1_n2": [(len(f[4]), len(f[6])) for f in cts + stc],
                     "giant_steps": "chained" if a.chained else "direct", "galois_keys": len(elts),
                     "galois_key_bytes": len(elts) * key_words * 8, "eval_mod_steps": len(plan.eval_mod.steps)},
           "equal": equal,
           "bootstrap_ms": timed(entry), "chain_ms": timed(chain), "multiply_and_raise_ms": timed(part_raise)}
    if with_keys:
        res["switch_to_sparse_ms"], res["switch_to_dense_ms"] = timed(part_switch_down), timed(part_switch_up)
    res["coeff_to_slot_ms"], res["eval_mod_ms"], res["slot_to_coeff_ms"] = timed(part_cts), timed(part_eval_mod), timed(part_stc)
    print(json.dumps(res))
    assert equal, "the entry and the chain of single entries differ"


if __name__ == "__main__":
    main()
