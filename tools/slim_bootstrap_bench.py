"""Times one slim-family refresh (hegpu_ckks_slim_bootstrap) and its parts as single entries -- SlotToCoeff on the four
limbs at the bottom of the chain, the modulus raise, CoeffToSlot with the conjugation and the real part, the one
polynomial -- on random residues (keys, diagonals and input: the time does not depend on the values), and checks that
the entry equals the chain bit for bit.  Degree 30, r = 3, K = 12, scale 2^40, three pieces each way.  It asserts nothing
but that equality; no time is a target.

    python tools/slim_bootstrap_bench.py [--iters 10] [--log-n 16] [--limbs 17] [--batch 1] [--function slim|bit|and|...]
    python tools/slim_bootstrap_bench.py --regular [...]     hegpu_ckks_bootstrap (no switch keys) on the same chain and batch

The chain {60, 50 x (limbs - 1)} | {60} of tools/bootstrap_bench.py; the slim plan spends 3 + 1 + 8 limbs from the top and
3 at the bottom.  Each timed call is bracketed by events on the stream; the median is reported.  The two forms are two
runs, so that each can sit under a time limit of its own:

    timeout -k 10 300 python tools/slim_bootstrap_bench.py && timeout -k 10 300 python tools/slim_bootstrap_bench.py --regular

`bench.py` runs none of this code."""
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
    ap.add_argument("--function", default="slim")
    ap.add_argument("--regular", action="store_true")
    a = ap.parse_args()
    import torch
    import heongpu_amd as hg
    n, Q, B = 1 << a.log_n, a.limbs, a.batch
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda words: torch.randint(0, 1 << 48, (words,), dtype=torch.int64, device="cuda", generator=g)  # noqa: E731
    new = lambda words: torch.empty(max(words, 1), dtype=torch.int64, device="cuda")  # noqa: E731
    key_words = c.switch_key_digits() * 2 * c.Q_prime_size * n
    pool = [rand(key_words) for _ in range(3)]
    conj, relin = rand(key_words), rand(key_words)

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

    if a.regular:
        plan = hg.bootstrap_plan(primes[:Q], 2.0 ** 40, Q - 1, K=12)
        cts, stc, elts = c.bootstrap_factors(plan, lambda e: pool[e % 3], lambda values, scale, limbs: rand(limbs * n))
        ct = rand(B * 2 * n)
        room = 2 * (plan.out_level + 2) * n
        out = torch.zeros(B * room, dtype=torch.int64, device="cuda")
        ws = new(c.bootstrap_workspace_bytes(plan, cts, stc, False, B) // 8)
        res = {"shape": {"n": n, "limbs": Q, "batch": B, "switch_keys": False, "out_level": plan.out_level},
               "regular_bootstrap_ms": timed(lambda: c.ckks_bootstrap(ct, 2 * n, out, room, plan, cts, stc, conj, relin, B, ws))}
        print(json.dumps(res))
        return

    plan = hg.slim_bootstrap_plan(primes[:Q], 2.0 ** 40, Q - 1, a.function)
    cts, stc, elts = c.slim_bootstrap_factors(plan, lambda e: pool[e % 3], lambda values, scale, limbs: rand(limbs * n))
    gate = plan.ratio == 3.0
    words = 2 * (plan.in_level + 1) * n
    ct, ct2 = rand(B * words), (rand(B * words) if gate else None)
    trig = plan.trig
    es = 2 * trig.out_limbs * n
    out, want = torch.zeros(B * es, dtype=torch.int64, device="cuda"), torch.zeros(B * es, dtype=torch.int64, device="cuda")
    ws = new(c.slim_bootstrap_workspace_bytes(plan, cts, stc, B) // 8)

    in_depth, rd = Q - 1 - plan.in_level, Q - 1 - plan.cts_level
    rs, hs = 2 * (plan.cts_level + 1) * n, 2 * (plan.eval_level + 1) * n
    summed, raised, real = new(B * words), new(B * rs), new(B * hs)
    ws_raise = c.workspace(hg.OP_CKKS_MOD_RAISE, rd, B)
    ws_poly = new(c.poly_eval_workspace_bytes(trig, Q - 1 - plan.eval_level, B) // 8)

    def transforms(cur, stride, factors, depth):
        """per factor hegpu_ckks_linear_transform + hegpu_ckks_rescale_inplace, every product in a buffer of its own"""
        for k, (diags, n_diag, index, bk, be, gk, ge) in enumerate(factors):
            d = depth + k
            if (id(factors), k) not in transforms.buffers:  # allocated on the first pass, outside every timed call
                transforms.buffers[(id(factors), k)] = (
                    new(B * 2 * (Q - d) * n), new(c.linear_transform_workspace_bytes(len(be), len(ge), d, B) // 8),
                    c.workspace(hg.OP_CKKS_RESCALE, d, B))
            buf = transforms.buffers[(id(factors), k)]
            c.ckks_linear_transform(cur, stride, buf[0], 2 * (Q - d) * n, diags, n_diag, index, bk, be, gk, ge, d, B, buf[1])
            c.ckks_rescale_inplace(buf[0], 2 * (Q - d) * n, d, B, buf[2])
            cur, stride = buf[0], 2 * (Q - d) * n
        return cur, stride
    transforms.buffers = {}
    state = {}

    def part_stc():
        cur = ct
        if gate:
            for b in range(B):
                c.addition(ct[b * words:(b + 1) * words], ct2[b * words:(b + 1) * words], summed[b * words:(b + 1) * words],
                           plan.in_level + 1, 2, 1, op=0)
            cur = summed
        state["bottom"] = transforms(cur, words, stc, in_depth)

    def part_raise():
        c.ckks_mod_raise(state["bottom"][0], state["bottom"][1], raised, rs, rd, B, ws_raise)

    d = rd + plan.cts_pieces
    conj_buf = new(B * 2 * (Q - d + 1) * n)
    ws_gal = c.workspace(hg.OP_CKKS_GALOIS, d, B)

    def part_cts():
        cur, stride = transforms(raised, rs, cts, rd)
        c.ckks_apply_galois(cur, stride, conj_buf, stride, conj, 2 * n - 1, d, B, ws_gal)
        c.ckks_conj_real(cur, stride, conj_buf, stride, real, hs, d, d + 1, B)

    def part_poly():
        c.ckks_poly_eval(real, hs, want, es, trig, relin, Q - 1 - plan.eval_level, B, ws_poly)

    def chain():
        part_stc()
        part_raise()
        part_cts()
        part_poly()

    def entry():
        c.ckks_slim_bootstrap(ct, words, out, es, plan, cts, stc, conj, relin, B, ws, ct2=ct2, cs2=words)

    chain()  # every part's input is in place from here on
    entry()
    torch.cuda.synchronize()
    ow = 2 * (plan.out_level + 1) * n
    equal = bool(torch.equal(out.view(B, es)[:, :ow], want.view(B, es)[:, :ow]))
    res = {"shape": {"n": n, "limbs": Q, "batch": B, "function": a.function, "ratio": plan.ratio, "in_level": plan.in_level,
                     "out_level": plan.out_level, "diagonals": [f[1] for f in stc + cts],
                     "n1_n2": [(len(f[4]), len(f[6])) for f in stc + cts], "galois_keys": len(elts),
                     "poly_steps": len(trig.steps)},
           "equal": equal,
           "slim_bootstrap_ms": timed(entry), "chain_ms": timed(chain), "slot_to_coeff_ms": timed(part_stc),
           "raise_ms": timed(part_raise), "coeff_to_slot_conj_real_ms": timed(part_cts), "polynomial_ms": timed(part_poly)}
    print(json.dumps(res))
    assert equal, "the entry and the chain of single entries differ"


if __name__ == "__main__":
    main()
