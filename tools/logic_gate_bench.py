"""Times the CKKS logic gates on two ciphertexts: the fused entry hegpu_ckks_logic_gate against the chain of single entries
that exists without it (multiply, relinearize, rescale, mod-drop copies, hegpu_addition, hegpu_ckks_constant_op per item),
and the one pass hegpu_ckks_gate_combine against the part of that chain after the product.  Two shapes: N = 2^16 with 16
limbs and batch 64, and N = 2^12 with 4 limbs and batch 1.  It asserts nothing about times; it does check that both ways
give the same words.

    python tools/logic_gate_bench.py [--iters 10]

Every shape runs in a child process of its own under `timeout -k 10`; the first child that fails, faults or runs out of time
ends the run, nothing is started after it.  Per gate the fused and the chained form alternate inside one timed loop; each call
is bracketed by events on the stream and the median is reported.  Next to the combine's time: the words it must move
(a, b and the product read, out written: 4 ciphertexts of [2][l - 1][N]; AND / NAND, which read only the product: 2; NOT: 2
of [2][l][N]) and the time that takes at the
copy rate of profiles/r6_final/copy_bw.txt."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RW_TBPS = 5.31  # profiles/r6_final/copy_bw.txt
SHAPES = {"large": (1 << 16, 16, 64, 900), "small": (1 << 12, 4, 1, 300)}  # N, limbs, batch, time limit of the child (s)
GATES = {"AND": (0, 0, 1), "OR": (0, 1, -1), "XOR": (0, 1, -2), "NAND": (1, 0, -1), "NOR": (1, -1, 1), "XNOR": (1, -1, 2),
         "NOT": (1, -1, 0)}


def run_shape(name, iters):
    import torch
    import heongpu_amd as hg
    n, Q, batch, _ = SHAPES[name]
    c = hg.Context.from_bit_sizes(hg.CKKS, n, [60] + [50] * (Q - 1), [60], sec=hg.SEC_NONE)
    c.upload()
    g = torch.Generator(device="cuda").manual_seed(1)
    l = Q
    w, wl, w3 = 2 * l * n, 2 * (l - 1) * n, 3 * l * n
    scale = 2.0 ** 50

    def rand(count):  # canonical residues of every modulus of the chain
        return torch.randint(0, 1 << 40, (count,), dtype=torch.int64, device="cuda", generator=g)

    def empty(count):
        return torch.empty(count, dtype=torch.int64, device="cuda")

    a, b = rand(batch * w), rand(batch * w)
    key = rand(c.switch_key_digits() * 2 * c.Q_prime_size * n)
    ws = c.workspace(hg.OP_CKKS_LOGIC_GATE, 0, batch)
    relin_ws, resc_ws = c.workspace(hg.OP_CKKS_RELIN, 0, batch), c.workspace(hg.OP_CKKS_RESCALE, 0, batch)
    prod, out_f, out_c = empty(batch * w3), empty(batch * w), empty(batch * w)
    a_low, s_low, p_low = empty(batch * wl), empty(batch * wl), empty(batch * wl)

    def product():
        c.ckks_multiply(a, w, b, w, prod, w3, 0, batch)
        c.ckks_relinearize_inplace(prod, w3, key, 0, batch, relin_ws)
        c.ckks_rescale_inplace(prod, w3, 0, batch, resc_ws)

    def drop(dst, src):  # mod_drop of an input: the first l - 1 limbs of both parts, one strided copy
        dst.view(batch, 2, l - 1, n).copy_(src.view(batch, 2, l, n)[:, :, :l - 1])

    def take_product(dst):  # the rescaled product out of its three-part buffer
        dst.view(batch, wl).copy_(prod.view(batch, w3)[:, :wl])

    def chain_tail(gate):
        """the part after the product with single entries, into out_c"""
        c0, c1, c2 = GATES[gate]
        if gate == "NOT":
            c.addition(a, a, out_c, l, 2, batch, op=2)
            for i in range(batch):
                c.ckks_constant_op(0, out_c[i * w:], scale, l, 2, out=out_c[i * w:])
            return
        r = out_c[:batch * wl]
        take_product(p_low)
        if abs(c2) == 2:
            c.addition(p_low, p_low, p_low, l - 1, 2, batch)
        if c1:
            drop(a_low, a)
            drop(s_low, b)
            c.addition(a_low, s_low, s_low, l - 1, 2, batch)
            if c1 < 0:
                c.addition(s_low, s_low, s_low, l - 1, 2, batch, op=2)
            c.addition(s_low, p_low, r, l - 1, 2, batch, op=0 if c2 > 0 else 1)
        elif c2 < 0:
            c.addition(p_low, p_low, r, l - 1, 2, batch, op=2)
        else:
            r.copy_(p_low)
        if c0:
            for i in range(batch):
                c.ckks_constant_op(0, r[i * wl:], scale, l - 1, 2, out=r[i * wl:])

    def combine(gate):
        unary = gate == "NOT"
        c.ckks_gate_combine(getattr(hg, "LOGIC_" + gate), a, w, l, None if unary else b, 0 if unary else 1, 0 if unary else w,
                            0 if unary else l, None if unary else prod, 0 if unary else w3, 0 if unary else l - 1, scale, out_f,
                            w if unary else wl, l if unary else l - 1, batch=batch)

    def fused(gate):
        unary = gate == "NOT"
        c.ckks_logic_gate(getattr(hg, "LOGIC_" + gate), a, w, None if unary else b, 0 if unary else 1, 0 if unary else w,
                          None if unary else key, scale, out_f, w if unary else wl, 0, batch, None if unary else ws)

    def chain(gate):
        if gate != "NOT":
            product()
        chain_tail(gate)

    def timed_pair(f0, f1):
        for _ in range(2):
            f0()
            f1()
        ms = ([], [])
        for _ in range(iters):
            for k, fn in enumerate((f0, f1)):  # alternating: both see the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [{"median": sorted(m)[len(m) // 2], "min": min(m), "max": max(m)} for m in ms]

    res = {"shape": {"name": name, "n": n, "limbs": l, "batch": batch}, "gates": {}}
    for gate in GATES:
        words = batch * (w if gate == "NOT" else wl)
        fused(gate)
        got = out_f[:words].clone()
        chain(gate)
        torch.cuda.synchronize()
        same = bool(torch.equal(got, out_c[:words]))
        whole = timed_pair(lambda: fused(gate), lambda: chain(gate))
        if gate != "NOT":
            product()  # the tails below read the rescaled product in `prod`
        tail = timed_pair(lambda: combine(gate), lambda: chain_tail(gate))
        passes = 4 if GATES[gate][1] and GATES[gate][2] else 2  # AND / NAND read only the product, NOT only a
        moved = passes * words * 8
        res["gates"][gate] = {"same_words": same, "fused_gate_ms": whole[0], "chain_gate_ms": whole[1],
                              "combine_ms": tail[0], "chain_tail_ms": tail[1], "combine_bytes": moved,
                              "combine_min_ms_at_copy_rate": moved / (COPY_RW_TBPS * 1e9)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", choices=sorted(SHAPES), help="run this shape in this process (what the children do)")
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.iters)
        return 0
    for name in ("small", "large"):
        limit = SHAPES[name][3]
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", name,
                            "--iters", str(a.iters)])
        if r.returncode != 0:
            print(f"shape {name}: exit status {r.returncode}; nothing further is started", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
