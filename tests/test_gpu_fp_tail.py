"""The FP64 mod-down tail of the fused CKKS key switch (ntt.hip ks_tail_store_fp: (acc - T) P^-1 + ct mod q on the FP64
moduli without leaving the doubles) on extreme values: the key-switched polynomial at the patterns that give the largest
digits next to an all-(q - 1) key, so the accumulators and the transformed P limb T reach their largest magnitudes, the
added ciphertext term 0 and q - 1 (tests/tail_inputs.py).  Relinearize (in place) and rotations (through the Galois
scatter of the tail), compared

  * with the same call under moddown_in_mac = 0, which takes the integer epilogue of the row pass of its own, at config
    C4's shape (N = 2^16, eight ciphertexts: the launch the benchmark runs), bit for bit;
  * with the CPU oracle, at N = 2^16 for relinearize and one rotation, and for everything in the instrumented run;
  * in the instrumented build (tests/audit/run_tail_audit.py): no violation at any executed operation -- every fp_mul
    compared with 128-bit integer arithmetic, every value an integer below 2^53, the added term below 2^52 -- and the
    largest magnitudes recorded at the new sites inside the bounds stated next to the code:
    |fp_reduce(acc) - T| <= 5.72 q, inv < q, |t| <= 2.65 q, the sums that are re-centred <= 7.88 q.
(The bounds themselves: tests/test_fp_model_tail.py.)

The same launches run the integer limbs q_0 and P (60 bits) through ks_row_mac / ks_row_mac_moddown and the integer
column pass, whose butterflies now correct on a schedule (ntt.hip cs_sched: a modulus below 2^60 has room for 16 q, so a
correction every second stage instead of every stage).  The second half of the file checks that schedule on the plain
transforms, bit for bit against the oracle: moduli just below 2^60 (the schedule), just below 2^61 (a correction in
every stage, as before) and just above the plan's lazy_q_max (scheduled column pass, correction-free row pass),
N = 2^12 ... 2^16, through the two-pass path, inputs at the top of both entry ranges: canonical residues up to q - 1
and un-reduced values up to 8 q - 1 (what a decomposing launch may feed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tail_inputs as ti
from helpers import backend_switches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, TAIL = 30, 31  # fpmod.cuh FP_STAGE_OUT, FP_STAGE_TAIL
B_D, B_T, B_ACC = 5.72, 2.65, 7.88 * (1 + 2.0 ** -40)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def c4(hg, oracle):
    """contexts of config C4's chain with moddown_in_mac 0 and 1, the oracle, the all-(q - 1) key"""
    log_q, log_p = ti.C4_CHAIN
    n = 65536
    cs = []
    for v in (0, 1):
        with backend_switches(HEGPU_MODDOWN_IN_MAC=v):
            c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_NONE)
        assert c.get_option("moddown_in_mac") == v
        c.upload()
        cs.append(c)
    primes = [int(x) for x in cs[0].table("modulus")]
    Q, Qp = len(log_q), len(log_q) + len(log_p)
    o = oracle.OracleContext(oracle.CKKS, 16, primes, Q, len(log_p))
    key = ti.max_key(primes, Q, Qp, n)
    return dict(cs=cs, o=o, primes=primes, n=n, l=Q, key=key, dkey=hg.to_device(key))


def test_relinearize_extremes_c4_shape(hg, torch, c4):
    n, l, primes = c4["n"], c4["l"], c4["primes"]
    cts = ti.cases(c4["cs"][1], primes, l, n, 2)
    batch = len(cts)
    assert batch == 8  # the large-launch fused path at N = 2^16 (see tests/test_gpu_moddown_in_mac.py)
    got = []
    for c in c4["cs"]:
        d = hg.to_device(np.concatenate([x for _, x in cts]))
        c.ckks_relinearize_inplace(d, 3 * l * n, c4["dkey"], 0, batch, c.workspace(hg.OP_CKKS_RELIN, 0, batch))
        torch.cuda.synchronize()
        got.append(hg.to_host(d).reshape(batch, -1)[:, :2 * l * n])
    assert np.array_equal(got[0], got[1]), "FP64 tail differs from the integer epilogue"
    for b, (label, x) in enumerate(cts):
        want = c4["o"].ckks_relinearize(x.copy(), c4["key"], 0)
        assert np.array_equal(got[1][b], want[:2 * l * n]), label


def test_rotation_extremes_c4_shape(hg, torch, c4):
    n, l, primes = c4["n"], c4["l"], c4["primes"]
    cts = ti.cases(c4["cs"][1], primes, l, n, 1)
    batch = len(cts)
    d = hg.to_device(np.concatenate([x for _, x in cts]))
    for steps in (1, -3):
        g = hg.steps_to_galois_elt(steps, n, 5)
        got = []
        for c in c4["cs"]:
            rot = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
            c.ckks_apply_galois(d, 2 * l * n, rot, 2 * l * n, c4["dkey"], g, 0, batch, c.workspace(hg.OP_CKKS_GALOIS, 0, batch))
            torch.cuda.synchronize()
            got.append(hg.to_host(rot).reshape(batch, -1))
        assert np.array_equal(got[0], got[1]), ("FP64 tail differs from the integer epilogue", steps)
        if steps == 1:
            for b, (label, x) in enumerate(cts):
                assert np.array_equal(got[1][b], c4["o"].ckks_apply_galois(x.copy(), c4["key"], g, 0)), label


@pytest.fixture(scope="module")
def tail_audit(tmp_path_factory):
    lib = os.path.join(ROOT, "tests", "audit", "lib", "libhegpu_audit.so")
    assert os.path.exists(lib), "the instrumented build is missing: make -C tests/audit (done by __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("tail_audit") / "tail_audit.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "audit", "run_tail_audit.py"), out], cwd=ROOT,
                       env=dict(os.environ, HEGPU_AUDIT_LIB=lib), capture_output=True, text=True, timeout=1500)
    sys.stdout.write(p.stdout[-4000:])
    sys.stderr.write(p.stderr[-4000:])
    assert os.path.exists(out), "the audit run did not finish"
    with open(out) as f:
        return json.load(f), p.returncode


def test_instrumented_tail_exact_and_inside_its_bounds(tail_audit):
    data, rc = tail_audit
    assert set(data) == {"relinearize", "rotate_1", "rotate_-3"}
    for workload, res in data.items():
        assert res["equal_to_oracle"], (workload, res["detail"])
        t = res["tables"]["ntt"]
        assert sum(t["violations"].values()) == 0, (workload, t["violations"], t["first_violation"])
        rows = {r["stage"]: r for r in t["rows"] if r["kind"] == "ks_row" and r["sub"] == 2}
        assert TAIL in rows and OUT in rows, (workload, sorted(rows))
        tail, out = rows[TAIL], rows[OUT]
        print("%s: |fp_reduce(acc) - T| / q %.4f (<= %.2f), inv / q %.4f, |t| / q %.4f (<= %.2f), re-centred |acc| / q %.4f (<= 7.88)"
              % (workload, tail["mul_y"], B_D, tail["mul_w"], tail["mul_t"], B_T, out["red_in"]))
        assert tail["sum"] <= B_D and tail["mul_y"] <= B_D, (workload, tail)
        assert tail["mul_w"] < 1.0 and tail["mul_t"] <= B_T, (workload, tail)
        assert tail["red_in"] == 0.0, (workload, tail)          # nothing is reduced at that stage
        assert out["red_in"] <= B_ACC and out["abs"] < 1.0 and tail["abs"] < 1.0, (workload, out, tail)
        # the tail saw un-reduced operands: T alone is beyond the q / 2 of a centred residue
        assert tail["mul_y"] > 0.5, (workload, tail)
    assert rc == 0


# ------------------------------------------------------------------ correction schedule of the integer butterflies
def _is_prime(v):
    if v < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if v % p == 0:
            return v == p
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3 * 10^24
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(r - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def _ntt_prime(n, start, step):
    """the first prime = 1 (mod 2n) from `start` on, going up (step 1) or down (step -1)"""
    v = start - start % (2 * n) + 1
    if step > 0 and v < start:
        v += 2 * n
    while v > start and step < 0:
        v -= 2 * n
    while not _is_prime(v):
        v += step * 2 * n
    return v


def schedule_chain(n_power):
    """[just above lazy_q_max, just below 2^60, just below 2^61] for degree 2^n_power, and that lazy_q_max"""
    n = 1 << n_power
    p61 = _ntt_prime(n, 2 ** 61 - 1, -1)
    p60 = _ntt_prime(n, 2 ** 60 - 1, -1)
    lazy_q_max = (2 ** 64 - 1 - 2 * p61) // (4 * n_power)  # context.cpp: the largest modulus of the plan is p61
    above = _ntt_prime(n, lazy_q_max + 1, 1)
    assert lazy_q_max < above < 2 ** 59 and 2 ** 59 < p60 < 2 ** 60 < p61 < 2 ** 61
    return [above, p60, p61], lazy_q_max


def schedule_inputs(primes, n, rng):
    """[(label, [limbs][n] uint64)]: canonical residues and un-reduced values at the top of [0, q) / [0, 8q)"""
    out = []
    for top, mul in (("q", 1), ("8q", 8)):
        rows = {"top": [], "alt": [], "random_high": []}
        for q in primes:
            hi = mul * q - 1
            rows["top"].append(np.full(n, hi, dtype=np.uint64))
            v = np.zeros(n, dtype=np.uint64)
            v[::2] = hi
            rows["alt"].append(v)
            # the upper eighth of the range: every value within q / 8 (or q) of the top
            rows["random_high"].append((rng.integers(0, (mul * q) // 8, n, dtype=np.uint64) + np.uint64(hi - (mul * q) // 8 + 1)))
        for k, r in rows.items():
            out.append(("%s/%s" % (top, k), np.concatenate(r)))
    return out


@pytest.mark.parametrize("n_power", [12, 13, 14, 15, 16])
def test_correction_schedule_transforms_match_oracle(hg, oracle, torch, n_power):
    n = 1 << n_power
    primes, lazy_q_max = schedule_chain(n_power)
    with backend_switches(HEGPU_SINGLE_PASS=0):  # column pass + row pass at every degree
        c = hg.Context.from_primes(hg.CKKS, n, primes, 2, 1)
    assert [int(x) for x in c.table("modulus")] == primes
    o = oracle.OracleContext(oracle.CKKS, n_power, primes, 2, 1)
    c.upload()
    rng = np.random.default_rng(100 + n_power)
    Qp = len(primes)
    for label, x in schedule_inputs(primes, n, rng):
        canon = np.concatenate([x[j * n:(j + 1) * n] % np.uint64(primes[j]) for j in range(Qp)])
        want = o.ntt(canon.copy(), Qp, Qp)
        for batch in (1, 3):  # small and larger launches
            d = hg.to_device(np.tile(x, batch))
            c.ntt(d, d, False, batch * Qp, Qp)
            torch.cuda.synchronize()
            got = hg.to_host(d).reshape(batch, -1)
            for b in range(batch):
                for j in range(Qp):
                    assert np.array_equal(got[b][j * n:(j + 1) * n], want[j * n:(j + 1) * n]), (label, batch, b, "modulus %d" % primes[j])
