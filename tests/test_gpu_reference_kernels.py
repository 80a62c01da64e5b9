"""The RNS kernels of this project against THE REFERENCE'S OWN KERNELS, run on the same GPU on the same inputs.

oracle/_ref/libref_kernels.so holds the reference's switchkey.cu, multiplication.cu and addition.cu, compiled unchanged
(oracle/ref_build.py) and launched through oracle/ref_kernels_driver.cpp with the grids of the reference's host code.
Every case runs the same inputs through three columns

    (a) the reference kernel, item by item (the reference is un-batched)       refk_*
    (b) the project's entry, batch 2 with a padded item stride where it takes one   hegpu_*
    (c) the CPU oracle's restatement, the function the existing parity tests use    o_*

and asserts (a) == (b) and (a) == (c) over EVERY word.  The tables (half, half_mod, last_q_modinv, rescaled_*, the m2_*
and BEHZ tables, upper_halfincrement, coeff_div_plain_modulus, ...) are read from the PROJECT's context by their
reference names and handed to the reference kernel, so a wrong table is a mismatch too.  Every reference output buffer
ends in N sentinel words that must come back unchanged.  The input builders and the planted corners (0, q - 1, q / 2,
the un-reduced q of the reference's negation) are those of tests/test_gpu_kernels.py.

What this pins: index arithmetic, loop structure, operand order, table use and launch geometry of the kernels of the
three files.  What it does NOT pin: the GPU-NTT primitives under them (oracle/ref_shim/ is this project's restatement
of add / sub / mult / reduce, the same as the oracle's) and the NTT.  Inside the Barrett domain (a * b < 2^(2 bit)) the
result of mult is the true product whatever the formula, so such a comparison rests on reference text alone; outside
it rests on the restated formula.  The oracle counts its out-of-domain products (o_barrett_domain_violations); every
case asserts the count around its oracle calls to be zero, except the cases listed in OUT_OF_DOMAIN.

The module skips only when the tree was built without the reference (no reference binary under oracle/_ref/ at all);
reference consumers without libref_kernels.so is a broken build and fails."""
import ctypes
import math

import numpy as np
import pytest

from helpers import synth_ct, synth_key
from oracle import ref_kernels as rk
from test_gpu_kernels import _bfv, _ckks, _limbs, _rescale_location, five_special_primes, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

if not rk.available() and not rk.reference_binaries():
    pytest.skip("built without the reference tree: no reference binaries under oracle/_ref/", allow_module_level=True)

SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 256  # words between the items of a batch on the project side (even: the kernels move two words at a time)

# the deliberately out-of-domain cases: cipher_broadcast_kernel's mult(1, x, q_i) with a 61-bit source limb
# (x up to 2^61) against 30-bit targets (domain: x < 2^60)
OUT_OF_DOMAIN = {"cipher_broadcast/q61_into_30_bit"}

TALLY = {}    # project entry -> [cases, compared words]
DOMAIN = {}   # case -> out-of-domain products the oracle counted


@pytest.fixture(scope="module", autouse=True)
def _report():
    assert rk.available(), "oracle/_ref/ holds reference consumers but no libref_kernels.so"
    rk.lib().refk_set_dry_run(0)
    yield
    print("\nreference-kernel parity: cases and compared words per entry")
    for entry in sorted(TALLY):
        print("  %-46s %3d cases %10d words" % (entry, TALLY[entry][0], TALLY[entry][1]))
    print("out-of-domain Barrett products counted by the oracle:", {k: v for k, v in DOMAIN.items() if v} or "none")


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault(torch):
    """a device fault poisons the process: end the session instead of launching the remaining cases on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001  (torch reports HIP errors as RuntimeError / AcceleratorError)
        pytest.exit("the GPU reported an error, nothing more is launched: %s" % e, returncode=3)


class Ref:
    """the reference column for one project context: device copies of its moduli and tables, guarded outputs"""

    def __init__(self, torch, hg, c):
        self.torch, self.hg, self.c = torch, hg, c
        self.n, self.n_power = c.n, c.n_power
        self._keep, self._tabs = [], {}
        self.mod = self.moduli([int(v) for v in c.table("modulus")])

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def moduli(self, values):
        primes = np.array([int(v) for v in values], dtype=np.uint64)
        staging = np.zeros(3 * len(primes), dtype=np.uint64)
        dev = self.torch.zeros(3 * len(primes), dtype=self.torch.int64, device="cuda")
        rc = rk.lib().refk_moduli_fill(primes.ctypes.data, len(primes), staging.ctypes.data, staging.size, dev.data_ptr(),
                                       len(primes), self.stream)
        assert rc == rk.OK, rc
        self.torch.cuda.synchronize()
        self._keep.append(staging)
        return dev

    def tab(self, name, offset=0):
        """the project context's host table `name` on the device, from word `offset` on"""
        if name not in self._tabs:
            self._tabs[name] = self.hg.to_device(self.c.table(name))
        return self._tabs[name][offset:]

    def scalar(self, name):
        return int(self.c.table(name)[0])

    def ints(self, values):
        return self.torch.tensor([int(v) for v in values], dtype=self.torch.int32, device="cuda")

    def out(self, words, fill=SENTINEL):
        t = self.torch.full((words + self.n,), SENTINEL, dtype=self.torch.int64, device="cuda")
        if fill != SENTINEL:
            t[:words] = fill
        return t

    def take(self, t, words):
        self.torch.cuda.synchronize()
        host = self.hg.to_host(t)
        assert host.size == words + self.n and bool(np.all(host[words:] == np.uint64(SENTINEL))), "the sentinel tail was written"
        return host[:words]

    def run(self, name, out_words, out_fill=SENTINEL, out_arg="out", **kw):
        out = self.out(out_words, out_fill)
        kw[out_arg] = out[:out_words]
        rc = rk.call(name, n_power=self.n_power, stream=self.stream, **kw)
        assert rc == rk.OK, (name, rc)
        return self.take(out, out_words)


def pack(hg, torch, items):
    """items of equal length at a padded stride; the padding holds the sentinel"""
    words = len(items[0])
    t = torch.full((len(items) * (words + PAD),), SENTINEL, dtype=torch.int64, device="cuda")
    for b, it in enumerate(items):
        t[b * (words + PAD):b * (words + PAD) + words] = hg.to_device(it)
    return t, words + PAD


def blank(torch, batch, words, fill=SENTINEL):
    t = torch.full((batch * (words + PAD),), SENTINEL, dtype=torch.int64, device="cuda")
    if fill != SENTINEL:
        t.view(batch, words + PAD)[:, :words] = fill
    return t, words + PAD


def unpack(hg, torch, t, batch, words):
    torch.cuda.synchronize()
    host = hg.to_host(t).reshape(batch, words + PAD)
    assert bool(np.all(host[:, words:] == np.uint64(SENTINEL))), "the project wrote between the items of the batch"
    return [host[b, :words] for b in range(batch)]


class domain:
    """the oracle's out-of-domain Barrett count around the oracle calls of one case"""

    def __init__(self, oracle, case):
        self.cell = ctypes.c_uint64.in_dll(oracle.lib(), "o_barrett_domain_violations")
        self.case = case

    def __enter__(self):
        self.before = int(self.cell.value)

    def __exit__(self, *exc):
        if exc[0] is None:
            seen = int(self.cell.value) - self.before
            DOMAIN[self.case] = DOMAIN.get(self.case, 0) + seen
            if self.case in OUT_OF_DOMAIN:
                assert seen > 0, "%s is listed as out of the Barrett domain and is not" % self.case
            else:
                assert seen == 0, "%s left the Barrett domain %d times" % (self.case, seen)


def same(entry, ref, got, want, what):
    """(a) == (b) and (a) == (c), every word"""
    assert ref.dtype == got.dtype == want.dtype == np.uint64 and ref.shape == got.shape == want.shape, what
    bad = np.flatnonzero(ref != got)
    assert bad.size == 0, ("reference kernel != project", what, int(bad[0]), int(ref[bad[0]]), int(got[bad[0]]), bad.size)
    bad = np.flatnonzero(ref != want)
    assert bad.size == 0, ("reference kernel != oracle", what, int(bad[0]), int(ref[bad[0]]), int(want[bad[0]]), bad.size)
    t = TALLY.setdefault(entry, [0, 0])
    t[0] += 1
    t[1] += int(ref.size)


def corners(arr, at, q):
    arr[at:at + 3] = [0, q - 1, q // 2]


CKKS_P1 = ([40, 35, 35, 35, 35], [40])
CKKS_P2 = ([40, 35, 35, 35, 35], [40, 40])


@pytest.fixture(scope="module")
def ckks_p1(hg, oracle, torch):
    c, o, primes = _ckks(hg, oracle, 4096, *CKKS_P1, sec=hg.SEC_NONE)
    return c, o, primes, Ref(torch, hg, c)


@pytest.fixture(scope="module")
def ckks_p2(hg, oracle, torch):
    c, o, primes = _ckks(hg, oracle, 4096, *CKKS_P2, sec=hg.SEC_NONE)
    return c, o, primes, Ref(torch, hg, c)


@pytest.fixture(scope="module")
def bfv_4096(hg, oracle, torch):
    c, o, primes = _bfv(hg, oracle, 4096, 1032193)
    return c, o, primes, Ref(torch, hg, c)


@pytest.fixture(scope="module")
def bfv_8192_p2(hg, oracle, torch):
    """BFV N = 2^13, default chain split 3 | 2: the method II forms of the BFV operators"""
    t = 1032193
    c = hg.Context.from_default(hg.BFV, 8192, 2, t)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, t)
    c.upload()
    return c, o, primes, Ref(torch, hg, c)


@pytest.fixture(scope="module")
def five_p(hg, oracle, torch, five_special_primes):
    c, o, primes = five_special_primes
    return c, o, primes, Ref(torch, hg, c)


# ------------------------------------------------------------------ addition.cu
@pytest.mark.parametrize("op", [0, 1, 2], ids=["addition", "substraction", "negation"])
def test_addition(hg, oracle, torch, ckks_p1, op):
    """hegpu_addition op 0 / 1 / 2 == addition / substraction / negation (addition.cu:10-48), three limbs, two parts;
    in1 holds 0, q - 1, q / 2 and the un-reduced q (sub(q, 0) == q)."""
    c, o, primes, R = ckks_p1
    n, limbs, parts, batch = c.n, 3, 2, 2
    a = [synth_ct(primes, range(limbs), parts, n, 11 + b) for b in range(batch)]
    b_ = [synth_ct(primes, range(limbs), parts, n, 31 + b) for b in range(batch)]
    for x in a:
        x[:4] = [0, primes[0] - 1, primes[0] // 2, primes[0]]
    b_[0][:4] = [0, 0, primes[0] - 1, 0]
    words = parts * limbs * n
    da, db = hg.to_device(np.concatenate(a)), hg.to_device(np.concatenate(b_))
    out = torch.full((batch * words,), SENTINEL, dtype=torch.int64, device="cuda")
    c.addition(da, None if op == 2 else db, out, limbs, parts, batch, op)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, words)
    fn = (o.L.o_addition, o.L.o_substraction, o.L.o_negation)[op]
    for b in range(batch):
        ref = R.run("refk_addition", words, op=op, in1=hg.to_device(a[b]), in2=None if op == 2 else hg.to_device(b_[b]),
                    modulus=R.mod, limbs=limbs, parts=parts)
        want = np.zeros(words, dtype=np.uint64)
        with domain(oracle, "addition"):
            if op == 2:
                fn(a[b].ctypes.data, want.ctypes.data, o.qp_mods, c.n_power, limbs, parts)
            else:
                fn(a[b].ctypes.data, b_[b].ctypes.data, want.ctypes.data, o.qp_mods, c.n_power, limbs, parts)
        same("hegpu_addition", ref, got[b], want, (op, b))


@pytest.mark.parametrize("sub", [0, 1], ids=["add", "sub"])
def test_bfv_plain_addsub(hg, oracle, torch, bfv_4096, sub):
    """hegpu_bfv_plain_addsub == addition_plain_bfv_poly / substraction_plain_bfv_poly (addition.cu:50-147) with the
    project's Q_mod_t, upper_threshold and coeff_div_plain_modulus.  The oracle has no function of its own for these two
    kernels; column (c) is the same formula in Python integers (every product is inside the Barrett domain: m < t)."""
    c, o, primes, R = bfv_4096
    n, Q, t = c.n, c.Q_size, 1032193
    ct = synth_ct(primes, range(Q), 2, n, 77)
    corners(ct, 0, primes[0])
    rng = np.random.default_rng(5)
    plain = rng.integers(0, t, n).astype(np.uint64)
    plain[:6] = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2, t // 3]
    q_mod_t, thr = R.scalar("Q_mod_t"), R.scalar("upper_threshold")
    cd = [int(v) for v in c.table("coeff_div_plain_modulus")]
    words = 2 * Q * n
    out = torch.full((words,), SENTINEL, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert c._lib.hegpu_bfv_plain_addsub(c._h, hg.to_device(ct).data_ptr(), hg.to_device(plain).data_ptr(), out.data_ptr(),
                                         sub, st) == 0
    torch.cuda.synchronize()
    ref = R.run("refk_bfv_plain_addsub", words, sub=sub, cipher=hg.to_device(ct), plain=hg.to_device(plain), modulus=R.mod,
                plain_mod=t, Q_mod_t=q_mod_t, upper_threshold=thr, coeffdiv_plain=R.tab("coeff_div_plain_modulus"),
                Q_size=Q, cipher_size=2)
    want = ct.copy()
    m = [int(v) for v in plain]
    for j in range(Q):
        q = primes[j]
        term = [(v * cd[j] + (v * q_mod_t + thr) // t) % q for v in m]
        row = [int(v) for v in ct[j * n:(j + 1) * n]]
        want[j * n:(j + 1) * n] = [((x - y) if sub else (x + y)) % q for x, y in zip(row, term)]
    same("hegpu_bfv_plain_addsub", ref, hg.to_host(out), want, sub)


CONSTANTS = [0.0, 1.0, -1.0, -0.4, -12345.678, 3.0 * 2.0 ** 70]


@pytest.mark.parametrize("op", [0, 1, 2], ids=["add", "sub", "mul"])
def test_ckks_constant_op(hg, oracle, torch, ckks_p1, op):
    """hegpu_ckks_constant_op == addition_constant_plain_ckks_poly, its substraction twin (addition.cu:219-307) and
    cipher_constant_plain_multiplication_kernel (multiplication.cu:333-372) for 0, +-1, -0.4 (rounds to a NEGATIVE zero:
    pt = sub(q, 0) = q), a negative non-integer and 3 * 2^70 (the high word of the 128-bit reduce)."""
    c, o, primes, R = ckks_p1
    n, limbs, parts = c.n, 3, 2
    ct = synth_ct(primes, range(limbs), parts, n, 5)
    corners(ct, 0, primes[0])
    words = parts * limbs * n
    d = hg.to_device(ct)
    for value in CONSTANTS:
        got = hg.to_host(c.ckks_constant_op(op, d, value, limbs, parts))
        ref = R.run("refk_ckks_constant_op", words, op=op, value=value, modulus=R.mod, limbs=limbs, parts=parts, **{"in": d})
        with domain(oracle, "ckks_constant_op"):
            want = o.ckks_constant_op(op, ct, value, limbs, parts)
        same("hegpu_ckks_constant_op", ref, got, want, (op, value))


def _round_away(v):
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


@pytest.mark.parametrize("op", [0, 1], ids=["add", "mul"])
def test_ckks_gaussian_integer_op(hg, oracle, torch, ckks_p1, op):
    """hegpu_ckks_gaussian_integer_op == cipher_add_by_gaussian_integer_kernel / cipher_mult_by_gaussian_integer_kernel
    (multiplication.cu:497-570); real_rns / imag_rns as the reference's host code forms them (ckks/operator.cu:583-617:
    round, non-negative residue), psi^(N/2) from the project's ntt_table."""
    c, o, primes, R = ckks_p1
    n, limbs, parts = c.n, 3, 2
    ct = synth_ct(primes, range(limbs), parts, n, 6)
    corners(ct, 0, primes[0])
    words = parts * limbs * n
    d = hg.to_device(ct)
    for re, im in ((3.0, -2.0), (0.0, 0.0), (-1.5e12, 7.25e11), (2.0 ** 70 + 2.0 ** 30, -1.0), (0.5, -0.5)):
        real = hg.to_device(np.array([_round_away(re) % q for q in primes[:limbs]], dtype=np.uint64))
        imag = hg.to_device(np.array([_round_away(im) % q for q in primes[:limbs]], dtype=np.uint64))
        got = hg.to_host(c.ckks_gaussian_integer_op(op, d, re, im, limbs, parts))
        ref = R.run("refk_ckks_gaussian_integer_op", words, op=op, real_rns=real, imag_rns=imag,
                    ntt_table=R.tab("ntt_table"), modulus=R.mod, limbs=limbs, parts=parts, **{"in": d})
        with domain(oracle, "ckks_gaussian_integer_op"):
            want = o.ckks_gaussian_integer_op(op, ct, re, im, limbs, parts)
        same("hegpu_ckks_gaussian_integer_op", ref, got, want, (op, re, im))


@pytest.mark.parametrize("divide", [False, True], ids=["mult_i", "div_i"])
def test_ckks_mult_i(hg, oracle, torch, ckks_p1, divide):
    """hegpu_ckks_mult_i == cipher_mult_by_i_kernel / cipher_div_by_i_kernel (multiplication.cu:441-495)"""
    c, o, primes, R = ckks_p1
    n, limbs, parts = c.n, 4, 2
    ct = synth_ct(primes, range(limbs), parts, n, 8)
    corners(ct, 0, primes[0])
    corners(ct, n // 2, primes[0])  # the sign of i changes at N / 2
    words = parts * limbs * n
    d = hg.to_device(ct)
    got = hg.to_host(c.ckks_mult_i(d, limbs, parts, divide))
    ref = R.run("refk_ckks_mult_i", words, divide=int(divide), ntt_table=R.tab("ntt_table"), modulus=R.mod, limbs=limbs,
                parts=parts, **{"in": d})
    with domain(oracle, "ckks_mult_i"):
        want = o.ckks_mult_i(ct, limbs, parts, divide)
    same("hegpu_ckks_mult_i", ref, got, want, divide)


# ------------------------------------------------------------------ multiplication.cu
def test_cross_multiplication(hg, oracle, torch, bfv_4096):
    """hegpu_cross_multiplication == cross_multiplication (multiplication.cu:102-126) on the Q' chain and on the merged
    q | Bsk moduli of the project's context."""
    c, o, primes, R = bfv_4096
    n, batch = c.n, 2
    for table_set, mods_list in ((hg.TABLES_QP, primes), (hg.TABLES_Q_BSK, [int(v) for v in c.table("q_Bsk_merge_modulus")])):
        L = len(mods_list)
        a = [_limbs(oracle, mods_list, list(range(L)) * 2, n, 11 + b) for b in range(batch)]
        b_ = [_limbs(oracle, mods_list, list(range(L)) * 2, n, 31 + b) for b in range(batch)]
        for x in a:
            corners(x, 0, mods_list[0])
            corners(x, (2 * L - 1) * n, mods_list[L - 1])
        da, sa = pack(hg, torch, a)
        db, sb = pack(hg, torch, b_)
        out, so = blank(torch, batch, 3 * L * n)
        c.cross_multiplication(da, sa, db, sb, out, so, L, batch, table_set=table_set)
        got = unpack(hg, torch, out, batch, 3 * L * n)
        rmod = R.mod if table_set == hg.TABLES_QP else R.moduli(mods_list)
        omods = o.mods(mods_list)
        for b in range(batch):
            ref = R.run("refk_cross_multiplication", 3 * L * n, in1=hg.to_device(a[b]), in2=hg.to_device(b_[b]), modulus=rmod,
                        decomp_size=L)
            want = np.zeros(3 * L * n, dtype=np.uint64)
            with domain(oracle, "cross_multiplication"):
                o.L.o_cross_multiplication(a[b].ctypes.data, b_[b].ctypes.data, want.ctypes.data, omods, c.n_power, L)
            same("hegpu_cross_multiplication", ref, got[b], want, (table_set, b))


def test_cipherplain_multiplication(hg, oracle, torch, ckks_p1):
    """hegpu_cipherplain_multiplication == cipherplain_kernel (multiplication.cu:298-311).  The oracle applies this
    product only inside o_bfv_multiply_plain; column (c) is the product in Python integers (reduced operands: inside the
    Barrett domain)."""
    c, o, primes, R = ckks_p1
    n, limbs = c.n, 3
    ct = synth_ct(primes, range(limbs), 2, n, 15)
    plain = _limbs(oracle, primes, range(limbs), n, 25)
    corners(ct, 0, primes[0])
    plain[:3] = primes[0] - 1
    corners(plain, 3, primes[0])
    ct[3:6] = primes[0] - 1
    words = 2 * limbs * n
    out = torch.full((words,), SENTINEL, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert c._lib.hegpu_cipherplain_multiplication(c._h, hg.to_device(ct).data_ptr(), hg.to_device(plain).data_ptr(),
                                                   out.data_ptr(), limbs, st) == 0
    torch.cuda.synchronize()
    ref = R.run("refk_cipherplain", words, cipher=hg.to_device(ct), plain=hg.to_device(plain), modulus=R.mod,
                decomp_size=limbs)
    want = np.zeros(words, dtype=np.uint64)
    for z in range(2):
        for j in range(limbs):
            at = (z * limbs + j) * n
            want[at:at + n] = [int(x) * int(y) % primes[j] for x, y in zip(ct[at:at + n], plain[j * n:(j + 1) * n])]
    same("hegpu_cipherplain_multiplication", ref, hg.to_host(out), want, "cipherplain")


def test_threshold_lift_of_bfv_plain_to_ntt(hg, oracle, torch, bfv_4096):
    """threshold_kernel (multiplication.cu:274-296) with the project's upper_halfincrement and upper_threshold against the
    oracle's lift (o_bfv_threshold_lift, the first half of o_bfv_plain_to_ntt).  hegpu_bfv_plain_to_ntt has no entry
    that stops before the transform: its output, transformed back, must be the reference kernel's output (canonical
    residues both), and the reference kernel's output transformed forward must be its output."""
    c, o, primes, R = bfv_4096
    n, Q, t = c.n, c.Q_size, 1032193
    rng = np.random.default_rng(3)
    plain = rng.integers(0, t, n).astype(np.uint64)
    thr = R.scalar("upper_threshold")
    plain[:6] = [0, 1, thr - 1, thr, thr + 1, t - 1]
    words = Q * n
    ref = R.run("refk_threshold", words, plain=hg.to_device(plain), modulus=R.mod,
                upper_half_increment=R.tab("upper_halfincrement"), upper_half_threshold=thr, decomp_size=Q)
    want = np.zeros(words, dtype=np.uint64)
    with domain(oracle, "threshold"):
        o.L.o_bfv_threshold_lift(o.h, plain.ctypes.data, want.ctypes.data)
    ntt = c.bfv_plain_to_ntt(hg.to_device(plain))
    back = torch.empty_like(ntt)
    c.ntt(ntt, back, True, Q, Q)
    fwd = hg.to_device(ref)
    c.ntt(fwd, fwd, False, Q, Q)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(fwd), hg.to_host(ntt)), "NTT(threshold_kernel) != hegpu_bfv_plain_to_ntt"
    same("hegpu_bfv_plain_to_ntt (threshold lift)", ref, hg.to_host(back), want, "threshold")


def _behz_case(hg, oracle, torch, env, t):
    c, o, primes, R = env
    n, Q, batch = c.n, c.Q_size, 2
    mm = [int(v) for v in c.table("q_Bsk_merge_modulus")]
    L = len(mm)
    B = L - Q
    obase = R.moduli(c.table("base_Bsk"))
    ct1 = [synth_ct(primes, range(Q), 2, n, 1 + b) for b in range(batch)]
    ct2 = [synth_ct(primes, range(Q), 2, n, 9 + b) for b in range(batch)]
    for x in ct1:
        corners(x, 0, primes[0])
    d1, s1 = pack(hg, torch, ct1)
    d2, s2 = pack(hg, torch, ct2)
    out, so = blank(torch, batch, 4 * L * n)
    c.fast_convertion(d1, s1, d2, s2, out, so, batch)
    got = unpack(hg, torch, out, batch, 4 * L * n)
    for b in range(batch):
        ref = R.run("refk_fast_convertion", 4 * L * n, in1=hg.to_device(ct1[b]), in2=hg.to_device(ct2[b]), ibase=R.mod,
                    obase=obase, m_tilde=1 << 32, inv_prod_q_mod_m_tilde=R.scalar("inv_prod_q_mod_m_tilde"),
                    inv_m_tilde_mod_Bsk=R.tab("inv_m_tilde_mod_Bsk"), prod_q_mod_Bsk=R.tab("prod_q_mod_Bsk"),
                    base_change_matrix_Bsk=R.tab("base_change_matrix_Bsk"),
                    base_change_matrix_m_tilde=R.tab("base_change_matrix_m_tilde"),
                    inv_punctured_prod_mod_base_array=R.tab("inv_punctured_prod_mod_base_array"), ibase_size=Q, obase_size=B)
        want = np.zeros(4 * L * n, dtype=np.uint64)
        with domain(oracle, "fast_convertion"):
            o.L.o_fast_convertion(o.h, ct1[b].ctypes.data, ct2[b].ctypes.data, want.ctypes.data)
        same("hegpu_fast_convertion", ref, got[b], want, (n, b))
    src = [_limbs(oracle, mm, list(range(L)) * 3, n, 33 + b) for b in range(batch)]
    for s in src:
        s[Q * n:Q * n + 2] = [0, mm[Q] - 1]
        corners(s, 0, mm[0])
        corners(s, (L - 1) * n, mm[L - 1])
    ds, ss = pack(hg, torch, src)
    fl, sf = blank(torch, batch, 3 * Q * n)
    c.fast_floor(ds, ss, fl, sf, batch)
    got = unpack(hg, torch, fl, batch, 3 * Q * n)
    for b in range(batch):
        ref = R.run("refk_fast_floor", 3 * Q * n, ibase=R.mod, obase=obase, plain_modulus=t,
                    inv_punctured_prod_mod_base_array=R.tab("inv_punctured_prod_mod_base_array"),
                    base_change_matrix_Bsk=R.tab("base_change_matrix_Bsk"), inv_prod_q_mod_Bsk=R.tab("inv_prod_q_mod_Bsk"),
                    inv_punctured_prod_mod_B_array=R.tab("inv_punctured_prod_mod_B_array"),
                    base_change_matrix_q=R.tab("base_change_matrix_q"), base_change_matrix_msk=R.tab("base_change_matrix_msk"),
                    inv_prod_B_mod_m_sk=R.scalar("inv_prod_B_mod_m_sk"), prod_B_mod_q=R.tab("prod_B_mod_q"), ibase_size=Q,
                    obase_size=B, **{"in": hg.to_device(src[b])})
        want = np.zeros(3 * Q * n, dtype=np.uint64)
        with domain(oracle, "fast_floor"):
            o.L.o_fast_floor(o.h, src[b].ctypes.data, want.ctypes.data)
        same("hegpu_fast_floor", ref, got[b], want, (n, b))


def test_fast_convertion_and_fast_floor_default_chain(hg, oracle, torch, bfv_4096):
    """hegpu_fast_convertion / hegpu_fast_floor == fast_convertion / fast_floor (multiplication.cu:10-100, 128-272) with
    every BEHZ table of the project's context, N = 2^12 default chain: Q = 2 primes of 36 bits, Bsk = 3 primes of 61
    bits (the widest moduli the reference generates)."""
    c = bfv_4096[0]
    assert [int(v).bit_length() for v in c.table("base_Bsk")] == [61, 61, 61]
    _behz_case(hg, oracle, torch, bfv_4096, 1032193)


def test_fast_convertion_and_fast_floor_four_primes(hg, oracle, torch):
    """the same at N = 2^13 (Q = 4, five 61-bit base primes) with t = 65537"""
    c, o, primes = _bfv(hg, oracle, 8192, 65537)
    _behz_case(hg, oracle, torch, (c, o, primes, Ref(torch, hg, c)), 65537)


# ------------------------------------------------------------------ switchkey.cu: decomposition
@pytest.mark.parametrize("case", ["bfv_default_in_domain", "q61_into_30_bit"])
def test_cipher_broadcast_non_leveled(hg, oracle, torch, bfv_4096, case):
    """hegpu_cipher_broadcast (split = nmods, level = 0) == cipher_broadcast_kernel (switchkey.cu:11-27), which reduces
    with mult(1, x, q_i).
      bfv_default_in_domain  BFV N = 2^12 default chain (36 / 36 / 37 bits): x < 2^37 < 2^(2 * 36), INSIDE the Barrett
                             domain -- the comparison rests on reference text alone.  Also bfv_duplicate_kernel
                             (switchkey.cu:1592-1619), the same decomposition of part 1 with reduce_forced.
      q61_into_30_bit        Q = {61, 30, 30} | {61}: the 61-bit limb (x up to 2^61) into the 30-bit moduli (domain
                             x < 2^60) is OUTSIDE the domain: (a) and (c) share this project's restatement of the Barrett
                             sequence there, (b) reduces exactly; the oracle's counter must report it."""
    if case == "bfv_default_in_domain":
        c, o, primes, R = bfv_4096
    else:
        c, o, primes = _ckks(hg, oracle, 4096, [61, 30, 30], [61], sec=hg.SEC_NONE)
        assert [p.bit_length() for p in primes] == [61, 30, 30, 61]
        R = Ref(torch, hg, c)
    n, Q, Qp, batch = c.n, c.Q_size, c.Q_prime_size, 2
    src = [_limbs(oracle, primes, range(Q), n, 5 + b) for b in range(batch)]
    for s in src:
        s[:4] = [0, primes[0] - 1, primes[0] // 2, primes[0]]
        s[4:8] = [1 << 60, (1 << 60) - 1, primes[1], primes[2] - 1] if case != "bfv_default_in_domain" else s[4:8]
    d, s_in = pack(hg, torch, src)
    out, s_out = blank(torch, batch, Q * Qp * n)
    c.cipher_broadcast(d, s_in, out, s_out, Q, Qp, Qp, 0, batch)
    got = unpack(hg, torch, out, batch, Q * Qp * n)
    for b in range(batch):
        ref = R.run("refk_cipher_broadcast", Q * Qp * n, modulus=R.mod, Q_size=Q, rns_mod_count=Qp,
                    **{"in": hg.to_device(src[b])})
        want = np.zeros(Q * Qp * n, dtype=np.uint64)
        with domain(oracle, "cipher_broadcast/" + case):
            o.L.o_cipher_broadcast(src[b].ctypes.data, want.ctypes.data, o.qp_mods, c.n_power, Q, Qp)
        same("hegpu_cipher_broadcast", ref, got[b], want, (case, b))
        if case == "bfv_default_in_domain":
            part0 = _limbs(oracle, primes, range(Q), n, 900 + b)
            cipher = hg.to_device(np.concatenate([part0, src[b]]))
            out1 = R.out(Q * n)
            dup = R.run("refk_bfv_duplicate", Q * Qp * n, out_arg="out2", cipher=cipher, out1=out1[:Q * n], modulus=R.mod,
                        Q_size=Q, rns_mod_count=Qp)
            assert np.array_equal(R.take(out1, Q * n), part0)
            same("hegpu_cipher_broadcast", dup, got[b], want, ("bfv_duplicate", b))


@pytest.mark.parametrize("depth", [0, 1, 3])
def test_cipher_broadcast_leveled(hg, oracle, torch, depth):
    """hegpu_cipher_broadcast (split = l, level = depth) == cipher_broadcast_leveled_kernel (switchkey.cu:29-59), and the
    same decomposition of part 1 of a ciphertext by cipher_broadcast_switchkey_leveled_kernel (:1370-1411) and
    ckks_duplicate_kernel (:1558-1590); CKKS N = 2^13 {40, 35 x 4} | {40} as the existing case.  reduce_forced only:
    no Barrett product."""
    n = 8192
    c, o, primes = _ckks(hg, oracle, n, *CKKS_P1, sec=hg.SEC_NONE)
    R = Ref(torch, hg, c)
    Q, Qp = 5, 6
    l, rc, batch = Q - depth, Qp - depth, 2
    src = [_limbs(oracle, primes, range(l), n, 9 + b) for b in range(batch)]
    for s in src:
        s[:4] = [0, primes[0] - 1, primes[0] // 2, primes[0]]
    d, s_in = pack(hg, torch, src)
    out, s_out = blank(torch, batch, l * rc * n)
    c.cipher_broadcast(d, s_in, out, s_out, l, rc, l, depth, batch)
    got = unpack(hg, torch, out, batch, l * rc * n)
    for b in range(batch):
        want = np.zeros(l * rc * n, dtype=np.uint64)
        with domain(oracle, "cipher_broadcast_leveled"):
            o.L.o_cipher_broadcast_leveled(src[b].ctypes.data, want.ctypes.data, o.qp_mods, Qp, rc, c.n_power, l)
        ref = R.run("refk_cipher_broadcast_leveled", l * rc * n, modulus=R.mod, first_rns_mod_count=Qp,
                    current_rns_mod_count=rc, current_decomp_count=l, **{"in": hg.to_device(src[b])})
        same("hegpu_cipher_broadcast", ref, got[b], want, ("leveled", depth, b))
        part0 = _limbs(oracle, primes, range(l), n, 700 + b)
        cipher = hg.to_device(np.concatenate([part0, src[b]]))
        out0 = R.out(l * n)
        sk = R.run("refk_cipher_broadcast_switchkey_leveled", l * rc * n, out_arg="out1", cipher=cipher, out0=out0[:l * n],
                   modulus=R.mod, first_rns_mod_count=Qp, current_rns_mod_count=rc, current_decomp_mod_count=l)
        assert np.array_equal(R.take(out0, l * n), part0)
        same("hegpu_cipher_broadcast", sk, got[b], want, ("switchkey_leveled", depth, b))
        dup = R.run("refk_ckks_duplicate", l * rc * n, cipher=cipher, modulus=R.mod, first_rns_mod_count=Qp,
                    current_rns_mod_count=rc, current_decomp_mod_count=l)
        same("hegpu_cipher_broadcast", dup, got[b], want, ("ckks_duplicate", depth, b))


def _m2_level(c, hg, depth):
    """where the tables of level `depth` start inside the project's concatenated m2_* tables"""
    Q, Qp = c.Q_size, c.Q_prime_size
    width = 2 if c.int("scheme") == hg.BFV else c.P_size
    off = dict(digits=0, mi=0, matrix=0, prod=0)
    for lvl in range(depth):
        l, rc = Q - lvl, Qp - lvl
        d = -(-l // width)
        off["digits"] += d
        off["mi"] += l
        off["matrix"] += l * rc
        off["prod"] += d * rc
    return off, -(-(Q - depth) // width)


def _dtoq_case(hg, oracle, torch, env, depth):
    c, o, primes, R = env
    n, Q, Qp = c.n, c.Q_size, c.Q_prime_size
    l, rc, batch = Q - depth, Qp - depth, 2
    off, d = _m2_level(c, hg, depth)
    ij = np.array(c.table("m2_I_j")[off["digits"]:off["digits"] + d], dtype=np.int32)
    il = np.array(c.table("m2_I_location")[off["digits"]:off["digits"] + d], dtype=np.int32)
    assert int(ij.sum()) == l and list(il) == [int(v) for v in np.cumsum(ij) - ij]
    dij, dil, dmi = R.ints(ij), R.ints(il), R.ints(range(rc))
    src = [_limbs(oracle, primes, range(l), n, 21 + b) for b in range(batch)]
    for s in src:
        corners(s, 0, primes[0])
        corners(s, (l - 1) * n, primes[l - 1])
    dsrc, s_in = pack(hg, torch, src)
    out, s_out = blank(torch, batch, d * rc * n)
    c.base_conversion_DtoQtilde(dsrc, s_in, out, s_out, depth, batch)
    got = unpack(hg, torch, out, batch, d * rc * n)
    leveled = int(c.int("scheme") != hg.BFV)
    for b in range(batch):
        ref = R.run("refk_base_conversion_DtoQtilde", d * rc * n, leveled=leveled, modulus=R.mod,
                    matrix=R.tab("m2_matrix", off["matrix"]), Mi_inv=R.tab("m2_Mi_inv", off["mi"]),
                    prod=R.tab("m2_prod", off["prod"]), I_j=dij, I_location=dil, I_len=d, h_I_j=ij.ctypes.data,
                    h_I_location=il.ctypes.data, mod_index=dmi, l=l, Q_tilda=rc, d=d, level=depth,
                    **{"in": hg.to_device(src[b])})
        want = np.zeros(d * rc * n, dtype=np.uint64)
        with domain(oracle, "base_conversion_DtoQtilde"):
            o.L.o_base_conversion_DtoQtilde(o.h, src[b].ctypes.data, want.ctypes.data, depth)
        same("hegpu_base_conversion_DtoQtilde", ref, got[b], want, (c.P_size, depth, b))


@pytest.mark.parametrize("depth", [0, 1])
def test_base_conversion_DtoQtilde_two_special_primes(hg, oracle, torch, ckks_p2, depth):
    """hegpu_base_conversion_DtoQtilde == base_conversion_DtoQtilde_relin_leveled_kernel (switchkey.cu:985-1046), digits
    of two primes, with the project's m2_matrix / m2_Mi_inv / m2_prod / m2_I_j / m2_I_location of that depth."""
    _dtoq_case(hg, oracle, torch, ckks_p2, depth)


@pytest.mark.parametrize("depth", [0, 1])
def test_base_conversion_DtoQtilde_five_special_primes(hg, oracle, torch, five_p, depth):
    """the same with digits of five primes (a full digit and a digit of one prime at depth 0, one full digit at depth 1)"""
    _dtoq_case(hg, oracle, torch, five_p, depth)


def test_base_conversion_DtoQtilde_bfv(hg, oracle, torch, bfv_8192_p2):
    """the BFV form, base_conversion_DtoQtilde_relin_kernel (switchkey.cu:872-927, bfv/operator.cu:600), N = 2^13 default
    chain split 3 | 2 (43 / 43 / 44 | 44 / 44 bits).  This kernel multiplies the digit residues without reducing them into
    the target modulus first (:914), where the oracle and the product reduce first (oracle/o_method2.c).  On this chain
    the un-reduced product stays inside the Barrett domain for every digit / target pair (largest residue times the
    actual matrix entry < 2^(2 bit)), so the two orders give the same words and the oracle's counter speaks for the
    reference column too."""
    _dtoq_case(hg, oracle, torch, bfv_8192_p2, 0)


# ------------------------------------------------------------------ switchkey.cu: inner product
def test_keyswitch_multiply_accumulate_method_I(hg, oracle, torch, bfv_4096):
    """hegpu_keyswitch_multiply_accumulate (split = nmods, level = 0) == keyswitch_multiply_accumulate_kernel
    (switchkey.cu:61-162) as bfv/operator.cu:542 launches it."""
    c, o, primes, R = bfv_4096
    n, Q, Qp, batch = c.n, c.Q_size, c.Q_prime_size, 2
    key = synth_key(primes, Q, Qp, n, 3)
    dig = [np.concatenate([_limbs(oracle, primes, range(Qp), n, 70 + 7 * b + d) for d in range(Q)]) for b in range(batch)]
    for x in dig:
        corners(x, 0, primes[0])
    key[:3] = primes[0] - 1
    dd, s_in = pack(hg, torch, dig)
    acc, s_out = blank(torch, batch, 2 * Qp * n)
    dkey = hg.to_device(key)
    c.keyswitch_multiply_accumulate(dd, s_in, dkey, acc, s_out, Q, Qp, Qp, Qp, 0, batch)
    got = unpack(hg, torch, acc, batch, 2 * Qp * n)
    for b in range(batch):
        ref = R.run("refk_keyswitch_multiply_accumulate", 2 * Qp * n, key=dkey, modulus=R.mod, Q_tilda_size=Qp, digits=Q,
                    **{"in": hg.to_device(dig[b])})
        want = np.zeros(2 * Qp * n, dtype=np.uint64)
        with domain(oracle, "keyswitch_mac"):
            o.L.o_keyswitch_mac(dig[b].ctypes.data, key.ctypes.data, want.ctypes.data, o.qp_mods, c.n_power, Qp, Q)
        same("hegpu_keyswitch_multiply_accumulate", ref, got[b], want, ("method I", b))


@pytest.mark.parametrize("depth", [0, 2])
def test_keyswitch_multiply_accumulate_leveled(hg, oracle, torch, ckks_p1, depth):
    """== keyswitch_multiply_accumulate_leveled_kernel (switchkey.cu:164-285): l + 1 rows, the last one the special prime
    read at key limb Q' - 1; l = 5 digits exercise the unrolled-by-four loop and its tail, l = 3 the tail alone."""
    c, o, primes, R = ckks_p1
    n, Q, Qp, batch = c.n, c.Q_size, c.Q_prime_size, 2
    l, rc = Q - depth, Qp - depth
    key = synth_key(primes, Q, Qp, n, 3)
    limb_ids = list(range(l)) + [Q]
    dig = [np.concatenate([_limbs(oracle, primes, limb_ids, n, 40 + 7 * b + d) for d in range(l)]) for b in range(batch)]
    for x in dig:
        corners(x, 0, primes[0])
        corners(x, l * n, primes[Q])
    dd, s_in = pack(hg, torch, dig)
    acc, s_out = blank(torch, batch, 2 * rc * n)
    dkey = hg.to_device(key)
    c.keyswitch_multiply_accumulate(dd, s_in, dkey, acc, s_out, l, rc, Qp, l, depth, batch)
    got = unpack(hg, torch, acc, batch, 2 * rc * n)
    for b in range(batch):
        ref = R.run("refk_keyswitch_multiply_accumulate_leveled", 2 * rc * n, key=dkey, modulus=R.mod,
                    first_rns_mod_count=Qp, current_decomp_mod_count=l, **{"in": hg.to_device(dig[b])})
        want = np.zeros(2 * rc * n, dtype=np.uint64)
        with domain(oracle, "keyswitch_mac_leveled"):
            o.L.o_keyswitch_mac_leveled(dig[b].ctypes.data, key.ctypes.data, want.ctypes.data, o.qp_mods, Qp, l, c.n_power)
        same("hegpu_keyswitch_multiply_accumulate", ref, got[b], want, ("leveled", depth, b))


def _mac_II_case(hg, oracle, torch, env, depth):
    c, o, primes, R = env
    n, Q, Qp, P, batch = c.n, c.Q_size, c.Q_prime_size, c.P_size, 2
    l, rc = Q - depth, Qp - depth
    digits, key_digits = -(-l // P), -(-Q // P)
    key = synth_key(primes, key_digits, Qp, n, 3)
    limb_ids = list(range(l)) + list(range(Q, Qp))
    dig = [np.concatenate([_limbs(oracle, primes, limb_ids, n, 40 + 7 * b + d) for d in range(digits)]) for b in range(batch)]
    for x in dig:
        corners(x, 0, primes[0])
        corners(x, l * n, primes[Q])
    dd, s_in = pack(hg, torch, dig)
    acc, s_out = blank(torch, batch, 2 * rc * n)
    dkey = hg.to_device(key)
    c.keyswitch_multiply_accumulate(dd, s_in, dkey, acc, s_out, digits, rc, Qp, l, depth, batch)
    got = unpack(hg, torch, acc, batch, 2 * rc * n)
    for b in range(batch):
        ref = R.run("refk_keyswitch_multiply_accumulate_leveled_method_II", 2 * rc * n, key=dkey, modulus=R.mod,
                    first_rns_mod_count=Qp, current_decomp_mod_count=l, current_rns_mod_count=rc, digits=digits, level=depth,
                    **{"in": hg.to_device(dig[b])})
        want = np.zeros(2 * rc * n, dtype=np.uint64)
        with domain(oracle, "keyswitch_mac_II"):
            o.L.o_keyswitch_mac_II(dig[b].ctypes.data, key.ctypes.data, want.ctypes.data, o.qp_mods, Qp, l, rc, digits,
                                   depth, c.n_power)
        same("hegpu_keyswitch_multiply_accumulate", ref, got[b], want, ("method II", P, depth, b))


@pytest.mark.parametrize("depth", [0, 2])
def test_keyswitch_multiply_accumulate_method_II(hg, oracle, torch, ckks_p2, depth):
    """== keyswitch_multiply_accumulate_leveled_method_II_kernel (switchkey.cu:287-398): rows past l read key limb
    y + depth; {40, 35 x 4} | {40, 40}: three digits at depth 0, two at depth 2"""
    _mac_II_case(hg, oracle, torch, ckks_p2, depth)


@pytest.mark.parametrize("depth", [0, 2])
def test_keyswitch_multiply_accumulate_method_II_five_special_primes(hg, oracle, torch, five_p, depth):
    """the same on the chain with five special primes (two digits / one digit, eleven / nine rows)"""
    _mac_II_case(hg, oracle, torch, five_p, depth)


# ------------------------------------------------------------------ switchkey.cu: mod-down
@pytest.mark.parametrize("switchkey", [0, 1])
def test_divide_round_lastq(hg, oracle, torch, bfv_4096, switchkey):
    """hegpu_divide_round_lastq == divide_round_lastq_kernel / _switchkey_kernel (switchkey.cu:400-478) with the
    project's half, half_mod and last_q_modinv."""
    c, o, primes, R = bfv_4096
    n, Q, Qp, batch = c.n, c.Q_size, c.Q_prime_size, 2
    src = [_limbs(oracle, primes, list(range(Qp)) * 2, n, 3 + b) for b in range(batch)]
    for s in src:
        s[:4] = [0, primes[0] - 1, 1, primes[0] // 2]
        corners(s, Q * n, primes[Q])
        corners(s, (Qp + Q) * n, primes[Q])
    cts = [synth_ct(primes, range(Q), 2, n, 50 + b) for b in range(batch)]
    ds, s_in = pack(hg, torch, src)
    dc, s_ct = pack(hg, torch, cts)
    out, s_out = blank(torch, batch, 2 * Q * n)
    c.divide_round_lastq(ds, s_in, dc, s_ct, out, s_out, switchkey, batch)
    got = unpack(hg, torch, out, batch, 2 * Q * n)
    half, half_mod, inv = o.table("half"), o.table("half_mod"), o.table("last_q_modinv")
    for b in range(batch):
        ref = R.run("refk_divide_round_lastq", 2 * Q * n, switchkey=switchkey, ct=hg.to_device(cts[b]), modulus=R.mod,
                    half=R.tab("half"), half_mod=R.tab("half_mod"), last_q_modinv=R.tab("last_q_modinv"),
                    decomp_mod_count=Q, **{"in": hg.to_device(src[b])})
        want = np.zeros(2 * Q * n, dtype=np.uint64)
        with domain(oracle, "divide_round_lastq"):
            o.L.o_divide_round_lastq(src[b].ctypes.data, cts[b].ctypes.data, want.ctypes.data, o.qp_mods, half.ctypes.data,
                                     half_mod.ctypes.data, inv.ctypes.data, c.n_power, Q, switchkey)
        same("hegpu_divide_round_lastq", ref, got[b], want, (switchkey, b))


def _moddown_inputs(oracle, primes, c, depth, n, batch, seed):
    Q, Qp = c.Q_size, c.Q_prime_size
    l = Q - depth
    ids = list(range(l)) + list(range(Q, Qp))
    src = [_limbs(oracle, primes, ids * 2, n, seed + b) for b in range(batch)]
    for s in src:
        s[0] = 0  # q - 0 = q is stored un-reduced by the reference's negation
        s[1:3] = [primes[0] - 1, primes[0] // 2]
        for k in range(Q, Qp):  # every special limb of both parts at its corners
            for part in range(2):
                corners(s, (part * len(ids) + l + k - Q) * n, primes[k])
    return src


def _permute_case(hg, oracle, torch, env, depth, g):
    c, o, primes, R = env
    n, Q, Qp, P, batch = c.n, c.Q_size, c.Q_prime_size, c.P_size, 2
    l, rc = Q - depth, Qp - depth
    src = _moddown_inputs(oracle, primes, c, depth, n, batch, 13)
    in2 = [_limbs(oracle, primes, range(l), n, 60 + b) for b in range(batch)]
    ds, s_in = pack(hg, torch, src)
    d2, s_2 = pack(hg, torch, in2)
    out, s_out = blank(torch, batch, 2 * l * n)
    c.divide_round_lastq_permute(ds, s_in, d2, s_2, out, s_out, g, depth, batch)
    got = unpack(hg, torch, out, batch, 2 * l * n)
    half, half_mod, inv = o.table("half"), o.table("half_mod"), o.table("last_q_modinv")
    bfv = int(c.int("scheme") == hg.BFV)
    for b in range(batch):
        ref = R.run("refk_divide_round_lastq_permute", 2 * l * n, bfv=bfv, in2=hg.to_device(in2[b]), modulus=R.mod,
                    half=R.tab("half"), half_mod=R.tab("half_mod"), last_q_modinv=R.tab("last_q_modinv"), galois_elt=g,
                    Q_prime_size=rc, Q_size=l, first_Q_prime_size=Qp, first_Q_size=Q, P_size=P,
                    **{"in": hg.to_device(src[b])})
        want = np.zeros(2 * l * n, dtype=np.uint64)
        with domain(oracle, "divide_round_lastq_permute"):
            o.L.o_divide_round_lastq_permute(src[b].ctypes.data, in2[b].ctypes.data, want.ctypes.data, o.qp_mods,
                                             half.ctypes.data, half_mod.ctypes.data, inv.ctypes.data, g, c.n_power, rc, l, Qp,
                                             Q, P)
        same("hegpu_divide_round_lastq_permute", ref, got[b], want, (bfv, P, depth, g, b))


@pytest.mark.parametrize("g", [3, 2 * 4096 - 1])
def test_divide_round_lastq_permute_bfv(hg, oracle, torch, bfv_4096, g):
    """hegpu_divide_round_lastq_permute on a BFV context == divide_round_lastq_permute_bfv_kernel (switchkey.cu:1720-1813)"""
    _permute_case(hg, oracle, torch, bfv_4096, 0, g)


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("g", [3, 2 * 4096 - 1])
def test_divide_round_lastq_permute_ckks(hg, oracle, torch, ckks_p1, depth, g):
    """... on a CKKS context == divide_round_lastq_permute_ckks_kernel (switchkey.cu:1621-1718), one special prime"""
    _permute_case(hg, oracle, torch, ckks_p1, depth, g)


@pytest.mark.parametrize("depth", [0, 2])
def test_divide_round_lastq_permute_ckks_two_special_primes(hg, oracle, torch, ckks_p2, depth):
    """two special primes (the method II callers, ckks/operator.cu:1691): the chain among the special primes"""
    _permute_case(hg, oracle, torch, ckks_p2, depth, hg.steps_to_galois_elt(1, 4096, 5))


@pytest.mark.parametrize("depth", [0, 1])
def test_divide_round_lastq_permute_five_special_primes(hg, oracle, torch, five_p, depth):
    _permute_case(hg, oracle, torch, five_p, depth, hg.steps_to_galois_elt(-2, 4096, 5))


def _extended_case(hg, oracle, torch, env, depth, modes):
    c, o, primes, R = env
    n, Q, Qp, P, batch = c.n, c.Q_size, c.Q_prime_size, c.P_size, 2
    l, rc = Q - depth, Qp - depth
    src = _moddown_inputs(oracle, primes, c, depth, n, batch, 33)
    cts = [synth_ct(primes, range(l), 2, n, 44 + b) for b in range(batch)]
    ds, s_in = pack(hg, torch, src)
    dc, s_ct = pack(hg, torch, cts)
    for mode in modes:
        out, s_out = blank(torch, batch, 2 * l * n)
        c.divide_round_lastq_extended(ds, s_in, dc, s_ct, out, s_out, mode, depth, batch)
        got = unpack(hg, torch, out, batch, 2 * l * n)
        for b in range(batch):
            ref = R.run("refk_divide_round_lastq_extended", 2 * l * n, mode=mode, ct=hg.to_device(cts[b]), modulus=R.mod,
                        half=R.tab("half"), half_mod=R.tab("half_mod"), last_q_modinv=R.tab("last_q_modinv"), Q_prime_size=rc,
                        Q_size=l, first_Q_prime_size=Qp, first_Q_size=Q, P_size=P, **{"in": hg.to_device(src[b])})
            want = np.zeros(2 * l * n, dtype=np.uint64)
            with domain(oracle, "divide_round_lastq_extended"):
                o.L.o_divide_round_lastq_extended(o.h, src[b].ctypes.data, cts[b].ctypes.data, want.ctypes.data, rc, l, mode)
            same("hegpu_divide_round_lastq_extended", ref, got[b], want, (P, depth, mode, b))


@pytest.mark.parametrize("depth", [0, 1])
def test_divide_round_lastq_extended_leveled(hg, oracle, torch, ckks_p2, five_p, depth):
    """hegpu_divide_round_lastq_extended mode 0 == divide_round_lastq_extended_leveled_kernel (switchkey.cu:1222-1282),
    two and five special primes, depth 0 / 1"""
    _extended_case(hg, oracle, torch, ckks_p2, depth, (0,))
    _extended_case(hg, oracle, torch, five_p, depth, (0,))


def test_divide_round_lastq_extended_with_ct(hg, oracle, torch, bfv_8192_p2, ckks_p2, five_p):
    """modes 1 / 2 == divide_round_lastq_extended_kernel / _extended_switchkey_kernel (switchkey.cu:480-611).  The
    reference has these two for the whole chain only (bfv/operator.cu:663, 1362 pass Q_prime_size / Q_size), so they are
    compared at depth 0: on the BFV chain that uses them and on the two CKKS chains."""
    for env in (bfv_8192_p2, ckks_p2, five_p):
        _extended_case(hg, oracle, torch, env, 0, (1, 2))


@pytest.mark.parametrize("depth", [0, 2])
def test_leveled_moddown_stages(hg, oracle, torch, ckks_p1, depth):
    """hegpu_divide_round_lastq_leveled_stage_one (relinearize and rescale forms), _stage_two (plain and switchkey),
    hegpu_move_cipher_leveled and hegpu_divide_round_lastq_rescale == the kernels of switchkey.cu:678-815 with the table
    offsets of the reference's callers (ckks/operator.cu:1003-1020, 1205-1231) applied to the PROJECT's tables."""
    c, o, primes, R = ckks_p1
    n, Q, np_, batch = c.n, c.Q_size, c.n_power, 2
    l = Q - depth
    # ---- stage one, relinearize form
    src = [_limbs(oracle, primes, (list(range(l)) + [Q]) * 2, n, 5 + b) for b in range(batch)]
    for s_ in src:
        corners(s_, l * n, primes[Q])
        corners(s_, (2 * l + 1) * n, primes[Q])
    ds, s_in = pack(hg, torch, src)
    out, s_out = blank(torch, batch, 2 * l * n)
    c.divide_round_lastq_leveled_stage_one(ds, s_in, out, s_out, 0, depth, batch)
    got = unpack(hg, torch, out, batch, 2 * l * n)
    half, half_mod, inv = o.table("half"), o.table("half_mod"), o.table("last_q_modinv")
    for b in range(batch):
        ref = R.run("refk_divide_round_lastq_leveled_stage_one", 2 * l * n, modulus=R.mod, half=R.tab("half"),
                    half_mod=R.tab("half_mod"), first_decomp_count=Q, current_decomp_count=l, **{"in": hg.to_device(src[b])})
        want = np.zeros(2 * l * n, dtype=np.uint64)
        with domain(oracle, "leveled_stage_one"):
            o.L.o_divide_round_lastq_leveled_stage_one(src[b].ctypes.data, want.ctypes.data, o.qp_mods, half.ctypes.data,
                                                       half_mod.ctypes.data, np_, Q, l)
        same("hegpu_divide_round_lastq_leveled_stage_one", ref, got[b], want, ("relinearize", depth, b))
    # ---- stage two, plain and switchkey
    last = [_limbs(oracle, primes, list(range(l)) * 2, n, 15 + b) for b in range(batch)]
    cts = [synth_ct(primes, range(l), 2, n, 70 + b) for b in range(batch)]
    for x in last:
        corners(x, 0, primes[0])
    dl, s_l = pack(hg, torch, last)
    dc, s_c = pack(hg, torch, cts)
    for sk in (0, 1):
        out, s_out = blank(torch, batch, 2 * l * n)
        c.divide_round_lastq_leveled_stage_two(dl, s_l, ds, s_in, dc, s_c, out, s_out, sk, depth, batch)
        got = unpack(hg, torch, out, batch, 2 * l * n)
        for b in range(batch):
            ref = R.run("refk_divide_round_lastq_leveled_stage_two", 2 * l * n, switchkey=sk, in_last=hg.to_device(last[b]),
                        ct=hg.to_device(cts[b]), modulus=R.mod, last_q_modinv=R.tab("last_q_modinv"), current_decomp_count=l,
                        **{"in": hg.to_device(src[b])})
            want = np.zeros(2 * l * n, dtype=np.uint64)
            with domain(oracle, "leveled_stage_two"):
                o.L.o_divide_round_lastq_leveled_stage_two(last[b].ctypes.data, src[b].ctypes.data, cts[b].ctypes.data,
                                                           want.ctypes.data, o.qp_mods, inv.ctypes.data, np_, l, sk)
            same("hegpu_divide_round_lastq_leveled_stage_two", ref, got[b], want, (sk, depth, b))
    # ---- rescale: stage one on [2][l][N], the copy of the kept limbs, the division
    loc = _rescale_location(Q, depth)
    rhalf, rhm, rinv = o.table("rescaled_half"), o.table("rescaled_half_mod"), o.table("rescaled_last_q_modinv")
    ct_in = [synth_ct(primes, range(l), 2, n, 90 + b) for b in range(batch)]
    for s_ in ct_in:
        corners(s_, (l - 1) * n, primes[l - 1])
        corners(s_, (2 * l - 1) * n, primes[l - 1])
    di, s_i = pack(hg, torch, ct_in)
    out1, s_o1 = blank(torch, batch, 2 * (l - 1) * n)
    c.divide_round_lastq_leveled_stage_one(di, s_i, out1, s_o1, 1, depth, batch)
    got = unpack(hg, torch, out1, batch, 2 * (l - 1) * n)
    for b in range(batch):
        ref = R.run("refk_divide_round_lastq_leveled_stage_one", 2 * (l - 1) * n, modulus=R.mod,
                    half=R.tab("rescaled_half", depth), half_mod=R.tab("rescaled_half_mod", loc), first_decomp_count=l - 1,
                    current_decomp_count=l - 1, **{"in": hg.to_device(ct_in[b])})
        want = np.zeros(2 * (l - 1) * n, dtype=np.uint64)
        with domain(oracle, "rescale_stage_one"):
            o.L.o_divide_round_lastq_leveled_stage_one(ct_in[b].ctypes.data, want.ctypes.data, o.qp_mods,
                                                       rhalf.ctypes.data + 8 * depth, rhm.ctypes.data + 8 * loc, np_, l - 1,
                                                       l - 1)
        same("hegpu_divide_round_lastq_leveled_stage_one", ref, got[b], want, ("rescale", depth, b))
    moved, s_m = blank(torch, batch, 2 * l * n, fill=7)
    c.move_cipher_leveled(di, s_i, moved, s_m, depth, batch)
    got = unpack(hg, torch, moved, batch, 2 * l * n)
    for b in range(batch):
        ref = R.run("refk_move_cipher_leveled", 2 * l * n, out_fill=7, current_decomp_count=l - 1,
                    **{"in": hg.to_device(ct_in[b])})
        want = np.full(2 * l * n, 7, dtype=np.uint64)  # the dropped limb's slots stay untouched
        o.L.o_move_cipher_leveled(ct_in[b].ctypes.data, want.ctypes.data, np_, l - 1)
        same("hegpu_move_cipher_leveled", ref, got[b], want, (depth, b))
    last = [_limbs(oracle, primes, list(range(l - 1)) * 2, n, 25 + b) for b in range(batch)]
    dl, s_l = pack(hg, torch, last)
    out1, s_o1 = blank(torch, batch, 2 * (l - 1) * n)
    c.divide_round_lastq_rescale(dl, s_l, di, s_i, out1, s_o1, depth, batch)
    got = unpack(hg, torch, out1, batch, 2 * (l - 1) * n)
    for b in range(batch):
        ref = R.run("refk_divide_round_lastq_rescale", 2 * (l - 1) * n, in_last=hg.to_device(last[b]), modulus=R.mod,
                    last_q_modinv=R.tab("rescaled_last_q_modinv", loc), current_decomp_count=l - 1,
                    **{"in": hg.to_device(ct_in[b])})
        want = np.zeros(2 * (l - 1) * n, dtype=np.uint64)
        with domain(oracle, "rescale"):
            o.L.o_divide_round_lastq_rescale(last[b].ctypes.data, ct_in[b].ctypes.data, want.ctypes.data, o.qp_mods,
                                             rinv.ctypes.data + 8 * loc, np_, l - 1)
        same("hegpu_divide_round_lastq_rescale", ref, got[b], want, (depth, b))


@pytest.mark.parametrize("shift", [0, 1, 4095, 4096, 8191])
def test_negacyclic_shift(hg, oracle, torch, bfv_4096, shift):
    """hegpu_negacyclic_shift == negacyclic_shift_poly_coeffmod_kernel (switchkey.cu:1433-1457) for shifts 0, 1, N - 1, N
    and 2N - 1; a zero coefficient that wraps comes back as the un-reduced q."""
    c, o, primes, R = bfv_4096
    n, Q, parts = c.n, c.Q_size, 2
    ct = synth_ct(primes, range(Q), parts, n, 17)
    corners(ct, 0, primes[0])
    corners(ct, n - 3, primes[0])
    words = parts * Q * n
    d = hg.to_device(ct)
    got = hg.to_host(c.negacyclic_shift(d, shift, Q, parts))
    ref = R.run("refk_negacyclic_shift", words, modulus=R.mod, shift=shift, limbs=Q, parts=parts, **{"in": d})
    with domain(oracle, "negacyclic_shift"):
        want = o.negacyclic_shift(ct, shift, Q, parts)
    same("hegpu_negacyclic_shift", ref, got, want, shift)
