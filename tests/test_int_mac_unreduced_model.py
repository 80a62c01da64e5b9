"""The bound under which the correcting integer butterflies hand a key-switch digit to the 128-bit inner product
un-reduced (ntt.hip: cs_sched with its exit bound, ks_row_digit's EXIT; ntt.hpp: ks_unreduced_exit), as a pure-Python
model in exact integers.  No GPU.

  * the model of cs_sched reproduces every schedule that ntt.hip pins with a static_assert (read from the source), so
    it is the compiled schedule that is propagated here;
  * propagating the bound chain in units of q: before every stage the upper input u of a butterfly satisfies
    u + 4q < 2^64 (room 16 for q < 2^60, room 8 for q < 2^61), and the pass leaves what its exit bound says;
  * for every (digits, modulus bits) the host flag accepts, digits * exit * q * q < 2^128 for the largest q of that
    many bits and key residues up to q - 1 -- the sum reduce128 is given fits its 128 bits;
  * the flag refuses the first digit count beyond the bound, where even the smallest exit bound (8 q) would overflow
    for the largest q of that many bits.
(The kernels on both sides of the bound: tests/test_gpu_int_mac_unreduced.py.)"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heongpu_amd", "csrc")


def cs_sched(stages, room, exit_b=8):
    """ntt.hip cs_sched: (c8, c4), bit s = csub by 8q / by 4q before local stage s"""
    c8 = c4 = 0
    b = 8
    for s in range(stages):
        need = exit_b - 4 if (s == stages - 1 and exit_b < room) else room - 4
        if b > need and b > 8:
            c8 |= 1 << s
            b = 8
        if b > need:
            c4 |= 1 << s
            b = 4
        b += 4
    return c8, c4


def unreduced_exit(digits, q_bits):
    """ntt.hpp ks_unreduced_exit"""
    if digits <= 0 or q_bits <= 0 or 2 * q_bits > 127:
        return 0
    room = 1 << (128 - 2 * q_bits)
    for b in (16, 12, 8):
        if digits * b <= room:
            return b
    return 0


def chain(stages, room, exit_b):
    """bounds (units of q) of the upper input of every stage after its corrections, and the bound the pass leaves"""
    c8, c4 = cs_sched(stages, room, exit_b)
    b, ins = 8, []
    for s in range(stages):
        if c8 >> s & 1:
            assert 8 < b <= 16  # csub by 8q: [0, 16q) -> [0, 8q)
            b = 8
        if c4 >> s & 1:
            assert 4 < b <= 8   # csub by 4q: [0, 8q) -> [0, 4q)
            b = 4
        ins.append(b)
        b += 4                  # shoup_lazy's product is below 4q for any operand
    return ins, b


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_model_is_the_compiled_schedule():
    pins = re.findall(r"static_assert\(cs_sched\(([\d, ]+)\)\.c8 == (\w+)u && cs_sched\(([\d, ]+)\)\.c4 == (\w+)u", _src("ntt.hip"))
    assert len(pins) >= 6, pins
    seen = set()
    for a8, c8, a4, c4 in pins:
        assert a8 == a4
        args = tuple(int(v) for v in a8.split(","))
        seen.add(args)
        assert cs_sched(*args) == (int(c8, 0), int(c4, 0)), args
    # the schedules of before and the new ones
    assert {(8, 8), (8, 16), (5, 16), (8, 16, 12), (8, 16, 16), (8, 8, 8)} <= seen
    flags = re.findall(r"ks_unreduced_exit\((\d+), (\d+)\) == (\d+)", _src("ntt.hip"))
    assert len(flags) >= 9, flags
    for d, bits, want in flags:
        assert unreduced_exit(int(d), int(bits)) == int(want), (d, bits)
    # the model's body is the header's: same candidates in the same order, same room
    hpp = _src("ntt.hpp")
    assert "for (int b = 16; b >= 8; b -= 4)" in hpp and "<< (128 - 2 * q_bits)" in hpp


@pytest.mark.parametrize("room,q_bits,exits", [(16, 60, (8, 12, 16)), (8, 61, (8,))])
@pytest.mark.parametrize("stages", [4, 5, 6, 7, 8])
def test_every_stage_has_its_room(room, q_bits, exits, stages):
    q = (1 << q_bits) - 1  # no smaller room than at the top of the range
    for exit_b in exits:
        ins, out = chain(stages, room, exit_b)
        for s, b in enumerate(ins):
            assert b * q + 4 * q < 1 << 64, (exit_b, s, b)  # u < b q: u + 4q and u + 4q - t do not wrap
            assert b + 4 <= room
        assert out <= exit_b, (exit_b, ins)  # (a pass of few stages may end on a correction and leave less)
        assert stages != 8 or out == exit_b
    if room == 16 and stages == 8:
        assert chain(8, 16, 8)[0] == [8, 12, 8, 12, 8, 12, 8, 4]
        assert chain(8, 16, 12)[0] == [8, 12, 8, 12, 8, 12, 8, 8]
        assert chain(8, 16, 16)[0] == [8, 12, 8, 12, 8, 12, 8, 12]
        # corrections per coefficient pair over the eight stages of a digit: 5, 4, 3
        assert [bin(c8).count("1") + bin(c4).count("1") for c8, c4 in (cs_sched(8, 16, e) for e in (8, 12, 16))] == [5, 4, 3]


@pytest.mark.parametrize("q_bits", [59, 60, 61])
def test_accepted_sums_fit_128_bits_and_the_first_beyond_is_refused(q_bits):
    q = (1 << q_bits) - 1  # at least every modulus of that bit length; key residues up to q - 1
    accepted = 0
    for digits in range(1, 65):  # ks_row_mac_launch takes at most 64 digits
        b = unreduced_exit(digits, q_bits)
        if b:
            # what a modulus of this launch leaves: 60 bits and below b q, 61 bits 8 q <= b q
            assert b in (8, 12, 16)
            assert digits * (b * q - 1) * (q - 1) < 1 << 128, (digits, b)
            accepted = digits
            # the largest candidate that fits was chosen
            assert b == 16 or digits * (b + 4) * (1 << (2 * q_bits)) > 1 << 128
        else:
            assert digits > accepted and all(unreduced_exit(d, q_bits) == 0 for d in range(digits, 65))
            # refused only where the smallest exit bound would not be safe for every modulus of that length
            assert digits * 8 * (1 << (2 * q_bits)) > 1 << 128
            break
    want_last = {59: 64, 60: 32, 61: 8}[q_bits]
    assert accepted == want_last
    if want_last < 64:
        assert unreduced_exit(want_last + 1, q_bits) == 0
        # one digit more of values just below 8 q next to keys of q - 1 does pass 2^128 there
        assert (want_last + 1) * (8 * q - 1) * (q - 1) >= 1 << 128
    # far beyond: 61-bit q, 8 q exit, 33 digits
    assert unreduced_exit(33, 61) == 0


def test_split_launches_are_judged_by_their_largest_range():
    """ks_index gives split s the digits [s d / S, (s + 1) d / S): the longest range is ceil(d / S), which is what
    keyswitch_ntt_mac passes to ks_unreduced_exit"""
    for d in range(4, 65):
        for S in (2, 4):
            if d < 2 * S:
                continue
            longest = max((s + 1) * d // S - s * d // S for s in range(S))
            assert longest == (d + S - 1) // S
    assert "(digits + splits - 1) / splits" in _src("ops.cpp")
