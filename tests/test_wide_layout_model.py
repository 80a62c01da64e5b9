"""The pair ownership of the wide row kernels (ntt.hip: ks_own, ks_own_read, ks_ld16 / ks_st16; KsMacArgs::wide),
modelled with numpy over one 16 x 256 row tile, as the kernels index it.

Past its last four row stages thread (row, i0) has written positions 16 i0 + 0..15 of its row into the LDS tile at
row_phys(.).  The natural forms read back the elements i0 + 16 k (k < 16); the wide forms the pairs
2 i0 + 32 m + {0, 1} (m < 8), value 2 m + s, and every global access that follows (key tiles, identity limb, added
ciphertext, results) is the 16 bytes at row * 256 + 2 i0 + 32 m of the operand's own tile.

Checked here:
  * the ownership is a bijection between (thread, value) and the tile's elements, and ks_own(k) is the offset the
    kernels use for value k (the Galois scatter's element index);
  * for a fixed m the 16 lanes of a row touch 256 contiguous, 256-byte aligned bytes: two whole 128-byte lines;
  * the LDS read-back address the kernels form, (b ^ 2 m) + 32 m with b = row * 256 + 2 i0, is row_phys of the pair's
    first element, stays 16-byte aligned, keeps the two elements of a pair adjacent, and the 16 lanes of a row hit 16
    distinct 16-byte slots that together cover all 64 banks once (no conflict inside a 16-lane group);
  * reading the tile back in the wide ownership gives each thread exactly the elements the natural ownership gives
    the threads of the same row, permuted: the same multiset per row, each at the address the stores then use.
"""
import numpy as np
import pytest

ROWS, COLS = 16, 256


def row_phys(e):
    return e ^ (((e >> 5) & 7) << 1)


def ks_own(pair, k):
    return 32 * (k >> 1) + (k & 1) if pair else 16 * k


def ks_own0(pair, i0):
    return 2 * i0 if pair else i0


def _threads():
    t = np.arange(256)
    return t >> 4, t & 15


def test_ownership_is_a_bijection_in_both_forms():
    row, i0 = _threads()
    for pair in (False, True):
        seen = np.zeros(ROWS * COLS, dtype=np.int64)
        for k in range(16):
            e = row * 256 + ks_own0(pair, i0) + ks_own(pair, k)
            assert e.min() >= 0 and e.max() < ROWS * COLS
            np.add.at(seen, e, 1)
        assert (seen == 1).all(), pair


def test_wide_accesses_cover_whole_lines():
    row, i0 = _threads()
    for m in range(8):
        first = (row * 256 + 2 * i0 + 32 * m) * 8  # byte address of the lane's 16-byte access inside the tile
        assert (first % 16 == 0).all()
        for r in range(ROWS):
            lanes = np.sort(first[row == r])
            assert lanes[0] % 256 == 0  # two whole, aligned 128-byte lines
            assert (np.diff(lanes) == 16).all() and lanes[-1] + 16 - lanes[0] == 256


def test_natural_accesses_are_half_lines():
    """what the wide forms replace: 16 lanes x 8 bytes = one 128-byte line per access (the model's own control)"""
    row, i0 = _threads()
    for k in range(16):
        first = (row * 256 + i0 + 16 * k) * 8
        for r in range(ROWS):
            lanes = np.sort(first[row == r])
            assert lanes[0] % 128 == 0 and (np.diff(lanes) == 8).all() and lanes[-1] + 8 - lanes[0] == 128


def test_lds_read_back_matches_the_swizzle_and_is_conflict_free():
    row, i0 = _threads()
    b = row * 256 + 2 * i0
    for m in range(8):
        addr = (b ^ (2 * m)) + 32 * m  # as ks_own_read forms it
        e = row * 256 + 2 * i0 + 32 * m
        assert (addr == row_phys(e)).all()
        assert (row_phys(e + 1) == addr + 1).all() and (addr % 2 == 0).all()  # one aligned 16-byte read
        for r in range(ROWS):
            slots = np.sort(addr[row == r] // 2)
            assert len(set(slots)) == 16
            banks = np.concatenate([(addr[row == r] * 2 + d) % 64 for d in range(4)])  # 4-byte banks
            assert len(set(banks)) == 64


def test_read_back_returns_the_rows_own_elements():
    row, i0 = _threads()
    lds = np.full(ROWS * COLS, -1, dtype=np.int64)
    # the last four stages' write: thread (row, i0) leaves positions 16 i0 + 2 k + {0, 1}
    for k in range(8):
        for s in range(2):
            lds[row_phys(row * 256 + 16 * i0 + 2 * k) + s] = row * 256 + 16 * i0 + 2 * k + s
    assert sorted(lds) == list(range(ROWS * COLS))
    b = row * 256 + 2 * i0
    for k in range(16):
        m, s = k >> 1, k & 1
        got = lds[(b ^ (2 * m)) + 32 * m + s]
        assert (got == row * 256 + ks_own0(True, i0) + ks_own(True, k)).all()
        nat = lds[row_phys(row * 256 + i0 + 16 * k)]
        assert (nat == row * 256 + i0 + 16 * k).all()


# ---- The row-pair layout of the half-transformed digits and T: the second index map of the plan.  It was built, found
# bit-identical on the device and measured slower (negative result), so no kernel uses it; the model
# stays as the record of the two things that are easy to get wrong should it be tried again: which words a column-pass
# thread pairs, and which operand of the swap is which.
def rowpair(r, c):
    """word offset of element (r, c) of a limb (256 columns) in the row-pair layout"""
    return ((r >> 1) * 256 + c) * 2 + (r & 1)


def permlane16_swap(vdst, src):
    """v_permlane16_swap_b32 over one wave64 (arrays of 64 lanes): the odd 16-lane rows of the first operand change
    places with the even rows of the second; returns (new vdst, new src)"""
    d, s = vdst.copy(), src.copy()
    for pair in range(2):
        even, odd = slice(32 * pair, 32 * pair + 16), slice(32 * pair + 16, 32 * pair + 32)
        d[odd], s[even] = src[even], vdst[odd]
    return d, s


def test_rowpair_is_a_bijection_and_keeps_row_tiles_contiguous():
    r, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    off = rowpair(r, c)
    assert sorted(off.ravel()) == list(range(256 * 256))
    for tile in range(16):
        t = off[16 * tile:16 * tile + 16]
        assert t.min() == 4096 * tile and t.max() == 4096 * tile + 4095


@pytest.mark.parametrize("s1", [4, 5, 6, 7, 8])
def test_column_pass_stores_row_pairs_in_whole_lines(s1):
    """a column-pass thread (col, r1) of workgroup bx holds rows 16 r1 + k of column bx CT + col: eight 16-byte stores"""
    ct = 4096 >> s1
    t = np.arange(256)
    col, r1 = t % ct, t // ct
    seen = np.zeros(256 * 256, dtype=np.int64)
    for bx in range(256 // ct):
        c = bx * ct + col
        for m in range(8):
            first = ((8 * r1 + m) * 256 + c) * 2  # the thread's m-th 16-byte store
            assert (first == rowpair(16 * r1 + 2 * m, c)).all() and (first + 1 == rowpair(16 * r1 + 2 * m + 1, c)).all()
            np.add.at(seen, first, 1)
            np.add.at(seen, first + 1, 1)
            for g in range(16):  # the 16-lane groups of the workgroup
                lanes = np.sort(first[16 * g:16 * g + 16] * 8)
                assert lanes[0] % 256 == 0 and (np.diff(lanes) == 16).all()  # two whole, aligned 128-byte lines
    assert (seen[:(256 << s1)] == 1).all() and seen.sum() == 256 << s1  # the limb has 2^s1 rows


def test_rowpair_load_and_swap_give_each_lane_its_own_row():
    """the row kernels' load: lane (row = 2 m + s, i0) loads the pairs of columns i0 + 16 (8 s + kk); one swap per 32-bit half,
    first operand the pair's first word, second its second word; afterwards value kk is column i0 + 16 kk and value
    8 + kk column i0 + 16 (8 + kk) of the lane's own row -- the natural ownership i0 + 16 k"""
    tile = np.empty(4096, dtype=np.int64)
    r, c = np.meshgrid(np.arange(16), np.arange(256), indexing="ij")
    tile[rowpair(r, c)] = r * 256 + c  # every word holds its natural index
    for wave in range(4):
        t = 64 * wave + np.arange(64)
        row, i0 = t >> 4, t & 15
        p = ((row >> 1) * 256 + i0 + 128 * (row & 1)) * 2
        for kk in range(8):
            first = p + 32 * kk
            for rr in range(4):  # 16 lanes: 256 contiguous, aligned bytes
                lanes = np.sort(first[16 * rr:16 * rr + 16] * 8)
                assert lanes[0] % 256 == 0 and (np.diff(lanes) == 16).all()
            x, y = permlane16_swap(tile[first], tile[first + 1])
            assert (x == row * 256 + i0 + 16 * kk).all()
            assert (y == row * 256 + i0 + 16 * (8 + kk)).all()
