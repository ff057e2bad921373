"""The numpy references of tests/coords_reference.py on their own (no GPU): the GPU tests of csrc/coords.hip compare the
kernels with these functions bit for bit, so a slip here would be taken for a kernel bug — or hide one."""
import numpy as np
import pytest

import coords_reference as R
from oracle import me_oracle as O


def slow_morton(row, ts):
    """one key, bit by bit, from the text of include/me_amd.h"""
    D = len(row) - 1
    bits = min(21, 56 // D)
    key = (int(row[0]) & 0x7f) << 56
    for d in range(D):
        cell = int(row[1 + d]) // int(ts[d])                     # python floor division
        v = (cell + 2 ** (bits - 1)) % 2 ** bits
        for b in range(bits):
            if (v >> b) & 1:
                key |= 1 << (b * D + d)
    return key


@pytest.mark.parametrize("D,ts", [(1, (1,)), (1, (3,)), (2, (2, 4)), (3, (1, 1, 1)), (3, (2, 4, 1)), (4, (2, 2, 2, 2)),
                                  (7, (1,) * 7)])
def test_morton_key_matches_bit_loop(D, ts):
    rng = np.random.default_rng(D)
    bits = R.key_bits(D)
    span = 2 ** bits * max(ts)                                   # beyond the key's range on both sides: the mask matters
    c = rng.integers(-span, span, size=(300, D + 1)).astype(np.int32)
    c[:, 0] = rng.integers(0, 200, 300)                          # batch indices beyond 7 bits
    c[:8, 1:] = [[v] * D for v in (-1, 0, 1, -ts[0], ts[0] - 1, -ts[0] - 1, 2 ** (bits - 1) * ts[0], -2 ** (bits - 1) * ts[0])]
    got = R.morton_keys(c, ts)
    want = np.array([slow_morton(r, ts) for r in c], np.uint64)
    assert got.dtype == np.uint64 and np.array_equal(got, want)


def test_morton_key_hand_values():
    # D = 2, 21 bits: bias 2^20.  (x, y) = (0, 0) -> both values 2^20: bits 40 (x) and 41 (y) set
    assert R.morton_keys([[0, 0, 0]], (1, 1))[0] == (1 << 40) | (1 << 41)
    # x = -1 with ts 2 -> cell -1 -> value 2^20 - 1: bits 0, 2, .., 38 of the x lane; y = 3 -> cell 1 -> 2^20 + 1
    x = sum(1 << (2 * b) for b in range(20))
    y = (1 << 41) | (1 << 1)
    assert R.morton_keys([[129, -1, 3]], (2, 2))[0] == (1 << 56) | x | y    # batch 129 & 0x7f == 1


@pytest.mark.parametrize("n,ncol,dup", [(1, 2, 0), (64, 3, 1), (300, 4, 3), (1025, 5, 2), (500, 8, 4)])
def test_first_occurrence_matches_oracle(n, ncol, dup):
    rng = np.random.default_rng(n)
    c = rng.integers(-5, 6, size=(n, ncol)).astype(np.int32)
    for _ in range(dup):
        c = np.concatenate((c, c[rng.integers(0, len(c), len(c) // 2 + 1)]))
    um, inv = R.first_occurrence(c)
    oum, oinv = O.insert_and_map(c)
    assert np.array_equal(um, oum) and np.array_equal(inv, oinv)
    assert np.array_equal(c[um][inv], c) and (np.diff(um) > 0).all()


def test_first_occurrence_of_nothing():
    um, inv = R.first_occurrence(np.zeros((0, 4), np.int32))
    assert um.shape == (0,) and inv.shape == (0,)
    assert np.array_equal(R.bounding_box(np.zeros((0, 3), np.int32)), np.zeros(6))


def test_supercell_key_hand_rows():
    # D = 2, ts = (2, 1), supercells of 2^1 x 2^2 cells; directory: batches 3..4, supercells x -2..1, y -1..0
    shift, ts, sc_min, sc_dim = (1, 2), (2, 1), (3, -2, -1), (2, 4, 2)
    rows = [[3, -7, -4],    # cells (-4, -4) -> supercells (-2, -1) -> (0, 0, 0) -> 0
            [3, -1, -1],    # cells (-1, -1) -> supercells (-1, -1) -> (0, 1, 0) -> 2
            [3, 0, 0],      # cells (0, 0)   -> supercells (0, 0)   -> (0, 2, 1) -> 5
            [4, 7, 3],      # cells (3, 3)   -> supercells (1, 0)   -> (1, 3, 1) -> 15
            [4, -5, 3],     # cells (-3, 3)  -> supercells (-2, 0)  -> (1, 0, 1) -> 9
            [3, -3, -4]]    # cells (-2, -4) -> supercells (-1, -1) -> 2   (NOT -3 // 2 == -1 rounded towards zero)
    assert R.supercell_keys(rows, shift, sc_min, sc_dim, ts).tolist() == [0, 2, 5, 15, 9, 2]
    order, pos, dir_start = R.spatial_index(rows, shift, sc_min, sc_dim, ts)
    assert order.tolist() == [0, 1, 5, 2, 4, 3] and pos.tolist() == [0, 1, 3, 5, 4, 2]     # stable: row 1 before row 5
    assert dir_start.tolist() == [0, 1, 1, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 6]
    with pytest.raises(AssertionError):
        R.supercell_keys([[3, 8, 0]], shift, sc_min, sc_dim, ts)               # cell 4 -> supercell 2: outside


def test_grid_rule_and_margins():
    c = np.array([[1, -9, 5], [2, 30, 64]], np.int32)
    sh, sc_min, sc_dim, ts = R.grid_of(c, 2, (2, 1))
    assert (sh, ts) == ([2, 2], [2, 1])
    assert sc_min == [1, -2, 1] and sc_dim == [2, 6, 16]          # x cells -5..15 -> sc -2..3; y cells 5..64 -> sc 1..16
    _, sc_min, sc_dim, _ = R.grid_of(c, 2, (2, 1), margin_lo=1, margin_hi=2)
    assert sc_min == [1, -3, 0] and sc_dim == [2, 9, 19]


def test_zorder_passes_names_the_branches():
    # D = 3: 18 bits per axis, bias 2^17
    assert R.zorder_passes(None, (1, 1, 1), 3) == (list(range(0, 54, 8)) + [56], [])
    box = lambda lo, hi, b0=0, b1=0: [b0] + list(lo) + [b1] + list(hi)          # noqa: E731
    assert R.zorder_passes(box((0, 0, 0), (15, 15, 15)), (1, 1, 1), 3) == ([0, 8], ["plain"] * 3)
    assert R.zorder_passes(box((0, 0, 0), (15, 15, 15), 0, 2), (1, 1, 1), 3) == ([0, 8, 56], ["plain"] * 3)
    assert R.zorder_passes(box((5, 5, 5), (5, 5, 5)), (1, 1, 1), 3) == ([0], ["plain"] * 3)
    hi = 2 ** 17
    assert R.zorder_passes(box((hi - 2, 0, 0), (hi + 1, 1, 1)), (1, 1, 1), 3)[1] == ["wrap", "plain", "plain"]
    assert R.zorder_passes(box((-hi, 0, 0), (hi - 1, 1, 1)), (1, 1, 1), 3)[1] == ["wide", "plain", "plain"]
    assert R.zorder_passes(box((-2 * hi, 0, 0), (2 * hi - 2, 1, 1)), (2, 1, 1), 3)[1] == ["wide", "plain", "plain"]


def test_pair_lists_and_transpose():
    nbr = np.array([[-1, 4, -1, 0], [2, -1, -1, -1], [-1, -1, -1, -1]], np.int32)
    i, o, k = R.pair_lists(nbr)
    assert (i.tolist(), o.tolist(), k.tolist()) == ([4, 0, 2], [1, 3, 0], [0, 2, 3, 3])
    i2, o2, _ = R.pair_lists(nbr, out_rows=[9, 8, 7, 6])
    assert (i2.tolist(), o2.tolist()) == ([4, 0, 2], [8, 6, 9])
    t = R.transposed_table(i, o, k, 5)
    assert t.tolist() == [[3, -1, -1, -1, 1], [-1, -1, 0, -1, -1], [-1] * 5]
    t = R.transposed_table(i, o, k, 5, pos_in=[4, 3, 2, 1, 0])
    assert t.tolist() == [[1, -1, -1, -1, 3], [-1, -1, 0, -1, -1], [-1] * 5]
