"""The dense-conversion launches themselves (csrc/dense.hip: k_cell_index, k_grid_scatter, k_tile_to_box, k_tile_to_rows,
k_row_move, k_occupied_mask, k_occupied_fill, k_all_coords) through the C ABI: me_dense_cell_index, me_dense_grid,
me_dense_rows_to_box, me_dense_box_to_rows, me_dense_occupied_workspace_bytes, me_dense_occupied_count,
me_dense_occupied_fill, me_dense_all_coords.  Every input is built with numpy; no SparseTensor and no module is involved.

tests/test_gpu_dense.py drives these kernels through the operators, where torch's allocator aligns every box and no
tensor is wider than 32 channels (130 in the round trips added with this file).  Here the claims of the kernel file and
of the header (include/me_amd.h, the me_dense_* block) are the subject:
  * the three tile modes of tile_launch (MODE 0: four cells per lane, Vec4 accesses, inner % 4 == 0 AND a 16-byte aligned
    box; MODE 1: inner >= 16; MODE 2: the rest), reached by the ADDRESS of the box as well as by its shape, for 2-, 4- and
    8-byte words, in both directions, with a grid and as identity; tiles that span several `o`, a partial last tile, an
    all-empty tile between occupied ones; the second and third pass of the channel loop (C > 64) and the second step of
    k_row_move's lane loop;
  * "EVERY element of the box is written exactly once, zeros included"; cell-stationary box_to_rows "writes only rows
    the grid names"; row-stationary box_to_rows "writes zeros into a row whose cell is -1": held against outputs that
    hold a pattern no result can be, inside guard bands;
  * the guards the kernels apply themselves: grid[cell] >= n counts as empty (tile_setup), a cell outside [0, n_cells) is
    ignored by k_grid_scatter and k_row_move;
  * the occupied-cell pipeline (wave ballots, the in-place exclusive_scan_u32 of the wave counts on either side of a
    round of the single-workgroup scan and beyond its limit, k_occupied_fill) with n_cells on wave, block and scan
    edges, the keep rule "all bits but the sign" word by word, a workspace of exactly the bytes the library asks for;
  * floor division on either side of min_coord in 64-bit arithmetic (int32 extremes, cell indices near 2^39), D = 1..7,
    extents of 1, the flag; decompose() against np.unravel_index;
  * the argument checks, which leave every output untouched.

Oracle: a plain numpy restatement of the header.  Cell indices are computed with Python integers and `//`; grid[cell[r]]
= r, -1 elsewhere; box[o, :, i] = rows[r] for cell[r] = o * inner + i and zero elsewhere; rows[r] = box[o, :, i]; a
cell is kept when any((bits & ~signbit) != 0) over its channels, kept cells in ascending order; coordinates by
np.unravel_index.  Payload words are random BITS over the whole 2-, 4- or 8-byte range (NaN, Inf, -0 and denormal
patterns are put in by hand as well), compared as unsigned integers of the same width with np.array_equal: nothing is
compared as a float, there is no tolerance and no measured number, and no expected value comes from the kernels.  The
only words the data avoids are the two patterns of the buffers (PRE, POISON below), so that "still the pattern" and
"a leaked guard word" are certain statements.

Buffers: inputs are views into the middle of a tensor of POISON (NaN bits; index arrays: of an out-of-range index that
the kernels guard against); every output is a GuardedBytes buffer whose inside holds PRE before the launch, which must be
gone from every element the header says is written and still there in every element it says is not; the occupied
workspace has exactly me_dense_occupied_workspace_bytes(n_cells) bytes inside a GuardedBytes and is poisoned.

Not here: boxes near 2^31 cells for the occupied, fill and all-coords paths (tens of GB; the 32-bit decompose() there is
covered by the argument checks and by the long thin box only)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import GUARD_PAD, GuardedBytes, middle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minkowskiengine_amd", "csrc")
# csrc/dense.hip: `constexpr int kThreads = 256;`, `kT = 64` (cells per tile), `kCC = 64` (channels per pass);
# csrc/coords.hip: k_scan_single walks kScanSingleThreads * kScanSingleItems = 8192 items per round, up to kScanSingleMax =
# 4 rounds; csrc/common.hpp: kScanBlock = kScanThreads * kScanItems = 1024 items per block of the three-launch scan
K_THREADS, K_T, K_CC, WAVE = 256, 64, 64, 64
SCAN_ROUND, SCAN_SINGLE_MAX, SCAN_BLOCK = 8192, 32768, 1024
ROW_STATIONARY, CELL_STATIONARY = 1, 2
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

ELEMS = (2, 4, 8)
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SINT = {2: np.int16, 4: np.int32, 8: np.int64}
TORCH_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
SIGN = {2: 0x8000, 4: 0x80000000, 8: 1 << 63}
INF = {2: 0x7f80, 4: 0x7f800000, 8: 0x7ff0 << 48}
NAN = {2: 0x7fc3, 4: 0x7fc00003, 8: (0x7ff8 << 48) | 3}
PRE = {2: 0x5a5b, 4: 0x5a5b5c5d, 8: 0x5a5b5c5d5e5f6061}       # the inside of every output before a launch
POISON = {2: 0x7fc1, 4: 0x7fc00001, 8: (0x7ff8 << 48) | 1}     # around every payload input: NaN bits
CELL_AROUND = 1 << 41                                          # around a cell array: >= n_cells of every case
PRE32 = PRE[4]

# (outer, inner) of the mover cases
SHAPES = ((3, 4), (5, 20), (2, 64), (1, 128), (2, 68), (2, 17), (3, 33), (1, 65), (70, 1), (130, 1), (9, 3), (5, 15),
          (7, 8), (1, 16))
# >= 192 cells: tile 1 can be empty between occupied tiles 0 and 2; one shape per mode when aligned
HOLE_SHAPES = ((3, 64), (3, 67), (67, 3))
CHANNELS = (1, 64, 65, 129)                   # on every shape
ALL_CHANNELS = (1, 3, 63, 64, 65, 129)        # on one (shape, offset) per mode
# (outer, inner, byte offset of the box): one per mode; each has a partial last tile and tiles that span several `o`
MODE_CASES = ((5, 20, 0), (5, 20, 8), (9, 3, 0))
# identity and the policies add misaligned MODE 2 (inner % 4 == 0, inner < 16) and a single-`o` MODE 1
PLACED_CASES = MODE_CASES + ((3, 4, 8), (1, 65, 0))
KINDS = ("half", "perm", "empty", "hole", "first", "last", "identity")
GRID_KINDS = ("perm", "half", "empty", "hole", "first", "last")

OCC_SIZES = (1, 63, 64, 65, 255, 256, 257, 64 * 8191 + 1, 64 * 8192, 64 * 8192 + 1, 64 * 32768, 64 * 32768 + 65)
OCC_EXTREMES = (65, 257, 64 * 32768 + 65)     # all kept / all empty
OCC_INNER = (1, 5, 64)
OCC_SHAPES = {1: (3, 431), 3: (3, 5, 7, 11), 7: (2, 3, 2, 1, 3, 2, 2, 3)}      # D -> (B, X1 .. XD)
COORD_N_CELLS = (1, 255, 256, 257)
INDEX_ROWS = (1, 255, 256, 257)


def offsets(e):
    """byte offsets of the box from a 16-byte boundary: 8 breaks the alignment for every word size, 4 and 2 for the sizes
    that allow them"""
    return (0, 8) + ((4,) if e == 4 else ()) + ((2,) if e == 2 else ())


def mode(inner, box_byte_offset):
    """the mirror of tile_launch's rule"""
    return 0 if inner % 4 == 0 and box_byte_offset % 16 == 0 else (1 if inner >= 16 else 2)


def tiles_span_several_o(outer, inner):
    n_cells = outer * inner
    return any(t // inner != min(t + K_T - 1, n_cells - 1) // inner for t in range(0, n_cells, K_T))


def n_waves(n_cells):
    return -(-max(n_cells, 1) // WAVE)


# ---- data -----------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([11] + [int(k) for k in key])


def _signed(v, e):
    return int(v) - (1 << 8 * e) if int(v) >= 1 << (8 * e - 1) else int(v)


def random_words(rng, shape, e):
    """random bits of e bytes per word, a few hand-picked patterns among them, never PRE or POISON"""
    size = int(np.prod(shape))
    a = np.frombuffer(rng.bytes(size * e), UINT[e]).copy()
    special = [0, SIGN[e], 1, SIGN[e] | 1, INF[e], SIGN[e] | INF[e], NAN[e], (1 << 8 * e) - 1]
    if size:
        at = rng.choice(size, min(size // 2, 16), replace=False)
        a[at] = np.array([special[k % len(special)] for k in range(len(at))], UINT[e])
    bad = (a == UINT[e](PRE[e])) | (a == UINT[e](POISON[e]))
    a[bad] ^= UINT[e](0x10)
    return a.reshape(shape)


def cells_of(kind, rng, n_cells):
    """cell[n] of the rows for a grid content; "half" also has rows outside the box (cell -1, as me_dense_cell_index marks
    them)"""
    if kind == "identity":
        return np.arange(n_cells, dtype=np.int64)
    if kind == "perm":
        return rng.permutation(n_cells).astype(np.int64)
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "first":
        return np.array([0], np.int64)
    if kind == "last":
        return np.array([n_cells - 1], np.int64)
    keep = rng.random(n_cells) < 0.5
    if kind == "hole":
        assert n_cells >= 3 * K_T
        keep[[0, K_T - 1, 2 * K_T, min(3 * K_T, n_cells) - 1]] = True
        keep[K_T:2 * K_T] = False
        return rng.permutation(np.flatnonzero(keep)).astype(np.int64)
    assert kind == "half"
    keep[rng.integers(n_cells)] = True
    occ = np.flatnonzero(keep)
    cell = np.concatenate([occ, np.full(len(occ) // 4 + 1, -1)])
    return rng.permutation(cell).astype(np.int64)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def oracle_grid(cell, n_cells):
    grid = np.full(n_cells, -1, np.int32)
    for r, c in enumerate(cell.tolist()):
        if 0 <= c < n_cells:
            grid[c] = r
    return grid


def _named(grid, n):
    """(cells, rows): the cells whose grid entry names a row in [0, n)"""
    cells = np.flatnonzero((grid >= 0) & (grid < n))
    return cells, grid[cells].astype(np.int64)


def box_from_cell(rows, cell, outer, inner):
    """box[o, :, i] = rows[r] for cell[r] = o * inner + i inside the box, zero elsewhere"""
    box = np.zeros((outer, rows.shape[1], inner), rows.dtype)
    ok = np.flatnonzero((cell >= 0) & (cell < outer * inner))
    box[cell[ok] // inner, :, cell[ok] % inner] = rows[ok]
    return box


def box_from_grid(rows, grid, n, outer, inner):
    box = np.zeros((outer, rows.shape[1], inner), rows.dtype)
    cells, r = _named(grid, n)
    box[cells // inner, :, cells % inner] = rows[r]
    return box


def rows_from_cell(box, cell, n):
    """rows[r] = box[o, :, i]; zeros for a row whose cell is outside the box (row-stationary)"""
    outer, C, inner = box.shape
    rows = np.zeros((n, C), box.dtype)
    ok = np.flatnonzero((cell >= 0) & (cell < outer * inner))
    rows[ok] = box[cell[ok] // inner, :, cell[ok] % inner]
    return rows


def rows_from_grid(box, grid, n):
    """(rows, named): the rows the grid names; every other row keeps PRE (cell-stationary)"""
    outer, C, inner = box.shape
    rows = np.full((n, C), PRE[box.dtype.itemsize], box.dtype)
    cells, r = _named(grid, n)
    rows[r] = box[cells // inner, :, cells % inner]
    named = np.zeros(n, bool)
    named[r] = True
    return rows, named


TILE_MUTANTS = ("one_pass", "drop_partial", "o_of_first")


def tile_walk(to_box, src, grid, n, outer, inner, C, mutant=None):
    """The tile kernels restated cell by cell on FLAT arrays starting from PRE — without a mutant a second statement of
    box_from_grid / rows_from_grid, with one a WRONG kernel (test_inputs_*): "one_pass" leaves the channels from 64 up
    stale, "drop_partial" the cells of a partial last tile, "o_of_first" takes `o` of a tile's first cell for all of
    its cells."""
    e = src.dtype.itemsize
    n_cells = outer * inner
    cells = np.arange(n_cells, dtype=np.int64)
    r = cells.copy() if grid is None else grid.astype(np.int64)
    r = np.where((r >= 0) & (r < n), r, -1)
    o = cells // inner
    if mutant == "o_of_first":
        o = (cells // K_T * K_T) // inner
    base = o * C * inner + (cells - o * inner)
    sel = np.ones(n_cells, bool)
    if mutant == "drop_partial":
        sel = cells < n_cells // K_T * K_T
    passes = min(C, K_CC) if mutant == "one_pass" else C
    flat = src.reshape(-1)
    if to_box:
        out = np.full(n_cells * C, PRE[e], src.dtype)
        for c in range(passes):
            v = np.where(r >= 0, flat[np.maximum(r, 0) * C + c] if n else 0, 0).astype(src.dtype)
            out[base[sel] + c * inner] = v[sel]
        return out.reshape(outer, C, inner)
    out = np.full(n * C, PRE[e], src.dtype)
    sel &= r >= 0
    for c in range(passes):
        out[r[sel] * C + c] = flat[base[sel] + c * inner]
    return out.reshape(n, C)


def oracle_cell_index(coords, mn, dv, shape, mutant=None):
    """(cell, flag) with Python integers and floor division; "trunc" restates a kernel that rounds towards zero"""
    D = len(shape) - 1
    mn = [0] * D if mn is None else [int(v) for v in mn]
    dv = [1] * D if dv is None else [int(v) for v in dv]
    cell = []
    for row in coords.tolist():
        lin, ok = row[0], 0 <= row[0] < shape[0]
        for k in range(D):
            v = row[1 + k] - mn[k]
            q = v // dv[k]
            if mutant == "trunc":
                q = abs(v) // dv[k] * (1 if v >= 0 else -1)
            ok = ok and 0 <= q < shape[1 + k]
            lin = lin * shape[1 + k] + q
        cell.append(lin if ok else -1)
    return np.array(cell, np.int64).reshape(-1), int(any(c < 0 for c in cell))


def oracle_coords(cells, shape):
    return np.stack(np.unravel_index(np.asarray(cells, np.int64), shape), 1).astype(np.int32).reshape(-1, len(shape))


def oracle_occupied(box, mutant=None):
    """ascending cells of box [outer, C, inner] with a channel that is not +-0; "keep_minus_zero" restates a kernel that
    tests the whole word"""
    e = box.dtype.itemsize
    bits = box if mutant == "keep_minus_zero" else box & UINT[e](SIGN[e] - 1)
    return np.flatnonzero((bits != 0).any(1).reshape(-1)).astype(np.int64)


def fill_walk(cells, n_cells, mutant=None):
    """k_occupied_fill restated on a cell array of len(cells) entries of PRE: position = offset of the wave + rank in the
    wave; "wave_offset" takes the INCLUSIVE sum of the wave counts for the offset (the off-by-one wave offset)"""
    kept = np.zeros(n_cells, bool)
    kept[cells] = True
    w = n_waves(n_cells)
    counts = np.zeros(w, np.int64)
    np.add.at(counts, cells // WAVE, 1)
    offs = np.cumsum(counts) - (0 if mutant == "wave_offset" else counts)
    rank = np.cumsum(kept) - 1
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pos = offs[cells // WAVE] + rank[cells] - first[cells // WAVE]
    out = np.full(len(cells), _signed(PRE[8], 8), np.int64)
    ok = pos < len(cells)
    out[pos[ok]] = cells[ok]
    return out


class Move:
    """one mover problem: rows [n, C] and cell [n] for rows -> box, a full box [outer, C, inner] of random words for box
    -> rows, the grid of the cells, and the oracle's four answers"""

    def __init__(self, e, outer, inner, C, kind="half", cell=None, grid=None):
        self.e, self.outer, self.inner, self.C, self.kind = e, outer, inner, C, kind
        self.n_cells = outer * inner
        rng = _rng(1, e, outer, inner, C, KINDS.index(kind))
        self.cell = cells_of(kind, rng, self.n_cells) if cell is None else np.asarray(cell, np.int64)
        self.n = len(self.cell)
        self.grid = oracle_grid(self.cell, self.n_cells) if grid is None else np.asarray(grid, np.int32)
        self.rows = random_words(rng, (self.n, C), e)
        self.box = random_words(rng, (outer, C, inner), e)

    def want_box(self, policy):
        if policy == ROW_STATIONARY:
            return box_from_cell(self.rows, self.cell, self.outer, self.inner)
        return box_from_grid(self.rows, self.grid, self.n, self.outer, self.inner)

    def want_rows(self, policy):
        """(rows, defined)"""
        if policy == ROW_STATIONARY:
            return rows_from_cell(self.box, self.cell, self.n), np.ones(self.n, bool)
        return rows_from_grid(self.box, self.grid, self.n)


def keep_rule_box(e, background):
    """(box [3, 3, 40], {name: cells}, {name: kept}): every deciding word in channel 0 only, in the last channel only and
    in every channel, on a background of +0 or of -0 words; cells in between hold the background alone"""
    sign = SIGN[e]
    words = {"minus_zero": (sign, False), "plus_zero": (0, False), "denormal": (1, True), "minus_denormal": (sign | 1, True),
             "nan": (NAN[e], True), "inf": (INF[e], True), "minus_inf": (sign | INF[e], True)}
    if e == 8:
        words.update(low_half=(1 << 20, True), bit_62=(1 << 62, True), low_half_minus=(sign | (1 << 31), True))
    outer, C, inner = 3, 3, 40
    box = np.full((outer, C, inner), background, UINT[e])
    where, kept = {}, {}
    cell = 2
    for name, (word, keep) in words.items():
        for place in ("first", "last", "all"):
            o, i = divmod(cell, inner)
            ch = {"first": [0], "last": [C - 1], "all": list(range(C))}[place]
            box[o, ch, i] = UINT[e](word)
            where[(name, place)] = cell
            kept[(name, place)] = keep
            cell += 4                                          # up to cell 118 of 120: across the wave edge at 64 and across `o`
    assert cell - 4 < outer * inner and max(where.values()) > WAVE and len(where) == 3 * len(words)
    return box, where, kept


def occupancy_box(e, outer, C, inner, kind, key=0):
    """random words in the kept cells, a random mix of +0 and -0 words in the others ("all": no other cells, "none": no
    kept ones)"""
    rng = _rng(2, e, outer, C, inner, ("half", "all", "none").index(kind), key)
    box = random_words(rng, (outer, C, inner), e)
    if kind == "all":
        box[:, 0, :] |= UINT[e](1)
        box[box == UINT[e](PRE[e])] ^= UINT[e](2)
        return box
    zeros = (np.frombuffer(rng.bytes(box.size), np.uint8).reshape(box.shape) & 1).astype(UINT[e]) * UINT[e](SIGN[e])
    if kind == "none":
        return zeros
    empty = rng.random((outer, 1, inner)) < 0.5
    return np.where(empty, zeros, box)


def index_case(D, n, all_inside=False):
    """(coords [n, D + 1], min_coord, divisor, shape): divisors 1, 2, 3 and 7, extents of 1 among the others; rows at
    min_coord - 1, at min_coord, at the last coordinate of the last cell and one beyond it per dimension and for the batch
    column (batch -1 and B), then random rows on either side of the box"""
    rng = _rng(3, D, n, all_inside)
    dv = [(1, 2, 3, 7)[(k + D) % 4] for k in range(D)]
    ext = rng.integers(2, 5, D).tolist()
    if D >= 2:
        ext[int(rng.integers(D))] = 1
    B = int(rng.integers(1, 4))
    shape = [B] + ext
    mn = rng.integers(-9, 10, D).tolist()
    first = [0] + mn
    last = [B - 1] + [mn[k] + dv[k] * ext[k] - 1 for k in range(D)]
    rows = [first, last]
    if not all_inside:
        for k in range(D):
            for frm in (first, last):
                for x in (mn[k] - 1, mn[k], last[1 + k], last[1 + k] + 1):
                    rows.append(frm[:1 + k] + [x] + frm[2 + k:])
        for frm in (first, last):
            rows += [[-1] + frm[1:], [B] + frm[1:], [B - 1] + frm[1:]]
    lo = [0 if all_inside else -1] + [mn[k] - (0 if all_inside else 2 * dv[k]) for k in range(D)]
    hi = [B if all_inside else B + 1] + [last[1 + k] + 1 + (0 if all_inside else 2 * dv[k]) for k in range(D)]
    rnd = rng.integers(lo, hi, (max(n - len(rows), 0), D + 1))
    coords = np.concatenate([np.array(rows, np.int64).reshape(-1, D + 1), rnd])[:n].astype(np.int32)
    return coords, mn, dv, shape


def extreme_cases():
    """int32 extremes on either side: (coords, min_coord, divisor, shape)"""
    xs = (INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX)
    coords = np.array([[0, a, b] for a in xs for b in xs], np.int32)
    out = []
    for mn in ((INT32_MAX, INT32_MIN), (INT32_MIN, INT32_MAX), (INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX)):
        for dv in ((1, 1), (INT32_MAX, INT32_MAX), (1, INT32_MAX), (INT32_MAX, 1)):
            out.append((coords, list(mn), list(dv), [1, 3, 3]))
    return out


def far_corner_case(mn0):
    """shape (1, 2^31 - 1, 255): a handful of rows near the far corner, cell indices about 2^39"""
    shape = [1, INT32_MAX, 255]
    top = INT32_MAX - 1 + mn0                                  # the coordinate of the last cell along X1
    coords = np.array([[0, top, 254], [0, top, 253], [0, top - 1, 254], [0, top, 255], [0, top - 1, 0], [0, mn0, 0],
                       [0, mn0 - 1, 0], [0, min(top + 1, INT32_MAX), 0], [0, INT32_MAX, 254], [1, top, 254]], np.int64)
    assert coords.max() <= INT32_MAX and coords.min() >= INT32_MIN
    return coords.astype(np.int32), [mn0, 0], [1, 1], shape


# =====================================================================================================================
# CPU-side checks of the inputs (no GPU)
# =====================================================================================================================
def test_inputs_constants_match_the_source():
    src = open(os.path.join(CSRC, "dense.hip")).read()
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) == K_THREADS
    assert int(re.search(r"constexpr int kT = (\d+);", src).group(1)) == K_T
    assert int(re.search(r"constexpr int kCC = (\d+);", src).group(1)) == K_CC
    src = open(os.path.join(CSRC, "coords.hip")).read()
    t, i = re.search(r"constexpr int kScanSingleThreads = (\d+), kScanSingleItems = (\d+);", src).groups()
    assert int(t) * int(i) == SCAN_ROUND
    f = re.search(r"constexpr int64_t kScanSingleMax = (\d+) \* kScanSingleThreads \* kScanSingleItems;", src).group(1)
    assert int(f) * SCAN_ROUND == SCAN_SINGLE_MAX
    src = open(os.path.join(CSRC, "common.hpp")).read()
    t = int(re.search(r"constexpr int kScanThreads = (\d+);", src).group(1))
    i = int(re.search(r"constexpr int kScanItems = (\d+);", src).group(1))
    assert re.search(r"constexpr int kScanBlock = kScanThreads \* kScanItems;", src) and t * i == SCAN_BLOCK
    assert int(re.search(r"constexpr int kWave = (\d+);", src).group(1)) == WAVE


def test_inputs_shapes_reach_every_mode_and_condition():
    for e in ELEMS:
        assert set(offsets(e)) == {0, 8} | ({4} if e == 4 else set()) | ({2} if e == 2 else set())
        aligned = {mode(inner, 0) for _, inner in SHAPES}
        assert aligned == {0, 1, 2}, e
        for off in offsets(e)[1:]:
            got = {mode(inner, off) for _, inner in SHAPES}
            assert got == {1, 2}, (e, off)                     # MODE 0 needs the alignment: the Vec4 shapes are demoted ...
            demoted = {mode(inner, off) for _, inner in SHAPES if inner % 4 == 0}
            assert demoted == {1, 2}, (e, off)                  # ... to both scalar modes
        for m in (0, 1, 2):
            for off in offsets(e):
                if m == 0 and off:
                    continue
                of_mode = [(o, i) for o, i in SHAPES if mode(i, off) == m]
                assert any((o * i) % K_T for o, i in of_mode), (e, m, off, "no partial last tile")
                assert any(tiles_span_several_o(o, i) for o, i in of_mode), (e, m, off, "no tile spans several o")
    assert (3 * 4 < K_T and 5 * 20 % K_T == 36 and tiles_span_several_o(5, 20) and not tiles_span_several_o(2, 64)
            and not tiles_span_several_o(1, 65))
    assert [mode(i, off) for _, i, off in MODE_CASES] == [0, 1, 2]
    assert [mode(i, off) for _, i, off in PLACED_CASES] == [0, 1, 2, 2, 1]
    assert all((o * i) % K_T and (tiles_span_several_o(o, i) or o == 1) for o, i, _ in PLACED_CASES)
    assert [mode(i, 0) for _, i in HOLE_SHAPES] == [0, 1, 2] and mode(HOLE_SHAPES[0][1], 8) == 1
    assert all(o * i >= 3 * K_T for o, i in HOLE_SHAPES)
    # the channel loop: one pass, exactly one, a second of one channel, a third of one channel; k_row_move's lanes alike
    assert [-(-c // K_CC) for c in ALL_CHANNELS] == [1, 1, 1, 1, 2, 3] and set(CHANNELS) <= set(ALL_CHANNELS)
    # THE LIST of what the launchers can select, and the cases of this file that select each of them:
    #   k_tile_to_box / k_tile_to_rows <word, MODE, IDENTITY>: test_movers_on_every_shape (grid; every word size, every
    #   offset: all three modes) and test_identity (IDENTITY; PLACED_CASES: all three modes), both directions in each;
    #   k_row_move <word, TO_BOX>: the row-stationary half of the same tests; k_occupied_mask <word>: test_occupied_keep_rule
    tile = {(e, mode(i, off), ident, to_box) for e in ELEMS for ident, cases in
            ((False, [(o, i, off) for o, i in SHAPES for off in offsets(e)]), (True, PLACED_CASES))
            for _, i, off in cases for to_box in (True, False)}
    assert tile == {(e, m, ident, to_box) for e in ELEMS for m in (0, 1, 2) for ident in (False, True)
                    for to_box in (True, False)} and len(tile) == 36
    # k_row_move and k_occupied_mask take no mode: check_both_policies launches both directions row-stationary for every
    # Move of every word size, test_occupied_keep_rule and test_occupied_inner_and_dimensions are parametrised over ELEMS
    assert set(ELEMS) == {2, 4, 8}


def test_inputs_occupied_sizes_sit_on_the_edges():
    assert OCC_SIZES == (1, WAVE - 1, WAVE, WAVE + 1, K_THREADS - 1, K_THREADS, K_THREADS + 1, WAVE * (SCAN_ROUND - 1) + 1,
                         WAVE * SCAN_ROUND, WAVE * SCAN_ROUND + 1, WAVE * SCAN_SINGLE_MAX, WAVE * SCAN_SINGLE_MAX + WAVE + 1)
    w = [n_waves(n) for n in OCC_SIZES]
    assert w == [1, 1, 1, 2, 4, 4, 5, SCAN_ROUND, SCAN_ROUND, SCAN_ROUND + 1, SCAN_SINGLE_MAX, SCAN_SINGLE_MAX + 2]
    # one round exactly, a second round of one item, the last size of the single-workgroup scan, then the three-launch
    # scan with a last block of two wave counts
    assert w[-2] <= SCAN_SINGLE_MAX < w[-1] and w[-1] % SCAN_BLOCK == 2
    assert max(OCC_SIZES) * 2 < 5 << 20                         # bf16, C = 1: a few MB
    for D, shape in OCC_SHAPES.items():
        assert len(shape) == D + 1 and int(np.prod(shape)) % K_THREADS and int(np.prod(shape)) > K_THREADS
    assert 1 in OCC_SHAPES[7]


def test_inputs_tile_mutants_differ_from_the_oracle():
    """the walk without a mutant IS the oracle; each wrong kernel differs from it on the inputs of the GPU tests, except
    where it is right by construction: "one_pass" with C <= 64, "drop_partial" without a partial last tile (towards the
    rows also when no named cell lies in it), "o_of_first" when no tile spans several `o` or C == 1 (the stride between
    two `o` is then `inner`, the stride between two cells: the same address) — towards the rows also when every named
    cell lies in the `o` of its tile's first cell"""
    seen = set()
    for e in ELEMS:
        for outer, inner in SHAPES + HOLE_SHAPES:
            for C in CHANNELS:
                p = Move(e, outer, inner, C)
                cells, _ = _named(p.grid, p.n)
                for to_box in (True, False):
                    src = p.rows if to_box else p.box
                    want = p.want_box(CELL_STATIONARY) if to_box else p.want_rows(CELL_STATIONARY)[0]
                    assert np.array_equal(tile_walk(to_box, src, p.grid, p.n, outer, inner, C), want)
                    full = p.n_cells // K_T * K_T
                    other_o = cells // inner != (cells // K_T * K_T) // inner
                    coincide = {
                        "one_pass": C <= K_CC,
                        "drop_partial": p.n_cells % K_T == 0 or (not to_box and not (cells >= full).any()),
                        "o_of_first": C == 1 or not tiles_span_several_o(outer, inner) or (not to_box and not other_o.any()),
                    }
                    for mutant in TILE_MUTANTS:
                        wrong = tile_walk(to_box, src, p.grid, p.n, outer, inner, C, mutant)
                        assert np.array_equal(wrong, want) == coincide[mutant], (mutant, e, outer, inner, C, to_box)
                        seen.add((mutant, to_box, coincide[mutant]))
    assert {(m, t) for m, t, c in seen if not c} == {(m, t) for m in TILE_MUTANTS for t in (True, False)}
    # identity, where the walk takes row = cell
    for outer, inner, _ in PLACED_CASES:
        p = Move(4, outer, inner, 65, "identity")
        for to_box in (True, False):
            src = p.rows if to_box else p.box
            want = p.want_box(CELL_STATIONARY) if to_box else p.want_rows(CELL_STATIONARY)[0]
            assert np.array_equal(tile_walk(to_box, src, None, p.n, outer, inner, 65), want)
            assert np.array_equal(want, p.want_box(ROW_STATIONARY) if to_box else p.want_rows(ROW_STATIONARY)[0])


def test_inputs_index_and_occupancy_mutants_differ_from_the_oracle():
    # truncation: differs wherever a divisor above 1 meets a coordinate below min_coord (every index_case with rows
    # outside); equal by construction when all rows are inside or every divisor is 1 (divisor NULL)
    for D in range(1, 8):
        coords, mn, dv, shape = index_case(D, 257)
        assert max(dv) > 1 and 1 in shape[1:] or D == 1
        assert not np.array_equal(oracle_cell_index(coords, mn, dv, shape, "trunc")[0], oracle_cell_index(coords, mn, dv, shape)[0])
        assert np.array_equal(oracle_cell_index(coords, mn, None, shape, "trunc")[0], oracle_cell_index(coords, mn, None, shape)[0])
        coords, mn, dv, shape = index_case(D, 257, all_inside=True)
        cell, flag = oracle_cell_index(coords, mn, dv, shape)
        assert flag == 0 and (cell >= 0).all()
        assert np.array_equal(oracle_cell_index(coords, mn, dv, shape, "trunc")[0], cell)
    differ = [not np.array_equal(oracle_cell_index(*c, mutant="trunc")[0], oracle_cell_index(*c)[0]) for c in extreme_cases()]
    assert any(differ)
    # the extremes never wrap: every cell is -1 or below 9, both occur, and the exact floor 2 = (2^32 - 1) // (2^31 - 1) does
    cells = np.concatenate([oracle_cell_index(*c)[0] for c in extreme_cases()])
    assert set(cells.tolist()) <= set(range(-1, 9)) and (cells == -1).any() and (cells >= 0).any()
    assert (INT32_MAX - INT32_MIN) // INT32_MAX == 2 and (INT32_MIN - INT32_MAX) // INT32_MAX == -3
    for mn0 in (0, -3):
        coords, mn, dv, shape = far_corner_case(mn0)
        cell, flag = oracle_cell_index(coords, mn, dv, shape)
        assert cell.max() == (INT32_MAX - 1) * 255 + 254 > 2 ** 38 and flag == 1 and (cell >= 0).sum() == 5
    # -0 kept: differs wherever an empty cell holds a -0 word
    for e in ELEMS:
        for background in (0, SIGN[e]):
            box, where, kept = keep_rule_box(e, UINT[e](background))
            cells = oracle_occupied(box)
            assert {c: True for c in cells.tolist()} == {where[k]: True for k in where if kept[k]}
            assert not np.array_equal(oracle_occupied(box, "keep_minus_zero"), cells)
        for n_cells in OCC_SIZES[:7]:
            box = occupancy_box(2, 1, 1, n_cells, "half")
            differs = not np.array_equal(oracle_occupied(box, "keep_minus_zero"), oracle_occupied(box))
            empty_minus_zero = bool((box == SIGN[2]).any())
            assert differs == empty_minus_zero, n_cells           # (one cell: +0 or -0 or kept)
    box = occupancy_box(2, 1, 1, OCC_SIZES[-1], "half")
    assert not np.array_equal(oracle_occupied(box, "keep_minus_zero"), oracle_occupied(box))
    # the wave offset: the walk without a mutant gives the cells in order; with the inclusive offsets it differs whenever
    # a cell is kept at all (the first kept cell no longer lands at position 0)
    for n_cells in OCC_SIZES[:9]:
        for kind in ("half", "all", "none"):
            cells = oracle_occupied(occupancy_box(2, 1, 1, n_cells, kind))
            assert len(cells) == {"all": n_cells, "none": 0}.get(kind, len(cells))
            assert np.array_equal(fill_walk(cells, n_cells), cells)
            assert np.array_equal(fill_walk(cells, n_cells, "wave_offset"), cells) == (len(cells) == 0), (n_cells, kind)


# =====================================================================================================================
# device buffers and launches
# =====================================================================================================================
def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _put(keep, a, device, fill, off=0):
    """the address of a copy of the integer array `a` in the middle of a tensor of `fill`, `off` bytes behind a 16-byte
    boundary"""
    flat = np.ascontiguousarray(a).reshape(-1)
    e = flat.dtype.itemsize
    assert off % e == 0
    t = torch.from_numpy(flat.view(SINT[e]))
    big, mid = middle(t.numel() + off // e, TORCH_INT[e], device, _signed(fill, e) if fill >= 0 else fill)
    if t.numel():
        mid[off // e:].copy_(t)
    addr = big.data_ptr() + GUARD_PAD * e + off                 # (data_ptr() of an empty view is NULL)
    assert (addr - off) % 16 == 0
    keep.append(big)
    return addr


class Out:
    """n words of e bytes, `off` bytes behind a 16-byte boundary, inside a GuardedBytes; PRE in every word before a launch"""

    def __init__(self, n, e, device, off=0):
        assert n > 0 and off % e == 0
        self.e, self.off = e, off
        self.g = GuardedBytes(off + n * e, device)
        self.lead = self.g.bytes[:off]
        self.lead.fill_(0xc3)
        self.words = self.g.bytes[off:].view(TORCH_INT[e])
        self.fill()

    def fill(self, word=None):
        self.words.fill_(_signed(PRE[self.e] if word is None else word, self.e))

    def ptr(self):
        return self.g.ptr() + self.off

    def intact(self):
        return self.g.intact() and bool((self.lead == 0xc3).all())

    def get(self):
        return self.words.cpu().numpy().view(UINT[self.e]).copy()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = tuple(int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} words differ, e.g. {at}: "
                             f"{int(got[at]):#x} for {int(want[at]):#x}")


class OnDevice:
    """the inputs of a Move on the device, the box `off` bytes behind a 16-byte boundary"""

    def __init__(self, p, device, off=0):
        self.p, self.device, self.off, self.keep = p, device, off, []
        self.rows = _put(self.keep, p.rows, device, POISON[p.e])
        self.box = _put(self.keep, p.box, device, POISON[p.e], off)
        self.cell = _put(self.keep, p.cell, device, CELL_AROUND)
        self.grid = _put(self.keep, p.grid, device, p.n + 99)

    def _args(self, cell, grid):
        return self.cell if cell else None, self.grid if grid else None

    def to_box(self, policy, cell=True, grid=True, what=""):
        """me_dense_rows_to_box into a fresh box of PRE -> its words [outer, C, inner]; every one must have been written"""
        L, lib = _lib()
        p = self.p
        out = Out(p.n_cells * p.C, p.e, self.device, self.off)
        L.check(lib.me_dense_rows_to_box(self.rows, p.e, *self._args(cell, grid), p.n, p.outer, p.C, p.inner, out.ptr(),
                                         policy, None))
        torch.cuda.synchronize()
        assert out.intact(), f"{what}: rows_to_box wrote outside the box"
        got = out.get()
        left = int((got == UINT[p.e](PRE[p.e])).sum())
        assert left == 0, f"{what}: rows_to_box left {left} of {got.size} box elements unwritten"
        return got.reshape(p.outer, p.C, p.inner)

    def to_rows(self, policy, cell=True, grid=True, what=""):
        L, lib = _lib()
        p = self.p
        out = Out(p.n * p.C, p.e, self.device)
        L.check(lib.me_dense_box_to_rows(self.box, p.e, *self._args(cell, grid), p.n, p.outer, p.C, p.inner, out.ptr(),
                                         policy, None))
        torch.cuda.synchronize()
        assert out.intact(), f"{what}: box_to_rows wrote outside the rows"
        return out.get().reshape(p.n, p.C)


def check_both_policies(p, d, what, cell=True, grid=True):
    """both directions under both policies against the oracle; -> the four results"""
    res = {}
    for policy in (CELL_STATIONARY, ROW_STATIONARY):
        w = f"{what} policy {policy}"
        res["box", policy] = d.to_box(policy, cell, grid, w)
        same(res["box", policy], p.want_box(policy), w + ": box")
        if p.n:
            res["rows", policy] = d.to_rows(policy, cell, grid, w)
            want, _ = p.want_rows(policy)
            # cell-stationary: PRE in the rows the grid does not name; row-stationary: zeros there, nothing left of PRE
            same(res["rows", policy], want, w + ": rows")
    if p.n:
        _, named = p.want_rows(CELL_STATIONARY)
        same(res["rows", CELL_STATIONARY][named], res["rows", ROW_STATIONARY][named], what + ": the two policies, rows")
        assert not res["rows", ROW_STATIONARY][~named].any(), what + ": a row outside the box is not all zero"
    return res


# =====================================================================================================================
# the movers
# =====================================================================================================================
@pytest.mark.parametrize("e", ELEMS)
def test_movers_on_every_shape(device, e):
    """every shape at every box offset and C in {1, 64, 65, 129}: about half the cells occupied, rows in random order,
    rows outside the box (cell -1) among them"""
    for outer, inner in SHAPES:
        for C in CHANNELS:
            p = Move(e, outer, inner, C)
            assert (p.cell < 0).any() and p.n > (p.grid >= 0).sum() > 0
            boxes = []
            for off in offsets(e):
                what = f"{e}-byte ({outer}, {inner}) C {C} box at +{off} (mode {mode(inner, off)})"
                res = check_both_policies(p, OnDevice(p, device, off), what)
                # the two policies agree on the whole box here: no guarded index is involved
                same(res["box", CELL_STATIONARY], res["box", ROW_STATIONARY], what + ": the two policies, box")
                boxes.append(res["box", CELL_STATIONARY])
            assert all(np.array_equal(b, boxes[0]) for b in boxes)


@pytest.mark.parametrize("e", ELEMS)
def test_movers_every_channel_count_in_every_mode(device, e):
    for outer, inner, off in MODE_CASES:
        for C in ALL_CHANNELS:
            for kind in ("half", "perm"):
                p = Move(e, outer, inner, C, kind)
                check_both_policies(p, OnDevice(p, device, off), f"{e}-byte ({outer}, {inner}) C {C} +{off} {kind}")


@pytest.mark.parametrize("e", ELEMS)
def test_movers_grid_contents(device, e):
    """every cell occupied in a random row order, half of them, none (rows -> box only: all zeros, all written), an empty
    tile between occupied ones (the zero path that skips the barriers), only the first cell, only the last cell"""
    cases = [(o, i, off) for o, i, off in MODE_CASES] + [(o, i, 0) for o, i in HOLE_SHAPES] + [HOLE_SHAPES[0] + (8,)]
    for outer, inner, off in cases:
        for kind in GRID_KINDS:
            if kind == "hole" and outer * inner < 3 * K_T:
                continue
            for C in (65, 3):
                p = Move(e, outer, inner, C, kind)
                what = f"{e}-byte ({outer}, {inner}) C {C} +{off} {kind}"
                if kind == "hole":
                    assert (p.grid[:K_T] >= 0).any() and (p.grid[K_T:2 * K_T] < 0).all() and (p.grid[2 * K_T:3 * K_T] >= 0).any()
                if kind == "perm":
                    assert (p.grid >= 0).all() and not np.array_equal(p.cell, np.arange(p.n))
                res = check_both_policies(p, OnDevice(p, device, off), what)
                if kind == "empty":
                    assert p.n == 0 and not res["box", CELL_STATIONARY].any() and not res["box", ROW_STATIONARY].any()


@pytest.mark.parametrize("e", ELEMS)
def test_policy_zero(device, e):
    """policy 0 is cell-stationary when the grid is given and row-stationary when only `cell` is: told apart by the rows
    outside the box, which only the row-stationary gather zeroes, and by a grid that names other rows than `cell`"""
    for outer, inner, off in PLACED_CASES:
        p = Move(e, outer, inner, 65)
        d = OnDevice(p, device, off)
        what = f"{e}-byte ({outer}, {inner}) +{off}"
        for cell in (True, False):
            same(d.to_rows(0, cell, True, what), p.want_rows(CELL_STATIONARY)[0], what + f" policy 0 with the grid, cell {cell}")
            same(d.to_box(0, cell, True, what), p.want_box(CELL_STATIONARY), what + " policy 0 with the grid")
        same(d.to_rows(0, True, False, what), p.want_rows(ROW_STATIONARY)[0], what + " policy 0 with cell only")
        same(d.to_box(0, True, False, what), p.want_box(ROW_STATIONARY), what + " policy 0 with cell only")
        assert not np.array_equal(p.want_rows(CELL_STATIONARY)[0], p.want_rows(ROW_STATIONARY)[0])
        # a grid that disagrees with `cell` (two rows swapped): the box says which of the two was used
        g = p.grid.copy()
        a, b = np.flatnonzero(g >= 0)[[0, -1]]
        g[[a, b]] = g[[b, a]]
        q = Move(e, outer, inner, 65, cell=p.cell, grid=g)
        dq = OnDevice(q, device, off)
        assert not np.array_equal(q.want_box(CELL_STATIONARY), q.want_box(ROW_STATIONARY))
        same(dq.to_box(0, True, True, what), q.want_box(CELL_STATIONARY), what + " policy 0, swapped grid")
        same(dq.to_box(0, True, False, what), q.want_box(ROW_STATIONARY), what + " policy 0, swapped grid, cell only")


@pytest.mark.parametrize("e", ELEMS)
def test_identity(device, e):
    """cell = grid = NULL, n = outer * inner: row r is cell r — as the explicit identity grid gives it, in all three modes,
    under both policies and policy 0, in both directions"""
    for outer, inner, off in PLACED_CASES:
        for C in (65, 1):
            p = Move(e, outer, inner, C, "identity")
            assert p.n == p.n_cells and np.array_equal(p.grid, np.arange(p.n))
            d = OnDevice(p, device, off)
            what = f"{e}-byte identity ({outer}, {inner}) C {C} +{off} (mode {mode(inner, off)})"
            explicit = check_both_policies(p, d, what + " explicit")
            implicit = check_both_policies(p, d, what + " NULL", cell=False, grid=False)
            for key in explicit:
                same(implicit[key], explicit[key], f"{what}: {key}")
            same(d.to_box(0, False, False, what), explicit["box", CELL_STATIONARY], what + " policy 0")
            same(d.to_rows(0, False, False, what), explicit["rows", CELL_STATIONARY], what + " policy 0")
            want = p.rows.reshape(outer, inner, C).transpose(0, 2, 1)
            same(explicit["box", CELL_STATIONARY], want, what + ": the transpose")


@pytest.mark.parametrize("e", ELEMS)
def test_row_stationary_ignores_cells_outside_the_box(device, e):
    """cell[r] in {-1, n_cells, n_cells + 5, 2^40} — the values k_row_move and k_grid_scatter check themselves: towards the
    box nothing is written for them, towards the rows they give zeros and the box is not read outside (it lies in NaN-bit
    poison, which no data word equals); me_dense_grid ignores them and writes every entry of the grid"""
    L, lib = _lib()
    for outer, inner, off in PLACED_CASES:
        for C in (65, 3):
            base = Move(e, outer, inner, C)
            cell = base.cell.copy()
            n_cells = base.n_cells
            outside = np.flatnonzero(cell < 0)
            extra = np.array([-1, n_cells, n_cells + 5, 1 << 40] * 2, np.int64)
            cell = np.concatenate([cell, extra])[_rng(4, e, outer, inner, C).permutation(len(cell) + len(extra))]
            p = Move(e, outer, inner, C, cell=cell)
            assert len(outside) and {-1, n_cells, n_cells + 5, 1 << 40} <= set(p.cell.tolist())
            d = OnDevice(p, device, off)
            what = f"{e}-byte ({outer}, {inner}) C {C} +{off}, cells outside"
            same(d.to_box(ROW_STATIONARY, True, False, what), p.want_box(ROW_STATIONARY), what + ": box")
            rows = d.to_rows(ROW_STATIONARY, True, False, what)
            same(rows, p.want_rows(ROW_STATIONARY)[0], what + ": rows")
            bad = (p.cell < 0) | (p.cell >= n_cells)
            assert not rows[bad].any() and not (rows == UINT[e](POISON[e])).any()
            # the grid of these cells
            g = Out(n_cells, 4, device)
            L.check(lib.me_dense_grid(d.cell, p.n, n_cells, g.ptr(), None))
            torch.cuda.synchronize()
            assert g.intact()
            same(g.get().view(np.int32), p.grid, what + ": grid")
            assert (p.grid == -1).any() and (p.grid >= 0).any()


@pytest.mark.parametrize("e", ELEMS)
def test_cell_stationary_takes_bad_grid_entries_as_empty(device, e):
    """grid[cell] in {-1, -7, n, n + 3} — what tile_setup checks itself — counts as empty: zeros in the box, no row written"""
    for outer, inner, off in PLACED_CASES:
        for C in (65, 3):
            occ = np.flatnonzero(np.arange(outer * inner) % 3 != 1)        # two cells of three, and two rows outside
            base = Move(e, outer, inner, C, cell=_rng(6, e, outer, inner, C).permutation(np.concatenate([occ, [-1, -1]])))
            g = base.grid.copy()
            empty = np.flatnonzero(g < 0)
            occupied = np.flatnonzero(g >= 0)
            bad = [-1, -7, base.n, base.n + 3]
            assert len(empty) >= 2 and len(occupied) >= 4
            g[empty[:2]] = [-7, base.n + 3]
            g[occupied[:4]] = bad                                 # their rows are no longer named
            p = Move(e, outer, inner, C, cell=base.cell, grid=g)
            d = OnDevice(p, device, off)
            what = f"{e}-byte ({outer}, {inner}) C {C} +{off}, bad grid entries"
            box = d.to_box(CELL_STATIONARY, False, True, what)
            same(box, p.want_box(CELL_STATIONARY), what + ": box")
            for c in np.concatenate([empty[:2], occupied[:4]]):
                assert not box[c // inner, :, c % inner].any()
            rows = d.to_rows(CELL_STATIONARY, False, True, what)
            want, named = p.want_rows(CELL_STATIONARY)
            same(rows, want, what + ": rows")
            assert (rows[~named] == UINT[e](PRE[e])).all() and (~named).sum() >= 4 + (base.cell < 0).sum()
            # n larger than the number of named rows, and smaller than some grid entries: n - 2 rows
            q = Move(e, outer, inner, C, cell=base.cell[:-2], grid=base.grid)
            dq = OnDevice(q, device, off)
            same(dq.to_box(CELL_STATIONARY, False, True, what), q.want_box(CELL_STATIONARY), what + ": box, n - 2 rows")
            same(dq.to_rows(CELL_STATIONARY, False, True, what), q.want_rows(CELL_STATIONARY)[0], what + ": rows, n - 2 rows")


@pytest.mark.parametrize("e", ELEMS)
def test_movers_twice(device, e):
    for outer, inner, off in MODE_CASES:
        p = Move(e, outer, inner, 129)
        d = OnDevice(p, device, off)
        for policy in (CELL_STATIONARY, ROW_STATIONARY):
            same(d.to_box(policy), d.to_box(policy), f"{e}-byte ({outer}, {inner}) policy {policy}: two launches, box")
            same(d.to_rows(policy), d.to_rows(policy), f"{e}-byte ({outer}, {inner}) policy {policy}: two launches, rows")


# =====================================================================================================================
# me_dense_cell_index and me_dense_grid
# =====================================================================================================================
def _i32(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


def _i64(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


def run_cell_index(device, coords, mn, dv, shape, n=None):
    """-> (cell [n] int64, flag); cell and flag are guarded, the flag holds 7 before the launch"""
    L, lib = _lib()
    n = len(coords) if n is None else n
    keep = []
    a = _put(keep, coords, device, INT32_MAX)
    cell, flag = Out(max(n, 1), 8, device), Out(1, 4, device)
    flag.fill(7)
    L.check(lib.me_dense_cell_index(a, n, len(shape), _i32(mn), _i32(dv), _i64(shape), cell.ptr(), flag.ptr(), None))
    torch.cuda.synchronize()
    assert cell.intact() and flag.intact(), "me_dense_cell_index wrote outside cell or flag"
    got = cell.get()
    if n == 0:
        assert (got == UINT[8](PRE[8])).all()
    return got.view(np.int64)[:n], int(flag.get().view(np.int32)[0])


def check_cell_index(device, coords, mn, dv, shape, what):
    cell, flag = run_cell_index(device, coords, mn, dv, shape)
    want, want_flag = oracle_cell_index(coords, mn, dv, shape)
    same(cell, want, what + ": cell")
    assert flag == want_flag, (what, flag, want_flag)
    return want


@pytest.mark.parametrize("D", range(1, 8))
def test_cell_index_floor_on_either_side(device, D):
    L, lib = _lib()
    coords, mn, dv, shape = index_case(D, 257)
    want = check_cell_index(device, coords, mn, dv, shape, f"D {D}")
    assert (want >= 0).any() and (want < 0).any()
    check_cell_index(device, coords, mn, None, shape, f"D {D} divisor NULL")
    check_cell_index(device, coords, None, dv, shape, f"D {D} min_coord NULL")
    check_cell_index(device, coords, None, None, shape, f"D {D} both NULL")
    inside = index_case(D, 257, all_inside=True)
    want = check_cell_index(device, *inside, f"D {D} all inside")                       # the flag is cleared from 7 to 0
    # the grid of the inside rows (duplicates among random rows: unique cells only, as the header requires)
    _, first = np.unique(want, return_index=True)
    cell = np.where(np.isin(np.arange(len(want)), first), want, -1)
    n_cells = int(np.prod(inside[3]))
    keep = []
    g = Out(n_cells, 4, device)
    L.check(lib.me_dense_grid(_put(keep, cell, device, CELL_AROUND), len(cell), n_cells, g.ptr(), None))
    torch.cuda.synchronize()
    assert g.intact()
    same(g.get().view(np.int32), oracle_grid(cell, n_cells), f"D {D}: grid")


def test_cell_index_rows_on_the_block_edge_and_the_flag(device):
    for n in INDEX_ROWS:
        for all_inside in (False, True):
            coords, mn, dv, shape = index_case(3, n, all_inside)
            assert len(coords) == n
            check_cell_index(device, coords, mn, dv, shape, f"n {n} inside {all_inside}")
    # one row outside, as the last of 257
    coords, mn, dv, shape = index_case(3, 257, True)
    coords[-1, 0] = shape[0]
    want = check_cell_index(device, coords, mn, dv, shape, "the last row outside")
    assert want[-1] == -1 and (want[:-1] >= 0).all()
    # n = 0 clears the flag and writes no cell
    cell, flag = run_cell_index(device, coords, mn, dv, shape, n=0)
    assert flag == 0 and len(cell) == 0
    # an extent of 0: every row is outside
    for k in range(4):
        zero = list(shape)
        zero[k] = 0
        cell, flag = run_cell_index(device, coords, mn, dv, zero)
        assert flag == 1 and (cell == -1).all(), k


def test_cell_index_int32_extremes(device):
    for coords, mn, dv, shape in extreme_cases():
        check_cell_index(device, coords, mn, dv, shape, f"min_coord {mn} divisor {dv}")


def test_cell_index_far_corner_of_a_2_to_39_box(device):
    for mn0 in (0, -3):
        coords, mn, dv, shape = far_corner_case(mn0)
        want = check_cell_index(device, coords, mn, dv, shape, f"shape {shape} min_coord {mn}")
        assert want.max() > 2 ** 38


# =====================================================================================================================
# me_dense_occupied_count / me_dense_occupied_fill
# =====================================================================================================================
WS_WORD = 0xdeadbeef


def run_occupied(device, box, shape, what):
    """count into a poisoned workspace of exactly the bytes asked for, the count against the oracle's BEFORE anything is
    filled, then fill into exactly sized guarded buffers -> (coords [count, D + 1], cell [count])"""
    L, lib = _lib()
    outer, C, inner = box.shape
    e = box.dtype.itemsize
    n_cells = outer * inner
    assert int(np.prod(shape)) == n_cells
    want = oracle_occupied(box)
    keep = []
    a = _put(keep, box, device, POISON[e])
    ws_bytes = int(lib.me_dense_occupied_workspace_bytes(n_cells))
    ws = GuardedBytes(ws_bytes, device)
    ws.fill(WS_WORD)
    cnt = ctypes.c_int64(-5)
    L.check(lib.me_dense_occupied_count(a, e, outer, C, inner, ws.ptr(), ws_bytes, ctypes.byref(cnt), None))
    torch.cuda.synchronize()
    assert ws.intact(), f"{what}: the count wrote outside its workspace"
    assert cnt.value == len(want), f"{what}: {cnt.value} occupied cells counted, {len(want)} expected"
    count, ncol = len(want), len(shape)
    rows = max(count, 1)                                        # (no row: one spare row that must stay untouched)
    coords, cell = Out(rows * ncol, 4, device), Out(rows, 8, device)
    L.check(lib.me_dense_occupied_fill(ws.ptr(), ws_bytes, ncol, _i64(shape), coords.ptr(), cell.ptr(), None))
    torch.cuda.synchronize()
    assert ws.intact() and coords.intact() and cell.intact(), f"{what}: the fill wrote outside a buffer"
    got_coords, got_cell = coords.get().view(np.int32).reshape(rows, ncol), cell.get().view(np.int64)
    if count == 0:
        assert (got_coords == np.int32(PRE32)).all() and (got_cell == _signed(PRE[8], 8)).all(), what
    same(got_cell[:count], want, what + ": cells")
    same(got_coords[:count], oracle_coords(want, shape), what + ": coordinates")
    return got_coords[:count], got_cell[:count]


@pytest.mark.parametrize("n_cells", OCC_SIZES)
def test_occupied_wave_block_and_scan_edges(device, n_cells):
    """bf16, C = 1, about half the cells kept, +0 and -0 in the others; twice, with the same bits"""
    box = occupancy_box(2, 1, 1, n_cells, "half")
    first = run_occupied(device, box, (1, n_cells), f"{n_cells} cells")
    again = run_occupied(device, box, (1, n_cells), f"{n_cells} cells, again")
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("n_cells", OCC_EXTREMES)
def test_occupied_all_kept_and_all_empty(device, n_cells):
    for kind, count in (("all", n_cells), ("none", 0)):
        box = occupancy_box(2, 1, 1, n_cells, kind)
        _, cell = run_occupied(device, box, (n_cells, 1), f"{n_cells} cells, {kind}")
        assert len(cell) == count


@pytest.mark.parametrize("e", ELEMS)
def test_occupied_keep_rule(device, e):
    """all bits but the sign, word by word: the deciding word in channel 0 only, in the last channel only, in every channel"""
    for background in (0, SIGN[e]):
        box, where, kept = keep_rule_box(e, UINT[e](background))
        _, cell = run_occupied(device, box, (3, 40), f"{e}-byte keep rule on {background:#x}")
        got = set(cell.tolist())
        for key, c in where.items():
            assert (c in got) == kept[key], (e, background, key)
        assert got == {where[k] for k in where if kept[k]}


@pytest.mark.parametrize("e", ELEMS)
def test_occupied_inner_and_dimensions(device, e):
    """a cell's channels `inner` apart, waves across `o`; coordinates for D = 1, 3 and 7"""
    for inner in OCC_INNER:
        for outer, C in ((7, 3), (131, 2)):
            box = occupancy_box(e, outer, C, inner, "half")
            run_occupied(device, box, (outer, inner), f"{e}-byte ({outer}, {C}, {inner})")
    for D, shape in OCC_SHAPES.items():
        n_cells = int(np.prod(shape))
        for outer, inner in ((shape[0], n_cells // shape[0]), (n_cells, 1)):
            box = occupancy_box(e, outer, 3, inner, "half", key=D)
            coords, _ = run_occupied(device, box, shape, f"{e}-byte D {D} ({outer}, 3, {inner})")
            assert coords.shape[1] == D + 1 and len(coords) > K_THREADS // 2


# =====================================================================================================================
# me_dense_all_coords
# =====================================================================================================================
def check_all_coords(device, shape):
    L, lib = _lib()
    n_cells = int(np.prod(shape))
    out = Out(n_cells * len(shape), 4, device)
    L.check(lib.me_dense_all_coords(len(shape), _i64(shape), out.ptr(), None))
    torch.cuda.synchronize()
    assert out.intact(), f"{shape}: me_dense_all_coords wrote outside its output"
    same(out.get().view(np.int32).reshape(n_cells, len(shape)), oracle_coords(np.arange(n_cells), shape), f"{shape}")


def test_all_coords(device):
    for D in range(1, 8):
        rng = _rng(5, D)
        ext = rng.integers(2, 5, D).tolist()
        if D >= 2:
            ext[int(rng.integers(D))] = 1
        check_all_coords(device, [3] + ext)
        check_all_coords(device, [1] * (D + 1))
        check_all_coords(device, [2] + [1] * (D - 1) + [5])
    for n_cells in COORD_N_CELLS:
        check_all_coords(device, (n_cells, 1))
        check_all_coords(device, (1, n_cells))
        check_all_coords(device, (1, 1, n_cells, 1))
    check_all_coords(device, (1, 1, 70001))
    check_all_coords(device, (3, 17, 1, 19))


# =====================================================================================================================
# argument checks
# =====================================================================================================================
def test_argument_checks_leave_the_outputs_untouched(device):
    """refused in the library's own checks, before any launch and any fill: an error through _lib.check, nothing written.
    The sizes are arguments only: nothing of that size exists"""
    L, lib = _lib()
    e, outer, inner, C = 4, 3, 20, 5
    p = Move(e, outer, inner, C)
    d = OnDevice(p, device)
    ident = Move(e, outer, inner, C, "identity")
    di = OnDevice(ident, device)
    box, rows = Out(p.n_cells * C, e, device), Out(max(ident.n, p.n) * C, e, device)
    coords, mn, dv, shape = index_case(3, 40)
    keep = []
    a_coords = _put(keep, coords, device, INT32_MAX)
    cell, flag, grid = Out(40, 8, device), Out(1, 4, device), Out(p.n_cells, 4, device)
    occ_coords, occ_cell = Out(p.n_cells * 2, 4, device), Out(p.n_cells, 8, device)
    ws_bytes = int(lib.me_dense_occupied_workspace_bytes(p.n_cells))
    ws = GuardedBytes(ws_bytes, device)
    outs = (box, rows, cell, flag, grid, occ_coords, occ_cell)

    def refused(name, rc):
        with pytest.raises(RuntimeError):
            L.check(rc)
        torch.cuda.synchronize()
        for o in outs:
            assert o.intact() and (o.get() == UINT[o.e](PRE[o.e])).all(), f"{name}: refused, yet something was written"
        assert ws.holds(WS_WORD) and ws.intact(), f"{name}: refused, yet the workspace was written"

    def move(to_box=True, elem=e, cell=d.cell, grid=d.grid, n=p.n, outer=outer, c=C, inner=inner, policy=0, rows_in=d.rows):
        if to_box:
            return lib.me_dense_rows_to_box(rows_in, elem, cell, grid, n, outer, c, inner, box.ptr(), policy, None)
        return lib.me_dense_box_to_rows(d.box, elem, cell, grid, n, outer, c, inner, rows.ptr(), policy, None)

    def index(ncol=4, mn=mn, dv=dv, shape=shape, flag_ptr=flag.ptr()):
        return lib.me_dense_cell_index(a_coords, 40, ncol, _i32(mn), _i32(dv), _i64(shape), cell.ptr(), flag_ptr, None)

    cnt = ctypes.c_int64(0)

    def count(elem=e, outer=outer, inner=inner, c=C, wsb=ws_bytes):
        return lib.me_dense_occupied_count(d.box, elem, outer, c, inner, ws.ptr(), wsb, ctypes.byref(cnt), None)

    def fill(ncol=2, shape=(outer, inner), wsb=ws_bytes):
        return lib.me_dense_occupied_fill(ws.ptr(), wsb, ncol, _i64(shape), occ_coords.ptr(), occ_cell.ptr(), None)

    ws.fill(WS_WORD)
    for to_box in (True, False):
        t = "to_box" if to_box else "to_rows"
        for name, over in (("elem_bytes 3", dict(elem=3)), ("policy -1", dict(policy=-1)), ("policy 3", dict(policy=3)),
                           ("c = 0", dict(c=0)), ("inner = 0", dict(inner=0)), ("n < 0", dict(n=-1)),
                           ("identity with n != outer * inner", dict(cell=None, grid=None, n=ident.n - 1, rows_in=di.rows)),
                           ("identity with n != outer * inner, row-stationary",
                            dict(cell=None, grid=None, n=ident.n + 1, rows_in=di.rows, policy=ROW_STATIONARY)),
                           ("cell-stationary without a grid", dict(grid=None, policy=CELL_STATIONARY)),
                           ("row-stationary without cell", dict(cell=None, policy=ROW_STATIONARY)),
                           ("outer * inner = 2^40", dict(outer=1 << 20, inner=1 << 20)),
                           ("outer * inner = 2^40, inner 1", dict(outer=1 << 40, inner=1))):
            refused(f"{t} {name}", move(to_box, **over))
    for name, over in (("ncol 1", dict(ncol=1)), ("ncol 9", dict(ncol=9)), ("shape NULL", dict(shape=None)),
                       ("a divisor of 0", dict(dv=[1, 0, 1])), ("a negative divisor", dict(dv=[1, 1, -2])),
                       ("an extent of -1", dict(shape=[2, 3, -1, 4])), ("an extent of 2^31", dict(shape=[2, 1 << 31, 1, 1])),
                       ("2^40 cells", dict(shape=[1 << 10, 1 << 10, 1 << 10, 1 << 10])), ("flag_dev NULL", dict(flag_ptr=None))):
        refused("cell_index " + name, index(**over))
    refused("grid n < 0", lib.me_dense_grid(d.cell, -1, p.n_cells, grid.ptr(), None))
    refused("grid n_cells < 0", lib.me_dense_grid(d.cell, p.n, -1, grid.ptr(), None))
    for name, over in (("2^31 cells", dict(outer=1 << 31, inner=1)), ("2^31 cells, inner 2^16", dict(outer=1 << 15, inner=1 << 16)),
                       ("a workspace one byte short", dict(wsb=ws_bytes - 1)), ("elem_bytes 3", dict(elem=3)),
                       ("c = 0", dict(c=0)), ("inner = 0", dict(inner=0))):
        refused("occupied_count " + name, count(**over))
    for name, over in (("a workspace one byte short", dict(wsb=ws_bytes - 1)), ("2^31 cells", dict(shape=(2, 1 << 30))),
                       ("ncol 1", dict(ncol=1, shape=(outer * inner,))), ("shape NULL", dict(shape=None))):
        refused("occupied_fill " + name, fill(**over))
    for name, shp in (("2^31 cells", (2, 1 << 30)), ("2^33 cells", (8, 1 << 30)), ("an extent of 2^31", (1, 1 << 31))):
        refused("all_coords " + name, lib.me_dense_all_coords(len(shp), _i64(shp), occ_coords.ptr(), None))
    refused("all_coords ncol 9", lib.me_dense_all_coords(9, _i64([1] * 9), occ_coords.ptr(), None))
    # ... and the same arguments, unchanged, run
    L.check(move(True))
    L.check(move(False, n=p.n))
    L.check(index())
    L.check(count())
    L.check(fill())
    torch.cuda.synchronize()
    same(box.get().reshape(outer, C, inner), p.want_box(CELL_STATIONARY), "good arguments: box")
    same(rows.get()[:p.n * C].reshape(p.n, C), p.want_rows(CELL_STATIONARY)[0], "good arguments: rows")
    same(cell.get().view(np.int64), oracle_cell_index(coords, mn, dv, shape)[0], "good arguments: cell")
    want = oracle_occupied(p.box)
    assert cnt.value == len(want)
    same(occ_cell.get().view(np.int64)[:len(want)], want, "good arguments: occupied cells")
    assert all(o.intact() for o in outs) and ws.intact()
