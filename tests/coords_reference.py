"""Plain numpy restatements of what csrc/coords.hip documents, for tests/test_gpu_coords_kernels.py (the GPU side) and
tests/test_coords_reference_cpu.py (which checks these functions on their own).  Nothing here calls the library: every
function is written from include/me_amd.h and the comments above the kernels."""
import numpy as np


def key_bits(D):
    """bits per axis of the Z-order key: min(21, 56 // D)"""
    return min(21, 56 // D)


def morton_keys(coords, tensor_stride):
    """me_coords_spatial_keys: batch & 0x7f at bit 56; bit b of axis d at position b * D + d; the value of an axis is
    floor(c / ts) + 2^(bits - 1), masked to `bits` bits.  -> uint64 [n]"""
    c = np.asarray(coords, np.int64)
    D = c.shape[1] - 1
    bits = key_bits(D)
    key = ((c[:, 0] & 0x7f) << 56).astype(np.uint64)
    for d in range(D):
        v = (np.floor_divide(c[:, 1 + d], int(tensor_stride[d])) + (1 << (bits - 1))) & ((1 << bits) - 1)
        for b in range(bits):
            key |= (((v >> b) & 1) << (b * D + d)).astype(np.uint64)
    return key


def zorder_passes(bbox, tensor_stride, D):
    """The 8-bit digit positions me_coords_zorder sorts for a bounding box (column minima, then maxima; None: unknown),
    and which of its branches every axis takes ("plain", "wrap": a > b, "wide": hi - lo >= mask) — restated so that a
    test can assert that its box reaches the branch it names.  -> (list of shifts, list of branch names)"""
    kbits = key_bits(D)
    ncol = D + 1
    span, batch_varies, branches = kbits * D, True, []
    if bbox is not None:
        bias, mask = 1 << (kbits - 1), (1 << kbits) - 1
        top = 0
        for d in range(D):
            lo, hi = int(bbox[1 + d]) // int(tensor_stride[d]), int(bbox[ncol + 1 + d]) // int(tensor_stride[d])
            if hi - lo >= mask:
                top = kbits
                branches.append("wide")
                continue
            a, b = (lo + bias) & mask, (hi + bias) & mask
            branches.append("plain" if a <= b else "wrap")
            x = (a ^ b) if a <= b else mask
            top = max(top, x.bit_length())
        span = top * D
        batch_varies = int(bbox[0]) != int(bbox[ncol])
    shifts = list(range(0, span, 8))
    if batch_varies:
        shifts.append(56)
    if not shifts:
        shifts.append(0)
    return shifts, branches


def first_occurrence(coords):
    """me_coords_insert_and_map: the FIRST input row of a coordinate wins, unique rows keep the order of their first
    occurrence.  -> (unique_map int64 [n_unique], inverse_map int64 [n])"""
    c = np.ascontiguousarray(np.asarray(coords, np.int32))
    n = c.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, inv = np.unique(c, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    rank = np.empty(len(first), np.int64)           # unique rows numbered by their first input row
    by_first = np.argsort(first, kind="stable")
    rank[by_first] = np.arange(len(first))
    return first[by_first].astype(np.int64), rank[inv].astype(np.int64)


def bounding_box(coords):
    """column minima, then maxima (me_coords_insert_and_map_bbox); all zeros for no rows"""
    c = np.asarray(coords, np.int64)
    if c.shape[0] == 0:
        return np.zeros(2 * c.shape[1], np.int64)
    return np.concatenate((c.min(0), c.max(0)))


def supercell_keys(coords, shift, sc_min, sc_dim, tensor_stride):
    """Linear supercell index of every row on a me_spatial_grid: batch - sc_min[0], then per axis
    (floor(c / ts) >> shift) - sc_min[1 + d], row-major over sc_dim.  Rows outside the directory raise."""
    c = np.asarray(coords, np.int64)
    D = c.shape[1] - 1
    lin = c[:, 0] - int(sc_min[0])
    assert ((lin >= 0) & (lin < int(sc_dim[0]))).all(), "batch index outside the directory"
    for d in range(D):
        sc = (np.floor_divide(c[:, 1 + d], int(tensor_stride[d])) >> int(shift[d])) - int(sc_min[1 + d])
        assert ((sc >= 0) & (sc < int(sc_dim[1 + d]))).all(), f"axis {d} outside the directory"
        lin = lin * int(sc_dim[1 + d]) + sc
    return lin


def grid_of(coords, shift, tensor_stride, margin_lo=0, margin_hi=0):
    """(shift, sc_min, sc_dim, ts) lists of the hosts' grid rule on the bounding box of `coords`: sc_min = (min // ts)
    >> shift, sc_dim = the supercells up to (max // ts) >> shift; `margin_*` widen every spatial axis by that many EMPTY
    supercells on the low / high side."""
    c = np.asarray(coords, np.int64)
    D = c.shape[1] - 1
    sh = [int(shift)] * D if np.isscalar(shift) else [int(s) for s in shift]
    ts = [int(tensor_stride)] * D if np.isscalar(tensor_stride) else [int(t) for t in tensor_stride]
    sc_min, sc_dim = [int(c[:, 0].min())], [int(c[:, 0].max() - c[:, 0].min()) + 1]
    for d in range(D):
        lo = (int(c[:, 1 + d].min()) // ts[d]) >> sh[d]
        hi = (int(c[:, 1 + d].max()) // ts[d]) >> sh[d]
        sc_min.append(lo - margin_lo)
        sc_dim.append(hi - lo + 1 + margin_lo + margin_hi)
    return sh, sc_min, sc_dim, ts


def spatial_index(coords, shift, sc_min, sc_dim, tensor_stride):
    """me_spatial_index_build: order = the stable argsort of the supercell keys, pos_of_row its inverse, dir_start the
    exclusive prefix of the key histogram with dir_start[m] = n.  -> (order, pos_of_row, dir_start) int64"""
    key = supercell_keys(coords, shift, sc_min, sc_dim, tensor_stride)
    m = int(np.prod([int(v) for v in sc_dim]))
    order = np.argsort(key, kind="stable")
    pos = np.empty(len(key), np.int64)
    pos[order] = np.arange(len(key))
    dir_start = np.concatenate(([0], np.cumsum(np.bincount(key, minlength=m)))).astype(np.int64)
    return order, pos, dir_start


def pair_lists(nbr, out_rows=None):
    """Per-offset pair lists of a neighbour table nbr [volume, n]: offset k holds its hits in ascending column order;
    the `out` entry of column u is out_rows[u] (None: u).  -> (in_pairs, out_pairs, k_offsets int64 [volume + 1])"""
    nbr = np.asarray(nbr)
    ins, outs, koffs = [], [], [0]
    for k in range(nbr.shape[0]):
        u = np.nonzero(nbr[k] >= 0)[0]
        ins.append(nbr[k, u])
        outs.append(u if out_rows is None else np.asarray(out_rows)[u])
        koffs.append(koffs[-1] + len(u))
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)  # noqa: E731
    return cat(ins), cat(outs), np.asarray(koffs, np.int64)


def transposed_table(in_pairs, out_pairs, k_offsets, n_in, pos_in=None):
    """nbrT [volume, n_in]: nbrT[k, pos_in[in row]] = out row of the pair (pos_in None: the row itself), -1 elsewhere"""
    volume = len(k_offsets) - 1
    t = np.full((volume, n_in), -1, np.int32)
    for k in range(volume):
        i = np.asarray(in_pairs[k_offsets[k]:k_offsets[k + 1]], np.int64)
        t[k, i if pos_in is None else np.asarray(pos_in)[i]] = out_pairs[k_offsets[k]:k_offsets[k + 1]]
    return t
