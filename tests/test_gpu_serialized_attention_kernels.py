"""Entry-point tests of serialized patch attention (csrc/serial_attention.hip and the _tab entry points of
csrc/attention.hip, ABI 1.19) through the C ABI on synthetic device tensors: no manager, no SparseTensor.

A. me_coords_serial_keys against `serial_code` of tests/test_serialized_attention_cpu.py: the uint64 keys themselves, at
   the widest legal codes, with batch bits above the code, at depth 0, with a negative bbox_min and per-axis strides, and
   with an extent of 2^31 or more under a stride that is no power of two.
B. me_attn_patch_lists against `row_patches`: deep keys over several sort tiles, the shortest sort, stability across tiles,
   the scan pipeline beyond one block, many instances with sparse batch indices, more instances than rows, patch-size edges,
   an empty map, a repeated call.  Every list call goes through `patch_lists`: outputs pre-filled with -7, a workspace of
   exactly the size asked for, pre-filled with 0xA5 and followed by a guard, a guard tail behind every output.
C. me_attn_forward_tab / me_attn_backward_tab on hand-built lists and tables (a window partition that no curve made, with
   empty segments; distinct partitions of the q and the kv side; a table with its entries permuted).

A and B compare integers exactly.  C compares the table path with the walk (null tables) bit for bit and holds both to the
rule of tests/test_gpu_attention_kernels.py: E_kernel <= FACTOR * E_torch per tensor against the float64 `reference`, every
figure printed before it is asserted (pytest -s).  Measured maxima: DESIGN 8.13."""
import ctypes
import math

import numpy as np
import pytest
import torch

from minkowskiengine_amd import _lib
from test_gpu_attention_kernels import draw, within_bound   # (within_bound: `reference`, `torch_attention` and FACTOR)
from test_serialized_attention_cpu import ORDERS, row_patches, serial_code, serial_geometry, serial_keys

pytestmark = pytest.mark.gpu

GUARD = 64            # elements behind every output
WS_GUARD = 4096       # bytes behind the workspace
FILL = -7


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _side_stream(dev):
    """a non-default stream that starts after everything queued so far"""
    torch.cuda.synchronize(dev)
    return torch.cuda.Stream(dev)


# ---- A. keys -------------------------------------------------------------------------------------------------------------------
def gpu_keys(coords, ts, lo, depth, order, dev, stream=None):
    """me_coords_serial_keys on an int array [n, 1 + D] -> np.uint64 [n]; the 64 elements behind the keys stay untouched"""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    n, ncol = coords.shape
    c = torch.from_numpy(coords).to(dev)
    keys = torch.full((n + GUARD,), FILL, dtype=torch.int64, device=dev)
    if stream is not None:
        torch.cuda.synchronize(dev)
    _lib.check(lib.me_coords_serial_keys(_ptr(c), n, ncol, _i32s(ts), _i32s(lo), depth, ORDERS.index(order), _ptr(keys),
                                         stream.cuda_stream if stream is not None else None))
    torch.cuda.synchronize(dev)
    out = keys.cpu().numpy()
    assert (out[n:] == FILL).all(), "the keys were written past their end"
    return out[:n].view(np.uint64)


def want_keys(coords, ts, lo, depth, order):
    """the definition of include/me_amd.h with Python ints: (batch << D depth) | code((coords - bbox_min) / stride)"""
    c = np.asarray(coords, dtype=np.int64)
    D = c.shape[1] - 1
    out = []
    for r in c.tolist():
        x = [(r[1 + a] - int(lo[a])) // int(ts[a]) for a in range(D)]
        assert all(0 <= v < (1 << depth) or (depth == 0 and v == 0) for v in x), (r, x, depth)
        out.append((r[0] << (D * depth)) | serial_code(x, depth, order))
    assert max(out) < (1 << 63)
    return np.array(out, dtype=np.uint64)


def assert_keys(coords, ts, lo, depth, order, dev, what, stream=None):
    got, want = gpu_keys(coords, ts, lo, depth, order, dev, stream), want_keys(coords, ts, lo, depth, order)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what} {order}: {bad.size} of {len(want)} keys differ; row {bad[0]} {np.asarray(coords)[bad[0]].tolist()}: "
                           f"got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}")


def _cells(D, depth, n_random, seed):
    """the all-zero cell, the all-ones cell, the one-axis extremes (one axis at 2^depth - 1, the others 0, and the reverse)
    and random cells, int64 [*, D]"""
    top = (1 << depth) - 1
    rng = np.random.default_rng(seed)
    rows = [np.zeros(D, dtype=np.int64), np.full(D, top, dtype=np.int64)]
    for a in range(D):
        one = np.zeros(D, dtype=np.int64)
        one[a] = top
        rows += [one, top - one]
    rows += list(rng.integers(0, top + 1, size=(n_random, D), dtype=np.int64))
    return np.stack(rows)


def _with_batch(cells, batch):
    b = np.broadcast_to(np.asarray(batch, dtype=np.int64), (cells.shape[0],))
    return np.concatenate([b[:, None], cells], 1)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D", [1, 2, 3, 4, 7])
def test_keys_at_the_widest_legal_code(device, D, order):
    """depth = min(31, 63 // D): 31, 62, 63, 60 and 63 code bits; batch 0, so the 63-bit codes stay within 63 bits"""
    depth = min(31, 63 // D)
    coords = _with_batch(_cells(D, depth, 300, seed=D), 0)
    assert_keys(coords, [1] * D, [0] * D, depth, order, device, f"widest D={D} depth={depth}")


@pytest.mark.parametrize("order", ORDERS)
def test_keys_carry_the_batch_above_the_code(device, order):
    """D = 3, depth 17: the batch indices 0, 5 and 1000 sit above 51 code bits"""
    cells = _cells(3, 17, 300, seed=17)
    coords = _with_batch(cells, np.array([0, 5, 1000])[np.arange(cells.shape[0]) % 3])
    assert_keys(coords, [1, 1, 1], [0, 0, 0], 17, order, device, "batch bits")
    got = gpu_keys(coords, [1, 1, 1], [0, 0, 0], 17, order, device)
    assert np.array_equal(got >> np.uint64(51), coords[:, 0].astype(np.uint64))


@pytest.mark.parametrize("order", ORDERS)
def test_keys_at_depth_zero_and_at_a_depth_beyond_the_data(device, order):
    """depth 0: every row in one cell, the key is the batch index.  depth 9 on cells below 16: the upper levels are zero
    bits of the z code and still turn the Hilbert cell"""
    rng = np.random.default_rng(3)
    batch = rng.integers(0, 700, size=200)
    one_cell = _with_batch(np.broadcast_to(np.array([5, -3, 7]), (200, 3)), batch)
    got = gpu_keys(one_cell, [1, 1, 1], [5, -3, 7], 0, order, device)
    assert np.array_equal(got, batch.astype(np.uint64))
    small = _with_batch(rng.integers(0, 16, size=(300, 3)), rng.integers(0, 3, size=300))
    assert_keys(small, [1, 1, 1], [0, 0, 0], 9, order, device, "depth 9 on 4-bit cells")
    assert_keys(small, [1, 1, 1], [0, 0, 0], 4, order, device, "depth 4 on 4-bit cells")


@pytest.mark.parametrize("order", ORDERS)
def test_keys_with_a_negative_bbox_min_and_per_axis_strides(device, order):
    lo, ts = np.array([-37, -1000, 4]), np.array([2, 3, 5])
    cells = _cells(3, 11, 300, seed=5)
    coords = _with_batch(lo + cells * ts, np.arange(cells.shape[0]) % 4)
    assert int(coords[:, 1:].min()) < 0
    assert_keys(coords, ts, lo, 11, order, device, "strides (2, 3, 5)")
    assert np.array_equal(want_keys(coords, ts, lo, 11, order), np.array(serial_keys(coords, ts, order), dtype=np.uint64))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D", [1, 2])
def test_keys_of_an_extent_beyond_int32_under_stride_three(device, D, order):
    """bbox_min = -2147483646, stride 3, cells up to 1431655764 (coordinate 2147483646): the extent needs 32 bits, an int32
    difference wraps (coordinate 2147483646: -4, and -4 / 3 = -1 gives the low bits 0x7fffffff instead of 1431655764).  The
    header allows the map: depth 31 with D <= 2 is at most 62 code bits"""
    lo, top = -2147483646, 1431655764
    rng = np.random.default_rng(31 + D)
    cells = np.concatenate([np.array([[0] * D, [top] * D, [top - 1] * D, [top // 2] * D, [top // 2 + 1] * D]),
                            rng.integers(0, top + 1, size=(300, D), dtype=np.int64)])
    cells[5:55] = rng.integers(715827883, top + 1, size=(50, D), dtype=np.int64)       # differences of 2^31 or more
    coords64 = _with_batch(lo + 3 * cells, 0)
    assert int(coords64[:, 1:].max()) == 2147483646 and int(coords64[:, 1:].min()) == lo
    assert int((coords64[:, 1:] - lo).max()).bit_length() == 32
    coords = coords64.astype(np.int32)
    assert np.array_equal(coords.astype(np.int64), coords64)
    assert serial_geometry(coords, [3] * D)[1] == 31
    assert_keys(coords, [3] * D, [lo] * D, 31, order, device, f"stride 3, extent 2^32 - 4, D={D}")


def test_key_launches(device):
    """n = 0 with null pointers returns 0 and launches nothing; n = 1; n = 257 (a second block of one row) on a
    non-default stream"""
    lib = _lib.load()
    assert lib.me_coords_serial_keys(None, 0, 4, _i32s([1, 1, 1]), _i32s([0, 0, 0]), 10, 2, None, None) == 0
    assert_keys(np.array([[3, 9, -2, 5]]), [1, 1, 1], [-1, -2, -3], 4, "hilbert", device, "n = 1")
    coords = _with_batch(_cells(3, 12, 250, seed=8), 2)
    assert coords.shape[0] == 258
    assert_keys(coords[:257], [1, 1, 1], [0, 0, 0], 12, "hilbert_trans", device, "side stream", stream=_side_stream(device))


# ---- B. lists ------------------------------------------------------------------------------------------------------------------
def list_sizes(n, n_batch, patch):
    n_seg = -(-n // patch) + n_batch
    return n_seg, dict(seg_ptr=n_seg + 1, seg_rows=n, blk_tab=2 * (-(-n // 64) + n_seg), row_patch=n)


def patch_lists(coords, ts, lo, depth, batch_max, order, n_batch, patch, dev, stream=None, ws=None, null_data=False):
    """me_attn_patch_lists under the harness rule -> (dict of numpy int32 arrays, the workspace tensor).  `ws`: reuse a
    workspace as an earlier call left it"""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    n, ncol = coords.shape
    n_seg, sizes = list_sizes(n, n_batch, patch)
    c = torch.from_numpy(coords).to(dev) if n > 0 else None
    out = {k: torch.full((m + GUARD,), FILL, dtype=torch.int32, device=dev) for k, m in sizes.items()}
    ws_bytes = int(lib.me_attn_patch_lists_workspace_bytes(n, n_batch, patch))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    if ws is None:
        ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws[ws_bytes:] = 0x5C
    assert ws.numel() == ws_bytes + WS_GUARD
    data = (lambda t: None) if null_data else _ptr
    if stream is not None:
        torch.cuda.synchronize(dev)
    _lib.check(lib.me_attn_patch_lists(
        _ptr(c), n, ncol, _i32s(ts), _i32s(lo), depth, batch_max, ORDERS.index(order), n_batch, patch, _ptr(out["seg_ptr"]),
        data(out["seg_rows"]), _ptr(out["blk_tab"]), data(out["row_patch"]), data(ws), ws_bytes,
        stream.cuda_stream if stream is not None else None))
    torch.cuda.synchronize(dev)
    assert bool((ws[ws_bytes:] == 0x5C).all()), "the workspace was written past the size asked for"
    res = {}
    for k, m in sizes.items():
        a = out[k].cpu().numpy()
        assert (a[m:] == FILL).all(), f"{k} was written past its end"
        res[k] = a[:m]
    return res, ws


def lists_from_row_patch(row_patch, n_seg):
    """seg_ptr, seg_rows (rows ascending inside a segment) and the whole block table (unused entries -1) of a segment id per
    row, in numpy"""
    row_patch = np.asarray(row_patch, dtype=np.int64)
    n = row_patch.shape[0]
    counts = np.bincount(row_patch, minlength=n_seg) if n else np.zeros(n_seg, dtype=np.int64)
    assert counts.shape[0] == n_seg
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    seg_rows = np.argsort(row_patch, kind="stable").astype(np.int32)
    nblk = -(-counts // 64)
    tab = np.full((-(-n // 64) + n_seg, 2), -1, dtype=np.int32)
    used = int(nblk.sum())
    tab[:used, 0] = np.repeat(np.arange(n_seg), nblk)
    tab[:used, 1] = 64 * (np.arange(used) - np.repeat(np.cumsum(nblk) - nblk, nblk))
    return dict(seg_ptr=seg_ptr, seg_rows=seg_rows, blk_tab=tab.reshape(-1), row_patch=row_patch.astype(np.int32))


def assert_lists(coords, ts, order, n_batch, patch, dev, what, stream=None, want_patch=None):
    """the four outputs against the yardstick of the same rows -> (outputs, workspace, expected row_patch)"""
    coords = np.asarray(coords, dtype=np.int64)
    lo, depth = serial_geometry(coords, ts)
    got, ws = patch_lists(coords, ts, lo, depth, int(coords[:, 0].max()), order, n_batch, patch, dev, stream=stream)
    if want_patch is None:
        want_patch = row_patches(coords, ts, order, patch)
    want = lists_from_row_patch(want_patch, list_sizes(coords.shape[0], n_batch, patch)[0])
    diff = int((got["row_patch"] != want["row_patch"]).sum())
    assert diff == 0, f"{what} {order} P={patch}: {diff} of {coords.shape[0]} rows in another patch"
    for k in ("seg_ptr", "seg_rows", "blk_tab"):
        assert np.array_equal(got[k], want[k]), f"{what} {order} P={patch}: {k} differs"
    return got, ws, want_patch


def _shuffled(rows, rng):
    rows = np.concatenate(rows)
    return rows[rng.permutation(rows.shape[0])]


@pytest.mark.parametrize("order", ORDERS)
def test_lists_of_deep_keys_over_three_sort_tiles(device, order):
    """n = 3000 (three 1024-row sort tiles), D = 3, coordinates in [0, 2^20): depth 20, 60 code bits and one batch bit, eight
    radix passes.  Half the rows are random; the other half are clusters (a base plus offsets in [0, 4)) and the same
    clusters translated by 2^19, so that the lowest and the highest key bytes both decide the order"""
    rng = np.random.default_rng(20)
    rand = rng.integers(0, 1 << 20, size=(1500, 3))
    base = np.repeat(rng.integers(0, (1 << 19) - 4, size=(75, 3)), 10, axis=0)
    near = base + rng.integers(0, 4, size=(750, 3))
    cells = np.concatenate([rand, near, near + (1 << 19)])
    cells[0], cells[1] = 0, (1 << 20) - 1                                              # the bounding box: depth 20
    coords = _with_batch(cells, rng.integers(0, 2, size=3000))
    coords = coords[rng.permutation(3000)]
    assert serial_geometry(coords, [1, 1, 1])[1] == 20
    got, _, _ = assert_lists(coords, [1, 1, 1], order, 2, 32, device, "deep keys")
    assert np.diff(got["seg_ptr"]).max() <= 32


@pytest.mark.parametrize("order", ORDERS)
def test_lists_of_the_shortest_sort(device, order):
    """D = 2 at depth 1 and 2 with two instances: 3 and 5 key bits, one radix pass.  Depth 0 with the one batch index 0: no
    key bit at all, the sort still takes its one pass.  Duplicate rows are allowed"""
    rng = np.random.default_rng(2)
    for depth in (1, 2):
        cells = rng.integers(0, 1 << depth, size=(10, 2))
        cells[0], cells[1] = 0, (1 << depth) - 1
        coords = _with_batch(cells, [0, 1, 1, 0, 0, 1, 0, 1, 1, 1])
        assert serial_geometry(coords, [1, 1])[1] == depth
        for patch in (1, 3, 10):
            assert_lists(coords, [1, 1], order, 2, patch, device, f"depth {depth}")
    same = _with_batch(np.broadcast_to(np.array([4, -9]), (9, 2)), 0)
    assert serial_geometry(same, [1, 1])[1] == 0
    got, _, _ = assert_lists(same, [1, 1], order, 1, 4, device, "depth 0")
    assert got["row_patch"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]                    # equal keys keep the row order


@pytest.mark.parametrize("order", ["z", "hilbert"])
def test_equal_keys_keep_their_row_order_across_sort_tiles(device, order):
    """n = 3000 rows over 50 distinct coordinates in two instances: runs of about 30 equal keys that cross the tile
    boundaries at rows 1024 and 2048.  The sort is stable, so equal keys keep ascending row order, as Python's sort in the
    yardstick does; P = 7 cuts inside the runs, where the order decides the patch"""
    rng = np.random.default_rng(50)
    distinct = rng.integers(0, 200, size=(50, 3))
    coords = _with_batch(distinct[rng.integers(0, 50, size=3000)], rng.integers(0, 2, size=3000))
    assert np.unique(coords[:, 1:], axis=0).shape[0] == 50
    assert_lists(coords, [1, 1, 1], order, 2, 7, device, "50 distinct coordinates")
    assert_lists(coords, [1, 1, 1], order, 2, 32, device, "50 distinct coordinates")


@pytest.fixture(scope="module")
def big_scene():
    """n = 40000 rows, above the single-block scan limit of 32768: instances of 25000, 14999 and 1 rows in [0, 1024)^3"""
    rng = np.random.default_rng(40000)
    sizes = (25000, 14999, 1)
    return _shuffled([_with_batch(rng.integers(0, 1024, size=(m, 3)), b) for b, m in enumerate(sizes)], rng)


@pytest.mark.parametrize("order,patch", [("hilbert", 48), ("z", 1)])
def test_lists_beyond_the_single_block_scan(device, big_scene, order, patch):
    """n = 40000: the instance scan takes the three-launch pipeline.  P = 1: S = 40003 segments, so the scan of the segment
    blocks takes it too, k_seg_blocks and k_blk_tab run on 157 workgroups and every row is its own patch"""
    got, _, _ = assert_lists(big_scene, [1, 1, 1], order, 3, patch, device, "n = 40000")
    if patch == 1:
        assert got["seg_ptr"].shape[0] == 40004 and np.array_equal(np.sort(got["row_patch"]), np.arange(40000))
        assert (got["seg_ptr"][40000:] == 40000).all()


def test_lists_of_many_instances_with_sparse_batch_indices(device):
    """300 instances whose batch indices are drawn without replacement from [0, 1000), 1 to 12 rows each, P = 4: more than
    256 instances, gaps between the indices.  n_batch = 320: the 20 surplus instances give empty trailing segments"""
    rng = np.random.default_rng(300)
    index = rng.choice(1000, size=300, replace=False)
    coords = _shuffled([_with_batch(rng.integers(0, 64, size=(int(rng.integers(1, 13)), 3)), b) for b in index], rng)
    n = coords.shape[0]
    assert 1500 < n < 2500 and np.unique(coords[:, 0]).shape[0] == 300
    for order in ("hilbert", "z_trans"):
        got, _, want = assert_lists(coords, [1, 1, 1], order, 300, 4, device, "300 instances")
        more, _, _ = assert_lists(coords, [1, 1, 1], order, 320, 4, device, "300 instances, n_batch 320", want_patch=want)
        assert np.array_equal(more["row_patch"], got["row_patch"]) and np.array_equal(more["seg_rows"], got["seg_rows"])
        assert np.array_equal(more["seg_ptr"][:got["seg_ptr"].shape[0]], got["seg_ptr"])
        assert (more["seg_ptr"][-21:] == n).all()


def test_lists_of_more_instances_than_rows(device):
    """n = 5 rows in two instances (batch indices 2 and 7), n_batch = 600: k_inst_start and k_inst_patches run past n"""
    coords = np.array([[7, 3, 1, 0], [2, 0, 0, 5], [7, 0, 2, 2], [2, 9, 9, 9], [7, 1, 1, 1]])
    for order in ORDERS:
        for patch in (1, 2, 5):
            got, _, _ = assert_lists(coords, [1, 1, 1], order, 600, patch, device, "5 rows, n_batch 600")
            assert got["row_patch"][[1, 3]].max() < got["row_patch"][[0, 2, 4]].min()


@pytest.mark.parametrize("n_b", [1, 63, 64, 65, 128, 129])
def test_patch_size_edges_on_one_instance(device, n_b):
    """P in {1, n_b, n_b + 1, 64, 65, 2^40}: 2^40 needs the int64 patch size (one patch) and the 64-bit r * m_b"""
    rng = np.random.default_rng(n_b)
    cells = np.unique(rng.integers(0, 32, size=(4 * n_b + 8, 3)), axis=0)
    coords = _with_batch(cells[rng.permutation(cells.shape[0])[:n_b]], 0)
    assert coords.shape[0] == n_b
    for patch in sorted({1, n_b, n_b + 1, 64, 65, 1 << 40}):
        for order in ("hilbert", "z_trans"):
            got, _, _ = assert_lists(coords, [1, 1, 1], order, 1, patch, device, f"n_b = {n_b}")
            sizes = np.diff(got["seg_ptr"])
            m_b = -(-n_b // patch)
            assert (sizes[:m_b] > 0).all() and (sizes[m_b:] == 0).all() and sizes.max() - sizes[:m_b].min() <= 1


@pytest.mark.parametrize("n_batch", [0, 3])
def test_lists_of_an_empty_map(device, n_batch):
    """n = 0: seg_ptr all zero, the table all -1, null data pointers accepted"""
    coords = np.zeros((0, 4), dtype=np.int32)
    got, _ = patch_lists(coords, [1, 1, 1], [0, 0, 0], 0, 0, "hilbert", n_batch, 16, device, null_data=True)
    assert got["seg_ptr"].shape == (n_batch + 1,) and (got["seg_ptr"] == 0).all()
    assert got["blk_tab"].shape == (2 * n_batch,) and (got["blk_tab"] == -1).all()


def test_a_second_call_on_the_same_workspace_and_a_side_stream(device):
    """two calls on one workspace (the second finds what the first left there) and a call on a non-default stream give
    identical outputs"""
    rng = np.random.default_rng(9)
    coords = _shuffled([_with_batch(rng.integers(-50, 300, size=(m, 3)), b) for b, m in ((0, 900), (3, 400), (4, 1))], rng)
    lo, depth = serial_geometry(coords, [1, 1, 1])
    first, ws, _ = assert_lists(coords, [1, 1, 1], "hilbert", 3, 48, device, "first call")
    second, _ = patch_lists(coords, [1, 1, 1], lo, depth, 4, "hilbert", 3, 48, device, ws=ws)
    side, _, _ = assert_lists(coords, [1, 1, 1], "hilbert", 3, 48, device, "side stream", stream=_side_stream(device))
    for k in first:
        assert np.array_equal(first[k], second[k]) and np.array_equal(first[k], side[k]), k


# ---- C. hand-built tables ------------------------------------------------------------------------------------------------------
HEADS = 2
DTYPES = (torch.float32, torch.bfloat16)
NAMES = ("out", "lse", "dq", "dk", "dv")
Q_SIZES = (0, 1, 63, 0, 64, 65, 129, 0, 300, 0)      # empty segments first, in the middle and last
KV_SIZES = (0, 70, 0, 5, 64, 1, 200, 0, 129, 3)      # segment 2: queries and no keys; segment 3: keys and no queries


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Side:
    """a partition that no curve made: one segment id per row, the ids drawn in shuffled row order; its lists and table"""

    def __init__(self, sizes, seed, dev):
        rng = np.random.default_rng(seed)
        self.n, self.n_seg = int(sum(sizes)), len(sizes)
        self.seg = rng.permutation(np.repeat(np.arange(self.n_seg), sizes))
        lists = lists_from_row_patch(self.seg, self.n_seg)
        assert np.diff(lists["seg_ptr"]).tolist() == list(sizes)
        self.used = int((lists["blk_tab"][0::2] >= 0).sum())
        self.seg_ptr, self.seg_rows, self.tab = (torch.from_numpy(lists[k]).to(dev) for k in ("seg_ptr", "seg_rows", "blk_tab"))
        self.seg_dev = torch.from_numpy(self.seg).to(dev)

    def permuted_table(self, seed):
        """the same table with its used entries in another order"""
        perm = torch.from_numpy(np.random.default_rng(seed).permutation(self.used)).to(self.tab.device)
        assert not torch.equal(perm, torch.arange(self.used, device=perm.device))
        tab = self.tab.clone().view(-1, 2)
        tab[:self.used] = tab[perm]
        return tab.reshape(-1).contiguous()


def attend(qs, ks, q, k, v, dout, tab_q, tab_kv):
    """me_attn_forward_tab and me_attn_backward_tab on the lists of the two sides -> out, lse, dq, dk, dv; every output is
    pre-filled with NaN"""
    lib = _lib.load()
    dev, dtype, c = q.device, q.dtype, q.shape[1]
    d, bf16 = c // HEADS, int(q.dtype == torch.bfloat16)
    scale = 1.0 / math.sqrt(d)
    stream = torch.cuda.current_stream(dev).cuda_stream
    r = dict(out=torch.full_like(q, math.nan), lse=torch.full((qs.n, HEADS), math.nan, dtype=torch.float32, device=dev),
             dq=torch.full_like(q, math.nan), dk=torch.full_like(k, math.nan), dv=torch.full_like(v, math.nan))
    lists = [_ptr(qs.seg_ptr), _ptr(qs.seg_rows), _ptr(ks.seg_ptr), _ptr(ks.seg_rows), _ptr(tab_q), _ptr(tab_kv)]
    _lib.check(lib.me_attn_forward_tab(_ptr(q), _ptr(k), _ptr(v), bf16, c, c, c, *lists, qs.n, ks.n, qs.n_seg, c, HEADS, scale,
                                       _ptr(r["out"]), c, _ptr(r["lse"]), stream))
    ws = torch.empty(lib.me_attn_workspace_bytes(qs.n, ks.n, qs.n_seg, HEADS), dtype=torch.uint8, device=dev)
    _lib.check(lib.me_attn_backward_tab(_ptr(q), _ptr(k), _ptr(v), _ptr(r["out"]), _ptr(r["lse"]), _ptr(dout), bf16, c, c, c,
                                        c, c, *lists, qs.n, ks.n, qs.n_seg, c, HEADS, scale, _ptr(r["dq"]), c, _ptr(r["dk"]),
                                        c, _ptr(r["dv"]), c, _ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize(dev)
    assert dtype == r["out"].dtype
    return r


def _operands(qs, ks, d, dtype, dev, seed):
    c = HEADS * d
    return (draw(qs.n, c, dtype, dev, seed), draw(ks.n, c, dtype, dev, seed + 1), draw(ks.n, c, dtype, dev, seed + 2),
            draw(qs.n, c, dtype, dev, seed + 3))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [32, 64])
def test_a_window_partition_with_empty_segments(device, d, dtype):
    """one partition for both sides, segment sizes (0, 1, 63, 0, 64, 65, 129, 0, 300, 0): with the hand-built table out, lse,
    dq, dk and dv equal the walk over seg_ptr (null tables) bit for bit, and stay within the bound"""
    side = Side(Q_SIZES, seed=d, dev=device)
    q, k, v, dout = _operands(side, side, d, dtype, device, 100 + d)
    tab = attend(side, side, q, k, v, dout, side.tab, side.tab)
    walk = attend(side, side, q, k, v, dout, None, None)
    for name in NAMES:
        assert torch.isfinite(tab[name].float()).all(), name
        assert _same(tab[name], walk[name]), name
    within_bound(tab, q, k, v, dout, side.seg_dev, side.seg_dev, HEADS, what=f"window partition d={d} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [32, 64])
def test_distinct_partitions_of_the_two_sides(device, d, dtype):
    """622 queries and 472 keys over the same ten segments, each side with its own lists and its own table.  Segment 2 has
    63 queries and no key: zero rows, lse = -inf and zero dq, as for an instance without keys in
    tests/test_gpu_attention_kernels.py and tests/test_gpu_cross_attention_kernels.py (`reference` and torch skip it).
    Segment 3 has 5 keys and no query: zero dk and dv"""
    qs, ks = Side(Q_SIZES, seed=d, dev=device), Side(KV_SIZES, seed=d + 1, dev=device)
    assert qs.n != ks.n and Q_SIZES[2] > 0 and KV_SIZES[2] == 0 and Q_SIZES[3] == 0 and KV_SIZES[3] > 0
    q, k, v, dout = _operands(qs, ks, d, dtype, device, 200 + d)
    tab = attend(qs, ks, q, k, v, dout, qs.tab, ks.tab)
    walk = attend(qs, ks, q, k, v, dout, None, None)
    for name in NAMES:
        assert _same(tab[name], walk[name]), name
    no_keys, no_queries = qs.seg_dev == 2, ks.seg_dev == 3
    assert int(no_keys.sum()) == 63 and int(no_queries.sum()) == 5
    zero = torch.zeros(1, HEADS * d, dtype=dtype, device=device)
    assert bool((tab["out"][no_keys] == zero).all()) and bool((tab["dq"][no_keys] == zero).all())
    assert bool(torch.isneginf(tab["lse"][no_keys]).all())
    assert bool((tab["dk"][no_queries] == zero).all()) and bool((tab["dv"][no_queries] == zero).all())
    within_bound(tab, q, k, v, dout, qs.seg_dev, ks.seg_dev, HEADS, what=f"distinct sides d={d} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [32, 64])
def test_the_order_of_the_table_entries_does_not_matter(device, d, dtype):
    """the grid is one workgroup per table entry, so the used entries may come in any order.  out, lse and dq with a permuted
    q-side table, dk and dv with a permuted kv-side table: bit for bit.  For dk and dv this holds because k_attn_bwd_kv
    keeps the sums of its 64 key rows in registers over the whole walk of the queries and writes every row once: no
    atomics, no accumulation across workgroups"""
    qs, ks = Side(Q_SIZES, seed=d, dev=device), Side(KV_SIZES, seed=d + 1, dev=device)
    q, k, v, dout = _operands(qs, ks, d, dtype, device, 300 + d)
    plain = attend(qs, ks, q, k, v, dout, qs.tab, ks.tab)
    mixed = attend(qs, ks, q, k, v, dout, qs.permuted_table(1), ks.permuted_table(2))
    for name in NAMES:
        assert _same(plain[name], mixed[name]), name
