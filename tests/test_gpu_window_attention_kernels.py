"""Entry-point tests of the window partition (csrc/serial_attention.hip, ABI 1.21) through the C ABI on synthetic device
tensors: no manager, no SparseTensor.

A. me_attn_window_ids against `row_windows` of tests/test_window_attention_cpu.py: row_window and the window count, over
   several radix passes and sort tiles, with negative coordinates, per-axis strides, sizes and shifts, extents of 2^31 and
   more, a wide scene, duplicate rows, one row, an empty map, a repeated call on one workspace and a side stream.
B. me_attn_segment_lists against `lists_from_row_patch` of tests/test_gpu_serialized_attention_kernels.py: hand-made
   segment ids with empty segments, more segments than the single-block scan takes, an empty map; and bit for bit against
   me_attn_patch_lists on the row_patch that function returns.

Every call goes through a harness: outputs pre-filled with -7 and followed by a guard, a workspace of exactly the size
asked for, pre-filled with 0xA5 and followed by a guard.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

from minkowskiengine_amd import _lib
from test_gpu_serialized_attention_kernels import lists_from_row_patch
from test_window_attention_cpu import row_windows

pytestmark = pytest.mark.gpu

GUARD = 64            # elements behind every output
WS_GUARD = 4096       # bytes behind the workspace
FILL = -7


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _axes(v, D):
    return [int(v)] * D if np.ndim(v) == 0 else [int(e) for e in v]


def _workspace(ws_bytes, dev):
    ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ws[ws_bytes:] = 0x5C
    return ws


def window_ids(coords, ts, window, shift, dev, stream=None, ws=None, bbox=None):
    """me_attn_window_ids under the harness rule -> (row_window int32 [n], W, the workspace tensor)"""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    n, ncol = coords.shape
    D = ncol - 1
    c = torch.from_numpy(coords).to(dev) if n > 0 else None
    row_window = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=dev)
    count = torch.full((1 + GUARD,), FILL, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.me_attn_window_ids_workspace_bytes(n))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    if ws is None:
        ws = _workspace(ws_bytes, dev)
    assert ws.numel() == ws_bytes + WS_GUARD
    if bbox is None:
        bbox = (coords[:, 1:].min(0), coords[:, 1:].max(0)) if n > 0 else ([0] * D, [0] * D)
    bmin, bmax = (int(coords[:, 0].min()), int(coords[:, 0].max())) if n > 0 else (0, 0)
    if stream is not None:
        torch.cuda.synchronize(dev)
    _lib.check(lib.me_attn_window_ids(_ptr(c), n, ncol, _i32s(_axes(ts, D)), _i32s(_axes(window, D)), _i32s(_axes(shift, D)),
                                      D, _i32s(bbox[0]), _i32s(bbox[1]), bmin, bmax, _ptr(row_window) if n > 0 else None,
                                      _ptr(count), _ptr(ws) if n > 0 else None, ws_bytes,
                                      stream.cuda_stream if stream is not None else None))
    torch.cuda.synchronize(dev)
    assert bool((ws[ws_bytes:] == 0x5C).all()), "the workspace was written past the size asked for"
    rw, cnt = row_window.cpu().numpy(), count.cpu().numpy()
    assert (rw[n:] == FILL).all() and (cnt[1:] == FILL).all(), "an output was written past its end"
    return rw[:n], int(cnt[0]), ws


def assert_ids(coords, ts, window, shift, dev, what, **kw):
    got, count, ws = window_ids(coords, ts, window, shift, dev, **kw)
    want = row_windows(coords, ts, window, shift)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what} w={window} s={shift}: {bad.size} of {len(want)} rows in another window; row {bad[0]} "
                           f"{np.asarray(coords)[bad[0]].tolist()}: got {got[bad[0]]}, want {want[bad[0]]}")
    assert count == (int(want.max()) + 1 if len(want) else 0), f"{what}: window count {count}"
    return got, count, ws


def _side_stream(dev):
    torch.cuda.synchronize(dev)
    return torch.cuda.Stream(dev)


def _scene(rng, sizes, D, lo, hi, stride=1, batches=None):
    """sizes[i] random rows (duplicates allowed) with coordinates stride * [lo, hi) in instance batches[i], shuffled"""
    batches = list(range(len(sizes))) if batches is None else batches
    rows = [np.concatenate([np.full((m, 1), b), stride * rng.integers(lo, hi, size=(m, D))], 1) for m, b in zip(sizes, batches)]
    rows = np.concatenate(rows)
    return rows[rng.permutation(rows.shape[0])]


# ---- A. window ids --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_scene():
    """n = 40000 rows, above the single-block scan limit of 32768 and 40 sort tiles: instances 0, 1 and 3 in [-512, 512)^3"""
    return _scene(np.random.default_rng(40000), (25000, 14999, 1), 3, -512, 512, batches=(0, 1, 3))


@pytest.mark.parametrize("window,shift", [(4, 0), (4, 2), ((7, 2, 64), (3, -1, 100)), (1, 0)])
def test_ids_beyond_the_single_block_scan(device, big_scene, window, shift):
    """n = 40000: window 4 gives 8 cell bits per axis and 2 batch bits, four radix passes; window 1 gives 10 bits per axis,
    32 key bits, and nearly every row a window of its own: the rank scan takes the three-launch pipeline"""
    got, count, _ = assert_ids(big_scene, 1, window, shift, device, "n = 40000")
    if window == 1:
        assert count == np.unique(big_scene, axis=0).shape[0] > 32768


@pytest.mark.parametrize("D", [1, 2, 3, 4, 7])
def test_ids_in_every_dimension_with_strides_sizes_and_shifts_per_axis(device, D):
    rng = np.random.default_rng(D)
    ts = [1, 2, 3, 5, 1, 4, 2][:D]
    coords = _scene(rng, (700, 500), D, -40, 90, batches=(1, 6)) * np.array([1] + ts)
    window, shift = [4, 2, 3, 1, 5, 8, 6][:D], [2, -1, 7, 0, -9, 3, 1][:D]
    assert_ids(coords, ts, window, shift, device, f"D={D}")
    assert_ids(coords, ts, 3, -2, device, f"D={D}")
    off_grid = coords + np.array([0] + [t - 1 for t in ts])               # coordinates that are no multiples of the stride
    assert_ids(off_grid, ts, window, shift, device, f"D={D} off the stride grid")


@pytest.mark.parametrize("D", [1, 2])
def test_ids_of_an_extent_beyond_int32(device, D):
    """coordinates from -2147483648 to 2147483647 under stride 3: an int32 difference to the lowest cell wraps, and the
    quotient of a negative coordinate must floor.  Window 5, shift 2: cells of 15 coordinates, 29 bits per axis"""
    rng = np.random.default_rng(31 + D)
    pts = rng.integers(-(1 << 31), 1 << 31, size=(400, D), dtype=np.int64)
    pts[0], pts[1], pts[2], pts[3] = -(1 << 31), (1 << 31) - 1, -1, 0
    pts[4:40] = rng.integers((1 << 31) - 64, 1 << 31, size=(36, D))      # several rows per window at the upper end
    pts[40:80] = rng.integers(-(1 << 31), -(1 << 31) + 64, size=(40, D))  # and at the lower end
    coords = np.concatenate([rng.integers(0, 2, size=(400, 1)), pts], 1)
    got, count, _ = assert_ids(coords, 3, 5, 2, device, f"int32 range D={D}")
    assert D > 1 or count < 400                                           # 76 rows in at most 12 cells at the two ends
    assert_ids(coords, 1, (1 << 31) - 1, 12345, device, f"int32 range, the widest window D={D}")
    assert_ids(coords, 1, 1 << 30, -1, device, f"int32 range, window 2^30 D={D}")


def test_ids_of_a_wide_scene(device):
    """600 rows over [0, 2^17) in x and y and [0, 64) in z under window 4: 15 + 15 + 4 cell bits and one batch bit"""
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.integers(0, 1 << 17, size=(600, 2)), rng.integers(0, 64, size=(600, 1))], 1)
    pts[0], pts[1] = (0, 0, 0), ((1 << 17) - 1, (1 << 17) - 1, 63)
    near = pts[2:200] + rng.integers(0, 4, size=(198, 3))                 # neighbours that share windows
    coords = np.concatenate([rng.integers(0, 2, size=(798, 1)), np.concatenate([pts, near])], 1)
    got, count, _ = assert_ids(coords, 1, 4, 0, device, "wide")
    assert count < 798
    assert_ids(coords, 1, 4, 2, device, "wide")
    assert_ids(coords, 1, 1, 0, device, "wide")                           # 17 + 17 + 6 + 1 bits


def test_ids_of_small_inputs(device):
    """one row; equal rows (one window, one radix pass over no key bit); 257 rows (a second block of one row); a bounding
    box wider than the rows; an empty map with null pointers"""
    assert_ids(np.array([[3, 9, -2, 5]]), 1, 4, 1, device, "n = 1")
    same = np.broadcast_to(np.array([0, 4, -9]), (9, 3))
    got, count, _ = assert_ids(same, 1, 4, 0, device, "equal rows")
    assert count == 1 and (got == 0).all()
    rng = np.random.default_rng(8)
    coords = _scene(rng, (257,), 3, -30, 30)
    assert_ids(coords, 1, 4, 2, device, "n = 257")
    assert_ids(coords, 1, 4, 2, device, "a wider box", bbox=([-100, -31, -30], [29, 1000, 77]))
    got, count, _ = window_ids(np.zeros((0, 4), dtype=np.int32), 1, 4, 0, device)
    assert got.shape == (0,) and count == 0


def test_a_second_call_on_the_same_workspace_and_a_side_stream(device):
    rng = np.random.default_rng(9)
    coords = _scene(rng, (900, 400, 1), 3, -50, 300, batches=(0, 3, 4))
    first, count, ws = assert_ids(coords, 1, 6, 3, device, "first call")
    second, count2, _ = window_ids(coords, 1, 6, 3, device, ws=ws)
    side, count3, _ = assert_ids(coords, 1, 6, 3, device, "side stream", stream=_side_stream(device))
    assert np.array_equal(first, second) and np.array_equal(first, side) and count == count2 == count3


# ---- B. segment lists -------------------------------------------------------------------------------------------------------------
def segment_lists(row_segment, n_seg, dev, stream=None):
    """me_attn_segment_lists under the harness rule -> dict of numpy int32 arrays"""
    lib = _lib.load()
    row_segment = np.ascontiguousarray(row_segment, dtype=np.int32)
    n = row_segment.shape[0]
    sizes = dict(seg_ptr=n_seg + 1, seg_rows=n, blk_tab=2 * (-(-n // 64) + n_seg))
    seg = torch.from_numpy(row_segment).to(dev) if n > 0 else None
    out = {k: torch.full((m + GUARD,), FILL, dtype=torch.int32, device=dev) for k, m in sizes.items()}
    ws_bytes = int(lib.me_attn_segment_lists_workspace_bytes(n, n_seg))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    ws = _workspace(ws_bytes, dev)
    if stream is not None:
        torch.cuda.synchronize(dev)
    _lib.check(lib.me_attn_segment_lists(_ptr(seg), n, n_seg, _ptr(out["seg_ptr"]), _ptr(out["seg_rows"]) if n > 0 else None,
                                         _ptr(out["blk_tab"]), _ptr(ws) if n > 0 else None, ws_bytes,
                                         stream.cuda_stream if stream is not None else None))
    torch.cuda.synchronize(dev)
    assert bool((ws[ws_bytes:] == 0x5C).all()), "the workspace was written past the size asked for"
    res = {}
    for k, m in sizes.items():
        a = out[k].cpu().numpy()
        assert (a[m:] == FILL).all(), f"{k} was written past its end"
        res[k] = a[:m]
    return res


def assert_segment_lists(row_segment, n_seg, dev, what, **kw):
    got, want = segment_lists(row_segment, n_seg, dev, **kw), lists_from_row_patch(row_segment, n_seg)
    for k in ("seg_ptr", "seg_rows", "blk_tab"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    return got


def test_segment_lists_with_empty_segments_and_block_edges(device):
    """segment sizes (0, 1, 63, 0, 64, 65, 129, 0, 300, 0), the ids in shuffled row order: empty segments first, in the
    middle and last; segments that end on, one before and one after a 64-row block"""
    sizes = (0, 1, 63, 0, 64, 65, 129, 0, 300, 0)
    seg = np.random.default_rng(1).permutation(np.repeat(np.arange(len(sizes)), sizes))
    got = assert_segment_lists(seg, len(sizes), device, "block edges")
    assert np.diff(got["seg_ptr"]).tolist() == list(sizes)
    tab = got["blk_tab"].reshape(-1, 2)
    assert tab[:12].tolist() == [[1, 0], [2, 0], [4, 0], [5, 0], [5, 64], [6, 0], [6, 64], [6, 128], [8, 0], [8, 64],
                                 [8, 128], [8, 192]]
    assert tab[12].tolist() == [8, 256] and (tab[13:, 0] == -1).all()
    assert_segment_lists(seg, len(sizes), device, "side stream", stream=_side_stream(device))
    assert_segment_lists(seg, len(sizes) + 700, device, "700 surplus segments")


def test_segment_lists_beyond_the_single_block_scan(device):
    """40000 rows in 39000 segments (some empty, some of several rows): the scan of the segment blocks takes the
    three-launch pipeline, k_seg_blocks and k_blk_tab run on 153 workgroups"""
    seg = np.random.default_rng(2).integers(0, 39000, size=40000)
    assert_segment_lists(seg, 39000, device, "39000 segments")
    assert_segment_lists(np.zeros(40000, dtype=np.int64), 1, device, "one segment of 40000 rows")


@pytest.mark.parametrize("n_seg", [0, 3])
def test_segment_lists_of_an_empty_map(device, n_seg):
    got = segment_lists(np.zeros(0, dtype=np.int32), n_seg, device)
    assert got["seg_ptr"].shape == (n_seg + 1,) and (got["seg_ptr"] == 0).all()
    assert got["blk_tab"].shape == (2 * n_seg,) and (got["blk_tab"] == -1).all()


def test_segment_lists_equal_the_patch_lists_on_their_row_patch(device):
    """me_attn_patch_lists returns row_patch and the lists it makes of it; me_attn_segment_lists on that row_patch with the
    same segment count gives the same three tensors bit for bit"""
    from test_gpu_serialized_attention_kernels import patch_lists
    from test_serialized_attention_cpu import serial_geometry
    rng = np.random.default_rng(3)
    coords = _scene(rng, (900, 400, 1), 3, -50, 300, batches=(0, 3, 4))
    lo, depth = serial_geometry(coords, [1, 1, 1])
    for patch in (1, 48, 500):
        want, _ = patch_lists(coords, [1, 1, 1], lo, depth, 4, "hilbert", 3, patch, device)
        got = segment_lists(want["row_patch"], want["seg_ptr"].shape[0] - 1, device)
        for k in ("seg_ptr", "seg_rows", "blk_tab"):
            assert np.array_equal(got[k], want[k]), (patch, k)


def test_ids_and_lists_chain_without_a_read_back_in_between(device):
    """the window count stays on the device: with the host's bound n for the segment count the lists of row_window are
    those of the yardstick, followed by empty segments"""
    coords = _scene(np.random.default_rng(4), (300, 200), 3, -20, 45, batches=(0, 2))
    got, count, _ = assert_ids(coords, 1, 4, 2, device, "chain")
    lists = assert_segment_lists(got, coords.shape[0], device, "n segments")
    assert (np.diff(lists["seg_ptr"])[count:] == 0).all() and (np.diff(lists["seg_ptr"])[:count] > 0).all()
