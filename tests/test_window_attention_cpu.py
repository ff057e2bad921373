"""Host-side checks of window attention (no GPU), and the numpy yardstick of its partition.

The yardstick `row_windows` is written from the definition in include/me_amd.h (me_attn_window_ids) with Python integer
floor division and shares no code with the kernels.  tests/test_gpu_window_attention*.py import it."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def _axes(v, D):
    return [int(v)] * D if np.ndim(v) == 0 else [int(e) for e in v]


def window_cells(coords, tensor_stride, window_size, shift):
    """(b, cell_0 .. cell_{D-1}) of every row as tuples of Python ints: cell_a = floor((c_a / t_a + s_a) / w_a), both
    divisions floors towards -inf, s_a reduced modulo w_a"""
    c = np.asarray(coords, dtype=np.int64)
    D = c.shape[1] - 1
    t, w, s = _axes(tensor_stride, D), _axes(window_size, D), _axes(shift, D)
    assert min(w) >= 1 and min(t) >= 1
    return [(int(r[0]),) + tuple((int(r[1 + a]) // t[a] + s[a] % w[a]) // w[a] for a in range(D)) for r in c.tolist()]


def row_windows(coords, tensor_stride, window_size, shift):
    """int64 [n]: the window of every row, the windows numbered 0 .. W - 1 in ascending lexicographic order of
    (b, cell_0 .. cell_{D-1})"""
    cells = window_cells(coords, tensor_stride, window_size, shift)
    rank = {cell: i for i, cell in enumerate(sorted(set(cells)))}
    return np.array([rank[cell] for cell in cells], dtype=np.int64)


def _grid(side, D, batch=0, lo=0):
    return np.array([(batch,) + p for p in itertools.product(range(lo, lo + side), repeat=D)], dtype=np.int64)


def test_yardstick_on_a_full_grid():
    grid = _grid(8, 3)
    w = row_windows(grid, 1, 4, 0)
    assert np.bincount(w).tolist() == [64] * 8
    assert w[0] == 0 and w[-1] == 7
    assert w[np.flatnonzero((grid[:, 1:] == (0, 0, 4)).all(1))[0]] == 1       # the last axis is the least significant
    assert w[np.flatnonzero((grid[:, 1:] == (4, 0, 0)).all(1))[0]] == 4
    shifted = row_windows(grid, 1, 4, 2)
    assert sorted(np.bincount(shifted).tolist()) == [8] * 8 + [16] * 12 + [32] * 6 + [64]
    assert len(set(shifted.tolist())) == 27


def test_yardstick_floors_negative_coordinates_towards_minus_infinity():
    coords = np.array([[0, -5], [0, -4], [0, -1], [0, 0], [0, 3], [0, 4]])
    assert window_cells(coords, 1, 4, 0) == [(0, -2), (0, -1), (0, -1), (0, 0), (0, 0), (0, 1)]
    assert row_windows(coords, 1, 4, 0).tolist() == [0, 1, 1, 2, 2, 3]
    assert window_cells(coords, 1, 4, 1) == [(0, -1), (0, -1), (0, 0), (0, 0), (0, 1), (0, 1)]
    assert window_cells(coords, 1, 4, -1) == window_cells(coords, 1, 4, 3)


def test_yardstick_counts_windows_in_units_of_the_tensor_stride():
    coords = np.array([[0, -8, 0], [0, -2, 2], [0, 0, 6], [0, 6, 8], [0, 8, 14]])
    assert window_cells(coords, 2, 4, 0) == [(0, -1, 0), (0, -1, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1)]
    assert window_cells(coords, (2, 1), (4, 8), 0) == [(0, -1, 0), (0, -1, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1)]
    fine = _grid(8, 2)
    assert np.array_equal(row_windows(fine * np.array([1, 2, 2]), 2, 4, 1), row_windows(fine, 1, 4, 1))


def test_yardstick_takes_sizes_and_shifts_per_axis_and_batches_first():
    grid = np.concatenate([_grid(6, 3, batch=2), _grid(6, 3, batch=0)])
    w = row_windows(grid, 1, (6, 3, 2), 0)
    assert np.bincount(w).tolist() == [36] * 12
    assert (w[216:] < 6).all() and (w[:216] >= 6).all()                        # batch 0 before batch 2
    w = row_windows(grid, 1, (6, 3, 2), (0, 1, 0))
    assert sorted(np.bincount(w).tolist()) == [12] * 6 + [24] * 6 + [36] * 6


@pytest.mark.parametrize("w,s", [(4, 1), (4, -3), (3, 2), ((4, 2, 3), (1, 1, 2))])
def test_yardstick_shift_and_shift_plus_window_give_one_partition(w, s):
    rng = np.random.default_rng(1)
    coords = np.concatenate([rng.integers(0, 3, size=(300, 1)), rng.integers(-20, 45, size=(300, 3))], 1)
    plus = tuple(a + b for a, b in zip(_axes(s, 3), _axes(w, 3)))
    minus = tuple(a - 2 * b for a, b in zip(_axes(s, 3), _axes(w, 3)))
    base = row_windows(coords, 1, w, s)
    assert np.array_equal(base, row_windows(coords, 1, w, plus)) and np.array_equal(base, row_windows(coords, 1, w, minus))
    assert not np.array_equal(base, row_windows(coords, 1, w, tuple(a + 1 for a in _axes(s, 3))))


# ---- scenes of the GPU tests (tests/test_gpu_window_attention.py), built by placing dense boxes ---------------------------------
WINDOW = 8
EDGE_SIZES = (1, 31, 32, 33, 65, 150)


def box_rows(m, origin, batch=0, side=WINDOW):
    """the first m cells, in lexicographic order, of the box of `side` cells per axis at `origin`: int64 [m, 1 + D]"""
    D = len(origin)
    cells = np.array(list(itertools.islice(itertools.product(range(side), repeat=D), m)), dtype=np.int64)
    assert cells.shape[0] == m
    return np.concatenate([np.full((m, 1), batch, dtype=np.int64), cells + np.asarray(origin, dtype=np.int64)], 1)


def edges_scene(seed=0):
    """windows of 1, 31, 32, 33, 65 and 150 rows under window 8 and shift 0: one dense box per window, windows on both
    sides of the origin, two instances (batch indices 0 and 3), rows shuffled -> int64 [312, 4]"""
    origins = [(-16, -8, 0), (-8, 8, -8), (0, 0, 0), (16, -8, 8), (-8, 0, 0), (8, 8, 8)]
    rows = np.concatenate([box_rows(m, o, batch=3 * (i % 2)) for i, (m, o) in enumerate(zip(EDGE_SIZES, origins))])
    return rows[np.random.default_rng(seed).permutation(rows.shape[0])]


def cube_scene():
    """a dense 5 x 5 x 5 block at [1, 6)^3: one window of 125 rows under window 8, eight windows under shift 4"""
    return box_rows(125, (1, 1, 1), side=5)


def three_boxes_scene():
    """three windows of 65 rows in a line along x (window 8, shift 0): a full y-z slab of 64 rows and one row more each"""
    return np.concatenate([box_rows(65, (8 * i - 8, 0, 0)) for i in range(3)])


def test_the_scenes_have_the_populations_they_are_named_for():
    edges = edges_scene()
    assert sorted(np.bincount(row_windows(edges, 1, WINDOW, 0)).tolist()) == sorted(EDGE_SIZES)
    assert np.unique(edges, axis=0).shape[0] == edges.shape[0] == sum(EDGE_SIZES) and int(edges[:, 1:].min()) < 0
    assert len(set(row_windows(edges, 1, WINDOW, WINDOW // 2).tolist())) > len(EDGE_SIZES)     # the shift cuts the boxes
    cube = cube_scene()
    assert np.bincount(row_windows(cube, 1, WINDOW, 0)).tolist() == [125]
    assert sorted(np.bincount(row_windows(cube, 1, WINDOW, 4)).tolist()) == [8, 12, 12, 12, 18, 18, 18, 27]
    boxes = three_boxes_scene()
    assert np.bincount(row_windows(boxes, 1, WINDOW, 0)).tolist() == [65, 65, 65]
    assert np.bincount(row_windows(boxes, 1, WINDOW, (0, 4, 0))).tolist() == [33, 32] * 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("scene,shift", [("edges", 0), ("edges", 4), ("cube", 0), ("cube", 4)])
def test_the_torch_side_of_the_bound_is_finite_on_these_scenes(scene, shift, dtype):
    """the bound of the GPU tests is E_kernel <= FACTOR * E_torch against float64: on the CPU, with the inputs the GPU tests
    draw, torch's own attention per window has a finite error in every tensor, and a positive one wherever a window holds
    more than one row (a one-row window returns v itself)"""
    from test_gpu_attention_kernels import NAMES, draw, reference, torch_attention
    coords = edges_scene() if scene == "edges" else cube_scene()
    seg = torch.from_numpy(row_windows(coords, 1, WINDOW, shift))
    heads, d = 2, 32
    cpu = torch.device("cpu")
    q, k, v, dout = (draw(coords.shape[0], heads * d, dtype, cpu, 10 * d + s) for s in range(4))
    ref = reference(q, k, v, dout, seg, seg, heads)
    theirs = torch_attention(q, k, v, dout, seg, seg, heads)
    assert torch.isfinite(ref["lse"]).all()
    for name in NAMES:
        e = (theirs[name].double() - ref[name]).abs()
        assert torch.isfinite(e).all() and torch.isfinite(ref[name]).all(), name
        assert float(e.max()) > 0.0, name


# ---- the module --------------------------------------------------------------------------------------------------------------
def test_constructor_errors():
    with pytest.raises(ValueError, match="window_size"):
        ME.MinkowskiWindowSelfAttention(64, 2, window_size=0)
    with pytest.raises(ValueError, match="window_size"):
        ME.MinkowskiWindowSelfAttention(64, 2, window_size=(4, 0, 4))
    with pytest.raises(ValueError, match="window_size"):
        ME.MinkowskiWindowSelfAttention(64, 2, window_size=4.5)
    with pytest.raises(ValueError, match="shift"):
        ME.MinkowskiWindowSelfAttention(64, 2, shift="half")
    with pytest.raises(ValueError, match="per spatial axis"):
        ME.MinkowskiWindowSelfAttention(64, 2, window_size=(4, 4, 4), shift=(1, 1))
    with pytest.raises(ValueError):
        ME.MinkowskiWindowSelfAttention(64, 3)
    with pytest.raises(ValueError):
        ME.MinkowskiWindowSelfAttention(0, 1)


def test_repr_shows_window_and_shift():
    m = ME.MinkowskiWindowSelfAttention(64, 2, window_size=(8, 8, 4), shift=(4, 4, 2), bias=False)
    assert repr(m) == "MinkowskiWindowSelfAttention(64, 2, window_size=(8, 8, 4), shift=(4, 4, 2), bias=False)"
    d = ME.MinkowskiWindowSelfAttention(64, 2)
    assert (d.window_size, d.shift) == (8, 0) and "window_size=8, shift=0, bias=True" in repr(d)


@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly_in_both_directions(bias):
    torch.manual_seed(0)
    a = ME.MinkowskiWindowSelfAttention(64, 2, window_size=6, shift=3, bias=bias)
    b = ME.MinkowskiSelfAttention(64, 2, bias=bias)
    assert sorted(a.state_dict()) == sorted(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])
    a2 = ME.MinkowskiWindowSelfAttention(64, 2, bias=bias)
    a2.load_state_dict(b.state_dict(), strict=True)
    mha = torch.nn.MultiheadAttention(64, 2, bias=bias, batch_first=True)
    mha.load_state_dict(a2.state_dict(), strict=True)
    a2.load_state_dict(mha.state_dict(), strict=True)
    if bias:
        assert float(a.in_proj_bias.detach().abs().max()) == 0.0 and float(a.out_proj.bias.detach().abs().max()) == 0.0


def test_package_exports():
    for name in ("MinkowskiWindowSelfAttention", "MinkowskiWindowAttentionFunction"):
        assert hasattr(ME, name)
    assert callable(ME.MinkowskiFunctional.window_attention)
    assert "window_attention" in ME.MinkowskiFunctional.__all__
    assert callable(ME.CoordinateManager.window_rows)
    assert issubclass(ME.MinkowskiWindowSelfAttention, ME.MinkowskiSelfAttention)


def test_a_dense_tensor_raises_type_error_before_anything_else():
    m = ME.MinkowskiWindowSelfAttention(64, 2)
    with pytest.raises(TypeError, match="SparseTensor"):
        m(torch.zeros(3, 64))


def test_cpu_tensors_have_no_operator():
    with pytest.raises(ValueError, match="WindowAttentionForwardCPU"):
        ME.get_minkowski_function("WindowAttentionForward", torch.zeros(1))
    with pytest.raises(ValueError, match="WindowAttentionBackwardCPU"):
        ME.get_minkowski_function("WindowAttentionBackward", torch.zeros(1))


def test_window_arguments_of_the_host_layers():
    from minkowskiengine_amd import backend
    assert backend.window_args(4, 0, 3) == ((4, 4, 4), (0, 0, 0))
    assert backend.window_args((4, 2, 3), (5, -1, 3), 3) == ((4, 2, 3), (1, 1, 0))
    assert backend.window_args(4, 6, 2) == backend.window_args(4, 2, 2) == backend.window_args(4, -2, 2)
    with pytest.raises(ValueError, match="window_size"):
        backend.window_args(0, 0, 3)
    with pytest.raises(ValueError, match="per spatial axis"):
        backend.window_args((4, 4), 0, 3)
    with pytest.raises(ValueError, match="per spatial axis"):
        backend.window_args(4, (1, 1, 1, 1), 3)


def test_both_host_layers_expose_the_operators_and_the_abi():
    from minkowskiengine_amd import _lib, backend, host
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in ("WindowAttentionForwardGPU", "WindowAttentionBackwardGPU"):
        assert callable(getattr(backend, name)) and hasattr(native, name), name
    assert hasattr(backend.CoordinateMapManagerGPU_c10, "_window_rows")
    assert hasattr(native.CoordinateMapManagerGPU_c10, "_window_rows")
    lib = _lib.load()
    assert lib.me_version() >= 310
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    assert re.search(r"1\.21 \(310\)", header)
    for name in ("me_attn_window_ids", "me_attn_window_ids_workspace_bytes", "me_attn_segment_lists",
                 "me_attn_segment_lists_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_the_c_abi_refuses_bad_arguments_without_a_gpu():
    """host-side argument errors come before any launch: they are reachable with dummy data pointers"""
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)   # noqa: E731
    one = ctypes.c_void_p(16)
    ts, w4, s0 = i32s(1, 1, 1), i32s(4, 4, 4), i32s(0, 0, 0)
    lo, hi = i32s(0, 0, 0), i32s(100, 100, 100)
    ws = lib.me_attn_window_ids_workspace_bytes(10)
    assert ws > 0 and ws % 256 == 0 and lib.me_attn_window_ids_workspace_bytes(-1) < 0

    def ids(ncol=4, ts=ts, w=w4, s=s0, n_axes=3, lo=lo, hi=hi, bmin=0, bmax=1, ws_bytes=ws):
        return lib.me_attn_window_ids(one, 10, ncol, ts, w, s, n_axes, lo, hi, bmin, bmax, one, one, one, ws_bytes, None)

    assert ids(w=i32s(4, 0, 4)) != 0                                            # a window size of 0
    assert b"window_size must be at least 1" in lib.me_last_error()
    assert ids(w=i32s(4, -2, 4)) != 0
    assert ids(n_axes=2) != 0                                                   # a wrong number of axes
    assert b"per spatial axis" in lib.me_last_error()
    assert ids(bmin=-1) != 0                                                    # a negative batch index
    assert b"negative" in lib.me_last_error()
    assert ids(ws_bytes=ws - 1) != 0                                            # a short workspace
    assert b"workspace too small" in lib.me_last_error()
    # window 1 on extents of 2^21 + 1 cells: 3 * 22 = 66 cell bits
    assert ids(w=i32s(1, 1, 1), hi=i32s(1 << 21, 1 << 21, 1 << 21), bmax=0) != 0
    assert b"63 bits" in lib.me_last_error()
    # 3 * 21 cell bits and one batch bit: 64
    assert ids(w=i32s(1, 1, 1), hi=i32s((1 << 21) - 1, (1 << 21) - 1, (1 << 21) - 1), bmax=1) != 0
    assert b"63 bits" in lib.me_last_error()
    # the whole int32 range on two axes under window 1: 64 cell bits; under window 2 with shift 1 the cells still take 32
    # bits each (2^31 + 1 of them)
    full_lo, full_hi = i32s(-2147483648, -2147483648), i32s(2147483647, 2147483647)
    assert lib.me_attn_window_ids(one, 10, 3, i32s(1, 1), i32s(1, 1), i32s(0, 0), 2, full_lo, full_hi, 0, 0, one, one, one,
                                  ws, None) != 0
    assert b"63 bits" in lib.me_last_error()
    assert lib.me_attn_window_ids(one, 10, 3, i32s(1, 1), i32s(2, 2), i32s(1, 1), 2, full_lo, full_hi, 0, 0, one, one, one,
                                  ws, None) != 0
    assert b"63 bits" in lib.me_last_error()
    assert ids(ts=i32s(1 << 16, 1, 1), w=i32s(1 << 15, 4, 4)) != 0              # window_size * tensor_stride = 2^31
    assert b"fit in int32" in lib.me_last_error()
    assert lib.me_attn_window_ids(None, 0, 4, ts, w4, s0, 3, None, None, 0, 0, None, None, None, 0, None) != 0   # no count
    seg_ws = lib.me_attn_segment_lists_workspace_bytes(10, 3)
    assert seg_ws > 0 and seg_ws % 256 == 0 and lib.me_attn_segment_lists_workspace_bytes(10, -1) < 0
    assert lib.me_attn_segment_lists(one, 10, 3, one, one, one, one, seg_ws - 1, None) != 0
    assert b"workspace too small" in lib.me_last_error()
    assert lib.me_attn_segment_lists(one, 10, 0, one, one, one, one, seg_ws, None) != 0      # rows without a segment
    assert lib.me_attn_segment_lists(one, 10, 1 << 31, one, one, one, one, 1 << 40, None) != 0
    assert lib.me_attn_segment_lists(one, 10, 3, None, one, one, one, seg_ws, None) != 0     # a null output
