"""Host-side checks of serialized patch attention (no GPU), and the numpy yardstick of its keys and patch lists.

The yardstick is written from the definitions in include/me_amd.h (me_coords_serial_keys, me_attn_patch_lists) and shares
no code with the kernels: `serial_code` (z-order by explicit bit placement; Hilbert by Skilling's AxesToTranspose, one point
at a time), `serial_keys`, `patch_of_rank` and `row_patches`.  tests/test_gpu_serialized_attention*.py import it."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME

ORDERS = ("z", "z_trans", "hilbert", "hilbert_trans")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def _interleave(x, depth):
    """bit l of axis a goes to code bit l * D + (D - 1 - a)"""
    D, code = len(x), 0
    for l in range(depth):
        for a in range(D):
            code |= ((int(x[a]) >> l) & 1) << (l * D + (D - 1 - a))
    return code


def _axes_to_transpose(x, depth):
    """J. Skilling, Programming the Hilbert curve (2004): AxesToTranspose on a list of ints with `depth` bits each"""
    x, n = [int(v) for v in x], len(x)
    if depth == 0:
        return x
    m = 1 << (depth - 1)
    q = m
    while q > 1:                       # inverse undo
        p = q - 1
        for i in range(n):
            if x[i] & q:
                x[0] ^= p
            else:
                t = (x[0] ^ x[i]) & p
                x[0] ^= t
                x[i] ^= t
        q >>= 1
    for i in range(1, n):              # Gray encode
        x[i] ^= x[i - 1]
    t, q = 0, m
    while q > 1:
        if x[n - 1] & q:
            t ^= q - 1
        q >>= 1
    return [v ^ t for v in x]


def serial_code(x, depth, order):
    x = [int(v) for v in x]
    if order.endswith("_trans") and len(x) >= 2:
        x[0], x[1] = x[1], x[0]
    if order.startswith("hilbert"):
        x = _axes_to_transpose(x, depth)
    return _interleave(x, depth)


def serial_geometry(coords, tensor_stride):
    """(bbox_min of the spatial axes, depth) of an int array [n, 1 + D]"""
    c = np.asarray(coords, dtype=np.int64)
    lo, hi = c[:, 1:].min(0), c[:, 1:].max(0)
    ext = (hi - lo) // np.asarray(tensor_stride, dtype=np.int64)
    return lo, max(int(e).bit_length() for e in ext)


def serial_keys(coords, tensor_stride, order):
    """python ints: (batch << D depth) | code((coords - bbox_min) / tensor_stride)"""
    c = np.asarray(coords, dtype=np.int64)
    lo, depth = serial_geometry(c, tensor_stride)
    D = c.shape[1] - 1
    ts = [int(t) for t in tensor_stride]
    return [(int(r[0]) << (D * depth)) | serial_code([(int(r[1 + a]) - int(lo[a])) // ts[a] for a in range(D)], depth, order)
            for r in c]


def patch_of_rank(r, n_b, patch_size):
    m_b = -(-n_b // patch_size)
    return (r * m_b) // n_b


def row_patches(coords, tensor_stride, order, patch_size):
    """the global patch of every row: instances in ascending batch index, patch_base the running sum of ceil(n_b / P)"""
    c = np.asarray(coords, dtype=np.int64)
    keys = serial_keys(c, tensor_stride, order)
    out = np.zeros(c.shape[0], dtype=np.int64)
    base = 0
    for b in sorted(set(c[:, 0].tolist())):
        rows = [i for i in range(c.shape[0]) if c[i, 0] == b]
        rows.sort(key=lambda i: keys[i])
        for r, i in enumerate(rows):
            out[i] = base + patch_of_rank(r, len(rows), patch_size)
        base += -(-len(rows) // patch_size)
    return out


# ---- the yardstick checks itself -------------------------------------------------------------------------------------------
def _grid(side, D):
    return np.array(list(itertools.product(range(side), repeat=D)), dtype=np.int64)


@pytest.mark.parametrize("side,D", [(8, 3), (16, 2)])
@pytest.mark.parametrize("order", ORDERS)
def test_every_order_is_a_permutation_of_the_full_grid(side, D, order):
    pts, depth = _grid(side, D), side.bit_length() - 1
    codes = sorted(serial_code(p, depth, order) for p in pts)
    assert codes == list(range(side ** D))


@pytest.mark.parametrize("side,D", [(8, 3), (16, 2)])
@pytest.mark.parametrize("order", ["hilbert", "hilbert_trans"])
def test_consecutive_hilbert_cells_are_neighbours(side, D, order):
    pts, depth = _grid(side, D), side.bit_length() - 1
    by_code = sorted(pts.tolist(), key=lambda p: serial_code(p, depth, order))
    steps = np.abs(np.diff(np.array(by_code), axis=0)).sum(1)
    assert (steps == 1).all()


def _deinterleave(code, D, depth):
    """the inverse of _interleave: code bit l * D + (D - 1 - a) is bit l of axis a"""
    x = [0] * D
    for l in range(depth):
        for a in range(D):
            x[a] |= ((code >> (l * D + (D - 1 - a))) & 1) << l
    return x


def _transpose_to_axes(x, depth):
    """J. Skilling, Programming the Hilbert curve (2004): TransposeToAxes, the inverse of AxesToTranspose.  Its loops run
    upwards from Q = 2 and it decodes the Gray code by one shift: it shares neither loop bounds nor the order of the steps
    with _axes_to_transpose"""
    x, n = [int(v) for v in x], len(x)
    if depth == 0:
        return x
    top = 1 << depth
    t = x[n - 1] >> 1                  # Gray decode
    for i in range(n - 1, 0, -1):
        x[i] ^= x[i - 1]
    x[0] ^= t
    q = 2
    while q != top:                    # undo the excess work
        p = q - 1
        for i in range(n - 1, -1, -1):
            if x[i] & q:
                x[0] ^= p
            else:
                t = (x[0] ^ x[i]) & p
                x[0] ^= t
                x[i] ^= t
        q <<= 1
    return x


def serial_decode(code, D, depth, order):
    """the cell of a code: the inverse of serial_code"""
    x = _deinterleave(int(code), D, depth)
    if order.startswith("hilbert"):
        x = _transpose_to_axes(x, depth)
    if order.endswith("_trans") and D >= 2:
        x[0], x[1] = x[1], x[0]
    return x


@pytest.mark.parametrize("order", ["hilbert", "hilbert_trans"])
@pytest.mark.parametrize("D", [2, 3, 4])
def test_deep_hilbert_codes_decode_to_neighbouring_cells(D, order):
    """depth = min(31, 63 // D): 62, 63 and 60 code bits, where the GPU keys are compared with serial_code.  For 2000 random
    codes h: serial_code(decode(h)) == h, and decode(h) and decode(h + 1) are one unit step apart on one axis — checked
    through Skilling's inverse transform, so independent of the forward transform's loop bounds.  hilbert_trans decodes to
    the cell of hilbert with the axes 0 and 1 exchanged, and has the same two properties"""
    import random
    depth = min(31, 63 // D)
    rng = random.Random(1000 * D + len(order))
    top = 1 << (D * depth)
    codes = [0, top - 2, (top >> 1) - 1] + [rng.randrange(top - 1) for _ in range(2000)]
    for h in codes:
        a, b = serial_decode(h, D, depth, order), serial_decode(h + 1, D, depth, order)
        assert all(0 <= v < (1 << depth) for v in a)
        assert serial_code(a, depth, order) == h and serial_code(b, depth, order) == h + 1
        assert sorted(abs(u - v) for u, v in zip(a, b)) == [0] * (D - 1) + [1], (h, a, b)
        if order == "hilbert_trans":
            plain = serial_decode(h, D, depth, "hilbert")
            assert a == [plain[1], plain[0]] + plain[2:]


@pytest.mark.parametrize("order", ["z", "z_trans"])
def test_deep_z_codes_round_trip(order):
    import random
    rng = random.Random(7)
    for D in (1, 2, 3, 4, 7):
        depth = min(31, 63 // D)
        for _ in range(300):
            h = rng.randrange(1 << (D * depth))
            assert serial_code(serial_decode(h, D, depth, order), depth, order) == h


def test_z_is_explicit_bit_interleaving():
    for x, y, z in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (5, 3, 6), (7, 7, 7)]:
        want = 0
        for l in range(3):
            want |= ((x >> l) & 1) << (3 * l + 2) | ((y >> l) & 1) << (3 * l + 1) | ((z >> l) & 1) << (3 * l)
        assert serial_code([x, y, z], 3, "z") == want
    assert serial_code([1, 0, 0], 3, "z") == 4 and serial_code([0, 0, 1], 3, "z") == 1


@pytest.mark.parametrize("order", ["z", "hilbert"])
def test_trans_orders_are_the_plain_orders_on_swapped_axes(order):
    for p in _grid(8, 3):
        assert serial_code(p, 3, order + "_trans") == serial_code([p[1], p[0], p[2]], 3, order)
    assert serial_code([5], 3, order + "_trans") == serial_code([5], 3, order)     # D = 1: nothing to exchange


def test_keys_put_the_batch_above_the_code_and_divide_by_the_stride():
    coords = np.array([[0, -4, 2], [1, -4, 2], [0, 2, 6], [1, 0, 4]])
    lo, depth = serial_geometry(coords, (2, 2))
    assert lo.tolist() == [-4, 2] and depth == 2                 # extents 6 / 2 = 3 and 4 / 2 = 2
    keys = serial_keys(coords, (2, 2), "z")
    assert keys == [0, 1 << 4, serial_code([3, 2], 2, "z"), (1 << 4) | serial_code([2, 1], 2, "z")]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 150])
def test_the_patch_rule(n):
    P = 32
    patches = [patch_of_rank(r, n, P) for r in range(n)]
    sizes = np.bincount(patches)
    assert sizes.sum() == n and len(sizes) == -(-n // P)
    assert sizes.max() - sizes.min() <= 1 and sizes.max() <= P and sizes.min() >= 1
    assert patches == sorted(patches)


def test_row_patches_number_the_instances_in_batch_order():
    coords = np.array([[1, 0, 0], [0, 3, 0], [1, 1, 0], [0, 0, 0], [1, 2, 0], [0, 1, 0]])
    assert row_patches(coords, (1, 1), "z", 2).tolist() == [2, 1, 2, 0, 3, 0]


# ---- the module --------------------------------------------------------------------------------------------------------------
def test_constructor_errors():
    with pytest.raises(ValueError, match="order"):
        ME.MinkowskiSerializedSelfAttention(64, 2, order="peano")
    with pytest.raises(ValueError, match="patch_size"):
        ME.MinkowskiSerializedSelfAttention(64, 2, patch_size=0)
    with pytest.raises(ValueError):
        ME.MinkowskiSerializedSelfAttention(64, 3)
    with pytest.raises(ValueError):
        ME.MinkowskiSerializedSelfAttention(0, 1)


def test_repr_shows_patch_size_and_order():
    m = ME.MinkowskiSerializedSelfAttention(64, 2, patch_size=128, order="hilbert_trans", bias=False)
    assert repr(m) == "MinkowskiSerializedSelfAttention(64, 2, patch_size=128, order='hilbert_trans', bias=False)"
    d = ME.MinkowskiSerializedSelfAttention(64, 2)
    assert (d.patch_size, d.order) == (1024, "z") and "patch_size=1024, order='z', bias=True" in repr(d)


@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly_in_both_directions(bias):
    torch.manual_seed(0)
    a = ME.MinkowskiSerializedSelfAttention(64, 2, patch_size=48, order="hilbert", bias=bias)
    b = ME.MinkowskiSelfAttention(64, 2, bias=bias)
    assert sorted(a.state_dict()) == sorted(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])
    a2 = ME.MinkowskiSerializedSelfAttention(64, 2, bias=bias)
    a2.load_state_dict(b.state_dict(), strict=True)
    torch.nn.MultiheadAttention(64, 2, bias=bias, batch_first=True).load_state_dict(a2.state_dict(), strict=True)
    if bias:
        assert float(a.in_proj_bias.detach().abs().max()) == 0.0 and float(a.out_proj.bias.detach().abs().max()) == 0.0


def test_package_exports():
    for name in ("MinkowskiSerializedSelfAttention", "MinkowskiSerializedAttentionFunction"):
        assert hasattr(ME, name)
    assert callable(ME.MinkowskiFunctional.serialized_attention)
    assert "serialized_attention" in ME.MinkowskiFunctional.__all__
    assert callable(ME.CoordinateManager.patch_rows)
    assert issubclass(ME.MinkowskiSerializedSelfAttention, ME.MinkowskiSelfAttention)


def test_a_tensor_field_raises_type_error_before_anything_else():
    m = ME.MinkowskiSerializedSelfAttention(64, 2)
    with pytest.raises(TypeError, match="SparseTensor"):
        m(torch.zeros(3, 64))


def test_both_host_layers_expose_the_operators_and_the_abi():
    from minkowskiengine_amd import _lib, backend, host
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in ("SerializedAttentionForwardGPU", "SerializedAttentionBackwardGPU"):
        assert callable(getattr(backend, name)) and hasattr(native, name), name
    assert hasattr(backend.CoordinateMapManagerGPU_c10, "_patch_rows")
    assert backend.SERIAL_ORDERS == ORDERS
    lib = _lib.load()
    assert lib.me_version() >= 290
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    assert re.search(r"1\.19 \(290\)", header)


def test_the_c_abi_refuses_bad_arguments_without_a_gpu():
    """host-side argument errors come before any launch: they are reachable with null data pointers"""
    import ctypes
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    i32 = ctypes.c_int32
    ts, lo = (i32 * 4)(1, 1, 1, 1), (i32 * 4)(0, 0, 0, 0)
    assert lib.me_coords_serial_keys(None, 10, 5, ts, lo, 16, 0, None, None) != 0          # 4 * 16 = 64 code bits
    assert lib.me_coords_serial_keys(None, 10, 4, ts, lo, 10, 7, None, None) != 0          # unknown order
    assert lib.me_coords_serial_keys(None, 0, 4, ts, lo, 10, 2, None, None) == 0           # nothing to do
    ws = lib.me_attn_patch_lists_workspace_bytes(10, 2, 4)
    assert ws > 0 and lib.me_attn_patch_lists_workspace_bytes(10, 2, 0) < 0
    one = ctypes.c_void_p(16)
    args = (one, one, one, one, one, ws, None)
    assert lib.me_attn_patch_lists(None, 10, 4, ts, lo, 20, 7, 0, 8, 4, *args) != 0        # 60 + bits(8) = 64 bits
    assert b"63 bits" in lib.me_last_error()
    assert lib.me_attn_patch_lists(None, 10, 4, ts, lo, 10, 1, 0, 2, 0, *args) != 0        # patch_size 0
    assert lib.me_attn_patch_lists(None, 10, 4, ts, lo, 10, 1, 4, 2, 4, *args) != 0        # unknown order
    assert lib.me_attn_patch_lists(None, 10, 4, ts, lo, 10, 1, 0, 2, 4, one, one, one, one, one, ws - 1, None) != 0
