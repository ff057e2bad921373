"""Host-side checks of rotary position embedding (no GPU), and the numpy yardstick of its definition.

The yardstick (`rope_angles`, `rope_table`, `rope_apply`) is written in float64 from the definition in include/me_amd.h
(me_rope_table / me_rope_apply) and shares no code with the kernels: omega_j = base^(-j / m) with Python's float pow,
theta = (c_a / u_a) * omega_j in that order.  tests/test_gpu_rope*.py import it."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def _units(unit, D):
    return [int(unit)] * D if np.ndim(unit) == 0 else [int(u) for u in unit]


def rope_angles(coords, d, base=10000.0, unit=1):
    """float64 [n, d / 2]: theta of every pair of one head on every row of coords int [n, 1 + D] (batch index first); the
    trailing pairs that pass through hold 0.  -> (theta, |c_a / u_a| of the pair's axis)"""
    c = np.asarray(coords, dtype=np.int64)
    n, D = c.shape[0], c.shape[1] - 1
    assert d % 2 == 0 and d // 2 >= D
    P = d // 2
    m = P // D
    u = _units(unit, D)
    assert min(u) >= 1
    theta, t_abs = np.zeros((n, P), dtype=np.float64), np.zeros((n, P), dtype=np.float64)
    for p in range(D * m):
        a, j = p // m, p % m
        omega = math.pow(float(base), -float(j) / float(m))
        t = c[:, 1 + a].astype(np.float64) / np.float64(u[a])
        theta[:, p] = t * np.float64(omega)
        t_abs[:, p] = np.abs(t)
    return theta, t_abs


_COS = np.vectorize(math.cos, otypes=[np.float64])      # the C library's cos / sin (below one ulp over the whole range);
_SIN = np.vectorize(math.sin, otypes=[np.float64])      # numpy's vector loops may be a few ulps off


def rope_table(coords, d, base=10000.0, unit=1):
    """float64 [n, d / 2, 2] = (cos theta, sin theta)"""
    theta, _ = rope_angles(coords, d, base, unit)
    if theta.size == 0:
        return np.zeros(theta.shape + (2,), dtype=np.float64)
    return np.stack([_COS(theta), _SIN(theta)], axis=-1)


def rope_apply(x, coords, heads, base=10000.0, unit=1, sign=1):
    """float64 [n, heads * d]: every pair (2p, 2p + 1) of every head rotated by sign * theta_p"""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape
    assert c % heads == 0 and sign in (1, -1)
    d = c // heads
    tab = rope_table(coords, d, base, unit)
    cs, sn = tab[:, None, :, 0], sign * tab[:, None, :, 1]
    xh = x.reshape(n, heads, d // 2, 2)
    y = np.empty_like(xh)
    y[..., 0] = xh[..., 0] * cs - xh[..., 1] * sn
    y[..., 1] = xh[..., 0] * sn + xh[..., 1] * cs
    return y.reshape(n, c)


def _coords(rng, n, D, lo, hi, batches=2):
    return np.concatenate([rng.integers(0, batches, size=(n, 1)), rng.integers(lo, hi, size=(n, D))], 1)


def test_yardstick_in_one_dimension_is_a_rotation_by_c_radians():
    coords = np.array([[0, 0], [0, 1], [0, -2], [1, 7]])
    x = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [3.0, 4.0]])
    y = rope_apply(x, coords, 1)
    want = [[1.0, 0.0], [math.cos(1), math.sin(1)], [-math.sin(-2), math.cos(-2)],
            [3 * math.cos(7) - 4 * math.sin(7), 3 * math.sin(7) + 4 * math.cos(7)]]
    assert np.allclose(y, want, rtol=0, atol=1e-15)
    theta, t_abs = rope_angles(coords, 2)
    assert theta[:, 0].tolist() == [0.0, 1.0, -2.0, 7.0] and t_abs[:, 0].tolist() == [0.0, 1.0, 2.0, 7.0]


def test_yardstick_preserves_norms_and_the_negative_sign_inverts():
    rng = np.random.default_rng(0)
    coords = _coords(rng, 50, 3, -1000, 1000)
    x = rng.standard_normal((50, 3 * 20))
    y = rope_apply(x, coords, 3)
    pairs = lambda v: np.hypot(v[:, 0::2], v[:, 1::2])   # noqa: E731
    assert np.allclose(pairs(y), pairs(x), rtol=1e-14, atol=0)
    assert np.abs(y - x).max() > 0.1
    back = rope_apply(y, coords, 3, sign=-1)
    assert np.allclose(back, x, rtol=0, atol=1e-14)


def test_yardstick_assigns_pairs_to_axes_and_passes_the_rest_through():
    """D = 3, d = 20: P = 10, m = 3: pairs 0-2 follow x, 3-5 y, 6-8 z, pair 9 passes through"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 20))
    for axis in range(3):
        coords = np.zeros((4, 4), dtype=np.int64)
        coords[:, 1 + axis] = [1, -3, 17, 250]
        y = rope_apply(x, coords, 1)
        moved = np.abs(y - x).reshape(4, 10, 2).max(axis=(0, 2)) > 0
        assert moved.tolist() == [p // 3 == axis for p in range(9)] + [False]
        theta, _ = rope_angles(coords, 20)
        assert np.array_equal(theta[:, 3 * axis], coords[:, 1 + axis].astype(np.float64))       # omega_0 = 1
        assert np.allclose(theta[:, 3 * axis + 2], coords[:, 1 + axis] * 10000.0 ** (-2 / 3), rtol=1e-15)
    tab = rope_table(np.array([[0, 5, 6, 7]]), 20)
    assert tab[0, 9].tolist() == [1.0, 0.0]
    # m = 1 (d = 6): one pair per axis at frequency 1
    theta, _ = rope_angles(np.array([[0, 5, -6, 7]]), 6)
    assert theta[0].tolist() == [5.0, -6.0, 7.0]


@pytest.mark.parametrize("offset", [(1, -1, 1), (1000, -2048, 512), (1 << 20, -(1 << 20), (1 << 20) - 1)])
def test_yardstick_scores_depend_on_coordinate_differences_only(offset):
    """<rope(q)_i, rope(k)_j> is unchanged when every coordinate moves by one offset of up to 2^20 cells: the double angle
    is wrong by |t| 2^-52 <= 2^-32, far inside 1e-9 relative to the largest score"""
    rng = np.random.default_rng(2)
    coords = _coords(rng, 40, 3, -300, 300, batches=1)
    q, k = rng.standard_normal((40, 2 * 32)), rng.standard_normal((40, 2 * 32))
    moved = coords + np.array((0,) + tuple(offset))

    def scores(c):
        rq, rk = rope_apply(q, c, 2).reshape(40, 2, 32), rope_apply(k, c, 2).reshape(40, 2, 32)
        return np.einsum("ihd,jhd->hij", rq, rk)

    s0, s1 = scores(coords), scores(moved)
    assert np.abs(s1 - s0).max() <= 1e-9 * np.abs(s0).max()
    plain = np.einsum("ihd,jhd->hij", q.reshape(40, 2, 32), k.reshape(40, 2, 32))
    assert np.abs(s0 - plain).max() > 1e-2 * np.abs(s0).max()


def test_yardstick_unit_divides_the_coordinates():
    rng = np.random.default_rng(3)
    coords = _coords(rng, 30, 3, -500, 500)
    x = rng.standard_normal((30, 24))
    doubled = coords * np.array([1, 2, 2, 2])
    assert np.array_equal(rope_apply(x, doubled, 2, unit=2), rope_apply(x, coords, 2, unit=1))
    mixed = coords * np.array([1, 4, 1, 2])
    assert np.array_equal(rope_apply(x, mixed, 2, unit=(4, 1, 2)), rope_apply(x, coords, 2))
    theta, _ = rope_angles(np.array([[0, 3, 3, 3]]), 6, unit=2)           # no floor is taken
    assert theta[0].tolist() == [1.5, 1.5, 1.5]


# ---- the modules -------------------------------------------------------------------------------------------------------------
SELF_ATTENTION = [
    (ME.MinkowskiSelfAttention, {}),
    (ME.MinkowskiSerializedSelfAttention, {"patch_size": 64}),
    (ME.MinkowskiWindowSelfAttention, {"window_size": 4, "shift": 2}),
]


def test_constructor_errors():
    with pytest.raises(ValueError, match="num_heads"):
        ME.MinkowskiRotaryEmbedding(0)
    with pytest.raises(ValueError, match="num_heads"):
        ME.MinkowskiRotaryEmbedding(2.5)
    for base in (0.0, -1.0, float("inf"), float("nan"), "big"):
        with pytest.raises(ValueError, match="base"):
            ME.MinkowskiRotaryEmbedding(2, base=base)
    for unit in (0, (1, 0, 1), 1.5, (), "one"):
        with pytest.raises(ValueError, match="unit"):
            ME.MinkowskiRotaryEmbedding(2, unit=unit)
    for cls, kw in SELF_ATTENTION:
        with pytest.raises(ValueError, match="base"):
            cls(64, 2, rope=True, rope_base=0.0, **kw)
        with pytest.raises(ValueError, match="even"):
            cls(9, 3, rope=True, **kw)
        cls(9, 3, **kw)                                                   # without rope an odd head size still constructs


def test_repr_with_and_without_rope():
    assert repr(ME.MinkowskiRotaryEmbedding(4)) == "MinkowskiRotaryEmbedding(num_heads=4, base=10000.0, unit=None)"
    assert repr(ME.MinkowskiRotaryEmbedding(4, base=100, unit=(2, 2, 1))) == \
        "MinkowskiRotaryEmbedding(num_heads=4, base=100.0, unit=(2, 2, 1))"
    assert repr(ME.MinkowskiSelfAttention(64, 2)) == "MinkowskiSelfAttention(64, 2, bias=True)"
    assert repr(ME.MinkowskiSelfAttention(64, 2, rope=True)) == "MinkowskiSelfAttention(64, 2, bias=True, rope=True)"
    assert repr(ME.MinkowskiSerializedSelfAttention(64, 2, patch_size=128)) == \
        "MinkowskiSerializedSelfAttention(64, 2, patch_size=128, order='z', bias=True)"
    assert repr(ME.MinkowskiSerializedSelfAttention(64, 2, patch_size=128, bias=False, rope=True)) == \
        "MinkowskiSerializedSelfAttention(64, 2, patch_size=128, order='z', bias=False, rope=True)"
    assert repr(ME.MinkowskiWindowSelfAttention(64, 2)) == \
        "MinkowskiWindowSelfAttention(64, 2, window_size=8, shift=0, bias=True)"
    assert repr(ME.MinkowskiWindowSelfAttention(64, 2, rope=True, rope_base=100.0)) == \
        "MinkowskiWindowSelfAttention(64, 2, window_size=8, shift=0, bias=True, rope=True, rope_base=100.0)"


@pytest.mark.parametrize("cls,kw", SELF_ATTENTION, ids=lambda v: getattr(v, "__name__", ""))
@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly_between_rope_on_and_off(cls, kw, bias):
    torch.manual_seed(0)
    plain = cls(64, 2, bias=bias, **kw)
    torch.manual_seed(0)
    rope = cls(64, 2, bias=bias, rope=True, **kw)
    assert sorted(plain.state_dict()) == sorted(rope.state_dict())
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in rope.named_parameters()]
    for k, v in plain.state_dict().items():
        assert torch.equal(v, rope.state_dict()[k]), k                    # the same initialisation from the same seed
    fresh_rope, fresh_plain = cls(64, 2, bias=bias, rope=True, **kw), cls(64, 2, bias=bias, **kw)
    fresh_rope.load_state_dict(plain.state_dict(), strict=True)
    fresh_plain.load_state_dict(fresh_rope.state_dict(), strict=True)
    for k, v in plain.state_dict().items():
        assert torch.equal(v, fresh_plain.state_dict()[k]), k
    assert len(ME.MinkowskiRotaryEmbedding(2).state_dict()) == 0


def test_package_exports():
    for name in ("MinkowskiRotaryEmbedding", "MinkowskiRotaryEmbeddingFunction"):
        assert hasattr(ME, name)
    assert callable(ME.MinkowskiFunctional.rotary_embedding)
    assert "rotary_embedding" in ME.MinkowskiFunctional.__all__
    assert callable(ME.CoordinateManager.rope_table)


def test_a_dense_tensor_and_a_tensor_field_raise_type_error():
    field = object.__new__(ME.TensorField)         # the type alone decides: nothing of the field is read
    m = ME.MinkowskiRotaryEmbedding(2)
    with pytest.raises(TypeError, match="SparseTensor"):
        m(torch.zeros(3, 64))
    with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
        m(field)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.rotary_embedding(torch.zeros(3, 64), 2)
    with pytest.raises(TypeError, match="TensorField"):
        ME.MinkowskiFunctional.rotary_embedding(field, 2)
    for cls, kw in SELF_ATTENTION:
        with pytest.raises(TypeError, match="SparseTensor"):
            cls(64, 2, rope=True, **kw)(torch.zeros(3, 64))
        with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
            cls(64, 2, rope=True, **kw)(field)


def test_cpu_tensors_have_no_operator():
    with pytest.raises(ValueError, match="RotaryEmbeddingForwardCPU"):
        ME.get_minkowski_function("RotaryEmbeddingForward", torch.zeros(1))
    with pytest.raises(ValueError, match="RotaryEmbeddingBackwardCPU"):
        ME.get_minkowski_function("RotaryEmbeddingBackward", torch.zeros(1))


def test_units_of_the_python_host():
    from minkowskiengine_amd import backend
    assert backend.rope_units(None, (2, 2, 2), 3) == (2, 2, 2)
    assert backend.rope_units(4, (2, 2, 2), 3) == (4, 4, 4)
    assert backend.rope_units((1, 2, 3), (2, 2, 2), 3) == (1, 2, 3)
    with pytest.raises(ValueError, match="per spatial axis"):
        backend.rope_units((1, 2), (1, 1, 1), 3)
    with pytest.raises(ValueError, match="at least 1"):
        backend.rope_units((1, 0, 1), (1, 1, 1), 3)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_both_host_layers_expose_the_operators_and_the_abi():
    from minkowskiengine_amd import _lib, backend, host
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in ("RotaryEmbeddingForwardGPU", "RotaryEmbeddingBackwardGPU"):
        assert callable(getattr(backend, name)) and hasattr(native, name), name
    assert hasattr(backend.CoordinateMapManagerGPU_c10, "_rope_table")
    assert hasattr(native.CoordinateMapManagerGPU_c10, "_rope_table")
    lib = _lib.load()
    assert lib.me_version() >= 320
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    assert re.search(r"1\.22 \(320\)", header)
    for name, nargs in (("me_rope_table", 9), ("me_rope_apply", 11)):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    for macro, value in (("ME_ROPE_F32", 0), ("ME_ROPE_BF16", 1), ("ME_ROPE_F64", 2)):
        assert re.search(r"#define " + macro + r" " + str(value) + r"\b", header), macro
        assert backend._ROPE_DTYPE[{0: torch.float32, 1: torch.bfloat16, 2: torch.float64}[value]] == value
    assert re.search(r"#define ME_ROPE_MAX_PAIRS 128\b", header)


def test_the_c_abi_refuses_bad_arguments_without_a_gpu():
    """host-side argument errors come before any launch: they are reachable with dummy data pointers"""
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)   # noqa: E731
    one = ctypes.c_void_p(256)
    u1 = i32s(1, 1, 1)

    def table(coords=one, n=10, ncol=4, unit=u1, d=32, base=10000.0, f64=0, out=one):
        return lib.me_rope_table(coords, n, ncol, unit, d, base, f64, out, None)

    def apply(x=one, xs=64, y=one, ys=64, n=10, heads=2, d=32, tab=one, sign=1, dtype=0):
        return lib.me_rope_apply(x, xs, y, ys, n, heads, d, tab, sign, dtype, None)

    for call in (table, apply):
        assert call(d=7) != 0                                                   # d odd
        assert b"must be even" in lib.me_last_error()
        assert call(d=0) != 0
        assert call(d=258) != 0                                                 # P above the cap of 128
        assert b"ME_ROPE_MAX_PAIRS" in lib.me_last_error()
    assert table(d=4) != 0                                                      # d / 2 < D
    assert b"d / 2 >= D" in lib.me_last_error()
    assert table(ncol=8, unit=i32s(*[1] * 7), d=12) != 0
    assert b"d / 2 >= D" in lib.me_last_error()
    for base in (0.0, -2.0, float("inf"), float("-inf"), float("nan")):
        assert table(base=base) != 0
        assert b"base must be finite and greater than 0" in lib.me_last_error()
    for unit in (i32s(1, 0, 1), i32s(-1, 1, 1)):
        assert table(unit=unit) != 0                                            # a unit below 1
        assert b"unit must be at least 1" in lib.me_last_error()
    assert table(ncol=1) != 0 and table(ncol=9) != 0
    assert table(coords=None) != 0 and b"must be given" in lib.me_last_error()  # a null pointer with n > 0
    assert table(out=None) != 0 and b"must be given" in lib.me_last_error()
    assert table(coords=None, out=None, n=0) == 0                               # n = 0 succeeds without a launch
    assert apply(xs=63) != 0                                                    # a row stride below heads * d
    assert b"row stride" in lib.me_last_error()
    assert apply(ys=63) != 0
    assert b"row stride" in lib.me_last_error()
    for sign in (0, 2, -2):
        assert apply(sign=sign) != 0
        assert b"sign must be +1 or -1" in lib.me_last_error()
    assert apply(dtype=3) != 0 and b"dtype" in lib.me_last_error()
    assert apply(heads=0) != 0
    for null in ("x", "y", "tab"):
        assert apply(**{null: None}) != 0
        assert b"must be given" in lib.me_last_error()
    assert apply(x=None, y=None, tab=None, n=0) == 0
    assert apply(x=None, y=None, tab=None, n=0, sign=3) != 0                    # the arguments are checked for n = 0 too
