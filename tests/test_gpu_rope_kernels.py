"""Entry-point tests of rotary position embedding (csrc/rope.hip, ABI 1.22) through the C ABI on synthetic device tensors:
no manager, no SparseTensor.  The yardstick is the float64 numpy definition of tests/test_rope_cpu.py.

Every output is pre-filled with FILL and followed by a guard of GUARD elements; the gaps between strided output rows
count as guard too.  Bounds (none of them tuned; each figure is printed before it is asserted, pytest -s):

  table, fp32     |e| <= 2^-25 + |t| 2^-51 with t = c / u: rounding a value of [-1, 1] to fp32 costs 2^-25, the angle
                  t omega carries one rounding of t and one of the product, 2 |t| 2^-53 together, and sin / cos move by no
                  more than the angle does; for |t| <= 2^20 that is below 2^-24, which is asserted as well.
  table, float64  |e| <= 2^-52 + |t| 2^-51: one ulp of [-1, 1] for sin / cos on either side instead of the fp32 rounding.
  apply, fp32     per pair |y - y64| <= 2^-21 hypot(x0, x1) for |t| <= 2^20: two table entries at 2^-24 each and three
                  roundings of the products and the sum, about 4 * 2^-24 relative to the pair, doubled.
  apply, float64  (2^-50 + |t|max 2^-50) hypot(x0, x1): the same count on the float64 table bound.
  apply, bf16     bit for bit the fp32 entry point on the widened rows, rounded to bf16 by torch."""
import ctypes

import numpy as np
import pytest
import torch

from minkowskiengine_amd import _lib
from test_rope_cpu import rope_angles, rope_apply, rope_table

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7.0
F32, BF16, F64 = 0, 1, 2
CODE = {torch.float32: F32, torch.bfloat16: BF16, torch.float64: F64}


def _i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _units(unit, D):
    return [int(unit)] * D if np.ndim(unit) == 0 else [int(u) for u in unit]


def _bits(t):
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(view)


def make_table(coords, d, dev, base=10000.0, unit=1, f64=False):
    """me_rope_table under the guard rule -> the table tensor [n, d / 2, 2] on the device"""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    n, ncol = coords.shape
    count = n * d
    c = torch.from_numpy(coords).to(dev) if n > 0 else None
    buf = torch.full((count + GUARD,), FILL, dtype=torch.float64 if f64 else torch.float32, device=dev)
    _lib.check(lib.me_rope_table(c.data_ptr() if n > 0 else None, n, ncol, _i32s(_units(unit, ncol - 1)), d, float(base),
                                 int(f64), buf.data_ptr() if n > 0 else None, None))
    torch.cuda.synchronize(dev)
    assert bool((buf[count:] == FILL).all()), "the table was written past its end"
    return buf[:count].view(n, d // 2, 2)


def apply(x, heads, d, table, sign=1, y_stride=None, out=None):
    """me_rope_apply under the guard rule.  x: a 2-D device tensor or view with a contiguous last dimension -> y as a
    [n, heads * d] view of a buffer of row stride y_stride (default heads * d); gap columns and the guard hold FILL"""
    lib = _lib.load()
    n, c = x.shape
    assert c == heads * d and x.stride(1) == 1
    y_stride = c if y_stride is None else y_stride
    buf = torch.full((n * y_stride + GUARD,), FILL, dtype=x.dtype, device=x.device) if out is None else out
    _lib.check(lib.me_rope_apply(x.data_ptr() if n else None, x.stride(0) if n > 1 else c,
                                 buf.data_ptr() if n else None, y_stride, n, heads, d,
                                 table.data_ptr() if n else None, sign, CODE[x.dtype], None))
    torch.cuda.synchronize(x.device)
    if out is not None:
        return None
    assert bool((buf[n * y_stride:] == FILL).all()), "y was written past its end"
    rows = buf[:n * y_stride].view(n, y_stride)
    assert bool((rows[:, c:] == FILL).all()), "the gap between the rows of y was written"
    return rows[:, :c]


def scene(rng, n, D, reach, unit=1, batches=3):
    """n rows (duplicates allowed) with |c_a / u_a| <= reach on every axis, both signs, the extremes included"""
    u = np.asarray(_units(unit, D), dtype=np.int64)
    pts = rng.integers(-reach, reach + 1, size=(n, D)) * u - rng.integers(0, u, size=(n, D)) * (rng.random((n, D)) < 0.5)
    pts = np.clip(pts, -reach * u, reach * u)
    pts[0] = reach * u
    pts[-1] = -reach * u
    return np.concatenate([rng.integers(0, batches, size=(n, 1)), pts], 1)


def pair_excess(y, y64, x64, bound):
    """the largest |y - y64| of a pair over bound * hypot of the pair (bound: a number or one value per row)"""
    err = np.abs(np.asarray(y, dtype=np.float64) - y64)
    err = np.maximum(err[:, 0::2], err[:, 1::2])
    norm = np.hypot(x64[:, 0::2], x64[:, 1::2])
    limit = np.asarray(bound, dtype=np.float64).reshape(-1, 1) * norm
    assert (norm > 0).all()
    return float((err / limit).max())


# ---- A. the table ---------------------------------------------------------------------------------------------------------------
TABLE_CASES = [(1, 5), (2, (3, 1)), (3, (2, 1, 4)), (4, (1, 2, 3, 7))]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("D,unit", TABLE_CASES, ids=["D1", "D2", "D3", "D4"])
def test_table_fp32_within_two_to_the_minus_24(device, D, unit, n):
    rng = np.random.default_rng(100 * D + n)
    coords = scene(rng, n, D, 1 << 20, unit)
    assert n == 1 or int(coords[:, 1:].min()) < 0
    got = make_table(coords, 32, device, unit=unit).cpu().numpy().astype(np.float64)
    want = rope_table(coords, 32, unit=unit)
    _, t_abs = rope_angles(coords, 32, unit=unit)
    assert float(t_abs.max()) <= float(1 << 20)
    err = np.abs(got - want)
    worst = float(err.max())
    print(f"table fp32 D={D} n={n}: max |e| = {worst * 2 ** 24:.3f} * 2^-24")
    assert worst <= 2.0 ** -24
    assert (err <= 2.0 ** -25 + t_abs[..., None] * 2.0 ** -51).all()
    m = 16 // D
    assert (got[:, D * m:] == np.array([1.0, 0.0])).all()                # the trailing pairs pass through, exactly


def test_table_beyond_one_pass_of_the_capped_grid(device):
    """n = 40000 rows of 16 pairs: 640000 threads' worth of entries under a grid capped at 2048 * 256"""
    rng = np.random.default_rng(40000)
    coords = scene(rng, 40000, 3, 1 << 20, (2, 1, 4))
    got = make_table(coords, 32, device, unit=(2, 1, 4)).cpu().numpy().astype(np.float64)
    err = np.abs(got - rope_table(coords, 32, unit=(2, 1, 4)))
    print(f"table fp32 n=40000: max |e| = {float(err.max()) * 2 ** 24:.3f} * 2^-24")
    assert float(err.max()) <= 2.0 ** -24


@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "float64"])
@pytest.mark.parametrize("D,unit", [(1, 1), (3, (1, 3, 1)), (4, 1)], ids=["D1", "D3", "D4"])
def test_table_over_the_whole_int32_range(device, D, unit, f64):
    rng = np.random.default_rng(7 + D)
    n = 257
    pts = rng.integers(-(1 << 31), 1 << 31, size=(n, D))
    pts[0], pts[1], pts[2] = (1 << 31) - 1, -(1 << 31), 0
    coords = np.concatenate([np.zeros((n, 1), dtype=np.int64), pts], 1)
    for d, base in ((32, 10000.0), (8, 100.0)):
        got = make_table(coords, d, device, base=base, unit=unit, f64=f64).cpu().numpy().astype(np.float64)
        want = rope_table(coords, d, base=base, unit=unit)
        _, t_abs = rope_angles(coords, d, base=base, unit=unit)
        err = np.abs(got - want)
        limit = (2.0 ** -52 if f64 else 2.0 ** -25) + t_abs[..., None] * 2.0 ** -51
        print(f"table {'float64' if f64 else 'fp32'} D={D} d={d}: max e / limit = {float((err / limit).max()):.3e}")
        assert (err <= limit).all()


def test_table_of_no_rows_and_other_bases(device):
    assert make_table(np.zeros((0, 4)), 32, device).shape == (0, 16, 2)
    coords = scene(np.random.default_rng(3), 100, 3, 1000)
    for base in (2.0, 500.0, 1e6):
        got = make_table(coords, 20, device, base=base).cpu().numpy().astype(np.float64)
        assert np.abs(got - rope_table(coords, 20, base=base)).max() <= 2.0 ** -24


# ---- B. apply ------------------------------------------------------------------------------------------------------------------
# (heads, d, D): d = 2 and 6 and 20 take the pair path for some or all dtypes, the others 16-byte pieces
SHAPES = [(1, 2, 1), (3, 6, 3), (8, 8, 3), (3, 20, 3), (8, 32, 3), (1, 64, 4), (3, 128, 2)]
N = 257


def _case(heads, d, D, seed, n=N, reach=1 << 20):
    rng = np.random.default_rng(seed)
    coords = scene(rng, n, D, reach)
    x64 = rng.standard_normal((n, heads * d))
    return coords, x64


@pytest.mark.parametrize("heads,d,D", SHAPES)
@pytest.mark.parametrize("sign", [1, -1])
def test_apply_fp32_within_the_derived_bound(device, heads, d, D, sign):
    coords, x64 = _case(heads, d, D, 1000 + d)
    x = torch.from_numpy(x64).float().to(device)
    x64 = x.cpu().numpy().astype(np.float64)
    table = make_table(coords, d, device)
    y = apply(x, heads, d, table, sign)
    excess = pair_excess(y.cpu().numpy(), rope_apply(x64, coords, heads, sign=sign), x64, 2.0 ** -21)
    print(f"apply fp32 heads={heads} d={d} sign={sign}: max |e| = {excess * 8:.3f} * 2^-24 hypot")
    assert excess <= 1.0
    back = apply(y, heads, d, table, -sign)
    excess = pair_excess(back.cpu().numpy(), x64, x64, 2.0 ** -20)
    print(f"  there and back: {excess * 16:.3f} * 2^-24 hypot")
    assert excess <= 1.0


@pytest.mark.parametrize("heads,d,D", SHAPES)
def test_apply_float64_within_the_derived_bound(device, heads, d, D):
    coords, x64 = _case(heads, d, D, 2000 + d)
    x = torch.from_numpy(x64).to(device)
    table = make_table(coords, d, device, f64=True)
    bound = 2.0 ** -50 + float(1 << 20) * 2.0 ** -50
    for sign in (1, -1):
        y = apply(x, heads, d, table, sign)
        excess = pair_excess(y.cpu().numpy(), rope_apply(x64, coords, heads, sign=sign), x64, bound)
        print(f"apply float64 heads={heads} d={d} sign={sign}: max e / bound = {excess:.3e}")
        assert excess <= 1.0
    back = apply(apply(x, heads, d, table, 1), heads, d, table, -1)
    assert pair_excess(back.cpu().numpy(), x64, x64, 2 * bound) <= 1.0


@pytest.mark.parametrize("heads,d,D", SHAPES)
@pytest.mark.parametrize("sign", [1, -1])
def test_apply_bf16_equals_the_fp32_entry_point_rounded_once(device, heads, d, D, sign):
    coords, x64 = _case(heads, d, D, 3000 + d)
    x = torch.from_numpy(x64).to(device).to(torch.bfloat16)
    table = make_table(coords, d, device)
    got = apply(x, heads, d, table, sign)
    want = apply(x.float(), heads, d, table, sign).to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(_bits(got), _bits(want))


def test_apply_beyond_one_pass_of_the_capped_grid(device):
    """n = 40000 rows of 8 heads of 32: 2.56 million 16-byte pieces under a grid capped at 2048 * 256"""
    heads, d = 8, 32
    coords, x64 = _case(heads, d, 3, 40000, n=40000)
    x = torch.from_numpy(x64).float().to(device)
    x64 = x.cpu().numpy().astype(np.float64)
    y = apply(x, heads, d, make_table(coords, d, device))
    excess = pair_excess(y.cpu().numpy(), rope_apply(x64, coords, heads), x64, 2.0 ** -21)
    print(f"apply fp32 n=40000: max |e| = {excess * 8:.3f} * 2^-24 hypot")
    assert excess <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_apply_on_the_qk_view_of_a_projected_matrix(device, dtype):
    """x = qkv[:, :2C] of qkv [n, 3C] as 2H heads: input stride 3C, output stride 2C and, in a second call, 2C + 8 with the
    gap untouched; qkv itself, the columns of v included, is not written"""
    heads, d, n = 2, 32, 255
    c = heads * d
    coords, x64 = _case(3 * heads, d, 3, 4000, n=n)
    qkv = torch.from_numpy(x64).to(device).to(dtype)
    before = qkv.clone()
    table = make_table(coords, d, device, f64=dtype == torch.float64)
    view = qkv[:, :2 * c]
    assert view.stride(0) == 3 * c
    y = apply(view, 2 * heads, d, table)
    want = apply(view.contiguous(), 2 * heads, d, table)
    assert torch.equal(_bits(y), _bits(want))
    wide = apply(view, 2 * heads, d, table, y_stride=2 * c + 8)
    assert torch.equal(_bits(wide), _bits(want))
    assert torch.equal(_bits(qkv), _bits(before))
    if dtype == torch.float32:
        x64 = view.cpu().numpy().astype(np.float64)
        assert pair_excess(y.cpu().numpy(), rope_apply(x64, coords, 2 * heads), x64, 2.0 ** -21) <= 1.0


@pytest.mark.parametrize("heads,d,D", [(3, 8, 3), (2, 32, 3), (1, 128, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_the_pair_path_gives_the_bits_of_the_vector_path(device, dtype, heads, d, D):
    """a view that starts one pair into a buffer whose row stride is an odd number of pairs (float64, whose piece IS a pair:
    one element in, an odd stride in elements) cannot be cut into aligned 16-byte pieces; the aligned copy of the same
    rows can"""
    n, c = 129, heads * d
    coords, x64 = _case(heads, d, D, 5000 + d, n=n)
    table = make_table(coords, d, device, f64=dtype == torch.float64)
    aligned = torch.from_numpy(x64).to(device).to(dtype)
    off, stride = (1, c + 3) if dtype == torch.float64 else (2, c + 2 + 2 * ((c // 2) % 2))
    assert dtype == torch.float64 or (stride // 2) % 2 == 1
    buf = torch.full((n, stride), FILL, dtype=dtype, device=device)
    view = buf[:, off:off + c]
    view.copy_(aligned)
    assert view.data_ptr() % 16 != 0 or view.stride(0) * view.element_size() % 16 != 0
    for sign in (1, -1):
        want = apply(aligned, heads, d, table, sign)
        got = apply(view, heads, d, table, sign)
        assert torch.equal(_bits(got), _bits(want))
        odd_out = apply(aligned, heads, d, table, sign, y_stride=c + 1)         # an unaligned output alone
        assert torch.equal(_bits(odd_out), _bits(want))


def test_apply_in_place_and_without_rows(device):
    heads, d = 3, 32
    coords, x64 = _case(heads, d, 3, 6000)
    x = torch.from_numpy(x64).float().to(device)
    table = make_table(coords, d, device)
    want = apply(x, heads, d, table)
    work = x.clone()
    apply(work, heads, d, table, out=work)
    assert torch.equal(_bits(work), _bits(want))
    lib = _lib.load()
    for code in (F32, BF16, F64):
        assert lib.me_rope_apply(None, heads * d, None, heads * d, 0, heads, d, None, 1, code, None) == 0
    empty = torch.zeros((0, heads * d), device=device)
    assert apply(empty, heads, d, table).shape == (0, heads * d)
