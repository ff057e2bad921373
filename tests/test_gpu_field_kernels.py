"""Entry-point tests of the three pieces every tensor-field operator runs on (csrc/field.hip): the stable CSR build
(me_csr_from_coo over the radix argsort of csrc/coords.hip), the weighted CSR gather-sum (k_csr_gather) and the
interpolation map (k_interp_probe / k_interp_count_wide / k_interp_fill), plus the fp32 coordinate arithmetic of
k_quantize / k_lookup.  Every expected value is a plain restatement on the CPU in numpy / torch float64 (integer maps in
numpy integers); every tolerance is worked out from the arithmetic in the comments, none from the kernels' output.

The inputs are built on the CPU by cached builders; the `test_inputs_*` tests check the properties the GPU tests rely on
(which corner counts occur, which row lengths, which radix pass counts) and need no GPU."""
import ctypes
import functools
import re
import os

import numpy as np
import pytest
import torch

from test_gpu_interpolation import _expected_map

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 2.0 ** -24          # unit roundoff of fp32 (half an ulp, relative)


def _me():
    import minkowskiengine_amd as ME
    return ME


def _backend():
    from minkowskiengine_amd import backend
    return backend


# =====================================================================================================================
# 1. CSR from COO
# =====================================================================================================================
# csrc/coords.hip: `constexpr int kRsTile = 1024;` (elements per block of a radix pass) and
# `constexpr int64_t kScanSingleMax = 4 * kScanSingleThreads * kScanSingleItems;  // 32768 items` with
# `kScanSingleThreads = 1024, kScanSingleItems = 8`.  The histogram of a pass has 256 * ceil(nnz / kRsTile) counters and is
# scanned by the single-workgroup kernel up to kScanSingleMax of them: nnz <= 32768 / 256 * 1024 = 131072.
K_RS_TILE = 1024
K_SCAN_SINGLE_MAX = 32768
NNZ_THREE_LAUNCH_SCAN = K_SCAN_SINGLE_MAX // 256 * K_RS_TILE + 1      # 131073: 129 blocks, 33024 counters

CSR_SHAPES = [
    (0, 5),                                  # nnz == 0: the memset of rowptr, no sort
    (1, 1),                                  # bits == 0: k_iota_copy, one entry
    (300, 1),                                # bits == 0: k_iota_copy (0 radix passes)
    (300, 2),                                # bits == 1: 1 pass
    (5000, 256),                             # bits == 8: 1 pass, lands in the outputs directly
    (5000, 257),                             # bits == 9: 2 passes, the first lands in the temporaries
    (70000, 65536),                          # bits == 16: 2 passes
    (70000, 65537),                          # bits == 17: 3 passes
    (K_RS_TILE - 1, 300),                    # one partial tile
    (K_RS_TILE, 300),                        # one full tile
    (K_RS_TILE + 1, 300),                    # a full tile and a one-element tile
    (NNZ_THREE_LAUNCH_SCAN - 1, 1000),       # 32768 counters: the last size of the single-workgroup scan
    (NNZ_THREE_LAUNCH_SCAN, 1000),           # 33024 counters: the three-launch scan
]
CSR_BIG = (3000, 2 ** 24 + 1)                # bits == 25: 4 passes
KEY_PATTERNS = ["uniform", "equal", "ends", "inner", "ascending", "descending"]


def _radix_passes(n_rows):
    bits = 0
    while bits < 32 and (1 << bits) < n_rows:
        bits += 1
    return (bits + 7) // 8


def _keys(pattern, nnz, n_rows, seed):
    """int32 keys of one pattern, or None where the pattern cannot exist at this shape"""
    rng = np.random.default_rng(seed)
    if pattern == "uniform":
        k = rng.integers(0, n_rows, nnz)
    elif pattern == "equal":                 # one populated row in the middle: leading and trailing empty rows
        k = np.full(nnz, n_rows // 2)
    elif pattern == "ends":                  # only rows 0 and n_rows - 1: every interior row empty
        k = rng.integers(0, 2, nnz) * (n_rows - 1)
    elif pattern == "inner":                 # first and last rows empty
        if n_rows < 3:
            return None
        k = rng.integers(1, n_rows - 1, nnz)
    elif pattern == "ascending":
        k = np.sort(rng.integers(0, n_rows, nnz))
    elif pattern == "descending":
        k = np.sort(rng.integers(0, n_rows, nnz))[::-1]
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(k, dtype=np.int32)


def _distinct_bits(nnz, nbytes):
    """nnz values with pairwise distinct bit patterns (a multiplicative hash by an odd constant is a bijection), so that
    no wrong permutation can pass; compared as integers, whatever they mean as floats (NaNs included)"""
    if nbytes == 4:
        return (np.arange(nnz, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32).view(np.int32)
    return (np.arange(nnz, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)).view(np.int64)


def _csr_reference(keys, n_rows, cols, vals):
    order = np.argsort(keys, kind="stable")
    rowptr = np.searchsorted(keys[order], np.arange(n_rows + 1))
    cols_out = cols[order] if cols is not None else order
    return rowptr, cols_out, (vals[order] if vals is not None else None)


def _csr_value_kinds(nnz, seed):
    """(cols | None, integer view of vals | None, torch dtype of vals) combinations run for every key pattern"""
    cols = np.random.default_rng(seed).integers(0, 2 ** 31 - 1, nnz).astype(np.int32)
    return [(None, None, None),                                     # entry indices, no values (voxel CSR of a field)
            (cols, None, None),                                     # spmm_average
            (cols, _distinct_bits(nnz, 4), torch.float32),          # k_csr_permute<uint32_t>
            (cols, _distinct_bits(nnz, 8), torch.float64)]          # k_csr_permute<uint64_t>


def _run_csr(device, keys, n_rows, cols, vbits, vdtype):
    B = _backend()
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)      # noqa: E731
    vals = None if vbits is None else t(vbits).view(vdtype)
    rowptr, cols_out, vals_out = B.CsrFromCooGPU(t(keys), n_rows, t(cols), vals)
    assert rowptr.dtype == torch.int32 and cols_out.dtype == torch.int32
    assert (vals_out is None) == (vals is None)
    if vals_out is not None:
        assert vals_out.dtype == vdtype
        vals_out = vals_out.view(torch.int32 if vdtype == torch.float32 else torch.int64).cpu().numpy()
    return rowptr, cols_out.cpu().numpy(), vals_out


def test_inputs_csr_shapes_cover_the_pass_counts():
    """the shapes reach 0, 1, 2, 3 and 4 radix passes, both sides of every flip, and both scan paths"""
    p = {s: _radix_passes(s[1]) for s in CSR_SHAPES + [CSR_BIG]}
    assert p[(300, 1)] == 0 and p[(1, 1)] == 0 and p[(300, 2)] == 1
    assert p[(5000, 256)] == 1 and p[(5000, 257)] == 2
    assert p[(70000, 65536)] == 2 and p[(70000, 65537)] == 3 and p[CSR_BIG] == 4
    counters = lambda nnz: 256 * -(-nnz // K_RS_TILE)                         # noqa: E731
    assert counters(NNZ_THREE_LAUNCH_SCAN - 1) == K_SCAN_SINGLE_MAX < counters(NNZ_THREE_LAUNCH_SCAN)
    src = open(os.path.join(HERE, "..", "minkowskiengine_amd", "csrc", "coords.hip")).read()
    assert int(re.search(r"constexpr int kRsTile = (\d+);", src).group(1)) == K_RS_TILE
    m = re.search(r"constexpr int kScanSingleThreads = (\d+), kScanSingleItems = (\d+);", src)
    assert re.search(r"kScanSingleMax = 4 \* kScanSingleThreads \* kScanSingleItems;", src)
    assert 4 * int(m.group(1)) * int(m.group(2)) == K_SCAN_SINGLE_MAX
    # the patterns have the empty rows their names promise
    k = _keys("inner", 5000, 257, 0)
    assert k.min() >= 1 and k.max() <= 255
    k = _keys("ends", 5000, 257, 0)
    assert set(k.tolist()) == {0, 256}


@pytest.mark.parametrize("nnz,n_rows", CSR_SHAPES, ids=lambda v: str(v))
def test_csr_from_coo(device, nnz, n_rows):
    for ip, pattern in enumerate(KEY_PATTERNS):
        keys = _keys(pattern, nnz, n_rows, 7 * ip + nnz)
        if keys is None:
            continue
        for cols, vbits, vdtype in _csr_value_kinds(nnz, ip):
            want = _csr_reference(keys, n_rows, cols, vbits)
            rowptr, cols_out, vals_out = _run_csr(device, keys, n_rows, cols, vbits, vdtype)
            tag = f"{pattern} cols={'given' if cols is not None else None} vals={vdtype}"
            assert np.array_equal(rowptr.cpu().numpy(), want[0]), tag
            assert np.array_equal(cols_out, want[1]), tag
            if vbits is not None:
                assert np.array_equal(vals_out, want[2]), tag


def test_csr_from_coo_four_passes(device):
    """n_rows = 2^24 + 1: bits == 25, 4 passes (the first lands in the temporaries).  The 64 MiB row pointer is compared
    on the device."""
    nnz, n_rows = CSR_BIG
    ar = np.arange(n_rows + 1)
    for ip, pattern in enumerate(KEY_PATTERNS):
        keys = _keys(pattern, nnz, n_rows, 11 * ip)
        order = np.argsort(keys, kind="stable")
        want_rowptr = torch.from_numpy(np.searchsorted(keys[order], ar).astype(np.int32)).to(device)
        for cols, vbits, vdtype in _csr_value_kinds(nnz, ip):
            _, want_cols, want_vals = _csr_reference(keys, 1, cols, vbits)
            rowptr, cols_out, vals_out = _run_csr(device, keys, n_rows, cols, vbits, vdtype)
            assert torch.equal(rowptr, want_rowptr), pattern
            assert np.array_equal(cols_out, want_cols), pattern
            if vbits is not None:
                assert np.array_equal(vals_out, want_vals), pattern


@pytest.mark.parametrize("n_rows,distinct", [(1, [0]), (200, [0, 3, 199]), (300, [0, 255, 256, 299]),
                                             (70000, [0, 255, 256, 65535, 65536, 69999])],
                         ids=["0pass", "1pass", "2pass", "3pass"])
def test_csr_from_coo_is_stable(device, n_rows, distinct):
    """cols=None with heavily repeated keys: the entry indices ascend within every row (what makes every backward built
    on this transpose bit-reproducible), for 0, 1, 2 and 3 passes"""
    B = _backend()
    nnz = 50000
    keys = np.random.default_rng(n_rows).choice(np.asarray(distinct, dtype=np.int32), nnz)
    rowptr, cols, _ = B.CsrFromCooGPU(torch.from_numpy(keys).to(device), n_rows)
    rowptr, cols = rowptr.cpu().numpy().astype(np.int64), cols.cpu().numpy().astype(np.int64)
    assert rowptr[0] == 0 and rowptr[-1] == nnz and np.all(np.diff(rowptr) >= 0)
    assert np.array_equal(np.sort(cols), np.arange(nnz))                       # a permutation of the entries
    starts = np.zeros(nnz, dtype=bool)
    starts[rowptr[:-1][rowptr[:-1] < nnz]] = True
    ascending = np.diff(cols) > 0
    assert np.all(ascending | starts[1:])                                      # descents only where a new row starts
    row_of = np.searchsorted(rowptr, np.arange(nnz), side="right") - 1
    assert np.array_equal(keys[cols], row_of)


# =====================================================================================================================
# 2. Gather-sum
# =====================================================================================================================
# one row of each length around EB = 8 (0, 1, 7, 8, 9, 16, 17) and 40 (five full blocks), shuffled; empty rows first,
# last and next to each other
ROW_LENGTHS = [0, 0, 17, 1, 0, 8, 40, 7, 0, 0, 16, 9, 0]
N_X = 50
GATHER_CHANNELS = {
    # fp32: 16-byte pieces (C % 4 == 0: 4, 8), 8-byte pieces (C % 2 == 0: 2, 6, 130), one channel (1, 3)
    torch.float32: [1, 2, 3, 4, 6, 8, 130],
    # bf16: 16-byte pieces (C % 8 == 0: 8, 24), 8-byte pieces (C % 4 == 0: 4, 12, 20), one channel (1, 2)
    torch.bfloat16: [1, 2, 4, 8, 12, 20, 24],
    # float64: 16-byte pieces (C % 2 == 0: 2, 4), one channel (1, 3, 7)
    torch.float64: [1, 2, 3, 4, 7],
}
GATHER_CASES = [(dt, c) for dt, cs in GATHER_CHANNELS.items() for c in cs]


@functools.lru_cache(maxsize=None)
def _gather_csr():
    """(rowptr, col, w64, scale64): hand-built CSR; columns repeat within a row and include row 0 and the last row of x.
    w and scale are fp32-representable so that the same values serve every dtype exactly."""
    rng = np.random.default_rng(5)
    rowptr = np.concatenate([[0], np.cumsum(ROW_LENGTHS)]).astype(np.int32)
    col = rng.integers(0, N_X, rowptr[-1]).astype(np.int32)
    for r, n in enumerate(ROW_LENGTHS):
        e0 = rowptr[r]
        if n >= 2:
            col[e0 + 1] = col[e0]                      # a repeated column
        if n >= 7:
            col[e0 + n - 1] = N_X - 1                  # the last row of x, as the row's last entry
            col[e0 + 2] = 0                            # row 0 of x
    w = (rng.uniform(0.25, 1.0, rowptr[-1]) * rng.choice([-1.0, 1.0], rowptr[-1])).astype(np.float32).astype(np.float64)
    scale = (rng.uniform(0.5, 2.0, len(ROW_LENGTHS)) * rng.choice([-1.0, 1.0], len(ROW_LENGTHS)))
    return rowptr, col, w, scale.astype(np.float32).astype(np.float64)


def _gather_x(dtype, c, device):
    """x [N_X, c] on the device and its exact float64 value.  fp32 / bf16: both signs (their bound is absolute in
    sum|w x|); float64: positive, with positive weights, so that the relative bound of the issue means something."""
    rng = np.random.default_rng(1000 + c)
    x = rng.uniform(0.5, 1.5, (N_X, c))
    if dtype != torch.float64:
        x *= rng.choice([-1.0, 1.0], (N_X, c))
    xt = torch.from_numpy(x).to(dtype).to(device)
    return xt, xt.double().cpu().numpy()


def _gather_reference(x64, rowptr, col, w64, scale64):
    """float64: y[r] = scale[r] * sum_e w[e] * x[col[e]]; and S[r] = |scale[r]| * sum_e |w[e] * x[col[e]]|"""
    n_rows, c = len(rowptr) - 1, x64.shape[1]
    y, S = np.zeros((n_rows, c)), np.zeros((n_rows, c))
    for r in range(n_rows):
        e = slice(rowptr[r], rowptr[r + 1])
        t = x64[col[e]] * (1.0 if w64 is None else w64[e, None])
        sc = 1.0 if scale64 is None else scale64[r]
        y[r], S[r] = sc * t.sum(0), abs(sc) * np.abs(t).sum(0)
    return y, S


def _fp32_bound(L, S, extra):
    """A chain of L fp32 fma (or additions) into one accumulator rounds L times, each by at most 2^-24 of a partial sum
    that is at most sum|w x|: L * 2^-24 * S.  `extra` further roundings of the finished sum (the product with the scale;
    a scale that is itself a rounded quotient) add 2^-24 * S each."""
    return (np.asarray(L, dtype=np.float64)[:, None] + extra) * U32 * S


def _bf16_half_ulp(y):
    """half a bf16 ulp (8 significant bits) of y: |y| in [2^(e-1), 2^e) has ulp 2^(e-8)"""
    _, e = np.frexp(np.abs(y))
    return np.where(y == 0, 0.0, np.ldexp(1.0, e - 9))


def _assert_gather(y, dtype, ref, S, lengths, scaled):
    got = y.double().cpu().numpy()
    assert np.all(np.isfinite(got))
    empty = np.asarray(lengths) == 0
    assert np.count_nonzero(got[empty]) == 0                                   # empty rows: exactly zero
    if dtype == torch.float64:
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
        return
    bound = _fp32_bound(lengths, S, 1 if scaled else 0)
    if dtype == torch.bfloat16:
        bound = bound + _bf16_half_ulp(ref)
    err = np.abs(got - ref)
    assert np.all(err <= bound), f"max error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}"


def test_inputs_gather_rows():
    rowptr, col, w, scale = _gather_csr()
    lengths = np.diff(rowptr).tolist()
    assert sorted(lengths) == sorted([0] * 6 + [1, 7, 8, 9, 16, 17, 40])
    assert lengths[0] == 0 and lengths[-1] == 0 and (0, 0) in set(zip(lengths, lengths[1:]))
    assert col.min() == 0 and col.max() == N_X - 1
    assert all(col[rowptr[r]] == col[rowptr[r] + 1] for r in range(len(lengths)) if lengths[r] >= 2)
    assert np.array_equal(w, w.astype(np.float32)) and np.array_equal(scale, scale.astype(np.float32))
    # the channel counts reach every piece width of every dtype (csr_gather: 16 bytes, else 8 bytes, else one channel)
    width = lambda c, es: 16 // es if c % (16 // es) == 0 else (8 // es if es < 8 and c % (8 // es) == 0 else 1)  # noqa: E731
    assert {width(c, 4) for c in GATHER_CHANNELS[torch.float32]} == {4, 2, 1}
    assert {width(c, 2) for c in GATHER_CHANNELS[torch.bfloat16]} == {8, 4, 1}
    assert {width(c, 8) for c in GATHER_CHANNELS[torch.float64]} == {2, 1}
    assert width(20, 2) == 4 and width(12, 2) == 4                              # the bf16 8-byte branch beyond C = 20


@pytest.mark.parametrize("dtype,c", GATHER_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_csr_gather(device, dtype, c):
    B = _backend()
    rowptr, col, w64, scale64 = _gather_csr()
    if dtype == torch.float64:
        w64 = np.abs(w64)
        scale64 = np.abs(scale64)
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    x, x64 = _gather_x(dtype, c, device)
    rp, cl = torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device)
    w, scale = torch.from_numpy(w64).to(acc).to(device), torch.from_numpy(scale64).to(acc).to(device)
    lengths = np.diff(rowptr)
    for use_w in (True, False):                    # fma(w, x, acc) / acc + x
        for use_s in (True, False):                # w with scale, scale without w, and neither
            ref, S = _gather_reference(x64, rowptr, col, w64 if use_w else None, scale64 if use_s else None)
            # the output is allocated right after a NaN-filled block of its size was freed: a row the kernel does not
            # write shows as NaN
            poison = torch.full((len(lengths), c), float("nan"), dtype=dtype, device=device)
            del poison
            y = B.CsrGatherGPU(x, rp, cl, w if use_w else None, scale if use_s else None)
            assert y.shape == (len(lengths), c) and y.dtype == dtype
            _assert_gather(y, dtype, ref, S, lengths, use_s)


@pytest.mark.parametrize("dtype,c", [(torch.float32, 8), (torch.float32, 6), (torch.bfloat16, 8), (torch.bfloat16, 12)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_csr_gather_bits_do_not_depend_on_the_piece_width(device, dtype, c):
    """the sum order is the entry order whatever the width: the 16-byte (C = 8) and 8-byte (fp32 C = 6, bf16 C = 12)
    kernels give, column by column, the bits of the one-channel kernel"""
    B = _backend()
    rowptr, col, w64, scale64 = _gather_csr()
    x, _ = _gather_x(dtype, c, device)
    rp, cl = torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device)
    w, scale = torch.from_numpy(w64).float().to(device), torch.from_numpy(scale64).float().to(device)
    for ww, ss in ((w, scale), (None, scale), (w, None), (None, None)):
        y = B.CsrGatherGPU(x, rp, cl, ww, ss)
        for j in range(c):
            yj = B.CsrGatherGPU(x[:, j:j + 1].contiguous(), rp, cl, ww, ss)
            assert torch.equal(y[:, j:j + 1], yj), j


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (1, 2)), (torch.bfloat16, (1, 4))], ids=["f32", "bf16"])
def test_csr_gather_c_abi_unaligned(device, dtype, offsets):
    """The alignment fallback of csr_gather (torch's own allocations never take it): x and y offset into larger
    allocations by 4 and 8 bytes (fp32, C = 8: one channel, 8-byte pieces) and by 2 and 8 bytes (bf16, C = 8: one channel,
    8-byte pieces) give the bits of the aligned 16-byte call.  Every offset is a multiple of the element size and stays
    inside its allocation; every column is inside x."""
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    fn = lib.me_csr_gather_f32 if dtype == torch.float32 else lib.me_csr_gather_bf16
    c = 8
    rowptr, col, w64, scale64 = _gather_csr()
    n_rows = len(rowptr) - 1
    assert col.min() >= 0 and col.max() < N_X
    x, _ = _gather_x(dtype, c, device)
    rp, cl = torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device)
    w, scale = torch.from_numpy(w64).float().to(device), torch.from_numpy(scale64).float().to(device)
    es = x.element_size()
    stream = torch.cuda.current_stream(device).cuda_stream

    def run(off):
        bx = torch.zeros(N_X * c + 16, dtype=dtype, device=device)
        by = torch.full((n_rows * c + 16,), float("nan"), dtype=dtype, device=device)
        xo, yo = bx[off:off + N_X * c].view(N_X, c), by[off:off + n_rows * c].view(n_rows, c)
        xo.copy_(x)
        assert bx.data_ptr() % 16 == 0 and by.data_ptr() % 16 == 0
        assert xo.data_ptr() == bx.data_ptr() + off * es and yo.data_ptr() == by.data_ptr() + off * es
        with torch.cuda.device(device):
            _lib.check(fn(xo.data_ptr(), c, rp.data_ptr(), cl.data_ptr(), w.data_ptr(), scale.data_ptr(), n_rows,
                          yo.data_ptr(), stream))
        torch.cuda.synchronize(device)
        # nothing outside the rows of y was written
        assert bool(torch.isnan(by[:off]).all()) and bool(torch.isnan(by[off + n_rows * c:]).all())
        return yo.clone()

    aligned = run(0)                                                 # 16-byte pieces
    assert torch.equal(aligned, _backend().CsrGatherGPU(x, rp, cl, w, scale))
    for off in offsets:
        assert (off * es) % 16 != 0                                  # routed to a narrower piece by aligned()
        assert torch.equal(run(off), aligned), off * es


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_coo_spmm_entry_points(device, dtype):
    """coo_spmm_int32 (w, no scale) and coo_spmm_average_int32 (scale, no w) against float64 restatements, on a matrix
    with empty rows (leading, trailing, interior) and 2 radix passes (300 rows)"""
    B = _backend()
    rng = np.random.default_rng(3)
    dim_i, dim_j, nnz, c = 300, 40, 2000, 6
    rows = rng.choice(np.arange(5, 280, 2), nnz).astype(np.int32)
    cols = rng.integers(0, dim_j, nnz).astype(np.int32)
    vals = rng.uniform(0.25, 1.0, nnz).astype(np.float32).astype(np.float64)
    mat = torch.from_numpy(rng.uniform(0.5, 1.5, (dim_j, c))).to(dtype)
    m64 = mat.double().numpy()
    t = lambda a: torch.from_numpy(a).to(device)                                # noqa: E731
    count = np.bincount(rows, minlength=dim_i)
    ref = np.zeros((dim_i, c))
    np.add.at(ref, rows, vals[:, None] * m64[cols])
    out = B.coo_spmm_int32(t(rows), t(cols), t(vals).to(dtype), dim_i, dim_j, mat.to(device))
    avg = np.zeros((dim_i, c))
    np.add.at(avg, rows, m64[cols])
    avg /= np.maximum(count, 1)[:, None]
    out_a, row_of, col_of, val_of = B.coo_spmm_average_int32(t(rows), t(cols), dim_i, dim_j, mat.to(device))
    order = np.argsort(rows, kind="stable")
    assert np.array_equal(row_of.cpu().numpy(), rows[order]) and np.array_equal(col_of.cpu().numpy(), cols[order])
    if dtype == torch.float64:
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out_a.cpu().numpy(), avg, rtol=1e-12, atol=0)
        np.testing.assert_allclose(val_of.cpu().numpy(), 1.0 / count[rows[order]], rtol=1e-15)
    else:
        # all terms positive: sum|w x| is the reference itself.  The average rounds the quotient 1 / count and the product
        assert np.all(np.abs(out.double().cpu().numpy() - ref) <= _fp32_bound(count, ref, 0))
        assert np.all(np.abs(out_a.double().cpu().numpy() - avg) <= _fp32_bound(count, avg, 2))
        np.testing.assert_allclose(val_of.double().cpu().numpy(), 1.0 / count[rows[order]], rtol=U32)
    assert np.count_nonzero(out.cpu().numpy()[count == 0]) == 0
    assert np.count_nonzero(out_a.cpu().numpy()[count == 0]) == 0


def test_empty_matrix_with_values(host_layer, device):
    """nnz == 0 WITH values (an empty tensor has a null address): me_csr_from_coo refused it ("vals and vals_out go
    together") before looking at nnz, so a product with an empty matrix and the backward of an interpolation whose
    samples have no corner at all raised instead of giving zeros"""
    ME = _me()
    from minkowskiengine_amd import host
    B = host.backend()
    e32 = torch.empty(0, dtype=torch.int32, device=device)
    rowptr, cols, vals = B.CsrFromCooGPU(e32, 5, e32, torch.empty(0, device=device))
    assert rowptr.tolist() == [0] * 6 and cols.numel() == 0 and vals.numel() == 0 and vals.dtype == torch.float32
    mat = torch.rand(4, 3, device=device)
    out = B.coo_spmm_int32(e32, e32, torch.empty(0, device=device), 5, 4, mat)
    assert torch.equal(out, torch.zeros(5, 3, device=device))
    vox = torch.tensor([[0, 0, 0, 0], [0, 1, 2, 3]], dtype=torch.int32, device=device)
    ff = torch.rand(2, 3, dtype=torch.float64, device=device, requires_grad=True)
    s = ME.SparseTensor(ff.detach(), coordinates=vox)
    q = torch.tensor([[0, 50.5, 50.5, 50.5], [0, -70.25, 3.0, 1.0]], dtype=torch.float64, device=device)
    out = ME.MinkowskiInterpolationFunction.apply(ff, q, s.coordinate_map_key, s.coordinate_manager)[0]
    assert torch.equal(out, torch.zeros(2, 3, dtype=torch.float64, device=device))
    (g,) = torch.autograd.grad(out, ff, torch.ones_like(out))
    assert torch.equal(g, torch.zeros_like(ff))


# =====================================================================================================================
# 3. Interpolation map beyond D = 2..4
# =====================================================================================================================
INTERP_SAMPLES = {
    1: 1000,     # NV = 2: 32 points per wave; 2000 corner threads, the last wave is partial (2000 % 64 == 16)
    5: 101,      # NV = 32: two points per wave; the last wave holds one point, its partner's lanes are invalid
    6: 70,       # NV = 64: one point owns the whole wave (shift count 64 - NV == 0)
    7: 40,       # NV = 128: no ballot, k_interp_count_wide
}
INTERP_MIXED = {1: [3], 5: [2, 1, 3, 1, 2], 6: [1, 2, 1, 3, 2, 1], 7: [2, 1, 1, 3, 1, 2, 1]}
INTERP_CASES = [(D, mixed) for D in (1, 5, 6, 7) for mixed in (False, True)]


@functools.lru_cache(maxsize=None)
def _interp_case(D, mixed):
    """-> (voxels int32 [M, D + 1] unique, samples float64 [n, D + 1], tensor stride): two batches; samples on voxel
    corners, at negative coordinates and far from every voxel; voxels = full 2^D blocks around some samples, blocks with
    one corner missing, single corners, random parts of blocks, and random voxels"""
    ts = INTERP_MIXED[D] if mixed else [1] * D
    tsa = np.asarray(ts, dtype=np.int64)
    n, nv = INTERP_SAMPLES[D], 1 << D
    rng = np.random.default_rng(10 * D + int(mixed))
    extent = 40 if D == 1 else 8
    x = (rng.random((n, D)) - 0.5) * 2 * extent * tsa                 # both signs
    k = max(n // 8, 4)
    x[:k] = np.round(x[:k] / tsa) * tsa                               # exactly on voxel corners
    x[k:k + 3] = 1000.0                                               # no corner present
    b = rng.integers(0, 2, (n, 1))
    q = np.concatenate([b.astype(np.float64), x], 1)
    base = (np.floor(x / tsa) * tsa).astype(np.int64)
    bits = (np.arange(nv)[:, None] >> (D - 1 - np.arange(D))[None, :]) & 1          # corner v -> offsets, [nv, D]
    vox = []
    if D == 1:
        cells = np.arange(-extent - 1, extent + 2)
        for bb in (0, 1):
            keep = cells[rng.random(len(cells)) < 0.35]
            vox.append(np.stack([np.full(len(keep), bb), keep * tsa[0]], 1))
    else:
        free = np.r_[np.arange(0, k), np.arange(k + 3, n)]
        rng.shuffle(free)
        groups = np.array_split(free, [6, 12, 18])                    # full, all but one, one corner, random parts
        for gi, group in enumerate(groups):
            for p in group:
                if gi == 0:
                    keep = np.ones(nv, dtype=bool)
                elif gi == 1:
                    keep = np.ones(nv, dtype=bool)
                    keep[rng.integers(0, nv)] = False
                elif gi == 2:
                    keep = np.zeros(nv, dtype=bool)
                    keep[rng.integers(0, nv)] = True
                else:
                    keep = rng.random(nv) < rng.choice([0.0, 0.1, 0.5, 0.9])
                c = base[p][None, :] + bits[keep] * tsa
                vox.append(np.concatenate([np.full((len(c), 1), b[p, 0]), c], 1))
        r = rng.integers(-extent, extent, (200, D)) * tsa
        vox.append(np.concatenate([rng.integers(0, 2, (200, 1)), r], 1))
    vox = np.unique(np.concatenate(vox, 0), axis=0).astype(np.int32)
    return vox, q, ts


def _corner_counts(vox, q, ts):
    want = _expected_map(vox, q, ts)
    return np.bincount([p for _, p, _ in want], minlength=len(q)), want


@pytest.mark.parametrize("D,mixed", INTERP_CASES)
def test_inputs_interpolation_corner_counts(D, mixed):
    """a property of the inputs: samples with 0, 1, 2^D - 1 and 2^D present corners all occur (D = 1: 0, 1 and 2), some
    samples sit on voxel corners, some at negative coordinates, and the launch shapes are the ones named above"""
    vox, q, ts = _interp_case(D, mixed)
    nv = 1 << D
    counts, _ = _corner_counts(vox, q, ts)
    assert {0, 1, nv - 1, nv} <= set(counts.tolist())
    assert len(set(counts.tolist())) >= min(nv + 1, 6)
    assert np.any(np.all(q[:, 1:] == np.round(q[:, 1:]), 1) & (counts > 0))
    assert np.any((q[:, 1:] < 0).all(1) if D == 1 else (q[:, 1:] < 0).any(1))
    assert set(q[:, 0].tolist()) == {0.0, 1.0} and set(vox[:, 0].tolist()) == {0, 1}
    assert len(q) == INTERP_SAMPLES[D]
    if D <= 5:
        assert (len(q) * nv) % 64 != 0                                # invalid lanes inside the last wave
    if D == 5:
        assert (len(q) * nv) % 64 == 32                               # ... which ends after the first point of a pair


@pytest.mark.parametrize("D,mixed", INTERP_CASES)
def test_interpolation_map_dims(host_layer, device, D, mixed):
    ME = _me()
    vox, q_np, ts = _interp_case(D, mixed)
    nv, n = 1 << D, len(q_np)
    g = torch.Generator().manual_seed(D)
    f = torch.rand(len(vox), 3, generator=g, dtype=torch.float64).to(device) + 0.5
    s = ME.SparseTensor(f, coordinates=torch.from_numpy(vox).to(device), tensor_stride=ts)
    assert s.C.shape == vox.shape
    q = torch.from_numpy(q_np).to(device)
    cm = s.coordinate_manager
    in_map, out_map, w = cm.interpolation_map_weight(s.coordinate_map_key, q)
    counts, want = _corner_counts(s.C.cpu().numpy(), q_np, ts)
    assert {0, 1, nv - 1, nv} <= set(counts.tolist())
    assert in_map.dtype == torch.int32 and out_map.dtype == torch.int32 and w.dtype == torch.float64
    assert np.array_equal(in_map.cpu().numpy(), np.asarray([r for r, _, _ in want], dtype=np.int64))
    assert np.array_equal(out_map.cpu().numpy(), np.asarray([p for _, p, _ in want], dtype=np.int64))
    np.testing.assert_allclose(w.cpu().numpy(), [x for _, _, x in want], rtol=1e-12, atol=0)
    # the row pointer of the forward gather: the entries of sample p are rowptr[p] .. rowptr[p + 1]
    _, _, _, rowptr = cm._manager._interpolation_map(s.coordinate_map_key, q)
    assert np.array_equal(rowptr.cpu().numpy(), np.searchsorted(out_map.cpu().numpy(), np.arange(n + 1)))
    assert np.array_equal(np.diff(rowptr.cpu().numpy()), counts)
    # weights of one sample sum to at most 1, and to 1 with all corners present
    tot = np.zeros(n)
    np.add.at(tot, out_map.cpu().numpy(), w.cpu().numpy())
    assert tot.max() <= 1 + 1e-12
    np.testing.assert_allclose(tot[counts == nv], 1.0, rtol=0, atol=1e-12)
    # forward / backward against the float64 index_add restatement (positive features and weights: no cancellation)
    ff = s.F.clone().requires_grad_(True)
    out = ME.MinkowskiInterpolationFunction.apply(ff, q, s.coordinate_map_key, cm)[0]
    ref = torch.zeros(n, 3, dtype=torch.float64, device=device).index_add(
        0, out_map.long(), ff[in_map.long()] * w[:, None])
    torch.testing.assert_close(out, ref, rtol=1e-10, atol=0)
    assert torch.equal(out[torch.from_numpy(counts == 0).to(device)], torch.zeros(int((counts == 0).sum()), 3,
                                                                                   dtype=torch.float64, device=device))
    gy = torch.rand(n, 3, generator=g, dtype=torch.float64).to(device) + 0.5
    (g1,) = torch.autograd.grad(out, ff, gy)
    (g2,) = torch.autograd.grad(ref, ff, gy)
    torch.testing.assert_close(g1, g2, rtol=1e-10, atol=0)


# =====================================================================================================================
# 4. fp32 coordinate arithmetic
# =====================================================================================================================
F32 = np.float32


def _voxel_f32(x, s):
    """floor(x / s) * s with every operation in float32: the kernels' (and the reference's) arithmetic"""
    x = np.asarray(x, dtype=F32)
    return (np.floor(x / F32(s)) * F32(s)).astype(F32)


def _candidates_f32(s):
    """fp32 coordinates around the voxel boundaries of stride s"""
    out = [F32(-0.0), F32(0.0), F32(0.5), F32(-0.5)]
    for k in (1, 2, 5, 7, -1, -2, -5, -7):                            # k * s and its two neighbours
        v = F32(k * s)
        out += [v, np.nextafter(v, F32(np.inf), dtype=F32), np.nextafter(v, F32(-np.inf), dtype=F32)]
    for big in (2.0 ** 20, -2.0 ** 20):                               # fp32 spacing here: 0.125 above, 0.0625 below 2^20
        for d in (0.0, 0.125, 0.5, 2.875, -0.125, -0.5, -3.0, s, -s, 3 * s + 0.25):
            out.append(F32(big + d))
    return np.asarray(out, dtype=F32)


@functools.lru_cache(maxsize=None)
def _fp32_case(ts):
    """samples float32 [n, 4]: every candidate once in all columns, then random mixes of candidates; batch column at
    b, b +- 0.25 and b + 0.5"""
    rng = np.random.default_rng(sum(ts))
    cands = [_candidates_f32(s) for s in ts]
    m = len(cands[0])
    n = m + 400
    x = np.empty((n, len(ts)), dtype=F32)
    for j, cj in enumerate(cands):
        x[:m, j] = cj
        x[m:, j] = rng.choice(cj, n - m)
    b = rng.choice(np.asarray([0.0, 1.0], dtype=F32), n) + rng.choice(np.asarray([0.0, 0.25, -0.25, 0.5], dtype=F32), n)
    return np.concatenate([b[:, None].astype(F32), x], 1)


def _expected_voxels_f32(q, ts):
    """int64 [n, D + 1]: (rint(x0), floor(x_j / s_j) * s_j) in float32"""
    cols = [np.rint(q[:, 0])] + [_voxel_f32(q[:, j + 1], s) for j, s in enumerate(ts)]
    return np.stack(cols, 1).astype(np.int64)


def _expected_map_f32(coords, q, ts):
    """interpolation_kernel in float32: rows in (sample, corner) order and the weight
    prod_j (1 - |x_j - c_j| / s_j), every operation rounded to float32"""
    table = {tuple(r): i for i, r in enumerate(coords.tolist())}
    D = len(ts)
    base = _expected_voxels_f32(q, ts)
    out = []
    for p in range(len(q)):
        for v in range(1 << D):
            c = [int(base[p, 0])] + [int(base[p, j + 1]) + (ts[j] if (v >> (D - 1 - j)) & 1 else 0) for j in range(D)]
            r = table.get(tuple(c))
            if r is not None:
                w = F32(1)
                for j in range(D):
                    w = F32(w * F32(F32(1) - F32(np.abs(F32(q[p, j + 1] - F32(c[j + 1]))) / F32(ts[j]))))
                out.append((r, p, float(w)))
    return out


FP32_STRIDES = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3)]


@pytest.mark.parametrize("ts", FP32_STRIDES, ids=lambda t: "x".join(map(str, t)))
def test_inputs_fp32_coordinates(ts):
    """properties of the fp32 samples, and the rounding cases stated as numpy computes them"""
    q = _fp32_case(ts)
    assert q.dtype == F32
    # lrint is round-half-to-even, as np.rint: b + 0.5 goes to the EVEN neighbour, b +- 0.25 to b
    assert np.rint(F32(0.5)) == 0 and np.rint(F32(1.5)) == 2
    assert np.rint(F32(0.25)) == 0 and np.rint(F32(-0.25)) == 0 and np.rint(F32(1.25)) == 1 and np.rint(F32(0.75)) == 1
    assert {0.5, 1.5, 0.25, -0.25, 0.75, 1.25} <= set(q[:, 0].tolist())
    for j, s in enumerate(ts):
        x = q[:, j + 1]
        v = _voxel_f32(x, s)
        assert np.all(v == np.round(v)) and np.all(np.abs(v) < 2 ** 24)       # exact integers in fp32 and int32
        # one ulp below a boundary: strictly below it, and the voxel fp32 arithmetic gives
        below = np.nextafter(F32(5 * s), F32(-np.inf), dtype=F32)
        assert below in x and below < F32(5 * s)
        assert np.any(np.signbit(x) & (x == 0))                                # -0.0
        assert np.any(np.abs(x) >= 2 ** 20) and np.any(x < 0)
    assert _voxel_f32(F32(-0.0), 3) == 0 and _voxel_f32(F32(-0.5), 3) == -3 and _voxel_f32(F32(-3.0), 3) == -3


@pytest.mark.parametrize("ts", FP32_STRIDES, ids=lambda t: "x".join(map(str, t)))
def test_fp32_coordinate_arithmetic(host_layer, device, ts):
    ME = _me()
    ts = list(ts)
    D = len(ts)
    q_np = _fp32_case(tuple(ts))
    n = len(q_np)
    q = torch.from_numpy(q_np).to(device)
    want = _expected_voxels_f32(q_np, ts)
    # k_quantize: sparse() gives exactly the voxels of the float32 restatement and the row of every point
    tf = ME.TensorField(torch.ones(n, 1, device=device), coordinates=q,
                        quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM)
    s = tf.sparse(tensor_stride=ts)
    coords = s.C.cpu().numpy().astype(np.int64)
    uniq, first, inv_want = np.unique(want, axis=0, return_index=True, return_inverse=True)
    assert len(coords) == len(uniq) and np.array_equal(np.unique(coords, axis=0), uniq)
    inv = tf.inverse_mapping(s.coordinate_map_key).cpu().numpy()
    assert np.array_equal(coords[inv], want)
    # (UNWEIGHTED_SUM of ones: the number of points of every voxel, small integers, exact in fp32)
    count = np.zeros(len(coords))
    np.add.at(count, inv, 1.0)
    assert np.array_equal(s.F.cpu().numpy()[:, 0], count)
    # k_lookup: every point finds its own voxel again, in field order
    cm = tf.coordinate_manager
    srow, frow = cm.field_to_sparse_map(tf.coordinate_field_map_key, s.coordinate_map_key)
    assert np.array_equal(frow.cpu().numpy(), np.arange(n)) and np.array_equal(srow.cpu().numpy(), inv)
    # the fp32 interpolation map: rows exact, weights within 2 ulp of 1 per factor (a difference, a quotient and a
    # difference from 1 in [0, 1], each correctly rounded, then D - 1 products): atol = D * 2^-22
    in_map, out_map, w = cm.interpolation_map_weight(s.coordinate_map_key, q)
    emap = _expected_map_f32(coords, q_np, ts)
    assert w.dtype == torch.float32
    assert np.array_equal(in_map.cpu().numpy(), np.asarray([r for r, _, _ in emap], dtype=np.int64))
    assert np.array_equal(out_map.cpu().numpy(), np.asarray([p for _, p, _ in emap], dtype=np.int64))
    np.testing.assert_allclose(w.double().cpu().numpy(), [x for _, _, x in emap], rtol=0, atol=D * 2.0 ** -22)
    # every sample has its own voxel as a corner
    assert np.array_equal(np.unique(out_map.cpu().numpy()), np.arange(n))
