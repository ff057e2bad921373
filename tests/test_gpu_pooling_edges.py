"""Edges of the pooling / broadcast kernels (csrc/pool.hip) that continuous random features never reach: ties (which
row is the argmax), non-finite and extreme values, the run path of global pooling that shuffled rows take, its chunk
geometry, many uneven batches, the channel limits and empty inputs.

Features and gradients are small integers (exact in fp32 and in bf16, every sum exact whatever its order), so sums,
maxima, argmax masks, max / sum gradients, global sums and broadcast results are compared with array_equal; averages
with float32(sum) / float32(count), rounded once to bf16 where the storage is bf16.

The argmax rule under test: local max pooling keeps the FIRST maximum in ascending kernel-offset order (the order of
the reference's CPU loop, src/pooling_max_kernel.hpp:36-96, on per-offset pair lists); global max pooling keeps the
first row in row order (global_pooling_cpu.cpp).  One documented difference from the reference: for kernel == stride
the reference builds ONE pair list in input-row order (stride_map, coordinate_map_manager.cpp:722-729), so its first
maximum is the first in input-row order; ours stays the first in kernel-offset order, as for every other region.  The
maxima are the same, only the tied row that receives the gradient differs; ours is pinned here (the oracle fed with
the per-offset map), the reference's in tests/test_oracle_pooling.py."""
import numpy as np
import pytest
import torch

from oracle import me_oracle as O
from helpers import make_cloud

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
REGIONS = [(2, 2), (3, 1), (3, 2)]
PAD = 512       # sentinel elements in front of and behind a guarded buffer (a multiple of 16 bytes in both dtypes)


# ---- small helpers -------------------------------------------------------------------------------------------------
def _ints(shape, seed, lo, hi):
    """integer-valued float32 features in [lo, hi)"""
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _np(t):
    return t.detach().float().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _guarded(rows, c, dtype, device):
    """(buffer, [rows, c] view in its middle): PAD sentinels (7.0) in front of and behind the view, one allocation"""
    buf = torch.full((2 * PAD + rows * c,), 7.0, dtype=dtype, device=device)
    return buf, buf[PAD:PAD + rows * c].view(rows, c)


def _sentinels_intact(buf):
    return bool((buf[:PAD] == 7.0).all()) and bool((buf[-PAD:] == 7.0).all())


def _same_exact(got, want, what):
    """NaN where the reference is NaN, the same infinity where it is infinite, every finite element EQUAL (the style
    of _same_nonfinite in test_gpu_conv.py, without a tolerance: the inputs are chosen so that none is needed)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), f"{what}: infinity positions differ"
    assert np.array_equal(got[inf], want[inf]), f"{what}: signs of infinities differ"
    fin = np.isfinite(want)
    assert np.array_equal(got[fin], want[fin]), f"{what}: finite values differ"


# ---- the C ABI, called as backend.py calls it -----------------------------------------------------------------------
def _tag(t):
    return "bf16" if t.dtype == torch.bfloat16 else "f32"


def _pool_max(x, tbl, n_out, dst=None):
    L, lib = _lib()
    c = x.shape[1]
    if dst is None:
        dst = torch.empty((n_out, c), dtype=x.dtype, device=x.device)
    mask = torch.empty((n_out, c), dtype=torch.int32, device=x.device)
    L.check(getattr(lib, "me_pool_max_" + _tag(x))(x.data_ptr(), c, tbl.data_ptr(), n_out, tbl.shape[0], dst.data_ptr(),
                                                  mask.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return dst, mask


def _pool_max_backward(gy, tbl_in, n_in, mask, grad_in):
    L, lib = _lib()
    L.check(getattr(lib, "me_pool_max_backward_" + _tag(gy))(gy.data_ptr(), gy.shape[1], tbl_in.data_ptr(), n_in,
                                                           tbl_in.shape[0], mask.data_ptr(), grad_in.data_ptr(),
                                                           _stream()))
    torch.cuda.synchronize()


def _pool_sum(x, tbl, n_out, average):
    L, lib = _lib()
    c = x.shape[1]
    dst = torch.empty((n_out, c), dtype=x.dtype, device=x.device)
    cnt = torch.empty(n_out, dtype=torch.float32, device=x.device)
    L.check(getattr(lib, "me_pool_sum_" + _tag(x))(x.data_ptr(), c, tbl.data_ptr(), n_out, tbl.shape[0], None,
                                                  1 if average else 0, dst.data_ptr(), cnt.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return dst, cnt


def _global_pool_rc(x, x2, rows, n_batch, mode, c=None, n=None):
    """-> (status, dst fp32 [n_batch, c], argmax int32 | None, count fp32 | None); the outputs start as 7 / 7 / 7 so that
    a refused call can be seen to have written nothing"""
    L, lib = _lib()
    dev = rows.device
    n = int(x.shape[0]) if n is None else n
    c = int(x.shape[1]) if c is None else c
    bf16 = x is not None and x.dtype == torch.bfloat16
    dst = torch.full((n_batch, c), 7.0, dtype=torch.float32, device=dev)
    arg = torch.full((n_batch, c), 7, dtype=torch.int32, device=dev) if mode == 2 else None
    cnt = torch.full((n_batch,), 7.0, dtype=torch.float32, device=dev) if mode != 2 else None
    ws = torch.empty(max(int(lib.me_global_pool_workspace_bytes(n, n_batch, c)), 1), dtype=torch.uint8, device=dev)
    fn = lib.me_global_pool_bf16 if bf16 else lib.me_global_pool_f32
    rc = fn(_ptr(x), _ptr(x2), c, _ptr(rows), n, n_batch, mode, dst.data_ptr(), _ptr(arg), _ptr(cnt), ws.data_ptr(),
            ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, dst, arg, cnt


def _global_pool(x, x2, rows, n_batch, mode):
    L, _ = _lib()
    rc, dst, arg, cnt = _global_pool_rc(x, x2, rows, n_batch, mode)
    L.check(rc)
    return dst.cpu().numpy(), None if arg is None else arg.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def np_global(x, rows, n_batch, x2=None):
    """Vectorised numpy statement of global pooling over float32 rows `x` [n, c] with origin rows `rows` [n]:
    -> (sum fp32, count fp32, max fp32, argmax int32).  Sums are accumulated in float64 and rounded once (exact for the
    integer inputs of this module; +-inf / NaN propagate as in fp32).  Maxima follow the reference's loop
    (`best < x` from -FLT_MAX / -1 in row order): NaN never wins, the FIRST row that attains the maximum is kept
    (numpy's argmax returns the first), a batch whose values never exceed -FLT_MAX keeps -FLT_MAX / -1."""
    x = np.asarray(x, np.float32)
    if x2 is not None:
        x = x * np.asarray(x2, np.float32)
    rows = np.asarray(rows, np.int64)
    n, c = x.shape
    s = np.zeros((n_batch, c), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(s, rows, x.astype(np.float64))
        s = s.astype(np.float32)
    cnt = np.bincount(rows, minlength=n_batch).astype(np.float32)
    mx = np.full((n_batch, c), -FLT_MAX, np.float32)
    arg = np.full((n_batch, c), -1, np.int32)
    val = np.where(np.isnan(x), -np.inf, x)
    for b in np.unique(rows):
        idx = np.nonzero(rows == b)[0]
        a = val[idx].argmax(0)
        m = val[idx[a], np.arange(c)]
        win = m > -FLT_MAX
        mx[b] = np.where(win, m, -FLT_MAX)
        arg[b] = np.where(win, idx[a] * c + np.arange(c), -1)
    return s, cnt, mx, arg


def np_avg(s, cnt):
    """float32(sum) / float32(count); rows without a point keep their sum (0)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (s / np.maximum(cnt, 1.0)[:, None].astype(np.float32)).astype(np.float32)


# ---- 1. local max pooling under ties --------------------------------------------------------------------------------
_CPU_MAPS, _MAPS, _REFS = {}, {}, {}


def cpu_map(ks, stride, n=6000, extent=24):
    """coordinates, strided output coordinates and the oracle's kernel map (no GPU work; tests/test_oracle_pooling.py
    checks the tie share on it)"""
    key = (ks, stride, n, extent)
    if key not in _CPU_MAPS:
        coords = make_cloud(n, extent, 3, seed=11, batch=2, negative=True)
        out_c, _ = O.stride_map(coords.numpy(), [stride] * 3)
        nbr, okm = O.kernel_map(coords.numpy(), out_c, O.make_region(3, ks, 1, 1))
        _CPU_MAPS[key] = dict(coords=coords, out_c=out_c, nbr=nbr, okm=okm, n_in=coords.shape[0], n_out=out_c.shape[0])
    return _CPU_MAPS[key]


def _local_map(device, ks, stride, n=6000, extent=24):
    """cpu_map plus the neighbour tables of the real kernel map of the same coordinates (python host manager)"""
    key = (ks, stride, n, extent)
    if key not in _MAPS:
        from minkowskiengine_amd import backend as MEB
        m = dict(cpu_map(ks, stride, n, extent))
        mgr = MEB.CoordinateMapManagerGPU_c10()
        ikey, _ = mgr.insert_and_map(m["coords"].to(device), [1, 1, 1], "")
        okey = mgr.stride(ikey, [stride] * 3)
        km = mgr._kernel_map(ikey, okey, [ks] * 3, [stride] * 3, [1] * 3, MEB.RegionType.HYPER_CUBE, None, False, True)
        assert np.array_equal(mgr.get_coordinates(okey).cpu().numpy(), m["out_c"])
        assert (km.n_in, km.n_out) == (m["n_in"], m["n_out"])
        tbl_out, tbl_in = km.table("out").contiguous(), km.table("in").contiguous()
        assert np.array_equal(tbl_out.cpu().numpy()[:, :km.n_out], m["nbr"]), "neighbour table differs from the oracle's"
        m.update(tbl_out=tbl_out, tbl_in=tbl_in, keep=(mgr, km))
        _MAPS[key] = m
    return _MAPS[key]


def tie_share(x, nbr, best):
    """share of the (output row, channel) cells whose maximum is attained by two or more inputs"""
    hits = np.zeros(best.shape, np.int32)
    for k in range(nbr.shape[0]):
        v = nbr[k] >= 0
        hits[v] += x[nbr[k][v]] == best[v]
    return float((hits >= 2).mean())


def tied_ref(ks, stride, c):
    """three-level features / five-level gradients on cpu_map(ks, stride) and the oracle's results on them, computed
    once per (region, c); no GPU work"""
    key = (ks, stride, c)
    if key not in _REFS:
        m = cpu_map(ks, stride)
        x = _ints((m["n_in"], c), 100 + c, 0, 3).numpy()
        gy = _ints((m["n_out"], c), 200 + c, -2, 3).numpy()
        best, mask = O.pool_forward(x, m["okm"], m["n_out"], "max")
        share = tie_share(x, m["nbr"], best)
        # the condition of this module: at least a quarter of the cells are decided by the tie rule alone
        assert share >= 0.25, f"only {share:.2f} of the cells are tied: fewer levels needed"
        gin = O.pool_backward(gy, m["okm"], m["n_in"], "max", mask)
        _REFS[key] = dict(x=x, gy=gy, best=best, mask=mask, gin=gin, share=share)
    return _REFS[key]


@pytest.mark.parametrize("ks,stride", REGIONS)
@pytest.mark.parametrize("dt,c,off", [("f32", 64, 0), ("bf16", 64, 0), ("f32", 20, 0), ("bf16", 20, 0), ("f32", 5, 0),
                                      ("bf16", 5, 0), ("f32", 8, 1), ("bf16", 8, 4), ("bf16", 8, 1)])
def test_local_max_ties_every_piece_width(device, ks, stride, dt, c, off):
    """me_pool_max_* / me_pool_max_backward_* on tied inputs: values, int32 masks and gradients bit for bit equal to the
    oracle.  Piece widths: c = 64 -> 16-byte pieces (4 floats / 8 bf16); c = 20 -> pieces of 4 in both dtypes; c = 5 ->
    scalar; c = 8 with the features (and the gradient buffer) starting `off` ELEMENTS into a wider allocation, which
    fails the 16-byte test: fp32 + 4 bytes and bf16 + 2 bytes -> scalar, bf16 + 8 bytes -> pieces of 4.  (One whole row
    of 8 channels is 32 / 16 bytes and would still be aligned.)"""
    m = _local_map(device, ks, stride)
    r = tied_ref(ks, stride, c)
    dtype, n_in, n_out = DTYPES[dt], m["n_in"], m["n_out"]
    wide = torch.zeros(n_in * c + 16, dtype=dtype, device=device)
    x = wide[off:off + n_in * c].view(n_in, c)
    x.copy_(torch.from_numpy(r["x"]).to(dtype))
    assert (x.data_ptr() % 16 != 0) == (off != 0)
    dst, mask = _pool_max(x, m["tbl_out"], n_out)
    assert np.array_equal(_np(dst), r["best"])
    assert np.array_equal(mask.cpu().numpy(), r["mask"]), "argmax: the first maximum in kernel-offset order"
    gwide = torch.full((2 * PAD + n_in * c + 16,), 7.0, dtype=dtype, device=device)
    grad_in = gwide[PAD + off:PAD + off + n_in * c].view(n_in, c)
    gy = torch.from_numpy(r["gy"]).to(dtype).to(device)
    _pool_max_backward(gy, m["tbl_in"], n_in, mask, grad_in)
    assert np.array_equal(_np(grad_in), r["gin"])
    assert bool((gwide[:PAD + off] == 7.0).all()) and bool((gwide[PAD + off + n_in * c:] == 7.0).all())


@pytest.mark.parametrize("ks,stride", REGIONS)
def test_local_max_ties_public_api(device, host_layer, ks, stride):
    """the same tied input through ME.MinkowskiMaxPooling on both hosts: output and x.F.grad equal the oracle's"""
    import minkowskiengine_amd as ME
    c = 20
    m = _local_map(device, ks, stride)
    r = tied_ref(ks, stride, c)
    x = ME.SparseTensor(torch.from_numpy(r["x"]).to(device), m["coords"].to(device), requires_grad=True)
    y = ME.MinkowskiMaxPooling(kernel_size=ks, stride=stride, dimension=3)(x)
    assert np.array_equal(y.C.cpu().numpy(), m["out_c"])
    assert np.array_equal(_np(y.F), r["best"])
    y.F.backward(torch.from_numpy(r["gy"]).to(device))
    assert np.array_equal(_np(x.F.grad), r["gin"]), "the gradient goes to the first tied row in kernel-offset order"


# ---- 2. non-finite and extreme inputs -------------------------------------------------------------------------------
def _local_nonfinite_input(nbr, n_in, c, big):
    """integer features with planted values; the output cells are chosen so that no two of them share an input.
    -> (x, {name: output row})"""
    x = _ints((n_in, c), 31, -2, 3).numpy()
    used, cells = set(), {}

    def pick(name):
        for o in range(nbr.shape[1]):
            ins = nbr[:, o][nbr[:, o] >= 0]
            if len(ins) >= 2 and not used.intersection(ins.tolist()):
                used.update(ins.tolist())
                cells[name] = o
                return ins
        raise AssertionError("no free cell left")
    x[pick("all_nan")] = np.nan
    x[pick("all_ninf")] = -np.inf
    ins = pick("both_inf")
    x[ins[0], 0], x[ins[1], 0] = np.inf, -np.inf
    x[pick("all_lowest"), 1] = -big            # finite, and still no winner in fp32: -FLT_MAX < -FLT_MAX is false
    x[pick("one_big")[0], 2] = big
    x[pick("one_nan")[0], 3] = np.nan
    x[pick("one_pinf")[-1], 4] = np.inf
    return x, cells


@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 1)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_local_pooling_nonfinite(device, ks, stride, dt):
    """+-inf, NaN, +-FLT_MAX (bf16: the largest finite bf16) through local sum / avg / max and max backward: NaN and
    infinity positions equal the oracle's, finite cells are equal.  A cell whose inputs are all NaN or all -inf, and in
    fp32 all -FLT_MAX, has no winner (`best < x` is never true): it keeps the start value and mask -1.  The start value
    is -FLT_MAX in fp32; a bf16 output stores (__bf16)(-FLT_MAX), which rounds to nearest and so is -inf (0xff80).
    Max backward with mask -1 adds that gradient nowhere — the reference's CPU loop would write grad_in[-1]
    (pooling_max_kernel.hpp:98-117), out of bounds; ours skips the entry: sentinels in front of and behind grad_in stay
    intact and a NaN gradient of such a cell reaches no input row."""
    c = 20
    m = _local_map(device, ks, stride, n=800, extent=12)
    dtype, n_in, n_out = DTYPES[dt], m["n_in"], m["n_out"]
    x, cells = _local_nonfinite_input(m["nbr"], n_in, c, FLT_MAX if dt == "f32" else BF16_MAX)
    xd = torch.from_numpy(x).to(dtype).to(device)
    assert np.array_equal(_np(xd), x, equal_nan=True), "the planted values are exact in the storage type"
    to_store = (lambda a: a) if dt == "f32" else _bf16_round
    with np.errstate(invalid="ignore", over="ignore"):
        w_sum, w_cnt = O.pool_forward(x, m["okm"], n_out, "sum")
        w_avg, _ = O.pool_forward(x, m["okm"], n_out, "avg")
        w_max, w_mask = O.pool_forward(x, m["okm"], n_out, "max")
    # the planted cells do what they were planted for
    for name in ("all_nan", "all_ninf"):
        assert (w_mask[cells[name]] == -1).all() and (w_max[cells[name]] == -FLT_MAX).all()
    assert np.isnan(w_sum[cells["all_nan"]]).all() and (w_sum[cells["all_ninf"]] == -np.inf).all()
    assert np.isnan(w_sum[cells["both_inf"], 0]) and w_max[cells["both_inf"], 0] == np.inf
    assert w_sum[cells["all_lowest"], 1] == -np.inf
    assert (w_mask[cells["all_lowest"], 1] == -1) == (dt == "f32")
    assert w_max[cells["one_big"], 2] == (FLT_MAX if dt == "f32" else BF16_MAX)
    assert np.isnan(w_sum[cells["one_nan"], 3]) and np.isfinite(w_max[cells["one_nan"], 3])
    assert w_sum[cells["one_pinf"], 4] == np.inf and w_max[cells["one_pinf"], 4] == np.inf
    for avg, want in ((False, w_sum), (True, w_avg)):
        got, cnt = _pool_sum(xd, m["tbl_out"], n_out, avg)
        _same_exact(_np(got), to_store(want), "avg" if avg else "sum")
        assert np.array_equal(cnt.cpu().numpy(), w_cnt)
    got, mask = _pool_max(xd, m["tbl_out"], n_out)
    mask_np = mask.cpu().numpy()
    assert np.array_equal(mask_np, w_mask)
    _same_exact(_np(got), to_store(w_max), "max")
    no_winner = _np(got)[mask_np == -1]
    assert no_winner.size >= 2 * c
    assert (no_winner == (-FLT_MAX if dt == "f32" else -np.inf)).all(), "start value as stored: -FLT_MAX | bf16 -inf"
    # backward: a NaN gradient on the cells without a winner must vanish
    gy = _ints((n_out, c), 32, -2, 3).numpy()
    gy[mask_np == -1] = np.nan
    buf, grad_in = _guarded(n_in, c, dtype, device)
    _pool_max_backward(torch.from_numpy(gy).to(dtype).to(device), m["tbl_in"], n_in, mask, grad_in)
    want_gin = O.pool_backward(gy, m["okm"], n_in, "max", w_mask)
    assert np.isfinite(want_gin).all()
    assert np.array_equal(_np(grad_in), want_gin)
    assert _sentinels_intact(buf), "max backward wrote outside grad_in"


def global_nonfinite_input(dt, c):
    """640 rows, origin rows 0 (rows 0..299), 1 (300..599), 3 (600..639); origin row 2 has no point.  With 256-row chunks:
    chunk 0 uniform, chunk 1 mixed (0 | 1), chunk 2 mixed (1 | 3)."""
    big = FLT_MAX if dt == "f32" else BF16_MAX
    x = _ints((640, c), 41, -2, 3).numpy()
    rows = np.concatenate([np.zeros(300), np.ones(300), np.full(40, 3)]).astype(np.int32)
    x[600:, 0] = np.nan                       # a batch that is all NaN in one channel ...
    x[600:, 1] = -np.inf                      # ... and all -inf in another: no winner
    x[10, 2], x[280, 2] = np.inf, -np.inf     # opposite infinities in different chunks of one batch: NaN sum, +inf max
    x[400, 3] = big                           # one huge value: the sum stays at it
    x[100, 4] = np.nan                        # one NaN: NaN sum, finite max
    x[300:600, 4] = -big                      # all at the lowest finite value: the sum overflows to -inf
    return x, rows, 4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [8, 5])
def test_global_pooling_nonfinite(device, dt, c):
    """global sum / avg / max (me_global_pool_*: fp32 results for both storage types) on planted non-finite values, in
    uniform and in mixed chunks; a batch without a winner and an origin row without any point give -FLT_MAX / -1,
    sum 0 and count 0."""
    x, rows, n_batch = global_nonfinite_input(dt, c)
    xd = torch.from_numpy(x).to(DTYPES[dt]).to(device)
    assert np.array_equal(_np(xd), x, equal_nan=True)
    rd = torch.from_numpy(rows).to(device)
    s, cnt, mx, arg = np_global(x, rows, n_batch)
    assert (arg[3, :2] == -1).all() and (arg[2] == -1).all() and (mx[2] == -FLT_MAX).all() and (s[2] == 0).all()
    assert np.isnan(s[0, 2]) and mx[0, 2] == np.inf and np.isnan(s[0, 4]) and s[1, 4] == -np.inf
    assert (arg[1, 4] == -1) == (dt == "f32")
    g_s, _, g_cnt = _global_pool(xd, None, rd, n_batch, 0)
    _same_exact(g_s, s, "sum")
    assert np.array_equal(g_cnt, cnt)
    g_a, _, g_cnt = _global_pool(xd, None, rd, n_batch, 1)
    _same_exact(g_a, np_avg(s, cnt), "avg")
    assert np.array_equal(g_cnt, cnt)
    g_m, g_arg, _ = _global_pool(xd, None, rd, n_batch, 2)
    assert np.array_equal(g_arg, arg)
    _same_exact(g_m, mx, "max")


# ---- 3. global pooling: every path ----------------------------------------------------------------------------------
def _check_global(device, x, rows, n_batch, dt, x2=None, modes=(0, 1, 2)):
    """all modes of me_global_pool_* on integer-valued input against np_global: everything exact"""
    xd = torch.from_numpy(x).to(DTYPES[dt]).to(device)
    x2d = None if x2 is None else torch.from_numpy(x2).to(DTYPES[dt]).to(device)
    rd = torch.from_numpy(np.asarray(rows, np.int32)).to(device)
    s, cnt, mx, arg = np_global(x, rows, n_batch, x2)
    for mode in modes:
        out, g_arg, g_cnt = _global_pool(xd, x2d, rd, n_batch, mode)
        if mode == 2:
            assert np.array_equal(out, mx), "max"
            assert np.array_equal(g_arg, arg), "argmax: the first row of the batch that attains the maximum"
        else:
            assert np.array_equal(out, s if mode == 0 else np_avg(s, cnt)), ("sum", "avg")[mode]
            assert np.array_equal(g_cnt, cnt), "count"
    return s, cnt, mx, arg


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 8, 64, 256])
def test_global_uniform_chunks_ties_across_row_lanes(device, dt, c):
    """one batch, 1000 rows of three levels: every chunk takes the row-lane path with R = 256 / (c / 4) = 256, 128, 16, 4
    row lanes; the maximum sits in many lanes and many chunks, the argmax is the first row"""
    x = _ints((1000, c), c, 0, 3).numpy()
    _, _, _, arg = _check_global(device, x, np.zeros(1000, np.int32), 1, dt)
    assert (arg // c < 64).all()          # ... which the tie rule alone finds: the first `2` of a channel comes early


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n,c,split", [(20000, 8, 9000), (140000, 4, 70100)])
def test_global_many_chunks_first_maximum_wins(device, dt, n, c, split):
    """n = 20000: 79 chunks of 256 rows, so k_global_final's lanes each merge two chunks; n = 140000: chunk_rows grows to
    274 (511 chunks).  Two batches, split inside a chunk.  The maximum of every channel is planted in an early and again
    in a late row of each batch: a merge that prefers the later chunk gives the wrong argmax."""
    x = _ints((n, c), n % 1000 + c, 0, 3).numpy()
    rows = (np.arange(n) >= split).astype(np.int32)
    for lo, hi in ((0, split), (split, n)):
        x[lo + 3], x[hi - 2] = 5.0, 5.0
    _, _, mx, arg = _check_global(device, x, rows, 2, dt)
    assert (mx == 5.0).all() and (arg[0] // c == 3).all() and (arg[1] // c == split + 3).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 5, 64])
def test_global_mixed_chunks(device, dt, c):
    """3000 rows whose origin rows are a random arrangement of 5 batches: every chunk is mixed and takes the
    one-thread-per-channel run path, which flushes run after run into the pre-initialised partials.  Sum, avg with its
    counts, max with its argmax; with and without the second factor (src2: the gradient of broadcast-multiplication with
    respect to the global row).  Batch 3 is negative in every channel, so its maxima must come from the -FLT_MAX start
    of the partials, not from a zero."""
    n, n_batch = 3000, 5
    rng = np.random.RandomState(c)
    rows = rng.randint(0, n_batch, n).astype(np.int32)
    x = _ints((n, c), 50 + c, -2, 3).numpy()
    x[rows == 3] = -1.0 - (x[rows == 3] > 0)         # {-2, -1}
    x2 = _ints((n, c), 60 + c, -2, 3).numpy()
    _, cnt, mx, _ = _check_global(device, x, rows, n_batch, dt)
    assert (mx[3] == -1.0).all() and (cnt > 500).all()
    x2[rows == 3] = 1.0 + (x2[rows == 3] > 0)        # products of batch 3 stay negative
    _, _, mx2, _ = _check_global(device, x, rows, n_batch, dt, x2=x2)
    assert (mx2[3] == -1.0).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("first", [256, 255, 257])
def test_global_batch_boundary_on_chunk_boundary(device, dt, first):
    """512 rows in two batches.  256 | 256: both chunks uniform, with different origin rows; 255 | 257 and 257 | 255:
    one chunk mixed, the other uniform."""
    c = 8
    x = _ints((512, c), first, -2, 3).numpy()
    rows = (np.arange(512) >= first).astype(np.int32)
    _, cnt, _, _ = _check_global(device, x, rows, 2, dt)
    assert cnt.tolist() == [first, 512 - first]
    _check_global(device, x, rows, 2, dt, x2=_ints((512, c), first + 1, -2, 3).numpy(), modes=(0,))


def _many_batches():
    """70 batch indices drawn with gaps from 0..200, 1 to 300 rows each (the first three: 1, 1 and 256 rows), unique
    voxels of an 8^3 grid per batch, all rows shuffled.  -> (coords int32 [n, 4], sorted batch indices, origin row of
    every row = the rank of its batch index)"""
    rng = np.random.RandomState(5)
    batches = np.sort(rng.choice(201, 70, replace=False))
    sizes = rng.randint(1, 301, 70)
    sizes[:3] = (1, 1, 256)
    parts = []
    for b, m in zip(batches, sizes):
        cell = rng.permutation(512)[:m]
        parts.append(np.stack([np.full(m, b), cell // 64, (cell // 8) % 8, cell % 8], 1))
    coords = np.concatenate(parts)[rng.permutation(int(sizes.sum()))].astype(np.int32)
    return coords, batches, np.searchsorted(batches, coords[:, 0]).astype(np.int32)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_many_uneven_batches_public_api(device, host_layer, dt):
    """70 shuffled batches with gaps in their indices through ME.SparseTensor, MinkowskiGlobal{Sum,Avg,Max}Pooling and
    MinkowskiBroadcast{Addition,Multiplication}, forward and backward, on both hosts.  Output rows come in ascending
    batch index; values and gradients are exact (bf16: the exact fp32 result rounded once), the gradient of the global
    row under multiplication (the src2 path) included."""
    import minkowskiengine_amd as ME
    c, dtype = 20, DTYPES[dt]
    to_store = (lambda a: a) if dt == "f32" else _bf16_round
    coords, batches, rows = _many_batches()
    n, nb = coords.shape[0], len(batches)
    assert 70 == nb and batches[-1] > 150 and np.bincount(rows).min() == 1
    x_np = _ints((n, c), 71, -2, 3).numpy()
    gy = _ints((nb, c), 72, -2, 3).numpy()
    s, cnt, mx, arg = np_global(x_np, rows, nb)
    x = ME.SparseTensor(torch.from_numpy(x_np).to(dtype).to(device), torch.from_numpy(coords).to(device),
                        requires_grad=True)
    with np.errstate(invalid="ignore"):
        g_avg = to_store(gy / cnt[:, None])[rows]
    g_max = np.zeros(n * c, np.float32)
    g_max[arg.reshape(-1)] = gy.reshape(-1)
    for cls, want, want_grad in ((ME.MinkowskiGlobalSumPooling, s, gy[rows]),
                                 (ME.MinkowskiGlobalAvgPooling, np_avg(s, cnt), g_avg),
                                 (ME.MinkowskiGlobalMaxPooling, mx, g_max.reshape(n, c))):
        x.F.grad = None
        y = cls()(x)
        assert y.C[:, 0].cpu().tolist() == batches.tolist(), "output rows in ascending batch index"
        assert y.F.dtype == dtype and np.array_equal(_np(y.F), to_store(want)), cls.__name__
        y.F.backward(torch.from_numpy(gy).to(dtype).to(device))
        assert np.array_equal(_np(x.F.grad), want_grad), cls.__name__ + " backward"
    glob_np = _ints((nb, c), 73, -2, 3).numpy()
    gout = _ints((n, c), 74, -2, 3).numpy()
    for cls, mul in ((ME.MinkowskiBroadcastAddition, False), (ME.MinkowskiBroadcastMultiplication, True)):
        x.F.grad = None
        glob = ME.SparseTensor(torch.from_numpy(glob_np).to(dtype).to(device).requires_grad_(True),
                               coordinate_map_key=y.coordinate_map_key, coordinate_manager=x.coordinate_manager)
        z = cls()(x, glob)
        per_row = glob_np[rows]
        assert np.array_equal(_np(z.F), x_np * per_row if mul else x_np + per_row), cls.__name__
        z.F.backward(torch.from_numpy(gout).to(dtype).to(device))
        assert np.array_equal(_np(x.F.grad), gout * per_row if mul else gout), cls.__name__ + " grad_in"
        want_glob = np_global(gout, rows, nb, x2=x_np if mul else None)[0]
        assert np.array_equal(_np(glob.F.grad), to_store(want_glob)), cls.__name__ + " grad_glob"


def test_global_channel_limits(device):
    """c = 1024 (fp32, aligned) is the widest row a thread-per-16-bytes block covers (P = 256): computed and correct.
    c = 300 is a multiple of 4 below that limit and is computed too (75 pieces, 3 row lanes).  c = 1028 (257 pieces) and
    c = 301 (more than 256 channels, no multiple of 4) are REFUSED: the C ABI returns a non-zero status and writes
    nothing, the Python layer raises RuntimeError — there is no fallback, and no wrong numbers come back."""
    from minkowskiengine_amd import backend as MEB
    n = 600
    rows = (np.arange(n) >= 300).astype(np.int32)
    for c in (1024, 300):
        x = _ints((n, c), c, -2, 3).numpy()
        _check_global(device, x, rows, 2, "f32")
    rd = torch.from_numpy(rows).to(device)
    for c in (1028, 301):
        xd = _ints((n, c), c, -2, 3).to(device)
        for mode in (0, 2):
            rc, dst, arg, cnt = _global_pool_rc(xd, None, rd, 2, mode)
            assert rc != 0
            assert bool((dst == 7.0).all()) and (arg is None or bool((arg == 7).all()))
            with pytest.raises(RuntimeError):
                MEB._global_pool(xd, None, rd, 2, mode)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_global_pooling_of_no_rows(device, dt):
    """n = 0 with n_batch = 3: sums and counts 0, maxima -FLT_MAX / -1, no launch error"""
    n_batch, c = 3, 8
    xd = torch.zeros((1, c), dtype=DTYPES[dt], device=device)
    rd = torch.zeros(1, dtype=torch.int32, device=device)
    for mode in (0, 1, 2):
        rc, dst, arg, cnt = _global_pool_rc(xd, None, rd, n_batch, mode, n=0)
        assert rc == 0
        if mode == 2:
            assert bool((dst == -FLT_MAX).all()) and bool((arg == -1).all())
        else:
            assert bool((dst == 0).all()) and bool((cnt == 0).all())


# ---- 4. broadcast ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [64, 20, 5])
def test_broadcast_many_batches(device, dt, c):
    """me_broadcast_* on the 70-batch layout: addition, multiplication and pure expansion (in == nullptr), exact, and
    nothing written outside the n x c output"""
    L, lib = _lib()
    dtype = DTYPES[dt]
    _, batches, rows = _many_batches()
    n, nb = rows.shape[0], len(batches)
    x = _ints((n, c), 80 + c, -2, 3).numpy()
    glob = _ints((nb, c), 90 + c, -2, 3).numpy()
    xd, gd = torch.from_numpy(x).to(dtype).to(device), torch.from_numpy(glob).to(dtype).to(device)
    rd = torch.from_numpy(rows).to(device)
    fn = getattr(lib, "me_broadcast_" + dt)
    for src, mul, want in ((xd, 0, x + glob[rows]), (xd, 1, x * glob[rows]), (None, 0, glob[rows])):
        buf, out = _guarded(n, c, dtype, device)
        L.check(fn(_ptr(src), gd.data_ptr(), rd.data_ptr(), n, c, mul, out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert np.array_equal(_np(out), want)
        assert _sentinels_intact(buf), "broadcast wrote outside its output"
