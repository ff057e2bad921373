"""GPU tests of the dense <-> sparse conversions (csrc/dense.hip through the operators of both host layers):
`SparseTensor.dense` / `.sparse`, `ME.to_sparse`, `ME.to_sparse_all`, `ME.dense_coordinates(device=)`,
`MinkowskiToSparseTensor`, `MinkowskiToDenseTensor` and the small helpers of MinkowskiOps.py.

Bounds.  Conversions copy values, so every comparison is BITWISE (`torch.equal` on tensors of the same dtype): against the
fixtures recorded from the reference (tests/golden/make_golden_dense.py; their values have 8 significant bits, so the cast
of a fixture to fp32 or bf16 is exact), against torch restatements of the reference's indexing on the device, between two
runs and between the two hosts.  gradcheck uses the project's float64 settings."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu
CASES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "dense_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)     # MinkowskiEngine/utils/gradcheck.py:37-39
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
DTYPE_IDS = ["f32", "f64", "bf16"]


def _t(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got, want)
    # NaN-free data: torch.equal is a bitwise statement up to the sign of zero, which the next line pins
    assert torch.equal(torch.signbit(got), torch.signbit(want))


# ---- the reference's formulations in torch, on the device -----------------------------------------------------------------
def torch_dense(feats, coords, shape, mn, div):
    out = torch.zeros(shape, dtype=feats.dtype, device=feats.device)
    idx = torch.div(coords[:, 1:] - torch.tensor(mn, dtype=torch.int32, device=coords.device),
                    torch.tensor(div, dtype=torch.int32, device=coords.device), rounding_mode="floor").long()
    out[(coords[:, 0].long(), slice(None)) + tuple(idx.t())] = feats
    return out


def torch_to_sparse(x, ch):
    b = torch.where(x.abs().sum(ch) != 0)
    index = list(b)
    index.insert(ch, slice(None))
    return torch.stack(b, 1).int(), x[tuple(index)]


def torch_to_sparse_all(x):
    d = x.ndim - 2
    return x.permute(0, *range(2, 2 + d), 1).reshape(-1, x.size(1))


def _sparse_input(ME, z, dtype, device, requires_grad=True):
    feats = _t(z["feats"], dtype, device).requires_grad_(requires_grad)
    return ME.SparseTensor(feats, _t(z["coords"], torch.int32, device), tensor_stride=int(z["tensor_stride"])), feats


def _dense_kwargs(z):
    kw = dict(contract_stride=bool(z["contract"]))
    if z["shape_arg"].size:
        kw["shape"] = torch.Size(z["shape_arg"].tolist())
    arg = str(z["min_arg"])
    if arg == "zero":
        kw["min_coordinate"] = 0
    elif arg == "tensor":
        kw["min_coordinate"] = torch.IntTensor(z["min_coordinate"].tolist())
    return kw


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fixture(device, host_layer, path, dtype):
    import minkowskiengine_amd as ME
    z = np.load(path)
    kind = str(z["kind"])
    if kind == "dense":
        x, feats = _sparse_input(ME, z, dtype, device)
        assert torch.equal(x.C.cpu(), torch.from_numpy(z["coords"]))
        out, ret_min, ret_stride = x.dense(**_dense_kwargs(z))
        _same(out.detach(), _t(z["dense"], dtype, device))
        if str(z["min_arg"]) == "zero":
            assert isinstance(ret_min, int) and ret_min == 0
        else:
            assert isinstance(ret_min, torch.Tensor) and ret_min.dtype == torch.int32
            assert ret_min.device == feats.device and tuple(ret_min.shape) == (1, x.D)
            assert ret_min.flatten().tolist() == z["ret_min"].tolist()
        assert isinstance(ret_stride, torch.Tensor) and ret_stride.dtype == torch.int32 and not ret_stride.is_cuda
        assert ret_stride.tolist() == z["ret_stride"].tolist()
        out.backward(_t(z["grad_out"], dtype, device))
        _same(feats.grad, _t(z["grad_feats"], dtype, device))
    elif kind == "to_sparse":
        x = _t(z["x"], dtype, device).requires_grad_(True)
        fmt = str(z["format"]) or None
        s = ME.to_sparse(x, format=fmt)
        assert isinstance(s, ME.SparseTensor) and s.F.dtype == dtype
        assert s.C.dtype == torch.int32 and torch.equal(s.C.cpu(), torch.from_numpy(z["coords"]))     # IN ORDER
        _same(s.F.detach(), _t(z["feats"], dtype, device))
        if len(s) > 0:
            s.F.backward(_t(z["grad_out"], dtype, device))
            _same(x.grad, _t(z["grad_x"], dtype, device))
        else:       # the all-zero input: a 0-row tensor that densifies to zeros of the input's shape
            back = ME.MinkowskiToDenseTensor(x.shape)(s)
            _same(back, torch.zeros_like(x))
    elif kind == "to_sparse_all":
        x = _t(z["x"], dtype, device).requires_grad_(True)
        for coordinates in (None, ME.dense_coordinates(x.shape)):
            x.grad = None
            s = ME.to_sparse_all(x, coordinates)
            assert torch.equal(s.C.cpu(), torch.from_numpy(z["coords"]))
            _same(s.F.detach(), _t(z["feats"], dtype, device))
            s.F.backward(_t(z["grad_out"], dtype, device))
            _same(x.grad, _t(z["grad_x"], dtype, device))
    elif kind == "dense_coordinates":
        got = ME.dense_coordinates(torch.Size(z["shape"].tolist()), device=device)
        assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(z["coords"]))
    elif kind == "module":
        x = _t(z["x"], dtype, device)
        coordinates = ME.dense_coordinates(x.shape) if bool(z["with_coordinates"]) else None
        s = ME.MinkowskiToSparseTensor(remove_zeros=bool(z["remove_zeros"]), coordinates=coordinates)(x)
        assert torch.equal(s.C.cpu(), torch.from_numpy(z["coords"]))
        _same(s.F, _t(z["feats"], dtype, device))
        back = ME.MinkowskiToDenseTensor(torch.Size(z["dense_shape_arg"].tolist()))(s)
        _same(back, _t(z["dense"], dtype, device))
    else:
        assert kind == "sparse"
        x, feats = _sparse_input(ME, z, dtype, device, requires_grad=False)
        kw = dict(contract_coords=bool(z["contract"]))
        if z["max_arg"].size:
            kw["max_coords"] = torch.IntTensor(z["max_arg"].tolist())
        if dtype == torch.bfloat16:
            with pytest.raises(ValueError):
                x.sparse(**kw)
            return
        sp, ret_min, ret_stride = x.sparse(**kw)
        assert sp.is_sparse and sp.device == feats.device
        _same(sp.to_dense(), _t(z["to_dense"], dtype, device))
        assert ret_min.dtype == torch.int32 and ret_min.tolist() == z["ret_min"].tolist()
        assert ret_stride.tolist() == z["ret_stride"].tolist()


# ---- round trips ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("fmt,shape", [(None, (2, 5, 9, 12)), ("BCXX", (3, 1, 33, 35)), ("BXXXC", (2, 6, 5, 7, 17)),
                                       ("BXCX", (2, 10, 16, 11)), ("BXXCXX", (2, 3, 4, 3, 5, 4)), ("BXC", (4, 70, 3)),
                                       # a second and a third pass of the channel loop: inner 60 (four cells per lane),
                                       # inner 35 (cell fastest, scalar), channels-last (channel fastest)
                                       (None, (2, 65, 6, 10)), (None, (1, 129, 5, 7)), ("BXXC", (2, 5, 7, 130))])
def test_round_trip_every_format(device, host_layer, fmt, shape, dtype):
    import minkowskiengine_amd as ME
    g = torch.Generator().manual_seed(7)
    ch = 1 if fmt is None else fmt.find("C")
    x = torch.randn(shape, generator=g)
    cells = [s for k, s in enumerate(shape) if k != ch]
    keep = (torch.rand(cells, generator=g) < 0.5).unsqueeze(ch)
    x = torch.where(keep, x, torch.zeros(())).to(device=device, dtype=dtype)      # (+0: a product with False would give -0)
    s = ME.to_sparse(x, format=fmt)
    coords, feats = torch_to_sparse(x, ch)
    assert torch.equal(s.C, coords)
    _same(s.F, feats)
    bcx = x.movedim(ch, 1).contiguous()
    back = s.dense(shape=bcx.shape, min_coordinate=0)[0]
    _same(back.movedim(1, ch), x)
    _same(ME.to_sparse_all(bcx).dense(shape=bcx.shape, min_coordinate=0)[0], bcx)


# ---- gradcheck --------------------------------------------------------------------------------------------------------------
def test_gradcheck(device, host_layer):
    import minkowskiengine_amd as ME
    g = torch.Generator().manual_seed(3)
    pts = torch.unique(torch.randint(0, 6, (40, 3), generator=g), dim=0)
    coords = torch.cat([torch.randint(0, 2, (pts.shape[0], 1), generator=g), pts], 1).int().to(device)
    feats = torch.rand(coords.shape[0], 3, generator=g, dtype=torch.float64).to(device).requires_grad_(True)
    x = ME.SparseTensor(feats, coords)
    shape = torch.Size([2, 3, 7, 6, 8])

    def dense_of(f):
        return ME.SparseTensor(f, coordinate_map_key=x.coordinate_map_key,
                               coordinate_manager=x.coordinate_manager).dense(shape=shape, min_coordinate=0)[0]
    assert gradcheck(dense_of, (feats,), **GC)
    for fmt, shp in ((None, (2, 3, 4, 5)), ("BXXC", (2, 4, 5, 3)), ("BXCX", (2, 4, 3, 5))):
        ch = 1 if fmt is None else fmt.find("C")
        xd = torch.rand(shp, generator=g, dtype=torch.float64) + 0.5
        cells = [s for k, s in enumerate(shp) if k != ch]
        keep = (torch.rand(cells, generator=g) < 0.5).unsqueeze(ch).to(device)
        xd = xd.to(device).requires_grad_(True)
        # the set of kept cells must not move under gradcheck's perturbations: empty cells are held at zero by `keep`
        assert gradcheck(lambda t: ME.to_sparse(t * keep, format=fmt).F, (xd,), **GC)
    xa = torch.rand((2, 3, 4, 3, 2), generator=g, dtype=torch.float64).to(device).requires_grad_(True)
    assert gradcheck(lambda t: ME.to_sparse_all(t).F, (xa,), **GC)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_rows_outside_the_box_raise_and_write_nothing(device, host_layer):
    import minkowskiengine_amd as ME
    coords = torch.IntTensor([[0, 1, 1], [0, 2, 3], [1, 0, 0], [1, 3, 3]]).to(device)
    feats = torch.arange(1, 13, dtype=torch.float32, device=device).reshape(4, 3)
    x = ME.SparseTensor(feats, coords)
    with pytest.raises(IndexError):                                  # above the box
        x.dense(shape=torch.Size([2, 3, 3, 4]), min_coordinate=0)
    with pytest.raises(IndexError):                                  # batch index above the box
        x.dense(shape=torch.Size([1, 3, 4, 4]), min_coordinate=0)
    with pytest.raises(IndexError):                                  # below the box (torch would wrap round silently)
        x.dense(shape=torch.Size([2, 3, 4, 4]), min_coordinate=torch.IntTensor([1, 0]))
    out = x.dense(shape=torch.Size([2, 3, 4, 4]), min_coordinate=0)[0]
    _same(out, torch_dense(feats, coords, (2, 3, 4, 4), [0, 0], [1, 1]))


@pytest.mark.parametrize("policy", [1, 2], ids=["row_stationary", "cell_stationary"])
@pytest.mark.parametrize("inner_dims", [(4, 4), (3, 5)], ids=["vector_stores", "scalar_stores"])
def test_guard_cells_survive_rows_outside_the_box(device, policy, inner_dims):
    """C ABI: the box sits inside a larger poisoned buffer; rows above and below the box raise the flag and leave the
    box's neighbours, and their own would-be cells, untouched."""
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream(device).cuda_stream
    shape = (2,) + inner_dims
    coords = torch.IntTensor([[0, 1, 1], [0, -1, 2], [1, 2, inner_dims[1]], [2, 0, 0], [-1, 0, 0], [1, 2, 1]]).to(device)
    valid = [0, 5]
    n, c, cells = coords.shape[0], 5, 2 * inner_dims[0] * inner_dims[1]
    rows = (torch.arange(n * c, dtype=torch.float32, device=device) + 1).reshape(n, c)
    cell = torch.empty(n, dtype=torch.int64, device=device)
    flag = torch.full((1,), 7, dtype=torch.int32, device=device)
    grid = torch.empty(cells, dtype=torch.int32, device=device)
    mn, dv = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(1, 1)
    shp = (ctypes.c_int64 * 3)(*shape)
    _lib.check(lib.me_dense_cell_index(coords.data_ptr(), n, 3, mn, dv, shp, cell.data_ptr(), flag.data_ptr(), st))
    _lib.check(lib.me_dense_grid(cell.data_ptr(), n, cells, grid.data_ptr(), st))
    assert int(flag.item()) == 1
    want_cell = [(b * inner_dims[0] + i) * inner_dims[1] + j if r in valid else -1
                 for r, (b, i, j) in enumerate(coords.tolist())]
    assert cell.tolist() == want_cell
    guard = 64
    buf = torch.full((guard + cells * c + guard,), -777.0, dtype=torch.float32, device=device)
    box = buf[guard:guard + cells * c]
    _lib.check(lib.me_dense_rows_to_box(rows.data_ptr(), 4, cell.data_ptr(), grid.data_ptr(), n, 2, c,
                                        inner_dims[0] * inner_dims[1], box.data_ptr(), policy, st))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[guard + cells * c:] == -777.0).all())
    want = torch.zeros((2, c, inner_dims[0] * inner_dims[1]), dtype=torch.float32, device=device)
    for r in valid:
        want[want_cell[r] // (inner_dims[0] * inner_dims[1]), :, want_cell[r] % (inner_dims[0] * inner_dims[1])] = rows[r]
    _same(box.reshape(want.shape), want)
    # a clean set of rows afterwards clears the flag
    _lib.check(lib.me_dense_cell_index(coords[valid].contiguous().data_ptr(), 2, 3, mn, dv, shp, cell.data_ptr(),
                                       flag.data_ptr(), st))
    assert int(flag.item()) == 0


def test_argument_errors(device, host_layer):
    import minkowskiengine_amd as ME
    coords = torch.IntTensor([[0, -2, 0], [0, 2, 4]]).to(device)
    x = ME.SparseTensor(torch.ones(2, 1, device=device), coords, tensor_stride=2)
    with pytest.raises(ValueError):
        x.dense()                                                    # negative coordinate, no min_coordinate
    with pytest.raises(AssertionError):
        x.dense(min_coordinate=torch.IntTensor([-3, 0]))             # not divisible by the stride
    with pytest.raises(AssertionError):
        x.dense(min_coordinate=torch.IntTensor([-2]))                # wrong length
    with pytest.raises(AssertionError):
        x.dense(shape=torch.Size([1, 1, 4]), min_coordinate=torch.IntTensor([-2, 0]))
    out, mn, _ = x.dense(min_coordinate=torch.IntTensor([-2, 0]))
    assert out.shape == (1, 1, 3, 3) and mn.tolist() == [[-2, 0]]
    empty = ME.to_sparse(torch.zeros(4, 1, 34, 34, device=device))
    assert len(empty) == 0 and empty.F.shape == (0, 1) and empty.C.shape == (0, 3)
    with pytest.raises(AssertionError):
        empty.dense()                                                # empty tensor without a shape
    d, mn, ts = empty.dense(shape=torch.Size([4, 1, 34, 34]))
    _same(d, torch.zeros(4, 1, 34, 34, device=device))
    assert mn.dtype == torch.int32 and mn.tolist() == [0, 0] and ts == [1, 1]


# ---- sizes a user would run -------------------------------------------------------------------------------------------------
def _random_cloud(n, extent, batch, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    lin = torch.randperm(batch * extent ** 3, generator=g)[:n]
    c = torch.stack([lin // extent ** 3, (lin // extent ** 2) % extent, (lin // extent) % extent, lin % extent], 1)
    return c.int().to(device)


@pytest.mark.parametrize("n,c,batch,extent,dtype", [(100000, 32, 2, 96, torch.float32), (50000, 17, 1, 64, torch.float32),
                                                    (50000, 17, 1, 64, torch.bfloat16), (3000, 8, 2, 96, torch.float64)],
                         ids=["100k_c32_2x96", "c17_1x64", "c17_1x64_bf16", "sparse_3k_2x96_f64"])
def test_dense_at_size(device, host_layer, n, c, batch, extent, dtype):
    import minkowskiengine_amd as ME
    coords = _random_cloud(n, extent, batch, device, 11)
    feats = torch.randn(n, c, device=device).to(dtype).requires_grad_(True)
    shape = torch.Size([batch, c] + [extent] * 3)
    out = ME.SparseTensor(feats, coords).dense(shape=shape, min_coordinate=0)[0]
    ref_in = feats.detach().double().requires_grad_(True)
    want = torch_dense(ref_in, coords, shape, [0] * 3, [1] * 3)
    _same(out.detach(), want.detach().to(dtype))
    gout = torch.randn(shape, device=device).to(dtype)
    out.backward(gout)
    want.backward(gout.double())
    _same(feats.grad, ref_in.grad.to(dtype))


def test_to_sparse_all_4d_at_size(device, host_layer):
    import minkowskiengine_amd as ME
    x = torch.randn(3, 4, 11, 11, 11, 11, device=device, requires_grad=True)
    s = ME.to_sparse_all(x)
    assert torch.equal(s.C.cpu(), ME.dense_coordinates(x.shape))
    _same(s.F.detach(), torch_to_sparse_all(x.detach().double()).float())
    gout = torch.randn_like(s.F)
    s.F.backward(gout)
    _same(x.grad, gout.reshape(3, 11, 11, 11, 11, 4).permute(0, 5, 1, 2, 3, 4).contiguous())


def test_to_sparse_five_percent_at_size(device, host_layer):
    import minkowskiengine_amd as ME
    g = torch.Generator(device="cpu").manual_seed(5)
    keep = (torch.rand(2, 1, 96, 96, 96, generator=g) < 0.05).to(device)
    x = (torch.randn(2, 16, 96, 96, 96, device=device) * keep).requires_grad_(True)
    s = ME.to_sparse(x)
    coords, feats = torch_to_sparse(x.detach().double(), 1)
    assert torch.equal(s.C, coords)
    _same(s.F.detach(), feats.float())
    gout = torch.randn_like(s.F)
    s.F.backward(gout)
    want = torch.zeros_like(x.detach())
    want[(coords[:, 0].long(), slice(None)) + tuple(coords[:, 1:].long().t())] = gout
    _same(x.grad, want)


# ---- determinism, the two hosts ---------------------------------------------------------------------------------------------
def test_two_runs_and_two_hosts_agree_bitwise(device):
    import minkowskiengine_amd as ME
    coords = _random_cloud(20000, 40, 2, device, 3)
    feats = torch.randn(20000, 24, device=device)
    gout = torch.randn(2, 24, 40, 40, 40, device=device)
    xs = torch.randn(2, 40, 40, 7, device=device) * (torch.rand(2, 40, 40, 1, device=device) < 0.3)
    results = []
    prev = ME.get_host()
    try:
        for host in ("python", "native", "python", "native"):
            ME.set_host(host)
            f = feats.clone().requires_grad_(True)
            out = ME.SparseTensor(f, coords).dense(shape=gout.shape, min_coordinate=0)[0]
            out.backward(gout)
            xd = xs.clone().requires_grad_(True)
            s = ME.to_sparse(xd, format="BXXC")
            s.F.backward(s.F.detach() * 2)
            results.append((out.detach(), f.grad, s.C, s.F.detach(), xd.grad))
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for a, b in zip(results[0], other):
            _same(a, b)


# ---- the dense-in / dense-out network of examples/dense_network.py ---------------------------------------------------------
def test_dense_network(device, host_layer):
    import minkowskiengine_amd as ME
    torch.manual_seed(0)
    dense_tensor = torch.rand(3, 4, 11, 11, 11, 11, device=device, requires_grad=True)
    coordinates = ME.dense_coordinates(dense_tensor.shape)
    conv = ME.MinkowskiConvolution(4, 5, stride=2, kernel_size=3, dimension=4).to(device)
    bn = ME.MinkowskiBatchNorm(5).to(device)
    up = ME.MinkowskiConvolutionTranspose(5, 6, stride=2, kernel_size=3, dimension=4).to(device)
    middle = torch.nn.Sequential(conv, bn, ME.MinkowskiReLU(), up)
    network = torch.nn.Sequential(torch.nn.ReLU(), ME.MinkowskiToSparseTensor(remove_zeros=False, coordinates=coordinates),
                                  middle, ME.MinkowskiToDenseTensor(dense_tensor.shape))
    out_shape = (3, 6, 11, 11, 11, 11)
    dev_coordinates = coordinates.to(device)

    def restated(x):
        s = ME.SparseTensor(torch_to_sparse_all(torch.relu(x)), dev_coordinates)
        y = middle(s)
        return torch_dense(y.F, y.C, out_shape, [0] * 4, [1] * 4)

    for _ in range(5):
        dense_tensor.grad = None
        output = network(dense_tensor)
        assert output.shape == out_shape and bool(torch.isfinite(output).all())
        output.sum().backward()
        assert dense_tensor.grad is not None
        got_out, got_grad = output.detach().clone(), dense_tensor.grad.clone()
        state = {k: v.clone() for k, v in bn.state_dict().items()}
        dense_tensor.grad = None
        for p in middle.parameters():
            p.grad = None
        want = restated(dense_tensor)
        want.sum().backward()
        _same(got_out, want.detach())
        _same(got_grad, dense_tensor.grad)
        assert all(k in state for k in bn.state_dict())


# ---- SparseTensor.sparse() and the small helpers ----------------------------------------------------------------------------
def test_sparse_coo_equals_dense(device, host_layer):
    import minkowskiengine_amd as ME
    coords = _random_cloud(500, 12, 2, device, 9)
    x = ME.SparseTensor(torch.randn(500, 5, device=device, dtype=torch.float64), coords)
    sp, mn, ts = x.sparse(min_coords=torch.IntTensor([0, 0, 0]), max_coords=torch.IntTensor([11, 11, 11]))
    d = x.dense(shape=torch.Size([2, 5, 12, 12, 12]), min_coordinate=0)[0]
    _same(sp.to_dense().permute(0, 4, 1, 2, 3).contiguous(), d)
    assert mn.tolist() == [[0, 0, 0]] and ts.tolist() == [1, 1, 1]


def test_small_helpers(device, host_layer):
    import minkowskiengine_amd as ME
    coords = _random_cloud(300, 8, 3, device, 13)
    a = ME.SparseTensor(torch.randn(300, 4, device=device), coords)
    mk = lambda f: ME.SparseTensor(f, coordinate_map_key=a.coordinate_map_key, coordinate_manager=a.coordinate_manager)
    b, c = mk(torch.randn(300, 4, device=device)), mk(torch.randn(300, 4, device=device))
    fs = [a.F, b.F, c.F]
    m = (a.F + b.F + c.F) / 3
    _same(ME.sum(a, b, c).F, a.F + b.F + c.F)
    _same(ME.mean(a, b, c).F, m)
    _same(ME.var([a, b, c]).F, ((a.F - m) ** 2 + (b.F - m) ** 2 + (c.F - m) ** 2) / 3)
    _same(ME.cat(a, b).F, torch.cat([a.F, b.F], 1))
    assert ME.sum(a, b).coordinate_map_key == a.coordinate_map_key
    with pytest.raises(AssertionError):
        ME.sum(a)
    with pytest.raises(AssertionError):
        ME.mean(a, ME.SparseTensor(torch.randn(300, 4, device=device), coords))       # another manager
    lin = ME.MinkowskiLinear(4, 2).to(device)
    _same(ME.MinkowskiStackCat(lin, lin)(a).F.detach(), torch.cat([lin(a).F, lin(a).F], 1).detach())
    two = torch.nn.Sequential(ME.MinkowskiLinear(4, 4).to(device), ME.MinkowskiReLU())
    for cls, want in ((ME.MinkowskiStackSum, lambda u, v: u + v), (ME.MinkowskiStackMean, lambda u, v: (u + v) / 2),
                      (ME.MinkowskiStackVar, lambda u, v: ((u - (u + v) / 2) ** 2 + (v - (u + v) / 2) ** 2) / 2)):
        _same(cls(two, ME.MinkowskiReLU())(a).F.detach(), want(two(a).F, torch.relu(a.F)).detach())
    assert ME.MinkowskiToFeature()(a) is a.F
    assert a.get_device() == a.F.get_device()
    perms = a.decomposition_permutations
    assert len(perms) == 3 and sorted(torch.cat(perms).tolist()) == list(range(300))
    cs, fs2 = a.decomposed_coordinates_and_features
    for bi in range(3):
        idx = (coords[:, 0] == bi).nonzero().flatten()
        assert torch.equal(perms[bi], idx)
        assert torch.equal(a.coordinates_at(bi), coords[idx, 1:]) and torch.equal(a.features_at(bi), a.F[idx])
        c1, f1 = a.coordinates_and_features_at(bi)
        assert torch.equal(c1, cs[bi]) and torch.equal(f1, fs2[bi])
    assert mk(a.F.clone()).double().F.dtype == torch.float64
