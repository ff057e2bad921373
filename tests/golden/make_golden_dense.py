"""Generate the dense <-> sparse conversion fixtures (dense_*.npz) from the reference's own `SparseTensor.dense`,
`ME.to_sparse`, `ME.to_sparse_all`, `ME.dense_coordinates`, `MinkowskiToSparseTensor` and `MinkowskiToDenseTensor`.

oracle.ref.import_reference_package() imports the reference's unmodified Python package over its compiled CPU extension;
this script runs the reference's functions on the CPU in float64 and stores, per case, the inputs, every returned value
and the gradient for a recorded upstream gradient.  Every recorded result is also asserted EXACTLY (these are copies, not
sums) against a plain numpy restatement:

    dense:          out[b, :, (x - min) // div] = feats[row], zeros elsewhere (div = tensor stride, or 1 when not contracted;
                    with min_coordinate=None the reference RETURNS the per-axis minimum but places the box at the origin)
    to_sparse:      rows = cells with abs(x).sum(channel) != 0 in ascending order of (B, X1, .., XD) (numpy's argwhere)
    to_sparse_all:  row r = cell r, all cells
    gradients:      the same index maps backwards

Feature values are float64 copies of fp32 numbers with at most 8 significant bits, so that a cast to fp32 or bf16 is exact
and the tests can ask for bitwise equality in every dtype.

Every file has a `kind` ("dense", "to_sparse", "to_sparse_all", "dense_coordinates", "module", "sparse") and a `source`:
"reference" when the values came out of the reference's code, "restatement" when the reference cannot run the case under
the installed torch and the values are the numpy restatement alone.  That is so for
  * `min_coordinate=0` of `dense()`: the reference documents it but its first assertion rejects an int;
  * `SparseTensor.sparse()`: it uses the removed `torch.sparse.FloatTensor` constructors.
The work runs in a subprocess: importing the reference package rewires sys.modules.

    python tests/golden/make_golden_dense.py
The .npz files are committed (each below 1 MiB, data only); tests never need the reference."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))


def values(shape, g):
    """fp32 numbers in (-2, 2) \\ {0} with 8 significant bits: exact in bf16, fp32 and float64"""
    v = torch.randint(1, 256, shape, generator=g).double() / 128.0
    return v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def save(name, **data):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    print(name, str(data["kind"]), str(data["source"]), "bytes", os.path.getsize(path))


# ---- numpy restatements ---------------------------------------------------------------------------------------------------
def dense_np(coords, feats, shape, mn, div):
    out = np.zeros(shape, dtype=feats.dtype)
    idx = (coords[:, 1:].astype(np.int64) - np.asarray(mn, dtype=np.int64)) // np.asarray(div, dtype=np.int64)
    assert (idx >= 0).all() and (idx < np.asarray(shape[2:])).all()
    for r in range(coords.shape[0]):
        out[(int(coords[r, 0]), slice(None)) + tuple(int(v) for v in idx[r])] = feats[r]
    return out, idx


def dense_grad_np(coords, idx, grad_out):
    return np.stack([grad_out[(int(coords[r, 0]), slice(None)) + tuple(int(v) for v in idx[r])]
                     for r in range(coords.shape[0])])


def to_sparse_np(x, ch):
    mask = np.abs(x).sum(ch) != 0
    coords = np.argwhere(mask).astype(np.int32)
    return coords, np.moveaxis(x, ch, -1)[mask], mask


def to_sparse_grad_np(x, ch, mask, grad_rows):
    g = np.zeros_like(np.moveaxis(x, ch, -1))
    g[mask] = grad_rows
    return np.moveaxis(g, -1, ch)


# ---- cases ------------------------------------------------------------------------------------------------------------------
def dense_case(RME, name, coords, c, seed, tensor_stride=1, shape=None, min_coordinate=None, contract=True,
               feats=None):
    """min_coordinate: None | "zero" | list of D ints"""
    g = torch.Generator().manual_seed(seed)
    D = coords.shape[1] - 1
    n = coords.shape[0]
    feats = values((n, c), g) if feats is None else feats
    leaf = feats.clone().requires_grad_(True)
    ts = [tensor_stride] * D
    co = coords.numpy()
    source = "reference"
    if min_coordinate == "zero":
        source = "restatement"
        mn = [0] * D
    elif min_coordinate is None:
        mn = [0] * D       # (the reference returns the per-axis minimum but does NOT shift by it: the box starts at the origin)
    else:
        mn = list(min_coordinate)
    div = ts if contract else [1] * D
    if shape is None:
        size = ((co[:, 1:].max(0) - np.asarray(mn)) // np.asarray(div) + 1).tolist()
        full = [int(co[:, 0].max()) + 1, c] + size
    else:
        full = [shape[0], c] + list(shape[2:])
    want, idx = dense_np(co, feats.numpy(), full, mn, div)
    grad_out = values(tuple(full), g)
    want_grad = dense_grad_np(co, idx, grad_out.numpy())
    if source == "reference":
        x = RME.SparseTensor(leaf, coords, tensor_stride=tensor_stride)
        assert torch.equal(x.C.int(), coords.int()), "the reference kept the row order"
        kw = {}
        if shape is not None:
            kw["shape"] = torch.Size(shape)
        if min_coordinate is not None:
            kw["min_coordinate"] = torch.IntTensor(mn)
        out, ret_min, ret_stride = x.dense(contract_stride=contract, **kw)
        out.backward(grad_out)
        assert list(out.shape) == full, (name, out.shape, full)
        assert np.array_equal(out.detach().numpy(), want), name
        assert np.array_equal(leaf.grad.numpy(), want_grad), name
        assert isinstance(ret_min, torch.Tensor) and ret_min.dtype == torch.int32 and tuple(ret_min.shape) == (1, D)
        assert isinstance(ret_stride, torch.Tensor) and ret_stride.dtype == torch.int32 and not ret_stride.is_cuda
        ret_min_want = co[:, 1:].min(0).tolist() if min_coordinate is None else mn
        assert ret_min.flatten().tolist() == ret_min_want and ret_stride.tolist() == ts
        ret_min_kind = "int32 tensor [1, D] on the device of the features"
    else:
        ret_min_kind = "the int 0 that was passed"
    save(name, kind="dense", source=source, coords=co.astype(np.int32), feats=feats.numpy(), tensor_stride=np.int32(tensor_stride),
         shape_arg=np.asarray([] if shape is None else shape, dtype=np.int64),
         min_arg=np.asarray("none" if min_coordinate is None else ("zero" if min_coordinate == "zero" else "tensor")),
         min_coordinate=np.asarray(mn, dtype=np.int32),
         ret_min=np.asarray(co[:, 1:].min(0) if min_coordinate is None else mn, dtype=np.int32), contract=np.bool_(contract), dense=want, ret_min_kind=ret_min_kind,
         ret_stride=np.asarray(ts, dtype=np.int32), grad_out=grad_out.numpy(), grad_feats=want_grad)


def strided_coords(RME, coords, D):
    """coordinates of the reference's stride-2 convolution output (tensor stride 2)"""
    x = RME.SparseTensor(torch.ones(coords.shape[0], 1), coords)
    y = RME.MinkowskiConvolution(1, 1, kernel_size=3, stride=2, dimension=D)(x)
    assert y.tensor_stride == [2] * D
    return y.C.int().clone()


def half_zero(shape, ch, g, zero_batch=None, keep=0.5):
    """a box with about half of its cells zero in every channel; one batch element may be zero altogether"""
    x = values(shape, g)
    cells = [s for k, s in enumerate(shape) if k != ch]
    mask = (torch.rand(cells, generator=g) < keep).double().unsqueeze(ch)
    x = x * mask
    if zero_batch is not None:
        x[zero_batch] = 0
    return x


def to_sparse_case(RME, name, shape, fmt, seed, zero_batch=None, keep=0.5):
    g = torch.Generator().manual_seed(seed)
    ch = 1 if fmt is None else fmt.find("C")
    x = half_zero(shape, ch, g, zero_batch, keep)
    leaf = x.clone().requires_grad_(True)
    s = RME.to_sparse(leaf) if fmt is None else RME.to_sparse(leaf, format=fmt)
    coords, feats, mask = to_sparse_np(x.numpy(), ch)
    assert np.array_equal(s.C.numpy(), coords), name          # the reference's row order IS ascending cell order
    assert np.array_equal(s.F.detach().numpy(), feats), name
    grad_out = values(tuple(feats.shape), g)
    want_grad = to_sparse_grad_np(x.numpy(), ch, mask, grad_out.numpy())
    if feats.shape[0] > 0:
        s.F.backward(grad_out)
        assert np.array_equal(leaf.grad.numpy(), want_grad), name
    save(name, kind="to_sparse", source="reference", x=x.numpy(), format=np.asarray("" if fmt is None else fmt),
         coords=coords, feats=feats, grad_out=grad_out.numpy(), grad_x=want_grad)


def to_sparse_all_case(RME, name, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = values(shape, g)
    leaf = x.clone().requires_grad_(True)
    s = RME.to_sparse_all(leaf)
    c = shape[1]
    feats = np.moveaxis(x.numpy(), 1, -1).reshape(-1, c)
    coords = np.argwhere(np.ones([shape[0]] + list(shape[2:]), dtype=bool)).astype(np.int32)
    assert np.array_equal(s.C.numpy(), coords) and np.array_equal(s.F.detach().numpy(), feats), name
    assert np.array_equal(RME.dense_coordinates(torch.Size(shape)).numpy(), coords), name
    grad_out = values(tuple(feats.shape), g)
    s.F.backward(grad_out)
    want_grad = np.moveaxis(grad_out.numpy().reshape([shape[0]] + list(shape[2:]) + [c]), -1, 1)
    assert np.array_equal(leaf.grad.numpy(), want_grad), name
    save(name, kind="to_sparse_all", source="reference", x=x.numpy(), coords=coords, feats=feats, grad_out=grad_out.numpy(),
         grad_x=want_grad)


def module_case(RME, name, shape, seed, remove_zeros, with_coordinates):
    g = torch.Generator().manual_seed(seed)
    x = half_zero(shape, 1, g)
    coordinates = RME.dense_coordinates(torch.Size(shape)) if with_coordinates else None
    s = RME.MinkowskiToSparseTensor(remove_zeros=remove_zeros, coordinates=coordinates)(x)
    # the routing as written in the reference: zeros are removed only with remove_zeros AND coordinates
    if remove_zeros and with_coordinates:
        coords, feats, _ = to_sparse_np(x.numpy(), 1)
    else:
        feats = np.moveaxis(x.numpy(), 1, -1).reshape(-1, shape[1])
        coords = np.argwhere(np.ones([shape[0]] + list(shape[2:]), dtype=bool)).astype(np.int32)
    assert np.array_equal(s.C.numpy(), coords) and np.array_equal(s.F.numpy(), feats), name
    # and back: MinkowskiToDenseTensor with a shape whose channel count is wrong on purpose
    wrong = torch.Size([shape[0], shape[1] + 3] + list(shape[2:]))
    back = RME.MinkowskiToDenseTensor(wrong)(s)
    assert np.array_equal(back.numpy(), x.numpy()), name
    save(name, kind="module", source="reference", x=x.numpy(), remove_zeros=np.bool_(remove_zeros),
         with_coordinates=np.bool_(with_coordinates), coords=coords, feats=feats, dense_shape_arg=np.asarray(wrong, dtype=np.int64),
         dense=back.numpy())


def sparse_case(name, coords, c, seed, tensor_stride, contract, with_max):
    """SparseTensor.sparse(): restatement only (the reference's constructors are gone from torch)"""
    g = torch.Generator().manual_seed(seed)
    co = coords.numpy()
    D = co.shape[1] - 1
    feats = values((co.shape[0], c), g).numpy()
    ts = np.full(D, tensor_stride, dtype=np.int64)
    mn = co[:, 1:].min(0).astype(np.int64)
    mx = co[:, 1:].max(0).astype(np.int64) + 2 * ts
    idx = co[:, 1:] - mn
    ret_min = mn.copy()
    if contract:
        idx, ret_min, mx = idx // ts, mn // ts, mx // ts
    if with_max:
        size = [int(co[:, 0].max()) + 1] + (mx - ret_min + 1).tolist() + [c]
    else:
        size = [int(co[:, 0].max()) + 1] + (idx.max(0) + 1).tolist() + [c]
    out = np.zeros(size)
    for r in range(co.shape[0]):
        out[(int(co[r, 0]),) + tuple(int(v) for v in idx[r])] = feats[r]
    save(name, kind="sparse", source="restatement", coords=co.astype(np.int32), feats=feats, tensor_stride=np.int32(tensor_stride),
         contract=np.bool_(contract), max_arg=(co[:, 1:].max(0) + 2 * ts).astype(np.int32) if with_max else np.zeros(0, np.int32),
         to_dense=out, ret_min=ret_min.astype(np.int32).reshape(1, D), ret_stride=ts.astype(np.int32))


def make_dense_cases():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import ref
    RME = ref.import_reference_package()
    from make_golden import cloud

    # the hand case of the reference's tests/python/dense.py:47-65
    hand = torch.IntTensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [1, 1, 1], [1, 1, 2], [1, 2, 1]])
    hand_f = torch.DoubleTensor([[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]])
    dense_case(RME, "dense_2d_hand", hand, 2, seed=1, feats=hand_f)
    pos = lambda c: torch.cat([c[:, :1], c[:, 1:] - c[:, 1:].min(0)[0]], 1)     # shifted to non-negative coordinates
    dense_case(RME, "dense_3d_b2_min_none_c3", pos(cloud(300, 10, 3, 41, batch=2)) + torch.IntTensor([[0, 2, 0, 1]]), 3, seed=2)
    s2 = strided_coords(RME, pos(cloud(500, 16, 3, 42, batch=2)), 3)
    dense_case(RME, "dense_3d_stride2_contracted_c16", s2, 16, seed=3, tensor_stride=2)
    dense_case(RME, "dense_3d_stride2_not_contracted_c4", s2, 4, seed=4, tensor_stride=2, contract=False)
    neg = cloud(300, 12, 3, 43, batch=2)
    assert int(neg[:, 1:].min()) < 0
    dense_case(RME, "dense_3d_negative_min_c17", neg, 17, seed=5, min_coordinate=[-8, -6, -7])
    dense_case(RME, "dense_3d_shape_larger_wrong_channels_c3", pos(cloud(200, 8, 3, 44, batch=2)), 3, seed=6,
               shape=[3, 7, 11, 9, 12], min_coordinate=[0, 0, 0])
    dense_case(RME, "dense_3d_min_zero_c1", pos(cloud(200, 8, 3, 45, batch=2)) + torch.IntTensor([[0, 1, 0, 2]]), 1, seed=7,
               min_coordinate="zero")
    dense_case(RME, "dense_4d_b2_c5", pos(cloud(250, 6, 4, 46, batch=2)), 5, seed=8)
    dense_case(RME, "dense_1d_b3_c2", pos(cloud(20, 40, 1, 47, batch=3)), 2, seed=9)

    to_sparse_case(RME, "dense_to_sparse_bcxx_c3", [3, 3, 13, 17], None, seed=11)
    to_sparse_case(RME, "dense_to_sparse_bxxxc_c16", [2, 9, 8, 7, 16], "BXXXC", seed=12)
    to_sparse_case(RME, "dense_to_sparse_bxcxx_c17", [2, 6, 17, 5, 7], "BXCXX", seed=13)
    to_sparse_case(RME, "dense_to_sparse_zero_batch_c1", [3, 1, 12, 12, 12], "BCXXX", seed=14, zero_batch=1)
    to_sparse_case(RME, "dense_to_sparse_all_zero_c2", [2, 2, 9, 9], None, seed=15, keep=0.0)
    to_sparse_all_case(RME, "dense_to_sparse_all_3d_c4", [2, 4, 7, 6, 5], seed=16)
    to_sparse_all_case(RME, "dense_to_sparse_all_4d_c3", [2, 3, 4, 5, 3, 4], seed=17)
    shape = [3, 4, 5, 6, 7, 8]
    save("dense_coordinates_4d", kind="dense_coordinates", source="reference", shape=np.asarray(shape, dtype=np.int64),
         coords=RME.dense_coordinates(torch.Size(shape)).numpy())
    module_case(RME, "dense_module_default", [2, 3, 6, 7], 21, remove_zeros=True, with_coordinates=False)
    module_case(RME, "dense_module_remove_zeros_with_coordinates", [2, 3, 6, 7], 22, remove_zeros=True, with_coordinates=True)
    module_case(RME, "dense_module_keep_zeros_with_coordinates", [2, 3, 6, 7], 23, remove_zeros=False, with_coordinates=True)
    sparse_case("dense_sparse_coo_3d_c3", pos(cloud(150, 8, 3, 48, batch=2)), 3, 31, tensor_stride=1, contract=True, with_max=False)
    sparse_case("dense_sparse_coo_3d_stride2_max_c2", s2[:200], 2, 32, tensor_stride=2, contract=True, with_max=True)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        make_dense_cases()
    else:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker"])
