"""Dense <-> sparse conversion and the feature-wise helpers of the reference's MinkowskiOps.py (lines 141-498):
`to_sparse`, `to_sparse_all`, `dense_coordinates`, `MinkowskiToSparseTensor`, `MinkowskiToDenseTensor`,
`MinkowskiToFeature`, `MinkowskiStackCat/Sum/Mean/Var`, `sum`, `mean`, `var`, and the machinery behind
`SparseTensor.dense()`.

The reference converts with torch indexing; here feature rows move between the matrix [N, C] and a strided box
[outer, C, inner] on the kernels of csrc/dense.hip (`Dense*GPU` operators of either host layer).  A cell is the linear
index over (B, X1, .., XD); only the movers see where the channel axis sits.  There is no CPU path: CPU tensors raise."""
import torch
from torch.autograd import Function

from . import host as _host
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .layers import _tuple_operator, cat
from .sparse_tensor import SparseTensor
from .tensor_field import TensorField

ROW_STATIONARY, CELL_STATIONARY = 1, 2


def _prod(values):
    n = 1
    for v in values:
        n *= int(v)
    return n


def _policy(n, n_cells, c, t, to_box):
    return int(_host.backend().DensePolicy(int(n), int(n_cells), int(c), t.element_size(), bool(to_box)))


class MinkowskiToDenseFunction(Function):
    """feature rows -> box [outer, C, inner]; the gradient is the box -> rows gather of the same cells.  `cell` /
    `grid` as made by DenseCellIndexGPU; grid may be None (built when a cell-stationary pass wants it)."""

    @staticmethod
    def forward(ctx, feats, cell, grid, outer, inner):
        fn = get_minkowski_function("DenseRowsToBox", feats)
        B = _host.backend()
        feats = feats.contiguous()
        n, c = feats.shape
        policy = _policy(n, outer * inner, c, feats, True)
        if policy == CELL_STATIONARY and grid is None:
            grid = B.DenseGridGPU(cell, outer * inner)
        ctx.misc = (cell, grid, int(n), int(outer), int(inner), B)
        return fn(feats, cell, grid if policy == CELL_STATIONARY else None, outer, inner, policy)

    @staticmethod
    def backward(ctx, grad_box):
        cell, grid, n, outer, inner, B = ctx.misc
        grad_box = grad_box.contiguous()
        c = grad_box.numel() // max(outer * inner, 1)
        policy = _policy(n, outer * inner, c, grad_box, False)
        if policy == CELL_STATIONARY and grid is None:
            grid = B.DenseGridGPU(cell, outer * inner)
        rows = B.DenseBoxToRowsGPU(grad_box, cell, grid if policy == CELL_STATIONARY else None, n, outer, inner, policy)
        return rows, None, None, None, None


class MinkowskiToSparseFunction(Function):
    """box [outer, C, inner] (contiguous, any view of it) -> the feature rows of `cell`; cell = None: every cell in
    order (row r is cell r).  The gradient is the rows -> box pass: zeros wherever no row came from."""

    @staticmethod
    def forward(ctx, box, cell, n, outer, inner):
        fn = get_minkowski_function("DenseBoxToRows", box)
        B = _host.backend()
        box = box.contiguous()
        c = box.numel() // (outer * inner)
        grid = None
        policy = CELL_STATIONARY
        if cell is not None:
            policy = _policy(n, outer * inner, c, box, False)
            if policy == CELL_STATIONARY:
                grid = B.DenseGridGPU(cell, outer * inner)
        ctx.misc = (cell, grid, int(outer), int(inner), tuple(box.shape), B)
        return fn(box, cell, grid, n, outer, inner, policy)

    @staticmethod
    def backward(ctx, grad_rows):
        cell, grid, outer, inner, shape, B = ctx.misc
        grad_rows = grad_rows.contiguous()
        n, c = grad_rows.shape
        policy = CELL_STATIONARY
        if cell is not None:
            policy = _policy(n, outer * inner, c, grad_rows, True)
            if policy == CELL_STATIONARY and grid is None:
                grid = B.DenseGridGPU(cell, outer * inner)
        box = B.DenseRowsToBoxGPU(grad_rows, cell, grid if policy == CELL_STATIONARY else None, outer, inner, policy)
        return box.view(shape), None, None, None, None


def sparse_tensor_to_dense(x, shape=None, min_coordinate=None, contract_stride=True):
    """SparseTensor.dense (MinkowskiSparseTensor.py:460-557).  Host synchronisations: one (the out-of-box flag) when
    `shape` and `min_coordinate` are both given; one more (the extent of the coordinates) when either is None."""
    D = x.D
    origin = isinstance(min_coordinate, int) and not isinstance(min_coordinate, bool) and min_coordinate == 0
    if min_coordinate is not None and not origin:
        assert isinstance(min_coordinate, torch.Tensor) and min_coordinate.dtype == torch.int32, \
            "min_coordinate must be a torch.IntTensor (or 0 for the origin)"
        assert min_coordinate.numel() == D
    if shape is not None:
        assert isinstance(shape, torch.Size)
        assert len(shape) == D + 2  # batch and channel
        if shape[1] != x.F.size(1):
            shape = torch.Size([shape[0], x.F.size(1), *shape[2:]])
    if len(x) == 0:
        assert shape is not None, "shape is required to densify an empty tensor"
        return (torch.zeros(shape, dtype=x.dtype, device=x.device),
                torch.zeros(D, dtype=torch.int32, device=x.device), x.tensor_stride)
    get_minkowski_function("DenseRowsToBox", x.F)        # (raises for CPU features before anything is computed)
    stride = [int(s) for s in x.tensor_stride]
    coords = x.C
    extent = None
    if min_coordinate is None or shape is None:
        extent = torch.stack((coords.min(0)[0], coords.max(0)[0])).cpu()      # the one read-back of this branch
    if min_coordinate is None:
        # as in the reference: the per-axis minimum is checked and RETURNED, but the box starts at the origin
        min_ret = coords.min(0, keepdim=True)[0][:, 1:]
        lowest = [int(v) for v in extent[0, 1:]]
        if any(v < 0 for v in lowest):
            raise ValueError(f"Coordinate has a negative value: {min_ret}. Please provide min_coordinate argument")
        assert all(m % s == 0 for m, s in zip(lowest, stride)), \
            "The minimum coordinates must be divisible by the tensor stride."
        mn = [0] * D
    elif origin:
        min_ret, mn = min_coordinate, [0] * D
    else:
        mn = [int(v) for v in min_coordinate.reshape(-1).cpu()]
        min_ret = min_coordinate.to(x.device)
        if min_ret.ndim == 1:
            min_ret = min_ret.unsqueeze(0)
    assert all(m % s == 0 for m, s in zip(mn, stride)), \
        "The minimum coordinates must be divisible by the tensor stride."
    div = stride if contract_stride else [1] * D
    if shape is None:
        size = [(int(extent[1, 1 + k]) - mn[k]) // div[k] + 1 for k in range(D)]
        shape = torch.Size([int(extent[1, 0]) + 1, x.F.size(1), *size])
    box_shape = [int(shape[0])] + [int(s) for s in shape[2:]]
    B = _host.backend_of(x.coordinate_map_key)
    outer, inner = box_shape[0], _prod(box_shape[1:])
    want_grid = (_policy(len(x), outer * inner, x.F.size(1), x.F, True) == CELL_STATIONARY or
                 (x.F.requires_grad and _policy(len(x), outer * inner, x.F.size(1), x.F, False) == CELL_STATIONARY))
    cell, grid, flag = B.DenseCellIndexGPU(coords.contiguous(), mn, div, box_shape, want_grid)
    dense = MinkowskiToDenseFunction.apply(x.F, cell, grid, outer, inner)
    if int(flag.item()) != 0:
        raise IndexError(f"dense(): a coordinate lies outside the box of shape {tuple(shape)} with min_coordinate {mn}"
                         f" (tensor stride {stride}, contract_stride={contract_stride}); no such row was written")
    return dense.view(shape), min_ret, torch.IntTensor(x.tensor_stride)


def dense_coordinates(shape, device=None):
    """int32 coordinates [B * X1 * .. * XD, D+1] of every cell of a B x C x X1 x .. x XD tensor, in the order of
    `to_sparse_all`'s rows (MinkowskiOps.py:246-276).  On the CPU as in the reference; `device=` (a GPU) generates them
    there instead of uploading a host mesh grid."""
    spatial_dim = len(shape) - 2
    assert spatial_dim > 0, "Invalid shape. Shape must be batch x channel x spatial dimensions."
    size = [int(shape[0])] + [int(s) for s in shape[2:]]
    if device is not None and torch.device(device).type != "cpu":
        return _host.backend().DenseCoordinatesGPU(size, torch.device(device))
    axes = torch.meshgrid(*[torch.arange(s, dtype=torch.int32) for s in size], indexing="ij")
    return torch.stack([a.reshape(-1) for a in axes], 1).contiguous()


def to_sparse(x, format=None, coordinates=None, device=None):
    """A batched dense tensor -> the SparseTensor of its cells with a non-zero channel, rows in ascending order of
    (B, X1, .., XD) (MinkowskiOps.py:279-317).  `format`: "B", one "C", "X" for every spatial axis; default "BCX..X".
    `coordinates` is accepted and unused, as in the reference.  Differentiable in x."""
    assert x.ndim > 2, "Input has 0 spatial dimension."
    assert isinstance(x, torch.Tensor)
    if format is None:
        format = "BC" + "X" * (x.ndim - 2)
    assert x.ndim == len(format), f"Invalid format: {format}. len(format) != x.ndim"
    assert "B" in format and "B" == format[0] and format.count("B") == 1, \
        "The input must have the batch axis and the format must include 'B' indicating the batch axis."
    assert "C" in format and format.count("C") == 1, "The format must indicate the channel axis"
    if device is None:
        device = x.device
    fn = get_minkowski_function("DenseOccupied", x)
    ch_dim = format.find("C")
    box_shape = [int(s) for k, s in enumerate(x.shape) if k != ch_dim]
    outer, inner = _prod(x.shape[:ch_dim]), _prod(x.shape[ch_dim + 1:])
    xc = x.contiguous()
    coords, cell = fn(xc.detach(), outer, inner, box_shape)
    n = int(cell.numel())
    if n == 0:
        features = xc.new_zeros((0, x.size(ch_dim)))
    else:
        features = MinkowskiToSparseFunction.apply(xc, cell, n, outer, inner)
    return SparseTensor(features=features, coordinates=coords, device=device)


def to_sparse_all(dense_tensor, coordinates=None):
    """A B x C x X1 x .. x XD tensor -> the SparseTensor of ALL its cells, zeros included; row r is cell r
    (MinkowskiOps.py:320-348).  coordinates=None generates them on the device; `dense_coordinates(shape)` may be passed
    to reuse one tensor.  Differentiable."""
    spatial_dim = dense_tensor.ndim - 2
    assert spatial_dim > 0, "Invalid shape. Shape must be batch x channel x spatial dimensions."
    get_minkowski_function("DenseBoxToRows", dense_tensor)
    size = [int(dense_tensor.shape[0])] + [int(s) for s in dense_tensor.shape[2:]]
    if coordinates is None:
        coordinates = dense_coordinates(dense_tensor.shape, device=dense_tensor.device)
    outer, inner = size[0], _prod(size[1:])
    features = MinkowskiToSparseFunction.apply(dense_tensor.contiguous(), None, outer * inner, outer, inner)
    return SparseTensor(features, coordinates, device=dense_tensor.device)


class MinkowskiToSparseTensor(MinkowskiModuleBase):
    """A dense tensor (B x C x X1 x .. x XD) or a TensorField -> SparseTensor (MinkowskiOps.py:351-411).  The routing
    is the reference's, as written there: `to_sparse` (zeros removed) only when `remove_zeros` is true AND coordinates
    were given; `to_sparse_all(input, coordinates)` otherwise — so the default module keeps every cell."""

    def __init__(self, remove_zeros=True, coordinates=None):
        super().__init__()
        self.remove_zeros = remove_zeros
        self.coordinates = coordinates

    def forward(self, input):
        if isinstance(input, TensorField):
            return input.sparse()
        elif isinstance(input, torch.Tensor):
            if self.remove_zeros and self.coordinates is not None:
                return to_sparse(input)
            else:
                return to_sparse_all(input, self.coordinates)
        else:
            raise ValueError("Unsupported type. Only TensorField and torch.Tensor are supported")

    def __repr__(self):
        return self.__class__.__name__ + "()"


class MinkowskiToDenseTensor(MinkowskiModuleBase):
    """SparseTensor -> B x C x X1 x .. x XD tensor, `input.dense(shape=shape)[0]` (MinkowskiOps.py:414-457)"""

    def __init__(self, shape=None):
        super().__init__()
        self.shape = shape

    def forward(self, input):
        dense_tensor, _, _ = input.dense(shape=self.shape)
        return dense_tensor

    def __repr__(self):
        return self.__class__.__name__ + "()"


class MinkowskiToFeature(MinkowskiModuleBase):
    """The feature matrix of a sparse tensor or tensor field (MinkowskiOps.py:460-477)"""

    def forward(self, x):
        assert isinstance(x, (SparseTensor, TensorField)), "Invalid input type for MinkowskiToFeature"
        return x.F


def _checked(sparse_tensors):
    if len(sparse_tensors) == 1:
        assert isinstance(sparse_tensors[0], (tuple, list))
        sparse_tensors = sparse_tensors[0]
    assert len(sparse_tensors) > 1, "Invalid number of inputs. The input must be at least two len(sparse_tensors) > 1"
    return tuple(sparse_tensors)


def _sum_of(xs):
    tmp = xs[0] + xs[1]
    for x in xs[2:]:
        tmp = tmp + x
    return tmp


def _var_of(xs):
    m = _sum_of(xs) / len(xs)
    v = (xs[0] - m) ** 2
    for x in xs[1:]:
        v = v + (x - m) ** 2
    return v / len(xs)


def _sum(*sparse_tensors):
    """Sum of the features of tensors on one coordinate map (MinkowskiOps.py:161-185); exported as `ME.sum`"""
    return _tuple_operator(_checked(sparse_tensors), _sum_of)


def mean(*sparse_tensors):
    """Mean of the features of tensors on one coordinate map (MinkowskiOps.py:188-212)"""
    return _tuple_operator(_checked(sparse_tensors), lambda xs: _sum_of(xs) / len(xs))


def var(*sparse_tensors):
    """Biased variance of the features of tensors on one coordinate map (MinkowskiOps.py:215-243)"""
    return _tuple_operator(_checked(sparse_tensors), _var_of)


class MinkowskiStackCat(torch.nn.Sequential):
    def forward(self, x):
        return cat([module(x) for module in self])


class MinkowskiStackSum(torch.nn.Sequential):
    def forward(self, x):
        return _sum([module(x) for module in self])


class MinkowskiStackMean(torch.nn.Sequential):
    def forward(self, x):
        return mean([module(x) for module in self])


class MinkowskiStackVar(torch.nn.Sequential):
    def forward(self, x):
        return var([module(x) for module in self])
