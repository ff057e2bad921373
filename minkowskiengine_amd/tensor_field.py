"""TensorField: features on continuous coordinates, one row per point (reference:
MinkowskiEngine/MinkowskiTensorField.py).  `sparse()` voxelises the field, `SparseTensor.slice(field)` brings a sparse
tensor's features back to the points, `splat()` / `SparseTensor.interpolate(field)` use trilinear weights.  Every
feature movement runs on the weighted CSR gather-sum of csrc/field.hip, in a fixed summation order: results and
gradients are bitwise reproducible.

Dtypes: float32 or float64 features with coordinates of any float type (the manager keeps fp32 coordinates, as the
reference does), and bf16 features (an extension of the reference: this project's networks run in bf16), which
accumulate in fp32 and use fp32 weights.  CPU tensors are rejected, as everywhere in the package."""
import torch
from torch.autograd import Function

from . import host as _host
from .common import convert_to_int_list
from .coordinate_manager import CoordinateManager
from .host import CoordinateMapKey
from .sparse_tensor import SparseTensor, SparseTensorQuantizationMode


def create_splat_coordinates(coordinates):
    """Integer corners of every point: floor(coordinates) + each of the 2^D offsets in {0, 1}^D (the batch column
    unchanged), point-major; the result may hold duplicates (MinkowskiTensorField.py:53-73)."""
    dimension = coordinates.shape[1] - 1
    region_offset = [[0] * (dimension + 1)]
    for d in reversed(range(1, dimension + 1)):
        new_offset = []
        for offset in region_offset:
            offset = offset.copy()
            offset[d] = 1
            new_offset.append(offset)
        region_offset.extend(new_offset)
    region_offset = torch.IntTensor(region_offset).to(coordinates.device)
    coordinates = torch.floor(coordinates).int().unsqueeze(1) + region_offset.unsqueeze(0)
    return coordinates.reshape(-1, dimension + 1)


def _acc(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _identity_rowptr(n, device):
    return torch.arange(n + 1, dtype=torch.int32, device=device)


class _VoxelSum(Function):
    """field -> voxels: y[v] = scale[v] * sum of the field rows of voxel v (in field row order) on the voxel CSR
    (rowptr, cols); backward: each point takes scale[v] * dy[v] of its voxel"""

    @staticmethod
    def forward(ctx, feats, inv32, rowptr, cols, average, B):
        scale = point_scale = None
        if average:
            count = (rowptr[1:] - rowptr[:-1]).to(_acc(feats))
            scale = torch.where(count > 0, 1.0 / count.clamp_min(1), torch.zeros_like(count))
            point_scale = scale[inv32.long()]
        ctx.misc = (inv32, point_scale, B)
        return B.CsrGatherGPU(feats.contiguous(), rowptr, cols, None, scale)

    @staticmethod
    def backward(ctx, grad):
        inv32, point_scale, B = ctx.misc
        g = B.CsrGatherGPU(grad.contiguous(), _identity_rowptr(inv32.numel(), grad.device), inv32, None, point_scale)
        return g, None, None, None, None, None


class _RowGather(Function):
    """y[p] = x[idx[p]] (one entry per row); backward: dx[r] = sum of dy over the rows that took r, in row order, on
    the CSR by r that `csr()` returns (built at most once per map by its owner)"""

    @staticmethod
    def forward(ctx, x, idx32, csr, B):
        ctx.misc = (csr, B)
        return B.CsrGatherGPU(x.contiguous(), _identity_rowptr(idx32.numel(), x.device), idx32)

    @staticmethod
    def backward(ctx, grad):
        csr, B = ctx.misc
        rowptr, cols = csr()
        return B.CsrGatherGPU(grad.contiguous(), rowptr, cols), None, None, None


def _gather_rows(x, idx, owner, csr=None):
    """x[idx] on the CSR kernels, differentiable (idx: int64 or int32 row indices of x).  csr: a callable that returns
    the CSR by row of x of the entries (rowptr, cols), cached by the caller; None: built in the backward."""
    idx32 = idx.to(torch.int32).contiguous()
    B = _host.backend_of(owner)
    n_x = int(x.shape[0])
    if csr is None:
        csr = lambda: B.CsrFromCooGPU(idx32, n_x)[:2]  # noqa: E731
    return _RowGather.apply(x, idx32, csr, B)


class TensorField:
    def __init__(self, features, coordinates=None, tensor_stride=1, coordinate_field_map_key=None,
                 coordinate_manager=None, quantization_mode=SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE,
                 allocator_type=None, minkowski_algorithm=None, requires_grad=None, device=None):
        assert isinstance(features, torch.Tensor), "Features must be a torch.Tensor"
        assert features.ndim == 2, f"The feature should be a matrix, The input feature is an order-{features.ndim} tensor."
        assert isinstance(quantization_mode, SparseTensorQuantizationMode)
        assert quantization_mode in (SparseTensorQuantizationMode.UNWEIGHTED_SUM,
                                     SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE,
                                     SparseTensorQuantizationMode.RANDOM_SUBSAMPLE,
                                     SparseTensorQuantizationMode.MAX_POOL), \
            "invalid quantization mode"
        self.quantization_mode = quantization_mode
        if coordinates is not None:
            assert isinstance(coordinates, torch.Tensor)
        if coordinate_field_map_key is not None:
            assert isinstance(coordinate_field_map_key, CoordinateMapKey)
            assert coordinate_manager is not None, "Must provide coordinate_manager if coordinate_field_map_key is provided"
            assert coordinates is None, "Must not provide coordinates if coordinate_field_map_key is provided"
        if coordinates is None and (coordinate_field_map_key is None or coordinate_manager is None):
            raise ValueError("Either coordinates or (coordinate_field_map_key, coordinate_manager) pair must be provided.")
        if device is not None:
            features = features.to(device)
            if coordinates is not None:
                coordinates = coordinates.to(device)
        if not features.is_cuda or (coordinates is not None and not coordinates.is_cuda):
            raise RuntimeError("minkowskiengine_amd has no CPU path: TensorField features and coordinates must be on "
                               "the GPU")
        self._D = coordinates.size(1) - 1 if coordinates is not None else coordinate_manager.D
        if coordinate_manager is None:
            coordinate_manager = CoordinateManager(D=self._D, allocator_type=allocator_type,
                                                   minkowski_algorithm=minkowski_algorithm)
        self._manager = coordinate_manager
        if coordinates is not None:
            assert features.shape[0] == coordinates.shape[0], \
                "The number of rows in features and coordinates must match."
            if not coordinates.is_floating_point():
                coordinates = coordinates.float()
            coordinate_field_map_key = coordinate_manager.insert_field(
                coordinates, convert_to_int_list(tensor_stride, self._D), "")
        else:
            assert coordinate_field_map_key.is_key_set(), "The coordinate key must be valid."
        if requires_grad is not None:
            features.requires_grad_(requires_grad)
        self._F = features
        self._C = coordinates
        self.coordinate_field_map_key = coordinate_field_map_key
        self._inverse_mapping = {}
        self._voxel_csrs = {}       # sparse key -> (rowptr, cols): the points of each voxel in field order
        self._splat = {}
        self._batch_rows = None

    # ---- accessors (MinkowskiTensorField.py:252-285) ------------------------------------------------------------------
    @property
    def coordinate_key(self):
        return self.coordinate_field_map_key

    @property
    def coordinate_map_key(self):
        return self.coordinate_field_map_key

    @property
    def coordinate_manager(self):
        return self._manager

    @property
    def C(self):
        if self._C is None:
            self._C = self._manager.get_coordinate_field(self.coordinate_field_map_key)
        return self._C

    coordinates = C

    @property
    def F(self):
        return self._F

    features = F

    @property
    def D(self):
        return self._D

    dimension = D

    @property
    def tensor_stride(self):
        return self.coordinate_field_map_key.get_tensor_stride()

    @property
    def requires_grad(self):
        return self._F.requires_grad

    def requires_grad_(self, requires_grad=True):
        self._F.requires_grad_(requires_grad)
        return self

    @property
    def dtype(self):
        return self._F.dtype

    @property
    def device(self):
        return self._F.device

    @property
    def shape(self):
        return self._F.shape

    def size(self):
        return self._F.size()

    def __len__(self):
        return len(self._F)

    def detach(self):
        return self._like(self._F.detach())

    def _like(self, features):
        """a field on the same coordinates with other features"""
        out = TensorField(features, coordinate_field_map_key=self.coordinate_field_map_key,
                          coordinate_manager=self._manager, quantization_mode=self.quantization_mode)
        out._C = self._C
        out._inverse_mapping = self._inverse_mapping
        out._voxel_csrs = self._voxel_csrs
        out._splat = self._splat
        return out

    @property
    def _batchwise_row_indices(self):
        # MinkowskiTensorField.py:276-281: the rows of each origin row (= batch index, ascending) from origin_field_map
        if self._batch_rows is None:
            rows = self._manager.origin_field_map(self.coordinate_field_map_key)[0][1].long()
            n_batch = self._manager.size(self._manager.origin_field(self.coordinate_field_map_key))
            order = torch.argsort(rows, stable=True)
            counts = torch.bincount(rows, minlength=n_batch).tolist()
            self._batch_rows = list(torch.split(order, counts))
        return self._batch_rows

    @property
    def decomposed_coordinates(self):
        return [self.C[idx, 1:] for idx in self._batchwise_row_indices]

    @property
    def decomposed_features(self):
        return [self._F[idx] for idx in self._batchwise_row_indices]

    def decomposed_coordinates_and_features(self):
        rows = self._batchwise_row_indices
        return [self.C[i, 1:] for i in rows], [self._F[i] for i in rows]

    # ---- field -> sparse (MinkowskiTensorField.py:286-380) ------------------------------------------------------------
    def sparse(self, tensor_stride=1, coordinate_map_key=None, quantization_mode=None):
        if quantization_mode is None:
            quantization_mode = self.quantization_mode
        if quantization_mode == SparseTensorQuantizationMode.MAX_POOL:
            raise NotImplementedError(
                "MAX_POOL quantisation of a TensorField is not wired to MinkowskiDirectMaxPoolingFunction yet; call it "
                "directly:\n"
                "    key, (_, inv) = mgr.field_to_sparse_insert_and_map(field.coordinate_field_map_key, tensor_stride)\n"
                "    F = ME.MinkowskiDirectMaxPoolingFunction.apply(torch.arange(len(field), device=field.device), inv, "
                "field.F, mgr.size(key))\n"
                "    voxels = ME.SparseTensor(F, coordinate_map_key=key, coordinate_manager=mgr)")
        assert quantization_mode != SparseTensorQuantizationMode.SPLAT_LINEAR_INTERPOLATION, \
            "Please use .splat() for splat quantization."
        mgr = self._manager
        B = _host.backend_of(mgr)
        if coordinate_map_key is None:
            tensor_stride = convert_to_int_list(tensor_stride, self.D)
            coordinate_map_key, (unique_index, inverse_mapping) = mgr.field_to_sparse_insert_and_map(
                self.coordinate_field_map_key, tensor_stride)
            n_rows = len(unique_index)
            sparse_rows, field_rows = inverse_mapping, None
        else:
            sparse_rows, field_rows = mgr.field_to_sparse_map(self.coordinate_field_map_key, coordinate_map_key)
            unique_index = None
            n_rows = mgr.size(coordinate_map_key)
            if len(sparse_rows) == len(self._F):
                field_rows = None          # every point hits: sparse_rows is the inverse mapping
        feats = self._F
        if field_rows is not None:         # points outside the map do not contribute
            feats = _gather_rows(feats, field_rows, mgr)
        if field_rows is None:
            self._inverse_mapping[coordinate_map_key] = sparse_rows
        if quantization_mode in (SparseTensorQuantizationMode.UNWEIGHTED_SUM,
                                 SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE):
            inv32 = sparse_rows.to(torch.int32).contiguous()
            if field_rows is None:
                rowptr, cols = self.voxel_csr(coordinate_map_key)
            else:
                rowptr, cols, _ = B.CsrFromCooGPU(inv32, n_rows)
            features = _VoxelSum.apply(feats, inv32, rowptr, cols,
                                       quantization_mode == SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, B)
        elif quantization_mode == SparseTensorQuantizationMode.RANDOM_SUBSAMPLE:
            if unique_index is None:       # first point of each voxel
                unique_index = torch.full((n_rows,), len(sparse_rows), dtype=torch.int64, device=feats.device)
                unique_index.scatter_reduce_(0, sparse_rows.long(),
                                             torch.arange(len(sparse_rows), device=feats.device), "amin")
                assert bool((unique_index < len(sparse_rows)).all()), "every voxel of the map needs a point"
            features = _gather_rows(feats, unique_index, mgr)
        else:
            raise ValueError("Invalid quantization mode")
        return SparseTensor(features, coordinate_map_key=coordinate_map_key, coordinate_manager=mgr)

    def splat(self):
        """Trilinear splat of the points onto the integer corners around them (MinkowskiTensorField.py:381-406)."""
        splat_coordinates = create_splat_coordinates(self.C)
        coordinate_map_key, _ = self._manager.insert_and_map(splat_coordinates)
        n_rows = self._manager.size(coordinate_map_key)
        tensor_map, field_map, weights = self._manager.interpolation_map_weight(coordinate_map_key, self.C)
        size = torch.Size([n_rows, len(self._F)])
        self._splat[coordinate_map_key] = (tensor_map, field_map, weights, size)
        from .sparse_matrix_functions import MinkowskiSPMMFunction
        features = MinkowskiSPMMFunction.apply(tensor_map, field_map, weights, size, self._F)
        return SparseTensor(features, coordinate_map_key=coordinate_map_key, coordinate_manager=self._manager)

    def inverse_mapping(self, sparse_tensor_map_key):
        """Row of `sparse_tensor_map_key` of every point (MinkowskiTensorField.py:408-450); a strided key resolves
        through the stride-1 map's stride_map."""
        if sparse_tensor_map_key not in self._inverse_mapping:
            mgr = self._manager
            if not mgr.exists_field_to_sparse(self.coordinate_field_map_key, sparse_tensor_map_key):
                sparse_keys = mgr.field_to_sparse_keys(self.coordinate_field_map_key)
                one_key = None
                for key in sparse_keys:
                    if all(s == 1 for s in key.get_tensor_stride()):
                        one_key = key
                if one_key is None:
                    raise RuntimeError("no stride-1 sparse tensor of this field: call sparse() first")
                if one_key not in self._inverse_mapping:
                    _, self._inverse_mapping[one_key] = mgr.get_field_to_sparse_map(self.coordinate_field_map_key,
                                                                                    one_key)
                _, stride_map = mgr.stride_map(one_key, sparse_tensor_map_key)
                self._inverse_mapping[sparse_tensor_map_key] = stride_map[self._inverse_mapping[one_key]]
            else:
                _, self._inverse_mapping[sparse_tensor_map_key] = mgr.get_field_to_sparse_map(
                    self.coordinate_field_map_key, sparse_tensor_map_key)
        return self._inverse_mapping[sparse_tensor_map_key]

    def voxel_csr(self, sparse_tensor_map_key):
        """(rowptr int32 [n_voxels + 1], cols int32 [N]): the points of each voxel of the key, in field row order — the
        stable transpose of inverse_mapping(key), built once per key (sparse() forward, slice backward)"""
        csr = self._voxel_csrs.get(sparse_tensor_map_key)
        if csr is None:
            inv = self.inverse_mapping(sparse_tensor_map_key)
            B = _host.backend_of(self._manager)
            rowptr, cols, _ = B.CsrFromCooGPU(inv.to(torch.int32).contiguous(),
                                              self._manager.size(sparse_tensor_map_key))
            csr = self._voxel_csrs[sparse_tensor_map_key] = (rowptr, cols)
        return csr

    # ---- arithmetic (MinkowskiTensorField.py:452-475) -------------------------------------------------------------------
    def _binary(self, other, op):
        if isinstance(other, TensorField):
            assert other._manager is self._manager, "coordinate managers must match"
            assert self.coordinate_field_map_key == other.coordinate_field_map_key, "coordinate field keys must match"
            return self._like(op(self._F, other._F))
        return self._like(op(self._F, other))

    def __add__(self, other):
        return self._binary(other, torch.add)

    def __radd__(self, other):
        return self._binary(other, torch.add)

    def __sub__(self, other):
        return self._binary(other, torch.sub)

    def __rsub__(self, other):
        return self._like(other - self._F)

    def __mul__(self, other):
        return self._binary(other, torch.mul)

    def __rmul__(self, other):
        return self._binary(other, torch.mul)

    def __truediv__(self, other):
        return self._binary(other, torch.div)

    def __neg__(self):
        return self._like(-self._F)

    def __repr__(self):
        return (f"{self.__class__.__name__}(\n  coordinates={self.C}\n  features={self._F}\n  "
                f"coordinate_field_map_key={self.coordinate_field_map_key}\n  coordinate_manager={self._manager}"
                f"  spatial dimension={self._D})")
