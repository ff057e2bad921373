"""SparseTensor: features F [N, C] + lazily fetched coordinates C [N, D+1] + the key of its
coordinate map + the manager that owns the map (reference:
MinkowskiEngine/MinkowskiSparseTensor.py:48-345 and MinkowskiTensor.py:139-604)."""
import enum
import warnings

import torch

from . import host as _host
from .host import CoordinateMapKey
from .common import convert_to_int_list
from .coordinate_manager import CoordinateManager


class SparseTensorOperationMode(enum.Enum):
    SEPARATE_COORDINATE_MANAGER = 0
    SHARE_COORDINATE_MANAGER = 1


class SparseTensorQuantizationMode(enum.Enum):
    RANDOM_SUBSAMPLE = 0
    UNWEIGHTED_AVERAGE = 1
    UNWEIGHTED_SUM = 2
    NO_QUANTIZATION = 3
    MAX_POOL = 4
    SPLAT_LINEAR_INTERPOLATION = 5


_sparse_tensor_operation_mode = SparseTensorOperationMode.SEPARATE_COORDINATE_MANAGER
_global_coordinate_manager = None


def set_sparse_tensor_operation_mode(operation_mode):
    """MinkowskiTensor.py:71-103"""
    assert isinstance(operation_mode, SparseTensorOperationMode)
    global _sparse_tensor_operation_mode
    _sparse_tensor_operation_mode = operation_mode


def sparse_tensor_operation_mode():
    return _sparse_tensor_operation_mode


def global_coordinate_manager():
    return _global_coordinate_manager


def set_global_coordinate_manager(coordinate_manager):
    global _global_coordinate_manager
    _global_coordinate_manager = coordinate_manager


def clear_global_coordinate_manager():
    set_global_coordinate_manager(None)


class SparseTensor:
    def __init__(self, features, coordinates=None, tensor_stride=1, coordinate_map_key=None,
                 coordinate_manager=None, quantization_mode=SparseTensorQuantizationMode.RANDOM_SUBSAMPLE,
                 allocator_type=None, minkowski_algorithm=None, requires_grad=None, device=None):
        assert isinstance(features, torch.Tensor), "Features must be a torch.Tensor"
        assert features.ndim == 2, f"The feature should be a matrix, The input feature is an order-{features.ndim} tensor."
        assert isinstance(quantization_mode, SparseTensorQuantizationMode)
        self.quantization_mode = quantization_mode
        if coordinates is not None:
            assert isinstance(coordinates, torch.Tensor)
        if coordinate_map_key is not None:
            assert isinstance(coordinate_map_key, CoordinateMapKey)
            assert coordinate_manager is not None, "Must provide coordinate_manager if coordinate_map_key is provided"
            assert coordinates is None, "Must not provide coordinates if coordinate_map_key is provided"
        if coordinate_manager is not None:
            assert isinstance(coordinate_manager, CoordinateManager)
        if coordinates is None and (coordinate_map_key is None or coordinate_manager is None):
            raise ValueError("Either coordinates or (coordinate_map_key, coordinate_manager) pair must be provided.")

        if device is not None:
            features = features.to(device)
            if coordinates is not None:
                coordinates = coordinates.to(device)

        self._D = coordinates.size(1) - 1 if coordinates is not None else coordinate_manager.D
        own_manager = False

        if coordinate_manager is None:
            if _sparse_tensor_operation_mode == SparseTensorOperationMode.SHARE_COORDINATE_MANAGER:
                coordinate_manager = global_coordinate_manager()
                if coordinate_manager is None:
                    coordinate_manager = CoordinateManager(D=self._D, allocator_type=allocator_type,
                                                           minkowski_algorithm=minkowski_algorithm)
                    set_global_coordinate_manager(coordinate_manager)
            else:
                coordinate_manager = CoordinateManager(D=self._D, allocator_type=allocator_type,
                                                       minkowski_algorithm=minkowski_algorithm)
                own_manager = True
        self._manager = coordinate_manager

        if coordinates is not None:
            assert features.shape[0] == coordinates.shape[0], \
                "The number of rows in features and coordinates must match."
            assert features.is_cuda == coordinates.is_cuda, "Features and coordinates must have the same backend."
            coordinate_map_key = _host.key_like(coordinate_manager, convert_to_int_list(tensor_stride, self._D), "")
            coordinates, features, coordinate_map_key = self.initialize_coordinates(
                coordinates, features, coordinate_map_key)
            if own_manager:
                from .coordinate_manager import _prefetch_from_previous
                _prefetch_from_previous(coordinate_manager)
        else:
            assert coordinate_map_key.is_key_set(), "The coordinate key must be valid."

        if requires_grad is not None:
            features.requires_grad_(requires_grad)
        self._F = features
        self._C = coordinates
        self.coordinate_map_key = coordinate_map_key

    # MinkowskiSparseTensor.py:293-345
    def initialize_coordinates(self, coordinates, features, coordinate_map_key):
        if coordinates.dtype != torch.int32:
            warnings.warn("coordinates implicitly converted to torch.IntTensor. To remove this warning, use "
                          "`.int()` to convert the coords into an torch.IntTensor")
            coordinates = torch.floor(coordinates).int()
        coordinates = coordinates.contiguous()
        coordinate_map_key, (unique_index, inverse_mapping) = self._manager.insert_and_map(
            coordinates, *coordinate_map_key.get_key())
        self.unique_index = unique_index.long()
        self.inverse_mapping = inverse_mapping
        n_unique = self.unique_index.numel()
        if n_unique == coordinates.shape[0]:
            # no duplicates: first-occurrence order == input order
            return coordinates, features, coordinate_map_key
        coordinates = coordinates[self.unique_index]
        mode = self.quantization_mode
        if mode in (SparseTensorQuantizationMode.UNWEIGHTED_SUM, SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE):
            # duplicate coordinates: rows of a voxel are summed in input order by one HIP kernel (deterministic;
            # the reference goes through cuSPARSE coo_spmm, MinkowskiSparseTensor.py:317-341)
            from .utils.quantization import segment_reduce
            features = segment_reduce(features, inverse_mapping, n_unique,
                                      average=(mode == SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE))
        elif mode == SparseTensorQuantizationMode.RANDOM_SUBSAMPLE:
            features = features[self.unique_index]
        return coordinates, features, coordinate_map_key

    # ---- accessors (MinkowskiTensor.py:139-330) ---------------------------------------------------
    @property
    def coordinate_key(self):
        return self.coordinate_map_key

    @property
    def coordinate_manager(self):
        return self._manager

    @property
    def tensor_stride(self):
        return self.coordinate_map_key.get_tensor_stride()

    @property
    def C(self):
        if self._C is None:
            self._C = self._manager.get_coordinates(self.coordinate_map_key)
        return self._C

    @property
    def coordinates(self):
        return self.C

    @property
    def F(self):
        return self._F

    @property
    def features(self):
        return self._F

    @property
    def D(self):
        return self._D

    @property
    def dimension(self):
        return self._D

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

    def float(self):
        self._F = self._F.float()
        return self

    def double(self):
        self._F = self._F.double()
        return self

    def get_device(self):
        return self._F.get_device()

    def detach(self):
        return SparseTensor(self._F.detach(), coordinate_map_key=self.coordinate_map_key,
                            coordinate_manager=self._manager)

    # ---- conversions (MinkowskiSparseTensor.py:348-557) ---------------------------------------------------------------
    def dense(self, shape=None, min_coordinate=None, contract_stride=True):
        """-> (tensor [B, C, X1, .., XD], min_coordinate, tensor_stride): the features at
        `(coordinate - min_coordinate) // tensor_stride` (no division with contract_stride=False), zeros elsewhere;
        gradients reach `self.F`.  `shape` (torch.Size; its channel count is corrected) and `min_coordinate` (an
        IntTensor divisible by the stride, possibly negative; 0 = the origin; None = the per-axis minimum, which must
        not be negative) default to the extent of the coordinates.  A coordinate outside the box raises IndexError, on
        either side (the reference's torch indexing wraps a negative index round to the far side).  HIP kernels
        (csrc/dense.hip); no CPU path."""
        from .ops import sparse_tensor_to_dense
        return sparse_tensor_to_dense(self, shape, min_coordinate, contract_stride)

    def sparse(self, min_coords=None, max_coords=None, contract_coords=True):
        """-> (torch sparse COO tensor [B, X1, .., XD, C], min_coords, tensor_stride); fp32 / float64 features.
        min_coords / max_coords: IntTensors of D values divisible by the stride (max inclusive; gives the size)."""
        D = self._D
        if min_coords is not None:
            assert isinstance(min_coords, torch.IntTensor)
            assert min_coords.numel() == D
        if max_coords is not None:
            assert isinstance(max_coords, torch.IntTensor)
            assert max_coords.numel() == D
        if self._F.dtype not in (torch.float32, torch.float64):
            raise ValueError("Feature type not supported.")
        tensor_stride = torch.IntTensor(self.tensor_stride)
        coords, batch_indices = self.C[:, 1:], self.C[:, :1]
        if min_coords is None:
            min_coords = coords.min(0, keepdim=True)[0].cpu()
        elif min_coords.ndim == 1:
            min_coords = min_coords.unsqueeze(0)
        assert (min_coords % tensor_stride).sum() == 0, "The minimum coordinates must be divisible by the tensor stride."
        if max_coords is not None:
            if max_coords.ndim == 1:
                max_coords = max_coords.unsqueeze(0)
            assert (max_coords % tensor_stride).sum() == 0, \
                "The maximum coordinates must be divisible by the tensor stride."
        coords = coords - min_coords.to(coords.device)
        if contract_coords:
            coords = torch.div(coords, tensor_stride.to(coords.device), rounding_mode="floor")
            if max_coords is not None:
                max_coords = torch.div(max_coords, tensor_stride, rounding_mode="floor")
            min_coords = torch.div(min_coords, tensor_stride, rounding_mode="floor")
        new_coords = torch.cat((batch_indices, coords), dim=1).long()
        size = None
        if max_coords is not None:
            extent = (max_coords - min_coords + 1).reshape(-1).tolist()      # inclusive
            size = torch.Size([int(batch_indices.max()) + 1, *[int(v) for v in extent], self._F.size(1)])
        if size is None:
            sparse_tensor = torch.sparse_coo_tensor(new_coords.t(), self._F)
        else:
            sparse_tensor = torch.sparse_coo_tensor(new_coords.t(), self._F, size)
        return sparse_tensor, min_coords, torch.IntTensor(self.tensor_stride)

    # ---- arithmetic between tensors: on a shared coordinate map, or on the union of two (MinkowskiTensor.py:390-546) -----
    def _binary(self, other, op):
        if isinstance(other, SparseTensor):
            assert other._manager is self._manager, "coordinate managers must match"
            if self.coordinate_map_key != other.coordinate_map_key:
                from .arithmetic import union_arithmetic      # the union of the two maps (csrc/union_arith.hip)
                return union_arithmetic(self, other, op)
            return SparseTensor(op(self._F, other._F), coordinate_map_key=self.coordinate_map_key,
                                coordinate_manager=self._manager)
        return SparseTensor(op(self._F, other), coordinate_map_key=self.coordinate_map_key,
                            coordinate_manager=self._manager)

    def __add__(self, other):
        return self._binary(other, torch.add)

    def __radd__(self, other):
        return self._binary(other, torch.add)

    def __iadd__(self, other):
        return self._binary(other, torch.add)

    def __sub__(self, other):
        return self._binary(other, torch.sub)

    def __mul__(self, other):
        return self._binary(other, torch.mul)

    def __truediv__(self, other):
        return self._binary(other, torch.div)

    def __neg__(self):
        return SparseTensor(-self._F, coordinate_map_key=self.coordinate_map_key, coordinate_manager=self._manager)

    # ---- back to the points (MinkowskiSparseTensor.py:541-720) ----------------------------------------------------------
    def interpolate(self, X):
        """Features at the points of the TensorField X: through the splat weights when this tensor is X.splat(),
        trilinear interpolation otherwise."""
        from .tensor_field import TensorField
        from .sparse_matrix_functions import MinkowskiSPMMFunction
        assert isinstance(X, TensorField)
        if self.coordinate_map_key in X._splat:
            tensor_map, field_map, weights, size = X._splat[self.coordinate_map_key]
            size = torch.Size([size[1], size[0]])
            features = MinkowskiSPMMFunction.apply(field_map, tensor_map, weights, size, self._F)
        else:
            features = self.features_at_coordinates(X.C)
        return X._like(features)

    def slice(self, X):
        """One row per ORIGINAL point of X (a TensorField, or the SparseTensor whose coordinates were quantised), in
        the original order: the features of the voxel each point fell in."""
        from .tensor_field import TensorField, _gather_rows
        if isinstance(X, TensorField):
            key = self.coordinate_map_key
            return X._like(_gather_rows(self._F, X.inverse_mapping(key), self._manager, lambda: X.voxel_csr(key)))
        if isinstance(X, SparseTensor):
            assert X.coordinate_map_key == self.coordinate_map_key, \
                "Slice can only be applied on the same coordinates (coordinate_map_key)"
            inv_map = X.inverse_mapping
            return TensorField(_gather_rows(self._F, inv_map, self._manager), coordinates=self.C[inv_map].float(),
                               coordinate_manager=self.coordinate_manager, quantization_mode=self.quantization_mode)
        raise ValueError("Invalid input. The input must be an instance of TensorField or SparseTensor.")

    def cat_slice(self, X):
        """slice(X) with X's own features concatenated after the sliced ones"""
        out = self.slice(X)
        xf = X.F if not isinstance(X, SparseTensor) else X.F[X.inverse_mapping]   # one row per point
        return out._like(torch.cat((out.F, xf), dim=1))

    def features_at_coordinates(self, query_coordinates):
        """Trilinear interpolation at continuous coordinates [N, D+1]; rows of queries without a present corner are
        zeros."""
        from .interpolation import MinkowskiInterpolationFunction
        assert query_coordinates.is_floating_point(), "query coordinates must be float32 or float64"
        assert query_coordinates.device == self.device, \
            f"query coordinates device ({query_coordinates.device}) does not match the sparse tensor device ({self.device})."
        return MinkowskiInterpolationFunction.apply(self._F, query_coordinates, self.coordinate_map_key,
                                                    self.coordinate_manager)[0]

    @property
    def _batchwise_row_indices(self):
        batch = self.C[:, 0]
        return [torch.nonzero(batch == b, as_tuple=False).flatten() for b in torch.unique(batch).tolist()]

    @property
    def decomposition_permutations(self):
        """per batch index, the rows of that batch: `decomposed_features[b] == F[decomposition_permutations[b]]`"""
        return self._batchwise_row_indices

    @property
    def decomposed_coordinates(self):
        return [self.C[idx, 1:] for idx in self._batchwise_row_indices]

    @property
    def decomposed_features(self):
        return [self._F[idx] for idx in self._batchwise_row_indices]

    @property
    def decomposed_coordinates_and_features(self):
        rows = self._batchwise_row_indices
        return [self.C[idx, 1:] for idx in rows], [self._F[idx] for idx in rows]

    def coordinates_at(self, batch_index):
        return self.C[self._batchwise_row_indices[batch_index], 1:]

    def features_at(self, batch_index):
        return self._F[self._batchwise_row_indices[batch_index]]

    def coordinates_and_features_at(self, batch_index):
        idx = self._batchwise_row_indices[batch_index]
        return self.C[idx, 1:], self._F[idx]

    def __repr__(self):
        return (f"{self.__class__.__name__}(\n  coordinates={self.C}\n  features={self._F}\n  "
                f"coordinate_map_key={self.coordinate_map_key}\n  coordinate_manager={self._manager}"
                f"  spatial dimension={self._D})")


def _get_coordinate_map_key(input, coordinates=None, tensor_stride=1, expand_coordinates=False):
    """Key of the output map of an operator (MinkowskiSparseTensor.py:754-783)."""
    if coordinates is not None and not expand_coordinates:
        assert isinstance(coordinates, (CoordinateMapKey, torch.Tensor, SparseTensor))
        if isinstance(coordinates, torch.Tensor):
            assert coordinates.ndim == 2
            key = _host.key_like(input._manager, convert_to_int_list(tensor_stride, coordinates.size(1) - 1), "")
            key, _ = input._manager.insert_and_map(coordinates, *key.get_key())
            return key
        if isinstance(coordinates, SparseTensor):
            return coordinates.coordinate_map_key
        return coordinates
    return _host.key_like(input.coordinate_map_key)
