"""KernelGenerator: kernel shape bookkeeping of a layer (reference:
MinkowskiEngine/MinkowskiKernelGenerator.py:245-345)."""
from functools import reduce

import torch

from .backend import RegionType, normalize_region_offsets
from .common import convert_to_int_list


def get_kernel_volume(region_type, kernel_size, region_offset, axis_types, dimension):
    """MinkowskiKernelGenerator.py:36-101 / src/kernel_region.hpp:250-270."""
    if region_type == RegionType.HYPER_CUBE:
        assert all(k > 0 for k in kernel_size), "kernel_size must be positive"
        return int(reduce(lambda a, b: a * b, kernel_size, 1))
    if region_type == RegionType.HYPER_CROSS:
        assert all(k > 0 for k in kernel_size), "kernel_size must be positive"
        assert all(k % 2 == 1 for k in kernel_size), "kernel_size must be odd for region_type HYPER_CROSS"
        return int(sum(k - 1 for k in kernel_size) + 1)
    if region_type == RegionType.CUSTOM:
        return int(normalize_region_offsets(region_offset, dimension).size(0))   # (raises ValueError when invalid)
    raise NotImplementedError()


def hybrid_region_offsets(axis_types, kernel_size, dimension):
    """-> IntTensor [K, D]: the offsets of a HYBRID kernel, for KernelGenerator(region_type=RegionType.CUSTOM,
    region_offsets=...): a hyper-cube over the axes whose type is RegionType.HYPER_CUBE and a hyper-cross over those
    whose type is RegionType.HYPER_CROSS (MinkowskiKernelGenerator.py's spatio-temporal kernel: a cube in space, a cross
    in time).  `axis_types` holds one RegionType per axis, `kernel_size` an int or one int per axis; odd sizes are
    centred, even sizes start at 0, as for the built-in regions.

    Row order (kernel[k] belongs to row k):
      1. the origin;
      2. the product of the HYPER_CUBE axes without the origin, the first cube axis fastest, all cross axes at 0;
      3. for every HYPER_CROSS axis in turn its off-centre taps — positive side first (1, 2, ..), then the negative side
         (-r, .., -1), the order of the built-in HYPER_CROSS — all other axes at 0.
    Sizes 3 over (cube, cube, cube, cross) give 1 + 26 + 2 = 29 rows; all-cube gives the hyper-cube's offsets with the
    origin moved to the front, all-cross the built-in cross in its own order."""
    axis_types = [RegionType(int(a)) for a in axis_types]
    kernel_size = convert_to_int_list(kernel_size, dimension)
    if len(axis_types) != dimension:
        raise ValueError(f"axis_types needs one RegionType per axis: got {len(axis_types)} for dimension {dimension}")
    if any(a == RegionType.CUSTOM for a in axis_types):
        raise ValueError("an axis of a hybrid kernel is HYPER_CUBE or HYPER_CROSS")
    if any(k < 1 for k in kernel_size):
        raise ValueError("kernel_size must be positive")
    taps = [list(range(k)) if k % 2 == 0 else list(range(-(k // 2), k // 2 + 1)) for k in kernel_size]
    cube = [d for d in range(dimension) if axis_types[d] == RegionType.HYPER_CUBE]
    rows = [[0] * dimension]
    total = reduce(lambda a, b: a * b, [len(taps[d]) for d in cube], 1)
    for i in range(total):
        row, rem = [0] * dimension, i
        for d in cube:
            row[d] = taps[d][rem % len(taps[d])]
            rem //= len(taps[d])
        if any(row):
            rows.append(row)
    for d in range(dimension):
        if axis_types[d] == RegionType.HYPER_CROSS:
            if kernel_size[d] % 2 == 0:
                raise ValueError("kernel_size must be odd on a HYPER_CROSS axis")
            r = kernel_size[d] // 2
            for v in list(range(1, r + 1)) + list(range(-r, 0)):
                row = [0] * dimension
                row[d] = v
                rows.append(row)
    return torch.IntTensor(rows)


class KernelGenerator:
    __slots__ = ("cache", "kernel_size", "kernel_stride", "kernel_dilation", "region_type", "region_offsets",
                 "axis_types", "dimension", "kernel_volume", "requires_strided_coordinates",
                 "expand_coordinates")

    def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False,
                 region_type=RegionType.HYPER_CUBE, region_offsets=None, expand_coordinates=False,
                 axis_types=None, dimension=-1):
        assert dimension > 0
        assert isinstance(region_type, RegionType)
        self.cache = {}
        self.kernel_size = convert_to_int_list(kernel_size, dimension)
        self.kernel_stride = convert_to_int_list(stride, dimension)
        self.kernel_dilation = convert_to_int_list(dilation, dimension)
        self.region_type = region_type
        # CUSTOM: a list, an ndarray or a tensor, normalised once to a contiguous CPU int32 [K, D] (kernel_size is then
        # not used: the default -1 is fine)
        self.region_offsets = (normalize_region_offsets(region_offsets, dimension)
                               if region_type == RegionType.CUSTOM else torch.IntTensor())
        self.axis_types = axis_types
        self.dimension = dimension
        self.kernel_volume = get_kernel_volume(region_type, self.kernel_size, self.region_offsets, axis_types,
                                               dimension)
        # NB the reference's name is a misnomer: it is True when ALL strides are 1
        # (MinkowskiKernelGenerator.py:307-309); kept for drop-in behaviour.
        self.requires_strided_coordinates = all(s == 1 for s in self.kernel_stride)
        self.expand_coordinates = expand_coordinates

    def __repr__(self):
        if self.region_type == RegionType.CUSTOM:
            return (f"{self.__class__.__name__}(region_type=RegionType.{self.region_type.name}, kernel_volume={self.kernel_volume}, "
                    f"kernel_stride={self.kernel_stride}, kernel_dilation={self.kernel_dilation}, "
                    f"expand_coordinates={self.expand_coordinates}, dimension={self.dimension})")
        return (f"{self.__class__.__name__}(kernel_size={self.kernel_size}, kernel_stride={self.kernel_stride}, "
                f"kernel_dilation={self.kernel_dilation}, region_type={self.region_type}, "
                f"expand_coordinates={self.expand_coordinates}, dimension={self.dimension})")
