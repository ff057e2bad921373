"""Rotary position embedding (RoPE) from voxel coordinates — the positional signal of sparse generative transformers and
of the successors of Point Transformer V3: the channel pairs of the queries and keys of an attention layer are rotated by
angles taken from the coordinates of their voxel, after which the score <q_i, k_j> depends on c_i - c_j only.

x is (N, heads * d) on a coordinate map with D spatial axes, d even and P = d / 2 >= D.  Pairs are interleaved: pair p of a
head is its channels (2p, 2p + 1).  m = P // D frequencies per axis; pair p < D m belongs to axis a = p // m and frequency
j = p % m; the P - D m trailing pairs pass through.  With omega_j = base^(-j / m) and theta = (c_a / u_a) omega_j

    y[2p]     = x[2p] cos(theta) - x[2p + 1] sin(theta)
    y[2p + 1] = x[2p] sin(theta) + x[2p + 1] cos(theta)

u_a is the unit of axis a: the tensor stride of the map by default, `unit=` (an int or one int per axis, each >= 1)
otherwise; queries and keys on maps of different strides take one common unit.  The definition is fixed in include/me_amd.h.

MinkowskiRotaryEmbeddingFunction runs `RotaryEmbedding{Forward,Backward}GPU` (both host layers) on csrc/rope.hip: one pass
over the rows and a (cos, sin) table that the coordinate manager builds in double once per (map, d, base, unit, dtype).
The rotation is orthogonal, so the backward pass is the same launch with the angles negated.
MinkowskiRotaryEmbedding is the module, MinkowskiFunctional.rotary_embedding the functional form, and the self-attention
modules take `rope=True` (they rotate q and k of the projected matrix in one launch).

Not covered: the half-split ("rotate_half") pair convention, learned or per-axis frequency tables, tensor fields,
MinkowskiLocalSelfAttention (it has rel_pos_bias) and MinkowskiCrossAttention (its context has no coordinates)."""
import math
import operator

import torch
from torch.autograd import Function

from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .sparse_tensor import SparseTensor


def _check_rope(num_heads, base, unit, dimension=None):
    """-> (num_heads, base, unit) as an int, a float and None / an int / a tuple of ints; ValueError otherwise"""
    try:
        num_heads = operator.index(num_heads)
    except TypeError:
        raise ValueError(f"num_heads must be an int, not {num_heads!r}") from None
    if num_heads < 1:
        raise ValueError(f"num_heads must be at least 1, not {num_heads}")
    try:
        base = float(base)
    except (TypeError, ValueError):
        raise ValueError(f"base must be a number, not {base!r}") from None
    if not math.isfinite(base) or base <= 0.0:
        raise ValueError(f"base must be finite and greater than 0, not {base}")
    if unit is not None:
        try:
            unit = operator.index(unit) if not hasattr(unit, "__len__") else tuple(operator.index(u) for u in unit)
        except TypeError:
            raise ValueError(f"unit must be None, an int or one int per spatial axis, not {unit!r}") from None
        units = unit if isinstance(unit, tuple) else (unit,)
        if len(units) == 0 or (isinstance(unit, tuple) and dimension is not None and len(unit) != dimension):
            raise ValueError("unit must be None, an int or one int per spatial axis"
                             + (f" ({dimension})" if dimension is not None else "") + f", not {unit!r}")
        if min(units) < 1:
            raise ValueError(f"every unit must be at least 1, not {unit!r}")
    return num_heads, base, unit


def _check_head(channels, num_heads, dimension):
    """-> the head size d; ValueError unless `channels` splits into `num_heads` heads of an even d with d / 2 >= D"""
    if channels % num_heads != 0:
        raise ValueError(f"the channel count {channels} must be a multiple of num_heads {num_heads}")
    d = channels // num_heads
    if d % 2 != 0:
        raise ValueError(f"the head dimension must be even for rotary embedding, not {d}")
    if d // 2 < dimension:
        raise ValueError(f"the head dimension {d} must hold one channel pair per spatial axis ({dimension})")
    return d


class MinkowskiRotaryEmbeddingFunction(Function):
    """y = x with the channel pairs of each of its `num_heads` heads rotated by the angles of the row's coordinates on the
    map `coords_key`.  x: (N, heads * d) features (a row view with a row stride is taken as it is); the output is
    contiguous.  `unit`: None for the tensor stride of the map, an int or one int per spatial axis."""

    @staticmethod
    def forward(ctx, x, num_heads, base, unit, coords_key, coords_manager):
        num_heads, base, unit = _check_rope(num_heads, base, unit, coords_manager.D)
        _check_head(x.shape[1], num_heads, coords_manager.D)
        fw_fn = get_minkowski_function("RotaryEmbeddingForward", x, coords_key)
        ctx.misc = (num_heads, base, unit, coords_key, coords_manager)
        return fw_fn(x.detach(), num_heads, base, unit, coords_key, coords_manager._manager)

    @staticmethod
    def backward(ctx, grad_out):
        num_heads, base, unit, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("RotaryEmbeddingBackward", grad_out, coords_key)
        return bw_fn(grad_out, num_heads, base, unit, coords_key, coords_manager._manager), None, None, None, None, None


class MinkowskiRotaryEmbedding(MinkowskiModuleBase):
    r"""Rotates the channel pairs of every one of the `num_heads` heads of a sparse tensor by angles taken from the voxel
    coordinates (see the module docstring); no parameters.  `unit`: None for the tensor stride of the input, an int or one
    int per spatial axis.  Sparse tensors only."""

    def __init__(self, num_heads, base=10000.0, unit=None):
        super().__init__()
        self.num_heads, self.base, self.unit = _check_rope(num_heads, base, unit)

    def __repr__(self):
        return self.__class__.__name__ + f"(num_heads={self.num_heads}, base={self.base}, unit={self.unit})"

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        key = input.coordinate_map_key
        out = MinkowskiRotaryEmbeddingFunction.apply(input.F, self.num_heads, self.base, self.unit, key, input._manager)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)


def rotate_qk(qkv, embed_dim, num_heads, base, key, manager):
    """(q, k, v) of a projected matrix qkv (N, 3 C) with q and k rotated: ONE call on the view qkv[:, :2 C] with 2 H heads;
    q and k are the two strided halves of its result, v stays a view of qkv"""
    c = embed_dim
    qk = MinkowskiRotaryEmbeddingFunction.apply(qkv[:, :2 * c], 2 * num_heads, base, None, key, manager)
    return qk[:, :c], qk[:, c:], qkv[:, 2 * c:]
