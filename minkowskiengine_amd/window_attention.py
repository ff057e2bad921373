"""Shifted-window attention — the attention layer of SST, DSVT, Swin3D and Stratified Transformer: space is cut into
axis-aligned boxes of `window_size` cells of the tensor stride, every voxel attends to the voxels of its own box, and every
second block moves the grid by `shift` (usually `window_size // 2`) so that the borders move.  The window of the row
(b, c_0 .. c_{D-1}) on a map of tensor stride t is (b, cell_0 .. cell_{D-1}) with

    cell_a = floor((c_a / t_a + s_a) / w_a)

The floor goes towards -inf (negative coordinates are legal), the grid is anchored at the origin of the coordinate system
and not at the scene's bounding box, and shifts count modulo the window.  Nothing is padded; there is no cyclic wrap and no
mask: a window holds the voxels that fall into it, however few.

MinkowskiWindowAttentionFunction runs `WindowAttention{Forward,Backward}GPU` (both host layers): the kernels of
csrc/attention.hip on the window row lists and the block table of csrc/serial_attention.hip, which the coordinate manager
builds once per (map, window sizes, reduced shifts).  Building the lists reads the window count back once (4 bytes); the
attention calls read nothing back, so run one forward pass (or CoordinateManager.window_rows) BEFORE a graph capture.
Rows are summed in ascending order inside a window: the gradients are bitwise reproducible.
MinkowskiWindowSelfAttention has MinkowskiSelfAttention's (torch.nn.MultiheadAttention's) parameters and state dict.
MinkowskiFunctional.window_attention is the functional form.

Not covered: relative-position bias inside windows, a head size of 16, masks, dropout, cyclic wrap, tensor fields, queries
and keys on different maps, attention over user-supplied partitions."""
import math
import operator

import torch
from torch.autograd import Function

from .attention import MinkowskiSelfAttention
from .common import get_minkowski_function
from .sparse_tensor import SparseTensor


def _per_axis(name, value, dimension=None):
    """an int, or a tuple of one int per spatial axis (checked against `dimension` when that is known)"""
    try:
        if not hasattr(value, "__len__"):
            return operator.index(value)
        value = tuple(operator.index(v) for v in value)
    except TypeError:
        raise ValueError(f"{name} must be an int or one int per spatial axis, not {value!r}") from None
    if len(value) == 0 or (dimension is not None and len(value) != dimension):
        raise ValueError(f"{name} must be an int or one int per spatial axis"
                         + (f" ({dimension})" if dimension is not None else "") + f", not {value!r}")
    return value


def _check_window(window_size, shift, dimension=None):
    """-> (window_size, shift) as ints or tuples of ints; ValueError for a size below 1 or a wrong number of axes"""
    window_size, shift = _per_axis("window_size", window_size, dimension), _per_axis("shift", shift, dimension)
    if min(window_size if isinstance(window_size, tuple) else (window_size,)) < 1:
        raise ValueError(f"window_size must be at least 1, not {window_size}")
    if isinstance(window_size, tuple) and isinstance(shift, tuple) and len(window_size) != len(shift):
        raise ValueError(f"window_size {window_size} and shift {shift} must have one value per spatial axis each")
    return window_size, shift


class MinkowskiWindowAttentionFunction(Function):
    """out[i, h] = sum_j softmax_j(scale <q[i, h], k[j, h]>) v[j, h] over the rows j of the window of row i: the box of
    `window_size` cells of the tensor stride (an int or one int per spatial axis) on a grid moved by `shift` cells.  q, k,
    v: (N, H * d) features on the map `coords_key` (row views with a row stride are taken as they are); d must be 32, 64 or
    128 for fp32 and bf16 features, anything for float64; scale: None for 1 / sqrt(d)."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, window_size, shift, coords_key, coords_manager):
        window_size, shift = _check_window(window_size, shift, coords_manager.D)
        num_heads = int(num_heads)
        if num_heads <= 0 or q.shape[1] % num_heads != 0:
            raise ValueError(f"the channel count {q.shape[1]} must be a multiple of num_heads {num_heads}")
        d = q.shape[1] // num_heads
        if q.dtype != torch.float64 and d not in (32, 64, 128):
            raise ValueError(f"the head dimension must be 32, 64 or 128 for {q.dtype} features (any for float64), not {d}")
        scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
        q, k, v = q.detach(), k.detach(), v.detach()
        fw_fn = get_minkowski_function("WindowAttentionForward", q, coords_key)
        out, lse = fw_fn(q, k, v, num_heads, scale, window_size, shift, coords_key, coords_manager._manager)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.misc = (num_heads, scale, window_size, shift, coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        num_heads, scale, window_size, shift, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("WindowAttentionBackward", grad_out, coords_key)
        grad_q, grad_k, grad_v = bw_fn(q, k, v, out, lse, grad_out, num_heads, scale, window_size, shift, coords_key,
                                       coords_manager._manager, need_grad_q=ctx.needs_input_grad[0],
                                       need_grad_k=ctx.needs_input_grad[1], need_grad_v=ctx.needs_input_grad[2])
        return grad_q, grad_k, grad_v, None, None, None, None, None, None


class MinkowskiWindowSelfAttention(MinkowskiSelfAttention):
    r"""MinkowskiSelfAttention inside axis-aligned windows of `window_size` voxels per axis (an int or one int per spatial
    axis, in units of the tensor stride) on a grid anchored at the origin and moved by `shift` voxels, instead of inside
    whole instances.  Swin-style stages alternate `shift=0` and `shift=window_size // 2`.  The parameters and their
    initialisation are MinkowskiSelfAttention's (torch.nn.MultiheadAttention's), so state dicts load strictly in both
    directions.  `embed_dim / num_heads` must be 32, 64 or 128 (any size after `.double()`).  Sparse tensors only."""

    def __init__(self, embed_dim, num_heads, window_size=8, shift=0, bias=True, rope=False, rope_base=10000.0):
        window_size, shift = _check_window(window_size, shift)
        super().__init__(embed_dim, num_heads, bias=bias, rope=rope, rope_base=rope_base)
        self.window_size = window_size
        self.shift = shift

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, window_size={self.window_size}, "
                f"shift={self.shift}, bias={self.in_proj_bias is not None}" + self._rope_repr() + ")")

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        q, k, v = self._qkv(input)
        key = input.coordinate_map_key
        attn = MinkowskiWindowAttentionFunction.apply(q, k, v, self.num_heads, None, self.window_size, self.shift, key,
                                                      input._manager)
        out = torch.nn.functional.linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)
