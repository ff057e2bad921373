"""Serialized patch attention — the attention layer of Point Transformer v3, OctFormer and FlatFormer on the fine levels of
a sparse network: the voxels of every instance are ordered along a space-filling curve (z-order or Hilbert, optionally with
the first two axes exchanged), the sequence is cut into patches of at most `patch_size` voxels, and every voxel attends to
the voxels of its own patch.  The cost is N * patch_size instead of the N^2 of MinkowskiSelfAttention, on the same MFMA
kernels; changing the order from layer to layer moves the patch borders.

MinkowskiSerializedAttentionFunction runs `SerializedAttention{Forward,Backward}GPU` (both host layers): the kernels of
csrc/attention.hip on the patch row lists and the block table of csrc/serial_attention.hip, which the coordinate manager
builds once per (map, patch size, order) with no read-back on an inserted map.  Patch sizes of an instance differ by at
most one row; no row is borrowed from a neighbour, nothing is padded, and the gradients are bitwise reproducible.
MinkowskiSerializedSelfAttention has MinkowskiSelfAttention's (torch.nn.MultiheadAttention's) parameters and state dict.
MinkowskiFunctional.serialized_attention is the functional form."""
import math

import torch
from torch.autograd import Function

from .attention import MinkowskiSelfAttention
from .common import get_minkowski_function
from .sparse_tensor import SparseTensor

SERIAL_ORDERS = ("z", "z_trans", "hilbert", "hilbert_trans")


def _check_order(order, patch_size):
    if order not in SERIAL_ORDERS:
        raise ValueError(f"order must be one of {SERIAL_ORDERS}, not {order!r}")
    if int(patch_size) < 1:
        raise ValueError(f"patch_size must be at least 1, not {patch_size}")


class MinkowskiSerializedAttentionFunction(Function):
    """out[i, h] = sum_j softmax_j(scale <q[i, h], k[j, h]>) v[j, h] over the rows j of the patch of row i: the rows of an
    instance in the order `order` ("z", "z_trans", "hilbert", "hilbert_trans"), cut into ceil(n_b / patch_size) patches
    whose sizes differ by at most one.  q, k, v: (N, H * d) features on the map `coords_key` (row views with a row stride are
    taken as they are); d must be 32, 64 or 128 for fp32 and bf16 features, anything for float64; scale: None for
    1 / sqrt(d)."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, patch_size, order, coords_key, coords_manager):
        _check_order(order, patch_size)
        num_heads, patch_size = int(num_heads), int(patch_size)
        if num_heads <= 0 or q.shape[1] % num_heads != 0:
            raise ValueError(f"the channel count {q.shape[1]} must be a multiple of num_heads {num_heads}")
        d = q.shape[1] // num_heads
        if q.dtype != torch.float64 and d not in (32, 64, 128):
            raise ValueError(f"the head dimension must be 32, 64 or 128 for {q.dtype} features (any for float64), not {d}")
        scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
        q, k, v = q.detach(), k.detach(), v.detach()
        fw_fn = get_minkowski_function("SerializedAttentionForward", q, coords_key)
        out, lse = fw_fn(q, k, v, num_heads, scale, patch_size, order, coords_key, coords_manager._manager)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.misc = (num_heads, scale, patch_size, order, coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        num_heads, scale, patch_size, order, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("SerializedAttentionBackward", grad_out, coords_key)
        grad_q, grad_k, grad_v = bw_fn(q, k, v, out, lse, grad_out, num_heads, scale, patch_size, order, coords_key,
                                       coords_manager._manager, need_grad_q=ctx.needs_input_grad[0],
                                       need_grad_k=ctx.needs_input_grad[1], need_grad_v=ctx.needs_input_grad[2])
        return grad_q, grad_k, grad_v, None, None, None, None, None, None


class MinkowskiSerializedSelfAttention(MinkowskiSelfAttention):
    r"""MinkowskiSelfAttention inside patches of at most `patch_size` voxels along the space-filling curve `order` ("z",
    "z_trans", "hilbert" or "hilbert_trans") of every instance, instead of inside whole instances.  The parameters and their
    initialisation are MinkowskiSelfAttention's (torch.nn.MultiheadAttention's), so state dicts load strictly in both
    directions.  `embed_dim / num_heads` must be 32, 64 or 128 (any size after `.double()`).  Sparse tensors only."""

    def __init__(self, embed_dim, num_heads, patch_size=1024, order="z", bias=True, rope=False, rope_base=10000.0):
        _check_order(order, patch_size)
        super().__init__(embed_dim, num_heads, bias=bias, rope=rope, rope_base=rope_base)
        self.patch_size = int(patch_size)
        self.order = order

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, patch_size={self.patch_size}, "
                f"order={self.order!r}, bias={self.in_proj_bias is not None}" + self._rope_repr() + ")")

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        q, k, v = self._qkv(input)
        key = input.coordinate_map_key
        attn = MinkowskiSerializedAttentionFunction.apply(q, k, v, self.num_heads, None, self.patch_size, self.order, key,
                                                          input._manager)
        out = torch.nn.functional.linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)
