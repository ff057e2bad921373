"""Multi-head self-attention inside every instance (batch index) of a sparse tensor — the attention layer of the coarse
levels of sparse diffusion and completion U-Nets, where a scene holds a few hundred to a few thousand voxels and every
voxel attends to the voxels of its own scene.

MinkowskiAttentionFunction runs `Attention{Forward,Backward}GPU` (both host layers) on the kernels of csrc/attention.hip:
rows in any order, instances of any sizes, no padding, no host loop, no read-back of sizes and no floating-point atomics
(the gradients are bitwise reproducible).  The rows of an instance are found through per-instance row lists that the
coordinate manager builds once per map.  MinkowskiSelfAttention is torch.nn.MultiheadAttention (batch_first, no mask, no
dropout) applied to the rows of each instance as one sequence, with that module's parameters and state dict; its two
projections are torch.nn.functional.linear, and q, k, v enter the kernels as the strided column views of the projected
matrix.  MinkowskiFunctional.scaled_dot_product_attention is the functional form, with queries and keys / values on
different maps of one manager."""
import math

import torch
from torch.autograd import Function
from torch.nn import Parameter

from . import host as _host
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .sparse_tensor import SparseTensor


class MinkowskiAttentionFunction(Function):
    """out[i, h] = sum_j softmax_j(scale <q[i, h], k[j, h]>) v[j, h] over the rows j of `kv_coords_key` with the batch
    index of row i of `q_coords_key`.  q: (Nq, H * d) features on the query map; k, v: (Nkv, H * d) on the key / value map
    of the same manager (it may be the same map); row views with a row stride are taken as they are.  d must be 32, 64 or
    128 for fp32 and bf16 features, anything for float64; scale: None for 1 / sqrt(d).  A query whose instance has no key
    row gives a zero row and zero gradients."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, q_coords_key, kv_coords_key, glob_coords_key=None, coords_manager=None):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(q_coords_key)
        num_heads = int(num_heads)
        if num_heads <= 0 or q.shape[1] % num_heads != 0:
            raise ValueError(f"the channel count {q.shape[1]} must be a multiple of num_heads {num_heads}")
        d = q.shape[1] // num_heads
        if q.dtype != torch.float64 and d not in (32, 64, 128):
            raise ValueError(f"the head dimension must be 32, 64 or 128 for {q.dtype} features (any for float64), not {d}")
        scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
        q, k, v = q.detach(), k.detach(), v.detach()
        fw_fn = get_minkowski_function("AttentionForward", q, q_coords_key)
        out, lse = fw_fn(q, k, v, num_heads, scale, q_coords_key, kv_coords_key, glob_coords_key, coords_manager._manager)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.misc = (num_heads, scale, q_coords_key, kv_coords_key, glob_coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        num_heads, scale, q_key, kv_key, glob_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("AttentionBackward", grad_out, q_key)
        grad_q, grad_k, grad_v = bw_fn(q, k, v, out, lse, grad_out, num_heads, scale, q_key, kv_key, glob_key,
                                       coords_manager._manager, need_grad_q=ctx.needs_input_grad[0],
                                       need_grad_k=ctx.needs_input_grad[1], need_grad_v=ctx.needs_input_grad[2])
        return grad_q, grad_k, grad_v, None, None, None, None, None, None


class MinkowskiSelfAttention(MinkowskiModuleBase):
    r"""torch.nn.MultiheadAttention(embed_dim, num_heads, bias=bias, batch_first=True) without mask and dropout, applied to
    the rows of every instance (batch index) of a sparse tensor as one sequence: every voxel attends to the voxels of its
    own scene.  The parameters are that module's — `in_proj_weight` (3C, C), `in_proj_bias` (3C,), `out_proj.weight`
    (C, C), `out_proj.bias` (C,), with the same initialisation — so state dicts load strictly in both directions.
    `embed_dim / num_heads` must be 32, 64 or 128 (any size after `.double()`); bf16 features run with bf16 parameters
    (`.bfloat16()`), float64 features need `.double()`.  Sparse tensors only."""

    def __init__(self, embed_dim, num_heads, bias=True):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0:
            raise ValueError("embed_dim and num_heads must be greater than 0")
        if embed_dim % num_heads != 0:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.in_proj_weight = Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = torch.nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            torch.nn.init.constant_(self.in_proj_bias, 0.0)
            torch.nn.init.constant_(self.out_proj.bias, 0.0)

    def __repr__(self):
        return self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, bias={self.in_proj_bias is not None})"

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        c = self.embed_dim
        qkv = torch.nn.functional.linear(input.F, self.in_proj_weight, self.in_proj_bias)
        key = input.coordinate_map_key
        attn = MinkowskiAttentionFunction.apply(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], self.num_heads, None, key, key,
                                                None, input._manager)
        out = torch.nn.functional.linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)
