"""Multi-head local attention over a kernel map: every voxel attends to the voxels inside a kernel region around it — the
attention of Fast Point Transformer, Stratified Transformer, Point Transformer v2 and neighbourhood-attention U-Nets.  Its
cost is N * K instead of the N^2 of MinkowskiSelfAttention (attention.py), so it is the layer of the fine levels.

MinkowskiLocalAttentionFunction runs `LocalAttention{Forward,Backward}GPU` (both host layers) on the kernels of
csrc/local_attention.hip: local pooling whose weights are a softmax of q.k, on the dense neighbour tables of the pooling
kernel map that the coordinate manager builds and caches.  Nothing of size [N, K, C] is materialised, there are no
floating-point atomics and the gradients (that of the bias included) are bitwise reproducible.  MinkowskiLocalSelfAttention
is the self-attention layer on one map with MinkowskiSelfAttention's parameters plus a learned scalar per head and kernel
offset (`rel_pos_bias`), without which the layer cannot tell neighbours apart by position.
MinkowskiFunctional.local_attention is the functional form; its query may sit on a coarser map (attention pooling)."""
import math

import torch
from torch.autograd import Function
from torch.nn import Parameter

from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .kernel_generator import KernelGenerator
from .sparse_tensor import SparseTensor


def check_head_dim(d, dtype):
    if dtype != torch.float64 and d not in (8, 16, 32, 64, 128):
        raise ValueError(f"the head dimension must be a power of two from 8 to 128 for {dtype} features "
                         f"(any for float64), not {d}")


class MinkowskiLocalAttentionFunction(Function):
    """out[i, h] = sum_k softmax_k(scale <q[i, h], k[j, h]> + rel_pos_bias[h, k]) v[j, h] over the offsets k of
    `kernel_generator` for which the kernel map `kv_coords_key` -> `q_coords_key` has a row j.  q: (N_out, H * d) features
    on the query map; k, v: (N_in, H * d) on the key / value map of the same manager (the same map, or a finer one whose
    stride the kernel generator carries); row views with a row stride are taken as they are.  rel_pos_bias: (H, K) or None.
    d must be a power of two from 8 to 128 for fp32 and bf16 features, anything for float64; scale: None for 1 / sqrt(d).
    A query without a neighbour gives a zero row and zero gradients."""

    @staticmethod
    def forward(ctx, q, k, v, rel_pos_bias, num_heads, scale, kernel_generator, q_coords_key, kv_coords_key,
                coords_manager):
        num_heads = int(num_heads)
        if num_heads <= 0 or q.shape[1] % num_heads != 0:
            raise ValueError(f"the channel count {q.shape[1]} must be a multiple of num_heads {num_heads}")
        d = q.shape[1] // num_heads
        check_head_dim(d, q.dtype)
        if rel_pos_bias is not None and tuple(rel_pos_bias.shape) != (num_heads, kernel_generator.kernel_volume):
            raise ValueError(f"rel_pos_bias must have the shape (num_heads, kernel volume) = "
                             f"{(num_heads, kernel_generator.kernel_volume)}, not {tuple(rel_pos_bias.shape)}")
        scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
        q, k, v = q.detach(), k.detach(), v.detach()
        bias = rel_pos_bias.detach() if rel_pos_bias is not None else None
        g = kernel_generator
        fw_fn = get_minkowski_function("LocalAttentionForward", q, q_coords_key)
        out, lse = fw_fn(q, k, v, bias, num_heads, scale, g.kernel_size, g.kernel_stride, g.kernel_dilation, g.region_type,
                         g.region_offsets, q_coords_key, kv_coords_key, coords_manager._manager)
        ctx.save_for_backward(q, k, v, out, lse, *(() if bias is None else (bias,)))
        ctx.misc = (num_heads, scale, g, q_coords_key, kv_coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse, *rest = ctx.saved_tensors
        bias = rest[0] if rest else None
        num_heads, scale, g, q_key, kv_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("LocalAttentionBackward", grad_out, q_key)
        grad_q, grad_k, grad_v, grad_bias = bw_fn(
            q, k, v, bias, out, lse, grad_out, num_heads, scale, g.kernel_size, g.kernel_stride, g.kernel_dilation,
            g.region_type, g.region_offsets, q_key, kv_key, coords_manager._manager,
            need_grad_q=ctx.needs_input_grad[0], need_grad_k=ctx.needs_input_grad[1], need_grad_v=ctx.needs_input_grad[2],
            need_grad_bias=bias is not None and ctx.needs_input_grad[3])
        if grad_bias is not None and grad_bias.dtype != bias.dtype:
            grad_bias = grad_bias.to(bias.dtype)
        return grad_q, grad_k, grad_v, grad_bias, None, None, None, None, None, None


class MinkowskiLocalSelfAttention(MinkowskiModuleBase):
    r"""Multi-head self-attention of every voxel over the voxels inside a kernel region around it, on one coordinate map
    (stride 1).  The parameters are MinkowskiSelfAttention's — `in_proj_weight` (3C, C), `in_proj_bias` (3C,),
    `out_proj.weight` (C, C), `out_proj.bias` (C,), with the same initialisation, so a checkpoint of the global layer loads
    with `strict=False` (`strict=True` when `rel_pos_bias=False`) — plus `rel_pos_bias` (H, K), one learned scalar per head
    and kernel offset, initialised to zero.  `embed_dim / num_heads` must be a power of two from 8 to 128 (any size after
    `.double()`); bf16 features run with bf16 parameters (`.bfloat16()`).  A `kernel_generator` replaces `kernel_size` and
    `dilation` (RegionType.CUSTOM lists go through it; its stride must be 1).  Sparse tensors only; no mask, no dropout."""

    def __init__(self, embed_dim, num_heads, kernel_size=3, dilation=1, bias=True, rel_pos_bias=True,
                 kernel_generator=None, dimension=None):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0:
            raise ValueError("embed_dim and num_heads must be greater than 0")
        if embed_dim % num_heads != 0:
            raise ValueError("embed_dim must be divisible by num_heads")
        if kernel_generator is None:
            assert dimension is not None and dimension > 0, f"Invalid dimension. Please provide a valid dimension argument. dimension={dimension}"
            kernel_generator = KernelGenerator(kernel_size=kernel_size, stride=1, dilation=dilation, dimension=dimension)
        elif dimension is not None:
            assert dimension == kernel_generator.dimension, "dimension does not match the kernel generator"
        if any(s != 1 for s in kernel_generator.kernel_stride):
            raise ValueError("MinkowskiLocalSelfAttention is self-attention on one map: the kernel stride must be 1 "
                             "(MinkowskiFunctional.local_attention takes a query on a coarser map)")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.kernel_generator = kernel_generator
        self.dimension = kernel_generator.dimension
        self.in_proj_weight = Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = torch.nn.Linear(embed_dim, embed_dim, bias=bias)
        if rel_pos_bias:
            self.rel_pos_bias = Parameter(torch.zeros(num_heads, kernel_generator.kernel_volume))
        else:
            self.register_parameter("rel_pos_bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            torch.nn.init.constant_(self.in_proj_bias, 0.0)
            torch.nn.init.constant_(self.out_proj.bias, 0.0)
        if self.rel_pos_bias is not None:
            torch.nn.init.constant_(self.rel_pos_bias, 0.0)

    def __repr__(self):
        g = self.kernel_generator
        region = (f"region_type={g.region_type}, kernel_volume={g.kernel_volume}" if g.region_offsets.numel()
                  else f"kernel_size={g.kernel_size}")
        return (self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, {region}, dilation={g.kernel_dilation}, "
                f"bias={self.in_proj_bias is not None}, rel_pos_bias={self.rel_pos_bias is not None})")

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        assert input.D == self.dimension, f"Dimension mismatch {self.dimension} != {input.D}"
        c = self.embed_dim
        qkv = torch.nn.functional.linear(input.F, self.in_proj_weight, self.in_proj_bias)
        key = input.coordinate_map_key
        attn = MinkowskiLocalAttentionFunction.apply(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], self.rel_pos_bias,
                                                     self.num_heads, None, self.kernel_generator, key, key, input._manager)
        out = torch.nn.functional.linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)
