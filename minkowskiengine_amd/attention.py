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
different maps of one manager.

MinkowskiCrossAttentionFunction and MinkowskiCrossAttention attend from the rows of a sparse tensor to a dense context
[B, L, C] — the text or image tokens of a conditional network — through `CrossAttention{Forward,Backward}GPU`: the same
kernels on the row lists of the context, with the dK / dV pass split over the queries where the context is short
(me_attn_kv_splits).  MinkowskiFunctional.cross_attention is the functional form."""
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
    (`.bfloat16()`), float64 features need `.double()`.  Sparse tensors only.
    `rope=True` rotates q and k by the rotary position embedding of the voxel coordinates (rotary.py; frequencies from
    `rope_base`, unit = the tensor stride of the input) before the scores are taken; it adds no parameter."""

    def __init__(self, embed_dim, num_heads, bias=True, rope=False, rope_base=10000.0):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0:
            raise ValueError("embed_dim and num_heads must be greater than 0")
        if embed_dim % num_heads != 0:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.rope = bool(rope)
        self.rope_base = float(rope_base)
        if self.rope:
            from .rotary import _check_rope
            _check_rope(num_heads, rope_base, None)
            if (embed_dim // num_heads) % 2 != 0:
                raise ValueError(f"the head dimension must be even for rope=True, not {embed_dim // num_heads}")
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

    def _rope_repr(self):
        """the tail of repr(): nothing unless rope is set"""
        if not self.rope:
            return ""
        return ", rope=True" + (f", rope_base={self.rope_base}" if self.rope_base != 10000.0 else "")

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, bias={self.in_proj_bias is not None}"
                + self._rope_repr() + ")")

    def _qkv(self, input):
        """(q, k, v) as column views of the projected matrix; with rope, q and k are the halves of ONE rotated [N, 2C]"""
        c = self.embed_dim
        qkv = torch.nn.functional.linear(input.F, self.in_proj_weight, self.in_proj_bias)
        if self.rope:
            from .rotary import rotate_qk
            return rotate_qk(qkv, c, self.num_heads, self.rope_base, input.coordinate_map_key, input._manager)
        return qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]

    def forward(self, input):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        q, k, v = self._qkv(input)
        key = input.coordinate_map_key
        attn = MinkowskiAttentionFunction.apply(q, k, v, self.num_heads, None, key, key, None, input._manager)
        out = torch.nn.functional.linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)


class MinkowskiCrossAttentionFunction(Function):
    """out[i, h] = sum_t softmax_t(scale <q[i, h], k[b, t, h]>) v[b, t, h] over the tokens t < context_lengths[b] of the
    context of the instance b of row i.  q: (Nq, H * d) features on `q_coords_key`; k, v: (B, L, H * d), B the number of
    instances of the manager; context row j belongs to the instance with the j-th smallest batch index (the rule of
    MinkowskiConditionalGroupNorm); views of one projection are taken as they are.  context_lengths: None (all L tokens)
    or B integers; tokens beyond a length are not read and get zero gradients, an instance of length 0 gives zero rows.
    d must be 32, 64 or 128 for fp32 and bf16 features, anything for float64; scale: None for 1 / sqrt(d).  kv_splits:
    None for the library's policy (or ME_AMD_ATTN_KV_SPLITS), else the query slices of the dK / dV pass."""

    @staticmethod
    def forward(ctx, q, k, v, context_lengths, num_heads, scale, q_coords_key, coords_manager, kv_splits=None):
        num_heads = int(num_heads)
        if k.dim() != 3 or v.dim() != 3 or k.shape[:2] != v.shape[:2]:
            raise ValueError(f"the context must be (instances, tokens, channels) for keys and values alike, got "
                             f"{tuple(k.shape)} and {tuple(v.shape)}")
        if k.dtype != q.dtype or v.dtype != q.dtype or k.device != q.device or v.device != q.device:
            raise ValueError(f"query and context must share dtype and device, got {q.dtype} on {q.device}, {k.dtype} on "
                             f"{k.device} and {v.dtype} on {v.device}")
        if num_heads <= 0 or q.shape[1] % num_heads != 0:
            raise ValueError(f"the channel count {q.shape[1]} must be a multiple of num_heads {num_heads}")
        if k.shape[2] != q.shape[1] or v.shape[2] != q.shape[1]:
            raise ValueError(f"keys and values must have the {q.shape[1]} channels of the queries, got {k.shape[2]} and "
                             f"{v.shape[2]}")
        d = q.shape[1] // num_heads
        if q.dtype != torch.float64 and d not in (32, 64, 128):
            raise ValueError(f"the head dimension must be 32, 64 or 128 for {q.dtype} features (any for float64), not {d}")
        instances = coords_manager.origin_map_size()
        if k.shape[0] != instances or k.shape[1] < 1:
            raise ValueError(f"the context must hold one row of at least one token per instance: {instances} instances, "
                             f"context {tuple(k.shape)}")
        if context_lengths is not None:
            context_lengths = torch.as_tensor(context_lengths)
            if context_lengths.dim() != 1 or context_lengths.numel() != instances or context_lengths.is_floating_point():
                raise ValueError(f"context_lengths must hold one integer per instance ({instances}), got "
                                 f"{tuple(context_lengths.shape)} {context_lengths.dtype}")
            context_lengths = context_lengths.to(device=q.device, dtype=torch.int32)
        scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
        q, k, v = q.detach(), k.detach(), v.detach()
        glob_coords_key = _host.key_like(q_coords_key)
        fw_fn = get_minkowski_function("CrossAttentionForward", q, q_coords_key)
        out, lse = fw_fn(q, k, v, context_lengths, num_heads, scale, q_coords_key, glob_coords_key, coords_manager._manager)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.misc = (context_lengths, num_heads, scale, q_coords_key, glob_coords_key, coords_manager, kv_splits)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        lengths, num_heads, scale, q_key, glob_key, coords_manager, kv_splits = ctx.misc
        bw_fn = get_minkowski_function("CrossAttentionBackward", grad_out, q_key)
        grad_q, grad_k, grad_v = bw_fn(q, k, v, lengths, out, lse, grad_out, num_heads, scale, q_key, glob_key,
                                       coords_manager._manager, need_grad_q=ctx.needs_input_grad[0],
                                       need_grad_k=ctx.needs_input_grad[1], need_grad_v=ctx.needs_input_grad[2],
                                       kv_splits=kv_splits)
        grad_k = grad_k.view(k.shape) if grad_k is not None else None
        grad_v = grad_v.view(v.shape) if grad_v is not None else None
        return grad_q, grad_k, grad_v, None, None, None, None, None, None


class MinkowskiCrossAttention(MinkowskiModuleBase):
    r"""torch.nn.MultiheadAttention(embed_dim, num_heads, kdim=kdim, vdim=vdim, bias=bias, batch_first=True) without
    dropout from the rows of a sparse tensor to a dense context: every voxel attends to the context tokens of its own
    instance.  `forward(input, context, context_lengths=None, value_context=None)`: context (B, L, kdim) with one row per
    instance — row j for the j-th smallest batch index, the rule of MinkowskiConditionalGroupNorm; context_lengths, B
    integers, plays the part of `key_padding_mask` for contexts padded to a common L (token t of instance b is masked
    when t >= context_lengths[b]); value_context (B, L, vdim) when the values come from other tokens than the keys.
    The parameters are torch's, with its initialisation — `in_proj_weight` (3C, C) when kdim == vdim == embed_dim, else
    `q_proj_weight` (C, C), `k_proj_weight` (C, kdim), `v_proj_weight` (C, vdim); `in_proj_bias` (3C,),
    `out_proj.weight`, `out_proj.bias` — so state dicts load strictly in both directions.  `embed_dim / num_heads` must
    be 32, 64 or 128 (any size after `.double()`).  No dropout, no mask but the lengths, sparse tensors only."""

    def __init__(self, embed_dim, num_heads, kdim=None, vdim=None, bias=True):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0:
            raise ValueError("embed_dim and num_heads must be greater than 0")
        if embed_dim % num_heads != 0:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.kdim = embed_dim if kdim is None else kdim
        self.vdim = embed_dim if vdim is None else vdim
        if self.kdim <= 0 or self.vdim <= 0:
            raise ValueError("kdim and vdim must be greater than 0")
        self._qkv_same_embed_dim = self.kdim == embed_dim and self.vdim == embed_dim
        if self._qkv_same_embed_dim:
            self.in_proj_weight = Parameter(torch.empty(3 * embed_dim, embed_dim))
            for name in ("q_proj_weight", "k_proj_weight", "v_proj_weight"):
                self.register_parameter(name, None)
        else:
            self.q_proj_weight = Parameter(torch.empty(embed_dim, embed_dim))
            self.k_proj_weight = Parameter(torch.empty(embed_dim, self.kdim))
            self.v_proj_weight = Parameter(torch.empty(embed_dim, self.vdim))
            self.register_parameter("in_proj_weight", None)
        if bias:
            self.in_proj_bias = Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = torch.nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        if self._qkv_same_embed_dim:
            torch.nn.init.xavier_uniform_(self.in_proj_weight)
        else:
            torch.nn.init.xavier_uniform_(self.q_proj_weight)
            torch.nn.init.xavier_uniform_(self.k_proj_weight)
            torch.nn.init.xavier_uniform_(self.v_proj_weight)
        if self.in_proj_bias is not None:
            torch.nn.init.constant_(self.in_proj_bias, 0.0)
            torch.nn.init.constant_(self.out_proj.bias, 0.0)

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.embed_dim}, {self.num_heads}, kdim={self.kdim}, vdim={self.vdim}, "
                f"bias={self.in_proj_bias is not None})")

    def forward(self, input, context, context_lengths=None, value_context=None):
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.embed_dim, f"Channel size mismatch {self.embed_dim} != {input.shape[1]}"
        values = context if value_context is None else value_context
        for name, t, dim in (("context", context, self.kdim), ("value_context", values, self.vdim)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != dim:
                raise ValueError(f"{name} must be a (instances, tokens, {dim}) tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        c, linear = self.embed_dim, torch.nn.functional.linear
        bq, bk, bv = (None,) * 3 if self.in_proj_bias is None else self.in_proj_bias.split(c)
        if self._qkv_same_embed_dim:
            wq, wk, wv = self.in_proj_weight.split(c)
        else:
            wq, wk, wv = self.q_proj_weight, self.k_proj_weight, self.v_proj_weight
        q = linear(input.F, wq, bq)
        if self._qkv_same_embed_dim and values is context:      # one projection of the context, k and v its column views
            kv = linear(context, self.in_proj_weight[c:], None if bk is None else self.in_proj_bias[c:])
            k, v = kv[..., :c], kv[..., c:]
        else:
            k, v = linear(context, wk, bk), linear(values, wv, bv)
        key = input.coordinate_map_key
        attn = MinkowskiCrossAttentionFunction.apply(q, k, v, context_lengths, self.num_heads, None, key, input._manager)
        out = linear(attn, self.out_proj.weight, self.out_proj.bias)
        return SparseTensor(out, coordinate_map_key=key, coordinate_manager=input._manager)
