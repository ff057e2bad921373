"""Functional twins of torch.nn.functional on sparse tensors and tensor fields (the reference's MinkowskiFunctional.py):
the torch function runs on the feature matrix `.F`.  Activations and the other feature-to-feature functions return a
tensor of the input's kind on the input's coordinates (a TensorField stays a TensorField); losses take a torch target
and return what torch returns.  No kernels of their own, except `group_norm` and `conditional_group_norm`:
torch's needs one dense tensor per sample, so they run MinkowskiGroupNorm's and MinkowskiConditionalGroupNorm's operators
(normalization.py, csrc/group_norm.hip); and `scaled_dot_product_attention`, which attends inside every instance on the
operators of attention.py (csrc/attention.hip); and `local_attention`, which attends inside a kernel region on the
operators of local_attention.py (csrc/local_attention.hip); and `serialized_attention`, which attends inside the patches
of a space-filling curve on the operators of serialized_attention.py (csrc/serial_attention.hip); and `cross_attention`,
which attends from the rows of a sparse tensor to a dense context (attention.py, csrc/attention.hip)."""
import torch.nn.functional as F

from .layers import _rewrap

_FEATURE_FUNCTIONS = (
    "threshold", "relu", "hardtanh", "hardswish", "relu6", "elu", "selu", "celu", "leaky_relu", "prelu", "rrelu", "glu",
    "gelu", "logsigmoid", "hardshrink", "tanhshrink", "softsign", "softplus", "softmin", "softmax", "softshrink",
    "gumbel_softmax", "log_softmax", "tanh", "sigmoid", "hardsigmoid", "silu", "batch_norm", "normalize", "linear",
    "dropout", "alpha_dropout")
_LOSSES = (
    "binary_cross_entropy", "binary_cross_entropy_with_logits", "poisson_nll_loss", "cross_entropy",
    "hinge_embedding_loss", "kl_div", "l1_loss", "mse_loss", "multilabel_margin_loss", "multilabel_soft_margin_loss",
    "multi_margin_loss", "nll_loss", "smooth_l1_loss", "soft_margin_loss")


def _feature_function(name):
    fn = getattr(F, name)

    def wrapped(input, *args, **kwargs):
        return _rewrap(input, fn(input.F, *args, **kwargs))
    wrapped.__name__ = wrapped.__qualname__ = name
    wrapped.__doc__ = f"torch.nn.functional.{name} on the features, re-wrapped on the input's coordinates"
    return wrapped


def _loss(name):
    fn = getattr(F, name)

    def wrapped(input, target, *args, **kwargs):
        return fn(input.F, target, *args, **kwargs)
    wrapped.__name__ = wrapped.__qualname__ = name
    wrapped.__doc__ = f"torch.nn.functional.{name}(input.F, target, ...)"
    return wrapped


for _name in _FEATURE_FUNCTIONS:
    globals()[_name] = _feature_function(_name)
for _name in _LOSSES:
    globals()[_name] = _loss(_name)
del _name



def group_norm(input, num_groups, weight=None, bias=None, eps=1e-5):
    """torch.nn.functional.group_norm on every instance (batch index) of a sparse tensor on its own: the statistics of a
    group run over the rows of the instance and the channels of the group.  weight / bias: (C,) tensors of the parameter
    dtype (fp32 for fp32 and bf16 features, float64 for float64) or None."""
    from .normalization import MinkowskiGroupNormFunction
    from .sparse_tensor import SparseTensor
    assert isinstance(input, SparseTensor)
    out = MinkowskiGroupNormFunction.apply(input.F, num_groups, weight, bias, eps, input.coordinate_map_key, None,
                                           input._manager)
    return SparseTensor(out, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


def conditional_group_norm(input, num_groups, weight=None, bias=None, scale=None, shift=None, activation=None, eps=1e-5):
    """group_norm modulated per instance and followed by an optional SiLU: act(gn(x) * (1 + scale[b]) + shift[b]).
    scale / shift: (instances, C) tensors of the parameter dtype or None, row j for the j-th smallest batch index;
    activation: None or "silu" (MinkowskiConditionalGroupNorm's operators, csrc/group_norm.hip)."""
    from .normalization import MinkowskiConditionalGroupNormFunction
    from .sparse_tensor import SparseTensor
    assert isinstance(input, SparseTensor)
    out = MinkowskiConditionalGroupNormFunction.apply(input.F, num_groups, weight, bias, scale, shift, activation, eps,
                                                      input.coordinate_map_key, None, input._manager)
    return SparseTensor(out, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


def scaled_dot_product_attention(query, key, value, num_heads, scale=None):
    """torch.nn.functional.scaled_dot_product_attention inside every instance (batch index): a row of `query` attends to
    the rows of `key` / `value` with its own batch index.  `key` and `value` share a coordinate map of `query`'s manager
    (it may be `query`'s map); the channels split into `num_heads` heads of 32, 64 or 128 (any size in float64); scale
    defaults to 1 / sqrt(head size).  No mask, no dropout.  The result sits on `query`'s map."""
    from .attention import MinkowskiAttentionFunction
    from .sparse_tensor import SparseTensor
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, SparseTensor):
            raise TypeError(f"scaled_dot_product_attention takes SparseTensors; {name} is a {type(t).__name__}")
    if key.coordinate_map_key != value.coordinate_map_key or key._manager is not value._manager:
        raise ValueError("key and value must share a coordinate map")
    if key._manager is not query._manager:
        raise ValueError("query and key / value must belong to the same coordinate manager")
    out = MinkowskiAttentionFunction.apply(query.F, key.F, value.F, num_heads, scale, query.coordinate_map_key,
                                           key.coordinate_map_key, None, query._manager)
    return SparseTensor(out, coordinate_map_key=query.coordinate_map_key, coordinate_manager=query._manager)


def cross_attention(query, key, value, num_heads, context_lengths=None, scale=None):
    """Multi-head attention from the rows of the sparse tensor `query` to a dense context: `key` and `value` are
    (instances, tokens, channels) tensors with one row per instance (row j for the j-th smallest batch index) and the
    channels of `query`; context_lengths: None or one integer per instance, the tokens beyond it being masked.  The
    channels split into `num_heads` heads of 32, 64 or 128 (any size in float64); scale defaults to 1 / sqrt(head size).
    No dropout.  The result sits on `query`'s map."""
    import torch
    from .attention import MinkowskiCrossAttentionFunction
    from .sparse_tensor import SparseTensor
    if not isinstance(query, SparseTensor):
        raise TypeError(f"cross_attention takes a SparseTensor as the query, not a {type(query).__name__}")
    for name, t in (("key", key), ("value", value)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"cross_attention takes dense tensors as the context; {name} is a {type(t).__name__}")
    out = MinkowskiCrossAttentionFunction.apply(query.F, key, value, context_lengths, num_heads, scale,
                                                query.coordinate_map_key, query._manager)
    return SparseTensor(out, coordinate_map_key=query.coordinate_map_key, coordinate_manager=query._manager)


def local_attention(query, key, value, num_heads, kernel_size=3, dilation=1, kernel_generator=None, rel_pos_bias=None,
                    scale=None):
    """Multi-head attention of every row of `query` over the rows of `key` / `value` inside the kernel region around it
    (`kernel_size`, `dilation`, or a `kernel_generator`, which RegionType.CUSTOM needs).  `key` and `value` share a
    coordinate map of `query`'s manager; `query` may sit on that map or on a coarser one (attention pooling): the stride
    is the ratio of the tensor strides.  rel_pos_bias: (num_heads, kernel volume) or None.  The channels split into
    `num_heads` heads of 8, 16, 32, 64 or 128 (any size in float64); scale defaults to 1 / sqrt(head size).  No mask, no
    dropout.  The result sits on `query`'s map."""
    from .kernel_generator import KernelGenerator
    from .local_attention import MinkowskiLocalAttentionFunction
    from .sparse_tensor import SparseTensor
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, SparseTensor):
            raise TypeError(f"local_attention takes SparseTensors; {name} is a {type(t).__name__}")
    if key.coordinate_map_key != value.coordinate_map_key or key._manager is not value._manager:
        raise ValueError("key and value must share a coordinate map")
    if key._manager is not query._manager:
        raise ValueError("query and key / value must belong to the same coordinate manager")
    num_heads = int(num_heads)
    if num_heads <= 0 or query.F.shape[1] % num_heads != 0:
        raise ValueError(f"the channel count {query.F.shape[1]} must be a multiple of num_heads {num_heads}")
    if kernel_generator is None:
        ts_q, ts_kv = query.tensor_stride, key.tensor_stride
        if any(a % b != 0 for a, b in zip(ts_q, ts_kv)):
            raise ValueError(f"the tensor stride of query {ts_q} must be a multiple of that of key / value {ts_kv}")
        kernel_generator = KernelGenerator(kernel_size=kernel_size, stride=[a // b for a, b in zip(ts_q, ts_kv)],
                                           dilation=dilation, dimension=query.D)
    out = MinkowskiLocalAttentionFunction.apply(query.F, key.F, value.F, rel_pos_bias, num_heads, scale, kernel_generator,
                                                query.coordinate_map_key, key.coordinate_map_key, query._manager)
    return SparseTensor(out, coordinate_map_key=query.coordinate_map_key, coordinate_manager=query._manager)


def serialized_attention(query, key, value, num_heads, patch_size, order="z", scale=None):
    """Multi-head attention inside patches of at most `patch_size` rows along the space-filling curve `order` ("z",
    "z_trans", "hilbert", "hilbert_trans") of every instance (MinkowskiSerializedSelfAttention without its projections).
    `query`, `key` and `value` sit on ONE coordinate map; the channels split into `num_heads` heads of 32, 64 or 128 (any
    size in float64); scale defaults to 1 / sqrt(head size).  No mask, no dropout.  The result sits on that map."""
    from .serialized_attention import MinkowskiSerializedAttentionFunction
    from .sparse_tensor import SparseTensor
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, SparseTensor):
            raise TypeError(f"serialized_attention takes SparseTensors; {name} is a {type(t).__name__}")
    for name, t in (("key", key), ("value", value)):
        if t.coordinate_map_key != query.coordinate_map_key or t._manager is not query._manager:
            raise ValueError(f"query, key and value must share one coordinate map; {name} sits on another")
    out = MinkowskiSerializedAttentionFunction.apply(query.F, key.F, value.F, num_heads, scale, patch_size, order,
                                                     query.coordinate_map_key, query._manager)
    return SparseTensor(out, coordinate_map_key=query.coordinate_map_key, coordinate_manager=query._manager)


def window_attention(query, key, value, num_heads, window_size, shift=0, scale=None):
    """Multi-head attention inside axis-aligned windows of `window_size` voxels per axis (an int or one int per spatial axis,
    in units of the tensor stride) on a grid anchored at the origin and moved by `shift` voxels
    (MinkowskiWindowSelfAttention without its projections).  `query`, `key` and `value` sit on ONE coordinate map; the
    channels split into `num_heads` heads of 32, 64 or 128 (any size in float64); scale defaults to 1 / sqrt(head size).
    No mask, no dropout, no cyclic wrap.  The result sits on that map."""
    from .window_attention import MinkowskiWindowAttentionFunction
    from .sparse_tensor import SparseTensor
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, SparseTensor):
            raise TypeError(f"window_attention takes SparseTensors; {name} is a {type(t).__name__}")
    for name, t in (("key", key), ("value", value)):
        if t.coordinate_map_key != query.coordinate_map_key or t._manager is not query._manager:
            raise ValueError(f"query, key and value must share one coordinate map; {name} sits on another")
    out = MinkowskiWindowAttentionFunction.apply(query.F, key.F, value.F, num_heads, scale, window_size, shift,
                                                 query.coordinate_map_key, query._manager)
    return SparseTensor(out, coordinate_map_key=query.coordinate_map_key, coordinate_manager=query._manager)


def rotary_embedding(input, num_heads, base=10000.0, unit=None):
    """Rotary position embedding from the voxel coordinates (MinkowskiRotaryEmbedding as a function): the channel pairs
    (2p, 2p + 1) of each of the `num_heads` heads of `input` rotated by theta = (c_a / u_a) base^(-j / m), axis a = p // m,
    frequency j = p % m, m = (d / 2) // D; `unit` u: None for the tensor stride of `input`, an int or one int per spatial
    axis.  The result sits on the map of `input`."""
    from .rotary import MinkowskiRotaryEmbeddingFunction
    from .sparse_tensor import SparseTensor
    if not isinstance(input, SparseTensor):
        raise TypeError(f"rotary_embedding takes a SparseTensor, not a {type(input).__name__}")
    out = MinkowskiRotaryEmbeddingFunction.apply(input.F, num_heads, base, unit, input.coordinate_map_key, input._manager)
    return SparseTensor(out, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


__all__ = list(_FEATURE_FUNCTIONS + _LOSSES) + ["group_norm", "conditional_group_norm", "scaled_dot_product_attention",
                                                "local_attention", "serialized_attention", "cross_attention",
                                                "window_attention", "rotary_embedding"]
