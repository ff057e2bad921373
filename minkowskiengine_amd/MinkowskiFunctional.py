"""Functional twins of torch.nn.functional on sparse tensors and tensor fields (the reference's MinkowskiFunctional.py):
the torch function runs on the feature matrix `.F`.  Activations and the other feature-to-feature functions return a
tensor of the input's kind on the input's coordinates (a TensorField stays a TensorField); losses take a torch target
and return what torch returns.  No kernels of their own, except `group_norm` and `conditional_group_norm`:
torch's needs one dense tensor per sample, so they run MinkowskiGroupNorm's and MinkowskiConditionalGroupNorm's operators
(normalization.py, csrc/group_norm.hip); and `scaled_dot_product_attention`, which attends inside every instance on the
operators of attention.py (csrc/attention.hip); and `local_attention`, which attends inside a kernel region on the
operators of local_attention.py (csrc/local_attention.hip); and `serialized_attention`, which attends inside the patches
of a space-filling curve on the operators of serialized_attention.py (csrc/serial_attention.hip); and `cross_attention`,
which attends from the rows of a sparse tensor to a dense context (attention.py, csrc/attention.hip); and `layer_norm` /
`rms_norm`, which run MinkowskiLayerNorm's operators (normalization.py, csrc/layer_norm.hip); and `feed_forward`, the fused
two-layer MLP of MinkowskiFeedForward (feed_forward.py, csrc/feed_forward.hip), and `gated_feed_forward`, its gated form
(gated_feed_forward.py, csrc/gated_feed_forward.hip)."""
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


def layer_norm(input, weight=None, bias=None, eps=1e-5):
    """torch.nn.functional.layer_norm over the channel axis of the features of a SparseTensor or a TensorField
    (MinkowskiLayerNorm as a function).  weight / bias: (C,) tensors or None."""
    from .normalization import _row_norm
    return _row_norm(input, None, weight, bias, eps, False)


def rms_norm(input, weight=None, eps=None):
    """torch.nn.functional.rms_norm over the channel axis of the features of a SparseTensor or a TensorField
    (MinkowskiRMSNorm as a function).  weight: a (C,) tensor or None; eps=None: torch.finfo(features.dtype).eps."""
    from .normalization import _row_norm
    return _row_norm(input, None, weight, None, eps, True)


def ada_layer_norm(input, scale=None, shift=None, residual=None, gate=None, weight=None, bias=None, eps=1e-6, rms=False):
    """MinkowskiAdaLayerNorm as a function: norm(stream) * (1 + scale[b]) + shift[b] over the channel axis of a
    SparseTensor, stream = residual + gate[b] * input.  scale / shift / gate: (instances, C) tensors or None; weight /
    bias: (C,) tensors or None.  -> normed, or (normed, stream) with a residual."""
    from .normalization import _ada_row_norm
    return _ada_row_norm(input, residual, weight, bias, scale, shift, gate, eps, rms)


def selective_scan(u, delta, A, B, C, Dskip=None, z=None, delta_bias=None, delta_softplus=False, order="z", reverse=False):
    """The selective state-space scan (Mamba's S6; MinkowskiMamba without its projections) along the curve `order` of
    every instance.  u, delta, z: SparseTensors of D channels on ONE coordinate map (z may be None); B, C: (N, S) matrices
    or SparseTensors on that map; A (D, S), Dskip (D,), delta_bias (D,): float32 tensors.  The result sits on u's map."""
    from .selective_scan import selective_scan as _scan
    from .sparse_tensor import SparseTensor
    if not isinstance(u, SparseTensor):
        raise TypeError(f"selective_scan takes a SparseTensor u, not a {type(u).__name__}")
    for name, t in (("delta", delta), ("z", z), ("B", B), ("C", C)):
        if isinstance(t, SparseTensor) and (t.coordinate_map_key != u.coordinate_map_key or t._manager is not u._manager):
            raise ValueError(f"u, delta, z, B and C must share one coordinate map; {name} sits on another")
    feats = [t.F if isinstance(t, SparseTensor) else t for t in (delta, B, C, z)]
    out = _scan(u.F, feats[0], A, feats[1], feats[2], Dskip, feats[3], delta_bias, delta_softplus, order, reverse,
                u.coordinate_map_key, u._manager)
    return SparseTensor(out, coordinate_map_key=u.coordinate_map_key, coordinate_manager=u._manager)


def ssd_scan(x, dt, A, B, C, D=None, dt_bias=None, dt_softplus=False, headdim=64, ngroups=1, order="z", reverse=False):
    """Mamba-2's state-space-dual scan (MinkowskiMamba2 without its projections) along the curve `order` of every instance.
    x: a SparseTensor of H * headdim channels; dt (N, H), B, C (N, ngroups * S): matrices or SparseTensors on x's map;
    A, D, dt_bias: (H,) float32 tensors.  The result sits on x's map."""
    from .ssd_scan import ssd_scan as _scan
    from .sparse_tensor import SparseTensor
    if not isinstance(x, SparseTensor):
        raise TypeError(f"ssd_scan takes a SparseTensor x, not a {type(x).__name__}")
    for name, t in (("dt", dt), ("B", B), ("C", C)):
        if isinstance(t, SparseTensor) and (t.coordinate_map_key != x.coordinate_map_key or t._manager is not x._manager):
            raise ValueError(f"x, dt, B and C must share one coordinate map; {name} sits on another")
    feats = [t.F if isinstance(t, SparseTensor) else t for t in (dt, B, C)]
    out = _scan(x.F, feats[0], A, feats[1], feats[2], D, dt_bias, dt_softplus, headdim, ngroups, order, reverse,
                x.coordinate_map_key, x._manager)
    return SparseTensor(out, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x._manager)


def causal_conv1d(input, weight, bias=None, activation=None, order="z", reverse=False):
    """The causal depthwise conv1d along the curve `order` of every instance of a SparseTensor (MinkowskiMamba's local
    mixing as a function): weight (D, K) or (D, 1, K), bias (D,) or None, activation None or "silu".  Tap j reads the voxel
    j positions back in the instance's sequence and nothing before its start.  The result sits on the input's map."""
    from .causal_conv1d import causal_conv1d as _conv
    from .sparse_tensor import SparseTensor
    if not isinstance(input, SparseTensor):
        raise TypeError(f"causal_conv1d takes a SparseTensor, not a {type(input).__name__}")
    out = _conv(input.F, weight, bias, activation, order, reverse, input.coordinate_map_key, input._manager)
    return SparseTensor(out, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


def feed_forward(input, w1, b1, w2, b2, activation="gelu"):
    """act(F w1^T + b1) w2^T + b2 over the features F of a SparseTensor or a TensorField (MinkowskiFeedForward as a
    function).  w1 [hidden, C], w2 [C_out, hidden], b1 / b2 vectors or None; activation: gelu, gelu_tanh, relu or silu."""
    from .feed_forward import feed_forward as _feed_forward
    return _feed_forward(input, w1, b1, w2, b2, activation)


def gated_feed_forward(input, wg, bg, wu, bu, w2, b2, activation="silu"):
    """(act(F wg^T + bg) * (F wu^T + bu)) w2^T + b2 over the features F of a SparseTensor or a TensorField
    (MinkowskiGatedFeedForward as a function).  wg, wu [hidden, C], w2 [C_out, hidden], bg / bu / b2 vectors or None;
    activation: silu (SwiGLU), gelu or gelu_tanh (GeGLU), relu (ReGLU)."""
    from .gated_feed_forward import gated_feed_forward as _gated_feed_forward
    return _gated_feed_forward(input, wg, bg, wu, bu, w2, b2, activation)


__all__ = list(_FEATURE_FUNCTIONS + _LOSSES) + ["group_norm", "conditional_group_norm", "scaled_dot_product_attention",
                                                "local_attention", "serialized_attention", "cross_attention",
                                                "window_attention", "rotary_embedding", "layer_norm", "rms_norm",
                                                "ada_layer_norm", "feed_forward", "gated_feed_forward",
                                                "selective_scan", "causal_conv1d", "ssd_scan"]
