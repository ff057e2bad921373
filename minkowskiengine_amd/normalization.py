"""Normalisations per instance of a sparse tensor: instance norm (the reference's) and group norm (torch.nn.GroupNorm's
arithmetic; the reference has none).

MinkowskiInstanceNorm, MinkowskiStableInstanceNorm and MinkowskiInstanceNormFunction (reference:
MinkowskiEngine/MinkowskiNormalization.py:194-399).  The reference normalises every instance (batch index) with a chain
of its global average pooling and broadcast operators plus torch element-wise ops; here one operator pair,
`InstanceNorm{Forward,Backward}GPU`, resolved in the backend by name as the other operators are, runs the kernels of
csrc/instance_norm.hip: per instance b and channel

    out[i] = (x[i] - mean[b_i]) / sqrt(var[b_i] + eps) * weight + bias        (var: biased)

in three passes over the feature matrix forward and five backward.

MinkowskiGroupNorm and MinkowskiGroupNormFunction run `GroupNorm{Forward,Backward}GPU` on csrc/group_norm.hip with the same
pass counts: per instance b and group g of C / num_groups consecutive channels

    out[i, c] = (x[i, c] - mean[b_i, g_c]) / sqrt(var[b_i, g_c] + eps) * weight[c] + bias[c]

with mean / var over the n_b rows of the instance and the channels of the group — torch.nn.functional.group_norm applied
to every instance's [1, C, n_b] tensor on its own.

MinkowskiConditionalGroupNorm and MinkowskiConditionalGroupNormFunction (AdaGN / FiLM) run
`ConditionalGroupNorm{Forward,Backward}GPU` on the k_gnc_* kernels of the same file, again with the same pass counts:

    out[i, c] = act(group_norm(x)[i, c] * (1 + scale[b_i, c]) + shift[b_i, c]),        act: identity or SiLU

with one row of scale / shift per instance.

The three fused Functions (`_InstanceNormAffineFunction`, `MinkowskiGroupNormFunction`,
`MinkowskiConditionalGroupNormFunction`) derive from `_SegNormFunction`, which holds what they share; a subclass only
says which operator pair it is and where its gradients go among its inputs.

MinkowskiLayerNorm, MinkowskiRMSNorm and MinkowskiLayerNormFunction normalise every ROW over its channels
(torch.nn.LayerNorm / torch.nn.RMSNorm on the feature matrix): no instance, no coordinate map.  One operator pair,
`LayerNorm{Forward,Backward}GPU` on csrc/layer_norm.hip, runs one pass forward and one pass plus a small merge backward,
and takes the residual add of a pre-norm block into the same launches (`forward_residual`).

MinkowskiAdaLayerNorm and MinkowskiAdaLayerNormFunction (adaLN, one half of a DiT block) add one row of scale / shift /
gate per instance to that: `stream = residual + gate[b] * input; normed = norm(stream) * (1 + scale[b]) + shift[b]` on
`AdaLayerNorm{Forward,Backward}GPU` (csrc/ada_layer_norm.hip), sparse tensors only."""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.nn import Parameter

from . import host as _host
from .backend import PoolingMode
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .layers import _rewrap
from .sparse_tensor import SparseTensor


_INSTANCE, _GROUP, _COND = "InstanceNorm", "GroupNorm", "ConditionalGroupNorm"     # <kind>{Forward,Backward}GPU


class _SegNormFunction(Function):
    """What the Functions of the three fused norms share: the preparation of the operands, what is kept for backward and
    the shapes of the parameter gradients.  The operators are called where `kind` is tested, with the arguments each of
    them takes, written out (a step of these layers is host-bound at small sizes: no argument lists are assembled here).
    num_groups is read by the two group norms; scale, shift and activation by the conditional one."""

    @staticmethod
    def _forward(ctx, kind, in_feat, num_groups, weight, bias, scale, shift, activation, eps, in_coords_key,
                 glob_coords_key, coords_manager):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(in_coords_key)
        in_feat = in_feat.contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        b = None if bias is None else bias.detach().reshape(-1).contiguous()
        w_shape, b_shape = None if weight is None else weight.shape, None if bias is None else bias.shape
        fw_fn = get_minkowski_function(kind + "Forward", in_feat, in_coords_key)
        manager = coords_manager._manager
        if kind is _INSTANCE:
            out, mean, rstd = fw_fn(in_feat, w, b, float(eps), in_coords_key, glob_coords_key, manager)
            ctx.save_for_backward(in_feat, w, mean, rstd)
            ctx.misc = (in_coords_key, glob_coords_key, coords_manager, w_shape, b_shape)
        elif kind is _GROUP:
            num_groups = int(num_groups)
            out, mean, rstd = fw_fn(in_feat, num_groups, w, b, float(eps), in_coords_key, glob_coords_key, manager)
            ctx.save_for_backward(in_feat, w, mean, rstd)
            ctx.misc = (num_groups, in_coords_key, glob_coords_key, coords_manager, w_shape, b_shape)
        else:
            num_groups = int(num_groups)
            sc = None if scale is None else scale.detach().contiguous()
            sh = None if shift is None else shift.detach().contiguous()
            out, mean, rstd = fw_fn(in_feat, num_groups, w, b, sc, sh, activation, float(eps), in_coords_key,
                                    glob_coords_key, manager)
            ctx.save_for_backward(in_feat, w, b, sc, sh, mean, rstd)
            ctx.misc = (num_groups, activation, in_coords_key, glob_coords_key, coords_manager, w_shape, b_shape)
        return out

    @staticmethod
    def _backward(ctx, kind, grad_out):
        """-> (grad_in, grad_weight, grad_bias) and, for the conditional norm, (grad_scale, grad_shift) after them; None
        where not needed"""
        need = ctx.needs_input_grad
        in_key, glob_key, coords_manager, w_shape, b_shape = ctx.misc[-5:]
        i = 1 if kind is _INSTANCE else 2                       # where weight stands among forward's inputs
        need_w, need_b = w_shape is not None and need[i], b_shape is not None and need[i + 1]
        bw_fn = get_minkowski_function(kind + "Backward", grad_out, in_key)
        grad_out, manager = grad_out.contiguous(), coords_manager._manager
        if kind is _COND:
            in_feat, w, b, sc, sh, mean, rstd = ctx.saved_tensors
            need_sc, need_sh = sc is not None and need[4], sh is not None and need[5]
            grad_in, grad_w, grad_b, grad_sc, grad_sh = bw_fn(
                in_feat, grad_out, ctx.misc[0], w, b, sc, sh, ctx.misc[1], mean, rstd, in_key, glob_key, manager,
                need_grad_in=need[0], need_grad_weight=need_w, need_grad_bias=need_b, need_grad_scale=need_sc,
                need_grad_shift=need_sh)
            return (grad_in, grad_w.view(w_shape) if need_w else None, grad_b.view(b_shape) if need_b else None,
                    grad_sc if need_sc else None, grad_sh if need_sh else None)
        in_feat, w, mean, rstd = ctx.saved_tensors
        if kind is _INSTANCE:
            grad_in, grad_w, grad_b = bw_fn(in_feat, grad_out, w, mean, rstd, in_key, glob_key, manager,
                                            need_grad_in=need[0], need_grad_weight=need_w, need_grad_bias=need_b)
        else:
            grad_in, grad_w, grad_b = bw_fn(in_feat, grad_out, ctx.misc[0], w, mean, rstd, in_key, glob_key, manager,
                                            need_grad_in=need[0], need_grad_weight=need_w, need_grad_bias=need_b)
        return grad_in, grad_w.view(w_shape) if need_w else None, grad_b.view(b_shape) if need_b else None


class _InstanceNormAffineFunction(_SegNormFunction):
    """The fused form the modules use: normalisation and affine map in one operator.  weight / bias: (1, C) or (C,)
    tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None."""

    @staticmethod
    def forward(ctx, in_feat, weight, bias, eps, in_coords_key, glob_coords_key, coords_manager):
        return _SegNormFunction._forward(ctx, _INSTANCE, in_feat, None, weight, bias, None, None, None, eps,
                                         in_coords_key, glob_coords_key, coords_manager)

    @staticmethod
    def backward(ctx, grad_out):
        return (*_SegNormFunction._backward(ctx, _INSTANCE, grad_out), None, None, None, None)


class MinkowskiInstanceNormFunction(Function):
    """The reference's Function (MinkowskiNormalization.py:194-310): the normalised features WITHOUT an affine map,
    eps = 1e-8.  `gpooling_mode` is accepted for compatibility; every global average mode computes the same mean."""

    @staticmethod
    def forward(ctx, in_feat, in_coords_key, glob_coords_key=None, coords_manager=None,
                gpooling_mode=PoolingMode.GLOBAL_AVG_POOLING_KERNEL):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(in_coords_key)
        in_feat = in_feat.contiguous()
        fw_fn = get_minkowski_function("InstanceNormForward", in_feat, in_coords_key)
        out, mean, rstd = fw_fn(in_feat, None, None, 1e-8, in_coords_key, glob_coords_key, coords_manager._manager)
        ctx.save_for_backward(in_feat, mean, rstd)
        ctx.saved_vars = (in_coords_key, glob_coords_key, coords_manager, gpooling_mode)
        return out

    @staticmethod
    def backward(ctx, out_grad):
        in_feat, mean, rstd = ctx.saved_tensors
        in_key, glob_key, coords_manager, _ = ctx.saved_vars
        bw_fn = get_minkowski_function("InstanceNormBackward", out_grad, in_key)
        grad_in, _, _ = bw_fn(in_feat, out_grad.contiguous(), None, mean, rstd, in_key, glob_key,
                              coords_manager._manager, need_grad_in=True, need_grad_weight=False, need_grad_bias=False)
        return grad_in, None, None, None, None


class _InstanceNormBase(MinkowskiModuleBase):
    eps = 1e-8

    def __init__(self, num_features):
        super().__init__()
        self.num_features = num_features
        self.weight = Parameter(torch.ones(1, num_features, dtype=torch.float32))
        self.bias = Parameter(torch.zeros(1, num_features, dtype=torch.float32))
        self.reset_parameters()

    def __repr__(self):
        return self.__class__.__name__ + f"(nchannels={self.num_features})"

    def reset_parameters(self):
        with torch.no_grad():
            self.weight.fill_(1)
            self.bias.zero_()

    def forward(self, input):
        assert isinstance(input, SparseTensor)
        assert input.shape[1] == self.num_features, f"Channel size mismatch {self.num_features} != {input.shape[1]}"
        output = _InstanceNormAffineFunction.apply(input.F, self.weight, self.bias, self.eps, input.coordinate_map_key,
                                                   None, input._manager)
        return SparseTensor(output, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


class MinkowskiInstanceNorm(_InstanceNormBase):
    r"""Instance normalisation of a sparse tensor: every batch index is normalised per channel with its own mean and
    biased variance (eps = 1e-8 inside the square root), then `* weight + bias` (MinkowskiNormalization.py:361-399).
    Parameters `weight`, `bias` of shape (1, num_features), fp32, as in the reference, so its state dicts load strictly.
    bf16 features run with the fp32 parameters and give bf16 outputs; float64 features need a `.double()` module."""

    def __init__(self, num_features):
        super().__init__(num_features)
        self.inst_norm = MinkowskiInstanceNormFunction       # (the reference keeps the Function as an attribute)


class MinkowskiStableInstanceNorm(_InstanceNormBase):
    r"""The formula MinkowskiNormalization.py:313-358 spells out — centre, biased variance, `1 / sqrt(var + 1e-6)`,
    affine — on the same kernels as MinkowskiInstanceNorm.  (The reference's forward reads `x.coords_key` /
    `x.coords_man`, attributes its 0.5.4 tensors no longer have; its five pooling / broadcast sub-modules have no
    parameters or buffers, so a reference state dict loads strictly without them.)"""
    eps = 1e-6

    def __init__(self, num_features):
        super().__init__(num_features)
        self.eps = 1e-6


class MinkowskiGroupNormFunction(_SegNormFunction):
    """Group normalisation of the feature rows of a coordinate map, every instance (batch index) on its own.  weight /
    bias: (C,) tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None."""

    @staticmethod
    def forward(ctx, in_feat, num_groups, weight, bias, eps, in_coords_key, glob_coords_key=None, coords_manager=None):
        return _SegNormFunction._forward(ctx, _GROUP, in_feat, num_groups, weight, bias, None, None, None, eps,
                                         in_coords_key, glob_coords_key, coords_manager)

    @staticmethod
    def backward(ctx, grad_out):
        grad_in, grad_w, grad_b = _SegNormFunction._backward(ctx, _GROUP, grad_out)
        return grad_in, None, grad_w, grad_b, None, None, None, None


class _GroupNormBase(MinkowskiModuleBase):
    """what MinkowskiGroupNorm and MinkowskiConditionalGroupNorm share: torch.nn.GroupNorm's arguments and parameters"""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True):
        super().__init__()
        if num_channels % num_groups != 0:
            raise ValueError("num_channels must be divisible by num_groups")
        self.num_groups = num_groups
        self.num_channels = num_channels
        self.eps = eps
        self.affine = affine
        if affine:
            self.weight = Parameter(torch.ones(num_channels, dtype=torch.float32))
            self.bias = Parameter(torch.zeros(num_channels, dtype=torch.float32))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.affine:
            with torch.no_grad():
                self.weight.fill_(1)
                self.bias.zero_()


class MinkowskiGroupNorm(_GroupNormBase):
    r"""torch.nn.GroupNorm for sparse tensors: every instance (batch index) is normalised per group of
    `num_channels / num_groups` consecutive channels with the mean and the biased variance over its rows and the
    channels of the group (eps inside the square root), then `* weight + bias` per channel.  `num_groups ==
    num_channels` is instance normalisation; `num_groups == 1` normalises over all channels and rows of an instance.
    Parameters `weight`, `bias` of shape (num_channels,), fp32, as torch.nn.GroupNorm's, so state dicts move between the
    two strictly; `affine=False` registers both as None.  bf16 features run with the fp32 parameters and give bf16
    outputs; float64 features need a `.double()` module."""

    def __repr__(self):
        return (self.__class__.__name__ +
                f"({self.num_groups}, {self.num_channels}, eps={self.eps}, affine={self.affine})")

    def forward(self, input):
        assert isinstance(input, SparseTensor)
        assert input.shape[1] == self.num_channels, f"Channel size mismatch {self.num_channels} != {input.shape[1]}"
        output = MinkowskiGroupNormFunction.apply(input.F, self.num_groups, self.weight, self.bias, self.eps,
                                                  input.coordinate_map_key, None, input._manager)
        return SparseTensor(output, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


class MinkowskiConditionalGroupNormFunction(_SegNormFunction):
    """Group normalisation of the feature rows of a coordinate map, every instance (batch index) on its own, modulated per
    instance and channel and followed by an optional SiLU: act(gn(x) * (1 + scale[b]) + shift[b]).  weight / bias: (C,)
    tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None; scale / shift:
    (instances, C) tensors of the parameter dtype or None, row j for row j of the origin map, that is for the j-th
    smallest batch index (the batch index itself when the indices are 0..B-1); activation: None or "silu"."""

    @staticmethod
    def forward(ctx, in_feat, num_groups, weight, bias, scale, shift, activation, eps, in_coords_key,
                glob_coords_key=None, coords_manager=None):
        return _SegNormFunction._forward(ctx, _COND, in_feat, num_groups, weight, bias, scale, shift, activation, eps,
                                         in_coords_key, glob_coords_key, coords_manager)

    @staticmethod
    def backward(ctx, grad_out):
        grad_in, grad_w, grad_b, grad_sc, grad_sh = _SegNormFunction._backward(ctx, _COND, grad_out)
        return grad_in, None, grad_w, grad_b, grad_sc, grad_sh, None, None, None, None, None


_GNC_ACTIVATIONS = (None, "silu")


class MinkowskiConditionalGroupNorm(_GroupNormBase):
    r"""MinkowskiGroupNorm modulated per instance (AdaGN / FiLM) with an optional fused SiLU, in the passes over the
    feature matrix of the plain layer:

        out = act(group_norm(x) * (1 + scale[b]) + shift[b])

    `forward(input, scale=None, shift=None)`: scale / shift of shape (instances, num_channels) hold one row per instance —
    row j belongs to row j of the origin map, that is to the j-th smallest batch index of the tensor; with batch indices
    0..B-1 it is the batch index itself.  They are converted to the parameter dtype with `.to()`, so their gradients
    flow back in the caller's dtype (for example to a bf16 `torch.nn.Linear` on a timestep embedding).  `activation`:
    None or "silu".  Parameters `weight`, `bias` of shape (num_channels,), fp32, as torch.nn.GroupNorm's, so state dicts
    move between the two strictly; `affine=False` registers both as None.  The gradients of scale and shift are
    fixed-order sums (no atomics), bitwise reproducible."""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True, activation=None):
        super().__init__(num_groups, num_channels, eps, affine)
        if activation not in _GNC_ACTIVATIONS:
            raise ValueError(f"activation must be None or 'silu', not {activation!r}")
        self.activation = activation

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.num_groups}, {self.num_channels}, eps={self.eps}, "
                f"affine={self.affine}, activation={self.activation!r})")

    def forward(self, input, scale=None, shift=None):
        assert isinstance(input, SparseTensor)
        assert input.shape[1] == self.num_channels, f"Channel size mismatch {self.num_channels} != {input.shape[1]}"
        pd = self.weight.dtype if self.affine else (torch.float64 if input.F.dtype == torch.float64 else torch.float32)
        scale = None if scale is None else scale.to(pd)
        shift = None if shift is None else shift.to(pd)
        output = MinkowskiConditionalGroupNormFunction.apply(
            input.F, self.num_groups, self.weight, self.bias, scale, shift, self.activation, self.eps,
            input.coordinate_map_key, None, input._manager)
        return SparseTensor(output, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input._manager)


_LNORM_MAX_C = 2048     # ME_LNORM_MAX_C: the widest fp32 / bf16 row of csrc/layer_norm.hip


class MinkowskiLayerNormFunction(Function):
    """Layer norm (rms=False) or RMS norm (rms=True) of the rows of a feature matrix over their channels, on
    `LayerNorm{Forward,Backward}GPU`.  weight / bias: (C,) tensors of the parameter dtype (fp32 for fp32 and bf16
    features, float64 for float64) or None.  With `residual` (same dtype and shape as in_feat) the Function returns
    (normed, stream): stream = residual + in_feat, normed = norm(stream), one launch per direction, bit-identical to the
    addition followed by the plain call; its one input gradient is returned for in_feat and for residual, without a copy.
    `owner`: a coordinate map key or manager of the call, which names the host layer that serves it."""

    @staticmethod
    def forward(ctx, in_feat, residual, weight, bias, eps, rms=False, owner=None):
        fw_fn = get_minkowski_function("LayerNormForward", in_feat, owner)
        w = None if weight is None else weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        out, stream, mean, rstd = fw_fn(in_feat, residual, w, b, float(eps), bool(rms))
        ctx.save_for_backward(in_feat if residual is None else stream, w, mean, rstd)
        ctx.misc = (bool(rms), owner, residual is not None, weight is not None, bias is not None)
        ctx.set_materialize_grads(False)
        return out if residual is None else (out, stream)

    @staticmethod
    def backward(ctx, grad_out, grad_stream=None):
        rms, owner, has_res, has_w, has_b = ctx.misc
        x, w, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_in, need_w, need_b = need[0] or (has_res and need[1]), has_w and need[2], has_b and need[3]
        if grad_out is None:                  # only the stream was used: the add alone
            return (grad_stream if need[0] else None, grad_stream if has_res and need[1] else None, None, None, None, None,
                    None)
        bw_fn = get_minkowski_function("LayerNormBackward", grad_out, owner)
        grad_in, grad_w, grad_b = bw_fn(x, grad_out, grad_stream, w, mean, rstd, rms, need_grad_in=need_in,
                                        need_grad_weight=need_w, need_grad_bias=need_b)
        return (grad_in if need[0] else None, grad_in if has_res and need[1] else None, grad_w, grad_b, None, None, None)


def _row_norm_key(input):
    """the key that names the host layer of a SparseTensor or a TensorField"""
    if isinstance(input, SparseTensor):
        return input.coordinate_map_key
    if hasattr(input, "coordinate_field_map_key"):
        return input.coordinate_field_map_key
    raise TypeError(f"a SparseTensor or a TensorField is expected, not a {type(input).__name__}")


def _row_norm(input, residual, weight, bias, eps, rms):
    """what the two modules and the two functionals run: features of `input` (plus those of `residual`) through the
    Function, or through torch for the shapes the kernels do not serve; re-wrapped as the kind of `input`"""
    key = _row_norm_key(input)
    f = input.F
    get_minkowski_function("LayerNormForward", f, key)              # (CPU features raise here, as everywhere)
    pd = torch.float64 if f.dtype == torch.float64 else torch.float32
    weight = weight if weight is None or weight.dtype == pd else weight.to(pd)
    bias = bias if bias is None or bias.dtype == pd else bias.to(pd)
    if eps is None:
        eps = torch.finfo(f.dtype).eps
    r = None
    if residual is not None:
        assert key == _row_norm_key(residual), "residual add needs a shared coordinate map"
        r = residual.F
        assert r.dtype == f.dtype and r.shape == f.shape, "input and residual must share dtype and shape"
    if f.dim() != 2 or (f.dtype != torch.float64 and f.shape[1] > _LNORM_MAX_C):
        stream = f if r is None else r + f
        shape, w, b = (f.shape[-1],), None if weight is None else weight.to(f.dtype), None if bias is None else bias.to(f.dtype)
        y = F.rms_norm(stream, shape, w, eps) if rms else F.layer_norm(stream, shape, w, b, eps)
        return _rewrap(input, y) if r is None else (_rewrap(input, y), _rewrap(input, stream))
    out = MinkowskiLayerNormFunction.apply(f, r, weight, bias, eps, rms, key)
    return _rewrap(input, out) if r is None else (_rewrap(input, out[0]), _rewrap(input, out[1]))


class _RowNormBase(MinkowskiModuleBase):
    """what MinkowskiLayerNorm and MinkowskiRMSNorm share: the normalised shape, forward and forward_residual"""
    _RMS = False

    def _set_shape(self, normalized_shape):
        shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
        if len(shape) != 1 or int(shape[0]) < 1:
            raise ValueError(f"normalized_shape must be an int or a 1-tuple (the channel axis), got {normalized_shape!r}")
        self.normalized_shape = (int(shape[0]),)

    def _check(self, input):
        _row_norm_key(input)
        assert input.F.shape[-1] == self.normalized_shape[0], \
            f"Channel size mismatch {self.normalized_shape[0]} != {input.F.shape[-1]}"

    def forward(self, input):
        self._check(input)
        return _row_norm(input, None, self.weight, getattr(self, "bias", None), self.eps, self._RMS)

    def forward_residual(self, input, residual):
        """-> (normed, stream): stream = residual + input, normed = self(stream) — the tail of one half of a pre-norm
        block and the head of the next, in one launch per direction, bit-identical to `stream = residual + input;
        normed = self(stream)`.  Both inputs share a coordinate map key, dtype and shape."""
        self._check(input)
        return _row_norm(input, residual, self.weight, getattr(self, "bias", None), self.eps, self._RMS)


class MinkowskiLayerNorm(_RowNormBase):
    r"""torch.nn.LayerNorm over the channel axis of the feature matrix of a SparseTensor or a TensorField (the same kind
    comes back): per row `(x - mean) / sqrt(var + eps) * weight + bias` with the biased variance over the channels.
    `normalized_shape`: an int or a 1-tuple.  Parameters `weight`, `bias` of shape (C,), initialised and named as
    torch.nn.LayerNorm's, so state dicts move between the two strictly (`bias=False`, `elementwise_affine=False`
    included).  They stay fp32 for fp32 and bf16 features (bf16 rows are normalised in fp32 and rounded once) and become
    float64 after `.double()`.  The parameter gradients are fixed-order sums, bitwise reproducible.  Fallback: rows wider
    than 2048 channels in fp32 / bf16, and features that are not 2-D, go to torch.nn.functional.layer_norm."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, bias=True):
        super().__init__()
        self._set_shape(normalized_shape)
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        if elementwise_affine:
            self.weight = Parameter(torch.ones(self.normalized_shape, dtype=torch.float32))
            if bias:
                self.bias = Parameter(torch.zeros(self.normalized_shape, dtype=torch.float32))
            else:
                self.register_parameter("bias", None)
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.normalized_shape[0]}, eps={self.eps}, "
                f"elementwise_affine={self.elementwise_affine}, bias={self.bias is not None})")


class MinkowskiRMSNorm(_RowNormBase):
    r"""torch.nn.RMSNorm over the channel axis of the feature matrix of a SparseTensor or a TensorField: per row
    `x / sqrt(mean(x^2) + eps) * weight`.  `eps=None` means torch.finfo(features.dtype).eps, as in torch.  Parameter
    `weight` of shape (C,), named as torch.nn.RMSNorm's; dtypes, gradients and fallback (to
    torch.nn.functional.rms_norm) as MinkowskiLayerNorm."""
    _RMS = True

    def __init__(self, normalized_shape, eps=None, elementwise_affine=True):
        super().__init__()
        self._set_shape(normalized_shape)
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        if elementwise_affine:
            self.weight = Parameter(torch.ones(self.normalized_shape, dtype=torch.float32))
        else:
            self.register_parameter("weight", None)

    def __repr__(self):
        return (self.__class__.__name__ +
                f"({self.normalized_shape[0]}, eps={self.eps}, elementwise_affine={self.elementwise_affine})")


class MinkowskiAdaLayerNormFunction(Function):
    """Layer norm (rms=False) or RMS norm (rms=True) of the rows of a coordinate map, modulated per instance, with a gated
    residual add, on `AdaLayerNorm{Forward,Backward}GPU`:

        stream = residual + gate[b] * in_feat            (without a residual: stream = in_feat, gate must be None)
        normed = norm(stream) * (1 + scale[b]) + shift[b]

    b: the row of the origin map of every row (the j-th smallest batch index).  weight / bias: (C,) tensors of the
    parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None; scale / shift / gate: (instances, C)
    tensors of the parameter dtype or None (0 / 0 / 1).  Returns normed, or (normed, stream) with a residual.  One launch
    forward; one launch plus two small merges backward; every gradient is a fixed-order sum, bitwise reproducible."""

    @staticmethod
    def forward(ctx, in_feat, residual, weight, bias, scale, shift, gate, eps, rms, in_coords_key, coords_manager):
        fw_fn = get_minkowski_function("AdaLayerNormForward", in_feat, in_coords_key)
        w, b, sc, sh, gt = (None if t is None else t.detach().contiguous() for t in (weight, bias, scale, shift, gate))
        out, stream, mean, rstd = fw_fn(in_feat, residual, w, b, sc, sh, gt, float(eps), bool(rms), in_coords_key,
                                        coords_manager._manager)
        ctx.save_for_backward(in_feat if residual is None else stream, None if gt is None else in_feat, w, b, sc, gt, mean,
                              rstd)
        ctx.misc = (bool(rms), in_coords_key, coords_manager, residual is not None, sh is not None)
        ctx.set_materialize_grads(False)
        return out if residual is None else (out, stream)

    @staticmethod
    def backward(ctx, grad_out, grad_stream=None):
        rms, in_key, coords_manager, has_res, has_sh = ctx.misc
        x, xin, w, b, sc, gt, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        tail = (None, None, None, None)
        if grad_out is None and (grad_stream is None or gt is None):          # nothing, or the add alone
            return (grad_stream if need[0] else None, grad_stream if has_res and need[1] else None, None, None, None, None,
                    None) + tail
        bw_fn = get_minkowski_function("AdaLayerNormBackward", x, in_key)
        grads = bw_fn(x, grad_out, grad_stream, xin, w, b, sc, gt, mean, rstd, rms, in_key, coords_manager._manager,
                      need_grad_in=need[0], need_grad_residual=has_res and need[1], need_grad_weight=w is not None and need[2],
                      need_grad_bias=b is not None and need[3], need_grad_scale=sc is not None and need[4],
                      need_grad_shift=has_sh and need[5], need_grad_gate=gt is not None and need[6])
        return tuple(grads) + tail


def _ada_modulation(name, t, instances, c, pd):
    """scale / shift / gate as the operators take them: (instances, C) in the parameter dtype"""
    if t is None:
        return None
    if t.dim() != 2 or t.shape[0] != instances:
        raise ValueError(f"{name} must have one row per instance: ({instances}, {c}), got {tuple(t.shape)}")
    if t.shape[1] != c:
        raise ValueError(f"{name} must have {c} channels, got {tuple(t.shape)}")
    return t.to(pd)


def _ada_row_norm(input, residual, weight, bias, scale, shift, gate, eps, rms):
    """what MinkowskiAdaLayerNorm and the functional run: the Function, or torch for the shapes the kernels do not serve"""
    if not isinstance(input, SparseTensor):
        raise TypeError(f"a SparseTensor is expected, not a {type(input).__name__}")
    key, f = input.coordinate_map_key, input.F
    get_minkowski_function("AdaLayerNormForward", f, key)              # (CPU features raise here, as everywhere)
    pd = torch.float64 if f.dtype == torch.float64 else torch.float32
    weight = weight if weight is None or weight.dtype == pd else weight.to(pd)
    bias = bias if bias is None or bias.dtype == pd else bias.to(pd)
    instances, c = input._manager.origin_map_size(), f.shape[-1]
    scale, shift, gate = (_ada_modulation(name, t, instances, c, pd)
                          for name, t in (("scale", scale), ("shift", shift), ("gate", gate)))
    r = None
    if residual is not None:
        if not isinstance(residual, SparseTensor):
            raise TypeError(f"a SparseTensor is expected, not a {type(residual).__name__}")
        assert key == residual.coordinate_map_key, "residual add needs a shared coordinate map"
        r = residual.F
        assert r.dtype == f.dtype and r.shape == f.shape, "input and residual must share dtype and shape"
    elif gate is not None:
        raise ValueError("a gate needs a residual")
    if f.dim() != 2 or (f.dtype != torch.float64 and c > _LNORM_MAX_C):
        rows = input._manager._manager._origin_rows(key).long()
        stream = f if r is None else (r + f if gate is None else r + gate.to(f.dtype)[rows] * f)
        w, b = None if weight is None else weight.to(f.dtype), None if bias is None else bias.to(f.dtype)
        y = F.rms_norm(stream, (c,), w, eps) if rms else F.layer_norm(stream, (c,), w, b, eps)
        if rms and b is not None:
            y = y + b
        if scale is not None:
            y = y * (1 + scale.to(f.dtype)[rows])
        if shift is not None:
            y = y + shift.to(f.dtype)[rows]
        return _rewrap(input, y) if r is None else (_rewrap(input, y), _rewrap(input, stream))
    out = MinkowskiAdaLayerNormFunction.apply(f, r, weight, bias, scale, shift, gate, eps, rms, key, input._manager)
    return _rewrap(input, out) if r is None else (_rewrap(input, out[0]), _rewrap(input, out[1]))


class MinkowskiAdaLayerNorm(_RowNormBase):
    r"""Adaptive layer norm (adaLN, one half of a DiT block) over the channel axis of a SparseTensor:

        stream = residual + gate[b] * input,    normed = norm(stream) * (1 + scale[b]) + shift[b]

    with one row of scale / shift / gate per instance — row j belongs to row j of the origin map, that is to the j-th
    smallest batch index of the tensor — in one launch forward and one pass plus two small merges backward.
    `forward(input, scale=None, shift=None)` returns normed; `forward_residual(input, residual, scale=None, shift=None,
    gate=None)` returns (normed, stream).  Absent operands mean 0 / 0 / 1 and are not read; with all three absent the
    layer equals MinkowskiLayerNorm (MinkowskiRMSNorm with `rms=True`) bit for bit.  scale / shift / gate are converted
    to the parameter dtype with `.to()`, so their gradients flow back in the caller's dtype; a row count other than the
    number of instances or a channel count other than C raises ValueError.  `elementwise_affine` defaults to False and
    eps to 1e-6, as DiT's norms; `weight` / `bias` are named as torch.nn.LayerNorm's (RMSNorm's with `rms=True`: no bias),
    so a checkpoint of MinkowskiLayerNorm loads strictly.  All gradients are fixed-order sums, bitwise reproducible.
    Sparse tensors only (a TensorField raises TypeError).  Fallback to torch: fp32 / bf16 rows wider than 2048 channels
    and features that are not 2-D."""

    def __init__(self, normalized_shape, eps=1e-6, elementwise_affine=False, bias=True, rms=False):
        super().__init__()
        self._set_shape(normalized_shape)
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        self.rms = self._RMS = bool(rms)
        if elementwise_affine:
            self.weight = Parameter(torch.ones(self.normalized_shape, dtype=torch.float32))
        else:
            self.register_parameter("weight", None)
        if not rms:
            if elementwise_affine and bias:
                self.bias = Parameter(torch.zeros(self.normalized_shape, dtype=torch.float32))
            else:
                self.register_parameter("bias", None)

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.normalized_shape[0]}, eps={self.eps}, "
                f"elementwise_affine={self.elementwise_affine}, bias={getattr(self, 'bias', None) is not None}, "
                f"rms={self.rms})")

    def forward(self, input, scale=None, shift=None):
        return self.forward_residual(input, None, scale, shift)

    def forward_residual(self, input, residual, scale=None, shift=None, gate=None):
        """-> (normed, stream) (normed alone with residual=None): stream = residual + gate[b] * input, normed = the
        modulated norm of stream — the gated tail of one half of a DiT block and the head of the next."""
        if not isinstance(input, SparseTensor):
            raise TypeError(f"a SparseTensor is expected, not a {type(input).__name__}")
        self._check(input)
        return _ada_row_norm(input, residual, self.weight, getattr(self, "bias", None), scale, shift, gate, self.eps,
                             self.rms)
