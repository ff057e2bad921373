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

with one row of scale / shift per instance."""
import torch
from torch.autograd import Function
from torch.nn import Parameter

from . import host as _host
from .backend import PoolingMode
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .sparse_tensor import SparseTensor


class _InstanceNormAffineFunction(Function):
    """The fused form the modules use: normalisation and affine map in one operator.  weight / bias: (1, C) or (C,)
    tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None."""

    @staticmethod
    def forward(ctx, in_feat, weight, bias, eps, in_coords_key, glob_coords_key, coords_manager):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(in_coords_key)
        in_feat = in_feat.contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        b = None if bias is None else bias.detach().reshape(-1).contiguous()
        fw_fn = get_minkowski_function("InstanceNormForward", in_feat, in_coords_key)
        out, mean, rstd = fw_fn(in_feat, w, b, float(eps), in_coords_key, glob_coords_key, coords_manager._manager)
        ctx.save_for_backward(in_feat, w, mean, rstd)
        ctx.misc = (in_coords_key, glob_coords_key, coords_manager,
                    None if weight is None else weight.shape, None if bias is None else bias.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        in_feat, w, mean, rstd = ctx.saved_tensors
        in_key, glob_key, coords_manager, w_shape, b_shape = ctx.misc
        need_w = w_shape is not None and ctx.needs_input_grad[1]
        need_b = b_shape is not None and ctx.needs_input_grad[2]
        bw_fn = get_minkowski_function("InstanceNormBackward", grad_out, in_key)
        grad_in, grad_w, grad_b = bw_fn(in_feat, grad_out.contiguous(), w, mean, rstd, in_key, glob_key,
                                        coords_manager._manager, need_grad_in=ctx.needs_input_grad[0],
                                        need_grad_weight=need_w, need_grad_bias=need_b)
        return (grad_in, grad_w.view(w_shape) if need_w else None, grad_b.view(b_shape) if need_b else None,
                None, None, None, None)


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


class MinkowskiGroupNormFunction(Function):
    """Group normalisation of the feature rows of a coordinate map, every instance (batch index) on its own.  weight /
    bias: (C,) tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None."""

    @staticmethod
    def forward(ctx, in_feat, num_groups, weight, bias, eps, in_coords_key, glob_coords_key=None, coords_manager=None):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(in_coords_key)
        in_feat = in_feat.contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        b = None if bias is None else bias.detach().reshape(-1).contiguous()
        fw_fn = get_minkowski_function("GroupNormForward", in_feat, in_coords_key)
        out, mean, rstd = fw_fn(in_feat, int(num_groups), w, b, float(eps), in_coords_key, glob_coords_key,
                                coords_manager._manager)
        ctx.save_for_backward(in_feat, w, mean, rstd)
        ctx.misc = (int(num_groups), in_coords_key, glob_coords_key, coords_manager,
                    None if weight is None else weight.shape, None if bias is None else bias.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        in_feat, w, mean, rstd = ctx.saved_tensors
        num_groups, in_key, glob_key, coords_manager, w_shape, b_shape = ctx.misc
        need_w = w_shape is not None and ctx.needs_input_grad[2]
        need_b = b_shape is not None and ctx.needs_input_grad[3]
        bw_fn = get_minkowski_function("GroupNormBackward", grad_out, in_key)
        grad_in, grad_w, grad_b = bw_fn(in_feat, grad_out.contiguous(), num_groups, w, mean, rstd, in_key, glob_key,
                                        coords_manager._manager, need_grad_in=ctx.needs_input_grad[0],
                                        need_grad_weight=need_w, need_grad_bias=need_b)
        return (grad_in, None, grad_w.view(w_shape) if need_w else None, grad_b.view(b_shape) if need_b else None,
                None, None, None, None)


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


class MinkowskiConditionalGroupNormFunction(Function):
    """Group normalisation of the feature rows of a coordinate map, every instance (batch index) on its own, modulated per
    instance and channel and followed by an optional SiLU: act(gn(x) * (1 + scale[b]) + shift[b]).  weight / bias: (C,)
    tensors of the parameter dtype (fp32 for fp32 and bf16 features, float64 for float64) or None; scale / shift:
    (instances, C) tensors of the parameter dtype or None, row j for row j of the origin map, that is for the j-th
    smallest batch index (the batch index itself when the indices are 0..B-1); activation: None or "silu"."""

    @staticmethod
    def forward(ctx, in_feat, num_groups, weight, bias, scale, shift, activation, eps, in_coords_key,
                glob_coords_key=None, coords_manager=None):
        if glob_coords_key is None:
            glob_coords_key = _host.key_like(in_coords_key)
        in_feat = in_feat.contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        b = None if bias is None else bias.detach().reshape(-1).contiguous()
        sc = None if scale is None else scale.detach().contiguous()
        sh = None if shift is None else shift.detach().contiguous()
        fw_fn = get_minkowski_function("ConditionalGroupNormForward", in_feat, in_coords_key)
        out, mean, rstd = fw_fn(in_feat, int(num_groups), w, b, sc, sh, activation, float(eps), in_coords_key,
                                glob_coords_key, coords_manager._manager)
        ctx.save_for_backward(in_feat, w, b, sc, sh, mean, rstd)
        ctx.misc = (int(num_groups), activation, in_coords_key, glob_coords_key, coords_manager,
                    None if weight is None else weight.shape, None if bias is None else bias.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        in_feat, w, b, sc, sh, mean, rstd = ctx.saved_tensors
        num_groups, activation, in_key, glob_key, coords_manager, w_shape, b_shape = ctx.misc
        need_w = w_shape is not None and ctx.needs_input_grad[2]
        need_b = b_shape is not None and ctx.needs_input_grad[3]
        need_sc = sc is not None and ctx.needs_input_grad[4]
        need_sh = sh is not None and ctx.needs_input_grad[5]
        bw_fn = get_minkowski_function("ConditionalGroupNormBackward", grad_out, in_key)
        grad_in, grad_w, grad_b, grad_sc, grad_sh = bw_fn(
            in_feat, grad_out.contiguous(), num_groups, w, b, sc, sh, activation, mean, rstd, in_key, glob_key,
            coords_manager._manager, need_grad_in=ctx.needs_input_grad[0], need_grad_weight=need_w, need_grad_bias=need_b,
            need_grad_scale=need_sc, need_grad_shift=need_sh)
        return (grad_in, None, grad_w.view(w_shape) if need_w else None, grad_b.view(b_shape) if need_b else None,
                grad_sc if need_sc else None, grad_sh if need_sh else None, None, None, None, None, None)


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
