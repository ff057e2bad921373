"""MinkowskiChannelwiseConvolution and its autograd Function (reference:
MinkowskiEngine/MinkowskiChannelwiseConvolution.py:37-218).  The reference runs the layer in Python (one gather,
multiply and index_put per kernel offset, autograd for the backward); here the Function resolves
`ChannelwiseConvolution{Forward,Backward}GPU` in the backend by name, as the other operators do, and those run the
HIP kernels of csrc/conv_channelwise.hip."""
import math

import torch
from torch.autograd import Function
from torch.nn import Parameter

from . import host as _host
from .backend import RegionType
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .kernel_generator import KernelGenerator
from .sparse_tensor import SparseTensor, _get_coordinate_map_key


class MinkowskiChannelwiseConvolutionFunction(Function):
    """out[u] = bias + sum_k kernel[k] * x[u + offset(k)] (elementwise over the channels).  kernel: [volume, C] with
    the dtype of the features (fp32 for bf16 features), bias: C values or None.  The gradients of the kernel and the
    bias have the kernel's dtype; the input gradient is skipped when autograd does not ask for it."""

    @staticmethod
    def forward(ctx, input_features, kernel_weights, bias, kernel_generator, in_coordinate_map_key,
                out_coordinate_map_key=None, coordinate_manager=None):
        if out_coordinate_map_key is None:
            out_coordinate_map_key = _host.key_like(in_coordinate_map_key)
        input_features = input_features.contiguous()
        ctx.input_features = input_features
        ctx.kernel_weights = kernel_weights
        ctx.bias_shape = None if bias is None else bias.shape
        ctx.misc = (kernel_generator, in_coordinate_map_key, out_coordinate_map_key, coordinate_manager)
        fw_fn = get_minkowski_function("ChannelwiseConvolutionForward", input_features, in_coordinate_map_key)
        return fw_fn(input_features, kernel_weights, bias, kernel_generator.kernel_size, kernel_generator.kernel_stride,
                     kernel_generator.kernel_dilation, kernel_generator.region_type, kernel_generator.region_offsets,
                     in_coordinate_map_key, out_coordinate_map_key, coordinate_manager._manager)

    @staticmethod
    def backward(ctx, grad_out_feat):
        grad_out_feat = grad_out_feat.contiguous()
        kernel_generator, in_key, out_key, coordinate_manager = ctx.misc
        need_bias = ctx.bias_shape is not None and ctx.needs_input_grad[2]
        bw_fn = get_minkowski_function("ChannelwiseConvolutionBackward", grad_out_feat, in_key)
        grad_in, grad_kernel, grad_bias = bw_fn(
            ctx.input_features, grad_out_feat, ctx.kernel_weights, kernel_generator.kernel_size,
            kernel_generator.kernel_stride, kernel_generator.kernel_dilation, kernel_generator.region_type,
            kernel_generator.region_offsets, in_key, out_key, coordinate_manager._manager,
            need_grad_in=ctx.needs_input_grad[0], need_grad_bias=need_bias)
        if grad_bias is not None:
            grad_bias = grad_bias.view(ctx.bias_shape)
        return (grad_in, grad_kernel if ctx.needs_input_grad[1] else None, grad_bias, None, None, None, None)


class MinkowskiChannelwiseConvolution(MinkowskiModuleBase):
    r"""Channelwise (depthwise) convolution of a sparse tensor: every channel has its own kernel,

        out_u = bias + sum_{i in N^D(u, K) ∩ C^in} W_i ⊙ x_{u + i}     for u in C^out

    (MinkowskiChannelwiseConvolution.py:37-68).  Parameters `kernel` (kernel_volume, in_channels) and `bias`
    (1, in_channels), fp32, as in the reference, so its state dicts load strictly.  bf16 features run with the fp32
    weights and give bf16 outputs; float64 features need a `.double()` module.

    `forward(input, coords=None)`: without `coords` the output map is stride(input map, stride), as in the reference.
    Given `coords` (coordinates, a coordinate map key or a sparse tensor) the output is computed on them, as
    MinkowskiConvolution and the pooling layers do; the reference accepts the argument and ignores it."""

    def __init__(self, in_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 dimension=-1):
        super().__init__()
        assert dimension > 0, f"Invalid dimension. Please provide a valid dimension argument. dimension={dimension}"
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size=kernel_size, stride=stride, dilation=dilation,
                                               dimension=dimension)
        self.kernel_generator = kernel_generator
        self.in_channels = in_channels
        self.dimension = dimension
        self.kernel_shape = (kernel_generator.kernel_volume, self.in_channels)
        self.kernel = Parameter(torch.empty(*self.kernel_shape, dtype=torch.float32))
        self.bias = Parameter(torch.empty(1, in_channels, dtype=torch.float32)) if bias else None
        self.reset_parameters()

    def forward(self, input, coords=None):
        assert isinstance(input, SparseTensor)
        assert input.D == self.dimension
        assert self.in_channels == input.shape[1], f"Channel size mismatch {self.in_channels} != {input.shape[1]}"
        out_coordinate_map_key = _get_coordinate_map_key(input, coords)
        outfeat = MinkowskiChannelwiseConvolutionFunction.apply(
            input.F, self.kernel, self.bias, self.kernel_generator, input.coordinate_map_key, out_coordinate_map_key,
            input._manager)
        return SparseTensor(outfeat, coordinate_map_key=out_coordinate_map_key, coordinate_manager=input._manager)

    def reset_parameters(self, is_transpose=False):
        with torch.no_grad():
            n = self.in_channels * self.kernel_generator.kernel_volume
            stdv = 1.0 / math.sqrt(n)
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def __repr__(self):
        rt = self.kernel_generator.region_type     # printed as the reference's pybind enum prints: RegionType.NAME
        s = "(in={}, region_type={}, ".format(self.in_channels, f"RegionType.{RegionType(int(rt)).name}")
        if self.kernel_generator.region_type in [RegionType.CUSTOM]:
            s += "kernel_volume={}, ".format(self.kernel_generator.kernel_volume)
        else:
            s += "kernel_size={}, ".format(self.kernel_generator.kernel_size)
        s += "stride={}, dilation={})".format(self.kernel_generator.kernel_stride, self.kernel_generator.kernel_dilation)
        return self.__class__.__name__ + s
