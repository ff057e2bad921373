"""MinkowskiInterpolation and its autograd Function (reference: MinkowskiEngine/MinkowskiInterpolation.py): trilinear
interpolation of a sparse tensor's features at continuous coordinates.  The map (me_field_interp_map) and both passes
(me_csr_gather, forward by sample, backward by voxel through a stable transpose) are HIP kernels of csrc/field.hip."""
import torch
from torch.autograd import Function

from . import host as _host
from .convolution import MinkowskiModuleBase


class MinkowskiInterpolationFunction(Function):
    """-> (out_feat, in_map, out_map, weights): out_feat[p] = sum over the present corners of sample p of
    w * input_features[corner row]; samples without a present corner give zero rows (and zero gradients)."""

    @staticmethod
    def forward(ctx, input_features, tfield, in_coordinate_map_key, coordinate_manager=None):
        input_features = input_features.contiguous()
        B = _host.backend_of(in_coordinate_map_key)
        mgr = coordinate_manager._manager
        out_feat, in_map, out_map, weights = B.InterpolationForwardGPU(input_features, tfield, in_coordinate_map_key,
                                                                       mgr)
        ctx.save_for_backward(in_map, out_map, weights)
        ctx.misc = (in_coordinate_map_key, mgr, B)
        ctx.mark_non_differentiable(in_map, out_map, weights)
        return out_feat, in_map, out_map, weights

    @staticmethod
    def backward(ctx, grad_out_feat=None, grad_in_map=None, grad_out_map=None, grad_weights=None):
        in_map, out_map, weights = ctx.saved_tensors
        in_key, mgr, B = ctx.misc
        grad_in = None
        if ctx.needs_input_grad[0]:
            grad_in = B.InterpolationBackwardGPU(grad_out_feat.contiguous(), in_map, out_map, weights, in_key, mgr)
        return grad_in, None, None, None


class MinkowskiInterpolation(MinkowskiModuleBase):
    """Features of a sparse tensor at continuous coordinates `tfield` [N, D+1] (float32 or float64), by trilinear
    interpolation over the present voxel corners.  bf16 features take fp32 coordinates (an extension of the reference,
    which requires the features' dtype)."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map = return_kernel_map
        self.return_weights = return_weights
        self.interp = MinkowskiInterpolationFunction

    def forward(self, input, tfield):
        out_feat, in_map, out_map, weights = self.interp.apply(input.F, tfield, input.coordinate_map_key,
                                                               input._manager)
        return_args = [out_feat]
        if self.return_kernel_map:
            return_args.append((in_map, out_map))
        if self.return_weights:
            return_args.append(weights)
        if len(return_args) > 1:
            return tuple(return_args)
        return out_feat

    def __repr__(self):
        return self.__class__.__name__ + "()"
