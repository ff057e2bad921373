"""Feature-only layers that MinkUNet-style networks need around the convolutions.  In the reference
these contain no native code: they apply torch modules to `.F` and re-wrap
(MinkowskiNormalization.py:51-140, MinkowskiNonlinearity.py, MinkowskiOps.py:141-158)."""
import os

import torch
import torch.nn as nn
from torch.autograd import Function

from . import backend as MEB
from . import host as _host
from .sparse_tensor import SparseTensor

_TORCH_BN = os.environ.get("ME_AMD_TORCH_BN", "0") != "0"   # 1: torch's batch-norm kernels (A/B timing)
_FUSE_RESIDUAL = os.environ.get("ME_AMD_FUSE_RESIDUAL", "1") != "0"   # bn + residual add + relu in one kernel


def _rewrap(x, feats):
    """the same kind of tensor on the same coordinates: a TensorField input gives a TensorField on its field key (the
    reference's MinkowskiNonlinearity.py does this), a SparseTensor a SparseTensor"""
    if not isinstance(x, SparseTensor) and hasattr(x, "coordinate_field_map_key"):
        return x._like(feats)
    return SparseTensor(feats, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x._manager)


class _BatchNormTrainFunction(Function):
    """Training-mode batch norm of a feature matrix on the HIP kernels of csrc/norm.hip (statistics in fp32,
    fixed summation order).  weight / bias may be None."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu=False, num_batches_tracked=None):
        x = x.contiguous()
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        mean, rstd = MEB.bn_stats(x, eps, momentum, running_mean, running_var, num_batches_tracked)
        y = MEB.bn_apply(x, mean, rstd, w32, b32, relu)
        ctx.save_for_backward(x, mean, rstd, w32, b32)
        ctx.param_dtype = weight.dtype if weight is not None else None
        ctx.has_bias = bias is not None
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w32, b32 = ctx.saved_tensors
        dx, gg, gb = MEB.bn_backward(x, dy, mean, rstd, w32, b32, ctx.relu)
        gw = gg.to(ctx.param_dtype) if ctx.param_dtype is not None else None
        gbias = gb.to(ctx.param_dtype) if ctx.has_bias else None
        return dx, gw, gbias, None, None, None, None, None, None


class _BatchNormResidualFunction(Function):
    """y = [relu] (batch_norm(x) + skip) on the fused kernels of csrc/norm.hip (me_bn_apply_residual /
    me_bn_backward_residual): the tail of a ResNet block in one pass per direction."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, running_mean, running_var, momentum, eps, relu, num_batches_tracked):
        x = x.contiguous()
        skip = skip.contiguous()
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        mean, rstd = MEB.bn_stats(x, eps, momentum, running_mean, running_var, num_batches_tracked)
        y = MEB.bn_apply_residual(x, skip, mean, rstd, w32, b32, relu)
        ctx.save_for_backward(x, y if relu else None, mean, rstd, w32, b32)
        ctx.param_dtype = weight.dtype if weight is not None else None
        ctx.has_bias = bias is not None
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, w32, b32 = ctx.saved_tensors
        dx, dskip, gg, gb = MEB.bn_backward_residual(x, dy, y, mean, rstd, w32, b32, ctx.relu,
                                                     need_dskip=ctx.needs_input_grad[1])
        gw = gg.to(ctx.param_dtype) if ctx.param_dtype is not None else None
        gbias = gb.to(ctx.param_dtype) if ctx.has_bias else None
        return dx, dskip, gw, gbias, None, None, None, None, None, None


def _all_gather_rows(t, group):
    """-> [world, *t.shape]: `t` of every rank of `group` in rank order, one collective.  all_gather_into_tensor on
    RCCL (backend "nccl"); every other backend takes all_gather into the rows of the result — gloo has no
    all_gather_into_tensor and stages GPU tensors through the host, mpi / ucc may lack it too."""
    import torch.distributed as dist
    out = t.new_empty((dist.get_world_size(group),) + tuple(t.shape))
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(out, t, group)
    else:
        dist.all_gather(list(out.unbind(0)), t, group)
    return out


class _SyncBatchNormFunction(Function):
    """Training-mode batch norm with statistics over the rows of ALL ranks of `group`, on the kernels of
    csrc/norm.hip: y = [relu] (batch_norm(x) [+ skip]).  skip None: the plain form (_BatchNormTrainFunction with a
    fused ReLU), else the residual form (_BatchNormResidualFunction).  One all-gather per direction: forward, each
    rank's record (row count, mean, M2), merged by every rank in rank order — bit-identical statistics everywhere;
    backward, each rank's [2c] sums, added in rank order (not an all-reduce, whose order is the backend's).  The
    global row count stays on the device.  A rank without rows enters both collectives.  grad_weight / grad_bias are
    the LOCAL sums, as in torch's SyncBatchNorm: DistributedDataParallel averages them.  One Python function for both
    host layers: the path is bound by its exchange, not by its launches."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, running_mean, running_var, momentum, eps, relu, num_batches_tracked, group):
        x = x.contiguous()
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        records = _all_gather_rows(MEB.bn_local_moments(x), group)
        mean, rstd, n_total = MEB.bn_stats_from_moments(records, eps, momentum, running_mean, running_var,
                                                        num_batches_tracked)
        if x.shape[0] == 0:
            y = torch.empty_like(x)
        elif skip is None:
            y = MEB.bn_apply(x, mean, rstd, w32, b32, relu)
        else:
            y = MEB.bn_apply_residual(x, skip.contiguous(), mean, rstd, w32, b32, relu)
        # (residual form: the ReLU mask of the backward pass is the stored output, which also holds the skip branch)
        ctx.save_for_backward(x, y if (relu and skip is not None) else None, mean, rstd, w32, b32, n_total)
        ctx.param_dtype = weight.dtype if weight is not None else None
        ctx.has_bias = bias is not None
        ctx.relu = relu
        ctx.residual = skip is not None
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, dy):
        x, yout, mean, rstd, w32, b32, n_total = ctx.saved_tensors
        dy = dy.to(x.dtype).contiguous()
        local = MEB.bn_backward_sums(x, dy, mean, rstd, w32, b32, ctx.relu, yout)
        sums = MEB.bn_backward_reduce(_all_gather_rows(local, ctx.group))
        dx, dskip = MEB.bn_backward_apply(x, dy, n_total, mean, rstd, w32, b32, sums, ctx.relu, yout,
                                          need_dskip=ctx.residual and ctx.needs_input_grad[1])
        gw = local[1].to(ctx.param_dtype) if ctx.param_dtype is not None else None
        gbias = local[0].to(ctx.param_dtype) if ctx.has_bias else None
        return dx, dskip, gw, gbias, None, None, None, None, None, None, None


class MinkowskiBatchNorm(nn.Module):
    """torch.nn.BatchNorm1d semantics on the feature matrix (MinkowskiNormalization.py:35-82).  The parameters
    and running statistics live in `self.bn` (same state-dict names as the reference); on the GPU the arithmetic
    runs on this package's kernels."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)
        # Not in the reference: set by a model whose next layer is ALWAYS a MinkowskiReLU.  The rectification is
        # then done by the batch-norm kernels (forward clamp, backward mask) and the output tensor is marked so
        # that the following MinkowskiReLU passes it through; the results are those of the two separate layers.
        self.fuse_relu = False

    _TORCH_MODULE = nn.BatchNorm1d    # what `self.bn` is (a subclass of it keeps torch's arithmetic)

    def _native(self, f, min_rows=2):
        bn = self.bn
        return (not _TORCH_BN and type(bn) is self._TORCH_MODULE and f.is_cuda and f.dim() == 2
                and f.shape[0] >= min_rows and f.dtype in (torch.float32, torch.bfloat16) and bn.momentum is not None
                and f.shape[1] <= 2048)

    def forward(self, input):
        f = input.F
        bn = self.bn
        if not self._native(f):
            return _rewrap(input, bn(f))
        use_batch_stats = bn.training or not bn.track_running_stats
        if use_batch_stats:
            rm = bn.running_mean if (bn.training and bn.track_running_stats) else None
            rv = bn.running_var if (bn.training and bn.track_running_stats) else None
            # (num_batches_tracked is incremented by the statistics kernel: 62 one-element torch kernels per
            # MinkUNet34C pass otherwise)
            nbt = bn.num_batches_tracked if rm is not None else None
            if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
                nbt.add_(1)
                nbt = None
            if getattr(input._manager, "_native", False):      # C++ autograd function of the native host layer
                y = _host.native_module().batch_norm_train(f, None, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps,
                                                           bool(self.fuse_relu), nbt)
            else:
                y = _BatchNormTrainFunction.apply(f, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, self.fuse_relu,
                                                  nbt)
            out = _rewrap(input, y)
            out._rectified = self.fuse_relu
            return out
        else:
            # evaluation: an affine map per channel, differentiable through torch (cheap: two fused passes)
            # (the kernels take float32 vectors: after `model.bfloat16()` the running statistics are bf16)
            rmean = bn.running_mean.float().contiguous()
            rstd = torch.rsqrt(bn.running_var.float() + bn.eps).contiguous()
            a = rstd * bn.weight.float() if bn.weight is not None else rstd
            b = (bn.bias.float() if bn.bias is not None else 0.0) - rmean * a
            y = (f * a.to(f.dtype) + b.to(f.dtype)) if f.requires_grad else \
                MEB.bn_apply(f.contiguous(), rmean, rstd,
                             bn.weight.float().contiguous() if bn.weight is not None else None,
                             bn.bias.float().contiguous() if bn.bias is not None else None)
        return _rewrap(input, y)

    def forward_residual(self, input, skip, relu=True):
        """[relu] (self(input) + skip) — the tail of a ResNet block (reference: modules/resnet_block.py:62-75 applies
        norm, `out += residual`, relu as three operators).  Training mode on the GPU: one fused kernel per direction,
        bit-identical to the separate operators; anything else falls back to them."""
        assert input.coordinate_map_key == skip.coordinate_map_key, "residual add needs a shared coordinate map"
        f, bn = input.F, self.bn
        fused = (_FUSE_RESIDUAL and self._native(f) and (bn.training or not bn.track_running_stats)
                 and skip.F.dtype == f.dtype and skip.F.shape == f.shape)
        if not fused:
            out = self.forward(input)
            y = out.F + skip.F
            return _rewrap(input, torch.relu(y) if relu else y)
        rm = bn.running_mean if (bn.training and bn.track_running_stats) else None
        rv = bn.running_var if (bn.training and bn.track_running_stats) else None
        nbt = bn.num_batches_tracked if rm is not None else None
        if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
            nbt.add_(1)
            nbt = None
        if getattr(input._manager, "_native", False):
            y = _host.native_module().batch_norm_train(f, skip.F, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps,
                                                       bool(relu), nbt)
        else:
            y = _BatchNormResidualFunction.apply(f, skip.F, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, bool(relu),
                                                 nbt)
        return _rewrap(input, y)

    def __repr__(self):
        b = self.bn
        return (f"{self.__class__.__name__}({b.num_features}, eps={b.eps}, momentum={b.momentum}, "
                f"affine={b.affine}, track_running_stats={b.track_running_stats})")


class MinkowskiSyncBatchNorm(MinkowskiBatchNorm):
    """MinkowskiBatchNorm with batch statistics over all ranks of a process group (MinkowskiNormalization.py:85-191).
    `self.bn` is a torch.nn.SyncBatchNorm (parameters, buffers, process group, state-dict names); in training mode on
    the GPU the arithmetic runs on this package's kernels around one all-gather per direction
    (_SyncBatchNormFunction), with `fuse_relu` and the fused `forward_residual` of the parent.  Without an exchange —
    torch.distributed not initialised, a group of one rank, evaluation — it is the parent's local path, as torch's
    module uses local statistics then.  momentum=None, CPU or non-2-D features, more than 2048 channels, float64 and
    ME_AMD_TORCH_BN=1 go to `self.bn(f)`."""
    _TORCH_MODULE = nn.SyncBatchNorm

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True,
                 process_group=None):
        nn.Module.__init__(self)
        self.fuse_relu = False
        self.bn = nn.SyncBatchNorm(num_features, eps=eps, momentum=momentum, affine=affine,
                                   track_running_stats=track_running_stats, process_group=process_group)

    def _exchange_group(self):
        """the process group to exchange statistics with, None when torch's SyncBatchNorm would use local ones"""
        import torch.distributed as dist
        bn = self.bn
        if not (bn.training and dist.is_available() and dist.is_initialized()):
            return None
        group = bn.process_group if bn.process_group else dist.group.WORLD
        return group if dist.get_world_size(group) > 1 else None

    def _train(self, f, skip, relu, group):
        bn = self.bn
        rm = bn.running_mean if bn.track_running_stats else None
        rv = bn.running_var if bn.track_running_stats else None
        nbt = bn.num_batches_tracked if rm is not None else None
        return _SyncBatchNormFunction.apply(f, skip, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, bool(relu), nbt,
                                            group)

    def forward(self, input):
        group = self._exchange_group()
        if group is None:
            return super().forward(input)
        f = input.F
        if not self._native(f, min_rows=0):       # (a rank may hold no rows: it still enters the collectives)
            return _rewrap(input, self.bn(f))
        out = _rewrap(input, self._train(f, None, self.fuse_relu, group))
        out._rectified = self.fuse_relu
        return out

    def forward_residual(self, input, skip, relu=True):
        group = self._exchange_group()
        f = input.F
        if (group is None or not _FUSE_RESIDUAL or not self._native(f, min_rows=0) or skip.F.dtype != f.dtype
                or skip.F.shape != f.shape):
            return super().forward_residual(input, skip, relu)      # (the three operators around self.forward)
        assert input.coordinate_map_key == skip.coordinate_map_key, "residual add needs a shared coordinate map"
        return _rewrap(input, self._train(f, skip.F, relu, group))

    @classmethod
    def convert_sync_batchnorm(cls, module, process_group=None):
        """MinkowskiNormalization.py:138-191.  Conscious divergence: the reference recurses into the children of a
        MinkowskiBatchNorm it has just converted and its `add_module("bn", <the old nn.BatchNorm1d>)` puts the
        UNSYNCHRONISED torch module back (MinkowskiNormalization.py:186-189), so its "sync" batch norm normalises with
        per-rank statistics; here a converted module keeps its nn.SyncBatchNorm
        (tests/test_gpu_distributed.py compares against one process on the batched scenes)."""
        out = module
        if isinstance(module, MinkowskiSyncBatchNorm):
            return module
        if isinstance(module, MinkowskiBatchNorm):
            out = cls(module.bn.num_features, module.bn.eps, module.bn.momentum, module.bn.affine,
                      module.bn.track_running_stats, process_group)
            out.fuse_relu = module.fuse_relu      # (not in the reference: the fused ReLU survives the conversion)
            if module.bn.affine:          # the same Parameter objects, as the reference (:176-179)
                out.bn.weight = module.bn.weight
                out.bn.bias = module.bn.bias
            if module.bn.track_running_stats:
                out.bn.running_mean = module.bn.running_mean
                out.bn.running_var = module.bn.running_var
                out.bn.num_batches_tracked = module.bn.num_batches_tracked
            return out
        for name, child in module.named_children():
            out.add_module(name, cls.convert_sync_batchnorm(child, process_group))
        return out


class _Elementwise(nn.Module):
    MODULE = None

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.module = self.MODULE(*args, **kwargs)

    def forward(self, input):
        return _rewrap(input, self.module(input.F))

    def __repr__(self):
        return self.__class__.__name__ + "()"


class MinkowskiReLU(_Elementwise):
    MODULE = nn.ReLU

    def forward(self, input):
        # the output of a MinkowskiBatchNorm with fuse_relu is already rectified
        if getattr(input, "_rectified", False):
            return input
        return _rewrap(input, self.module(input.F))


class MinkowskiLeakyReLU(_Elementwise):
    MODULE = nn.LeakyReLU


class MinkowskiELU(_Elementwise):
    MODULE = nn.ELU


class MinkowskiSigmoid(_Elementwise):
    MODULE = nn.Sigmoid


class MinkowskiTanh(_Elementwise):
    MODULE = nn.Tanh


class MinkowskiDropout(_Elementwise):
    MODULE = nn.Dropout


# The rest of MinkowskiNonlinearity.py: one class per torch module, applied to the feature matrix and re-wrapped on the
# input's coordinates (thin torch wrappers as in the reference, no kernels of their own).  The wrapped module
# is `self.module`, so state-dict keys are `module.*` as in the reference.  Modules with a `dim` (the softmax family)
# see [N, C]: dim=1 is the channel axis.
def _elementwise(name, module):
    return type(name, (_Elementwise,), {"MODULE": module, "__module__": __name__,
                                        "__doc__": f"torch.nn.{module.__name__} on the features"})


_NONLINEARITIES = ("PReLU", "ReLU6", "RReLU", "SELU", "CELU", "GELU", "SiLU", "Hardshrink", "Hardsigmoid", "Hardtanh",
                   "Hardswish", "LogSigmoid", "Softplus", "Softshrink", "Softsign", "Tanhshrink", "Threshold", "Softmin",
                   "Softmax", "LogSoftmax", "AdaptiveLogSoftmaxWithLoss", "AlphaDropout")
for _n in _NONLINEARITIES:
    globals()["Minkowski" + _n] = _elementwise("Minkowski" + _n, getattr(nn, _n))
del _n


class MinkowskiSinusoidal(nn.Module):
    """coef * sin(F @ kernel + bias): a learned sinusoidal embedding of the features (parameters `kernel`
    [in_channel, out_channel], `bias` and `coef` [1, out_channel], uniform in [0, 1) as in the reference)."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.kernel = nn.Parameter(torch.rand(in_channel, out_channel))
        self.bias = nn.Parameter(torch.rand(1, out_channel))
        self.coef = nn.Parameter(torch.rand(1, out_channel))

    def forward(self, input):
        return _rewrap(input, torch.sin(input.F.mm(self.kernel) + self.bias) * self.coef)


class MinkowskiLinear(nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, input):
        return _rewrap(input, self.linear(input.F))


def _tuple_operator(sparse_tensors, operator):
    """`operator(list of feature matrices)` of tensors that share one coordinate map, re-wrapped on that map: sparse
    tensors, or tensor fields on one field key (MinkowskiOps.py:70-138)."""
    if len(sparse_tensors) == 1 and isinstance(sparse_tensors[0], (list, tuple)):
        sparse_tensors = tuple(sparse_tensors[0])
    first = sparse_tensors[0]
    if not isinstance(first, SparseTensor) and hasattr(first, "coordinate_field_map_key"):
        for s in sparse_tensors:
            assert hasattr(s, "coordinate_field_map_key"), "Inputs must all be tensor fields."
            assert s._manager is first._manager, "coordinate managers must match"
            assert s.coordinate_field_map_key == first.coordinate_field_map_key, "cat needs a shared field key"
        return _rewrap(first, operator([s.F for s in sparse_tensors]))
    for s in sparse_tensors:
        assert isinstance(s, SparseTensor), "Inputs must be sparse tensors."
        assert s._manager is first._manager, "coordinate managers must match"
        assert s.coordinate_map_key == first.coordinate_map_key, "cat needs a shared coordinate map"
    return _rewrap(first, operator([s.F for s in sparse_tensors]))


def cat(*sparse_tensors):
    """Concatenate the features of tensors that share one coordinate map (MinkowskiOps.py:141-158): sparse tensors,
    or tensor fields on one field key."""
    return _tuple_operator(sparse_tensors, lambda xs: torch.cat(xs, dim=1))
