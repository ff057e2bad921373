"""The MLP of a transformer block on sparse tensors as one fused operator (not in the reference):

    y = act(x W1^T + b1) W2^T + b2

`MinkowskiFeedForward` holds two torch.nn.Linear submodules `fc1`, `fc2` (a PTv3 / timm `Mlp` state dict loads strictly)
and runs them on the kernels of csrc/feed_forward.hip: the hidden matrix [N, hidden] is never written, forward or
backward; the Function saves only its inputs and the backward kernels recompute the 32-wide chunk of the hidden
activation they need.  Row-local: no coordinate map, no manager state.

Width rule (one predicate, `backend.feed_forward_fused`): fp32 or bf16 CUDA rows, all operands of one dtype,
`in_features` and `out_features` multiples of 32 up to 128 (bf16) / 64 (fp32), `hidden_features` any multiple of 32.  The
kernels themselves reach 256 (bf16) / 128 (fp32) (`backend.feed_forward_supported`, `me_ffn_supported`), and
MinkowskiFeedForwardFunction serves those widths when called directly, but above the rule's widths torch's two GEMMs were
faster at both measured row counts.  Everything else (float64, other widths, CPU tensors, mixed dtypes)
runs the torch formulation `linear -> activation -> linear` inside the same module; `MinkowskiFeedForward.is_fused(x)`
tells which path a call takes."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import backend as _backend
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .layers import _rewrap
from .normalization import _row_norm_key

ACTIVATIONS = {
    "gelu": F.gelu,
    "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"),
    "relu": F.relu,
    "silu": F.silu,
}


def _check_activation(activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, not {activation!r}")


class MinkowskiFeedForwardFunction(Function):
    """apply(x, w1, b1, w2, b2, activation) -> act(x w1^T + b1) w2^T + b2 on `FeedForward{Forward,Backward}GPU`.
    x [N, C], w1 [Hd, C], b1 [Hd] | None, w2 [Cout, Hd], b2 [Cout] | None, all of one dtype (fp32 or bf16), widths that
    the kernels serve (`backend.feed_forward_supported`).  Only the inputs are saved.  Gradients go to all five tensors (`needs_input_grad` is honoured) and are
    bitwise reproducible.  `owner`: a coordinate map key or manager of the call, which names the host layer."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, activation="gelu", owner=None):
        fw_fn = get_minkowski_function("FeedForwardForward", x, owner)
        x = x.contiguous()
        out = fw_fn(x, w1, b1, w2, b2, activation)
        ctx.save_for_backward(x, w1, b1, w2)
        ctx.misc = (activation, owner, b1 is not None, b2 is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        activation, owner, has_b1, has_b2 = ctx.misc
        x, w1, b1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_fc1, need_fc2 = need[1] or (has_b1 and need[2]), need[3] or (has_b2 and need[4])
        bw_fn = get_minkowski_function("FeedForwardBackward", grad_out, owner)
        dx, dw1, db1, dw2, db2 = bw_fn(x, grad_out, w1, b1, w2, activation, need_grad_in=need[0], need_grad_fc1=need_fc1,
                                       need_grad_fc2=need_fc2)
        return (dx if need[0] else None, dw1 if need[1] else None, db1 if has_b1 and need[2] else None,
                dw2 if need[3] else None, db2 if has_b2 and need[4] else None, None, None)


def is_fused(f, w1, b1, w2, b2):
    """whether feed_forward runs the rows `f` through the kernels (True) or through torch (False)"""
    if not (torch.is_tensor(f) and f.is_cuda and f.dim() == 2 and w1.dim() == 2 and w2.dim() == 2):
        return False
    if any(t is not None and (t.dtype != f.dtype or t.device != f.device) for t in (w1, b1, w2, b2)):
        return False
    return _backend.feed_forward_fused(int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0]), f.dtype)


def feed_forward(input, w1, b1, w2, b2, activation="gelu"):
    """act(F w1^T + b1) w2^T + b2 over the features F of a SparseTensor or a TensorField; the same kind comes back on the
    same coordinate map (MinkowskiFunctional.feed_forward)."""
    _check_activation(activation)
    key = _row_norm_key(input)
    f = input.F
    if f.shape[-1] != w1.shape[1] or w2.shape[1] != w1.shape[0]:
        raise ValueError(f"channel mismatch: features {tuple(f.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}")
    if is_fused(f, w1, b1, w2, b2):
        out = MinkowskiFeedForwardFunction.apply(f, w1, b1, w2, b2, activation, key)
    else:
        out = F.linear(ACTIVATIONS[activation](F.linear(f, w1, b1)), w2, b2)
    return _rewrap(input, out)


class MinkowskiFeedForward(MinkowskiModuleBase):
    r"""The two-layer MLP of a transformer block over the features of a SparseTensor or a TensorField (the same kind
    comes back on the same map): `fc2(act(fc1(x)))` with `fc1 = Linear(in_features, hidden_features)`,
    `fc2 = Linear(hidden_features, out_features or in_features)`, `activation` one of "gelu", "gelu_tanh", "relu", "silu".
    The parameters are those two torch.nn.Linear submodules (torch's initialisation and names): the `mlp.fc1.*` /
    `mlp.fc2.*` entries of a PTv3 / timm `Mlp` checkpoint load strictly, and so does the state dict of
    `nn.Sequential(Linear, act, Linear)` after renaming `0 -> fc1`, `2 -> fc2`.  Within the width rule (see the module
    docstring) one fused launch serves the forward pass and the hidden matrix is never stored; otherwise the module runs
    the torch formulation.  `is_fused(x)` tells which."""

    def __init__(self, in_features, hidden_features, out_features=None, activation="gelu", bias=True):
        super().__init__()
        _check_activation(activation)
        self.activation = activation
        self.fc1 = torch.nn.Linear(in_features, hidden_features, bias=bias)
        self.fc2 = torch.nn.Linear(hidden_features, in_features if out_features is None else out_features, bias=bias)

    def is_fused(self, input):
        f = input if torch.is_tensor(input) else input.F
        return is_fused(f, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)

    def forward(self, input):
        return feed_forward(input, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.activation)

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.fc1.in_features}, {self.fc1.out_features}, {self.fc2.out_features}, "
                f"activation={self.activation!r}, bias={self.fc1.bias is not None})")
