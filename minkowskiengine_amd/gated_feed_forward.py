"""The gated MLP of current transformer blocks (SwiGLU / GeGLU / ReGLU) on sparse tensors as one fused operator (not in
the reference):

    y = (act(x Wg^T + bg) * (x Wu^T + bu)) W2^T + b2

`MinkowskiGatedFeedForward` holds three torch.nn.Linear submodules `fc1_g` (gate), `fc1_x` (up) and `fc2` (a timm `SwiGLU`
state dict loads strictly; `from_packed` takes a packed `[2 Hd, C]` first layer) and runs them on the kernels of
csrc/gated_feed_forward.hip: none of the three [N, hidden] matrices of the unfused form is written, forward or backward; the
Function saves only its inputs and the backward kernels recompute the 32-wide chunk they need.  Row-local: no coordinate map,
no manager state.

Width rule (one predicate, `backend.gated_feed_forward_fused`): fp32 or bf16 CUDA rows, all operands of one dtype,
`in_features` and `out_features` multiples of 32 up to 128 (bf16) / 64 (fp32), `hidden_features` any multiple of 32
(DESIGN 8.19).  Everything else (float64, other widths, CPU tensors, mixed dtypes) runs the torch formulation
`fc2(act(fc1_g(x)) * fc1_x(x))` inside the same module; `MinkowskiGatedFeedForward.is_fused(x)` tells which path a call
takes."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import backend as _backend
from .common import get_minkowski_function
from .convolution import MinkowskiModuleBase
from .feed_forward import ACTIVATIONS, _check_activation
from .layers import _rewrap
from .normalization import _row_norm_key


class MinkowskiGatedFeedForwardFunction(Function):
    """apply(x, wg, bg, wu, bu, w2, b2, activation, owner) -> (act(x wg^T + bg) * (x wu^T + bu)) w2^T + b2 on
    `GatedFeedForward{Forward,Backward}GPU`.  x [N, C], wg and wu [Hd, C], bg and bu [Hd] | None, w2 [Cout, Hd],
    b2 [Cout] | None, all of one dtype (fp32 or bf16), widths that the kernels serve
    (`backend.gated_feed_forward_supported`).  Only the inputs are saved.  Gradients go to all seven tensors
    (`needs_input_grad` is honoured) and are bitwise reproducible.  `owner`: a coordinate map key or manager of the call,
    which names the host layer."""

    @staticmethod
    def forward(ctx, x, wg, bg, wu, bu, w2, b2, activation="silu", owner=None):
        fw_fn = get_minkowski_function("GatedFeedForwardForward", x, owner)
        x = x.contiguous()
        out = fw_fn(x, wg, bg, wu, bu, w2, b2, activation)
        ctx.save_for_backward(x, wg, bg, wu, bu, w2)
        ctx.misc = (activation, owner, bg is not None, bu is not None, b2 is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        activation, owner, has_bg, has_bu, has_b2 = ctx.misc
        x, wg, bg, wu, bu, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_fc1 = need[1] or need[3] or (has_bg and need[2]) or (has_bu and need[4])
        need_fc2 = need[5] or (has_b2 and need[6])
        bw_fn = get_minkowski_function("GatedFeedForwardBackward", grad_out, owner)
        dx, dwg, dbg, dwu, dbu, dw2, db2 = bw_fn(x, grad_out, wg, bg, wu, bu, w2, activation, need_grad_in=need[0],
                                                 need_grad_fc1=need_fc1, need_grad_fc2=need_fc2)
        return (dx if need[0] else None, dwg if need[1] else None, dbg if has_bg and need[2] else None,
                dwu if need[3] else None, dbu if has_bu and need[4] else None, dw2 if need[5] else None,
                db2 if has_b2 and need[6] else None, None, None)


def is_fused(f, wg, bg, wu, bu, w2, b2):
    """whether gated_feed_forward runs the rows `f` through the kernels (True) or through torch (False)"""
    if not (torch.is_tensor(f) and f.is_cuda and f.dim() == 2 and wg.dim() == 2 and wu.dim() == 2 and w2.dim() == 2):
        return False
    if any(t is not None and (t.dtype != f.dtype or t.device != f.device) for t in (wg, bg, wu, bu, w2, b2)):
        return False
    return _backend.gated_feed_forward_fused(int(wg.shape[1]), int(wg.shape[0]), int(w2.shape[0]), f.dtype)


def gated_feed_forward(input, wg, bg, wu, bu, w2, b2, activation="silu"):
    """(act(F wg^T + bg) * (F wu^T + bu)) w2^T + b2 over the features F of a SparseTensor or a TensorField; the same kind
    comes back on the same coordinate map (MinkowskiFunctional.gated_feed_forward)."""
    _check_activation(activation)
    key = _row_norm_key(input)
    f = input.F
    if f.shape[-1] != wg.shape[1] or wu.shape != wg.shape or w2.shape[1] != wg.shape[0]:
        raise ValueError(f"channel mismatch: features {tuple(f.shape)}, wg {tuple(wg.shape)}, wu {tuple(wu.shape)}, "
                         f"w2 {tuple(w2.shape)}")
    if is_fused(f, wg, bg, wu, bu, w2, b2):
        out = MinkowskiGatedFeedForwardFunction.apply(f, wg, bg, wu, bu, w2, b2, activation, key)
    else:
        out = F.linear(ACTIVATIONS[activation](F.linear(f, wg, bg)) * F.linear(f, wu, bu), w2, b2)
    return _rewrap(input, out)


class MinkowskiGatedFeedForward(MinkowskiModuleBase):
    r"""The gated MLP of a transformer block over the features of a SparseTensor or a TensorField (the same kind comes
    back on the same map): `fc2(act(fc1_g(x)) * fc1_x(x))` with `fc1_g`, `fc1_x = Linear(in_features, hidden_features)`,
    `fc2 = Linear(hidden_features, out_features or in_features)`; `activation` "silu" (SwiGLU, the default), "gelu" /
    "gelu_tanh" (GeGLU) or "relu" (ReGLU).  The parameters are those three torch.nn.Linear submodules, named as in timm's
    `SwiGLU` (DINOv2, EVA), whose state dict loads strictly; LLaMA's `gate_proj` / `up_proj` / `down_proj` are
    `fc1_g` / `fc1_x` / `fc2` with `bias=False`.  A packed first layer goes through `from_packed`.  Within the width rule
    (see the module docstring) one fused launch serves the forward pass and no hidden matrix is ever stored; otherwise the
    module runs the torch formulation.  `is_fused(x)` tells which."""

    def __init__(self, in_features, hidden_features, out_features=None, activation="silu", bias=True):
        super().__init__()
        _check_activation(activation)
        self.activation = activation
        self.fc1_g = torch.nn.Linear(in_features, hidden_features, bias=bias)
        self.fc1_x = torch.nn.Linear(in_features, hidden_features, bias=bias)
        self.fc2 = torch.nn.Linear(hidden_features, in_features if out_features is None else out_features, bias=bias)

    @classmethod
    def from_packed(cls, fc1_weight, fc1_bias, fc2_weight, fc2_bias, activation="silu", gate_first=True):
        """A module from a packed first layer `fc1_weight` [2 Hd, C] (`fc1_bias` [2 Hd] | None) and `fc2_weight` [Cout, Hd]
        (`fc2_bias` [Cout] | None); all biases or none.  The rows are split in halves (`chunk(2)`): with `gate_first=True`
        rows [0, Hd) are the gate, the half that goes through the activation, and rows [Hd, 2 Hd) the up projection: LLaMA's
        `gate_up_proj`, and timm's `GluMlp(gate_last=False)`.  timm's default `GluMlp(gate_last=True)` activates the
        second half: pass `gate_first=False`."""
        if fc1_weight.dim() != 2 or fc1_weight.shape[0] % 2 != 0 or fc2_weight.shape[1] * 2 != fc1_weight.shape[0]:
            raise ValueError(f"fc1_weight {tuple(fc1_weight.shape)} is not a packed first layer of fc2_weight "
                             f"{tuple(fc2_weight.shape)}")
        if (fc1_bias is None) != (fc2_bias is None):
            raise ValueError("fc1_bias and fc2_bias must both be given or both be None")
        hd, c = fc1_weight.shape[0] // 2, fc1_weight.shape[1]
        self = cls(c, hd, fc2_weight.shape[0], activation, bias=fc1_bias is not None)
        self.to(device=fc1_weight.device, dtype=fc1_weight.dtype)
        g, u = (0, 1) if gate_first else (1, 0)
        with torch.no_grad():
            halves = fc1_weight.chunk(2)
            self.fc1_g.weight.copy_(halves[g])
            self.fc1_x.weight.copy_(halves[u])
            self.fc2.weight.copy_(fc2_weight)
            if fc1_bias is not None:
                halves = fc1_bias.chunk(2)
                self.fc1_g.bias.copy_(halves[g])
                self.fc1_x.bias.copy_(halves[u])
                self.fc2.bias.copy_(fc2_bias)
        return self

    def _operands(self):
        return (self.fc1_g.weight, self.fc1_g.bias, self.fc1_x.weight, self.fc1_x.bias, self.fc2.weight, self.fc2.bias)

    def is_fused(self, input):
        f = input if torch.is_tensor(input) else input.F
        return is_fused(f, *self._operands())

    def forward(self, input):
        return gated_feed_forward(input, *self._operands(), self.activation)

    def __repr__(self):
        return (self.__class__.__name__ + f"({self.fc1_g.in_features}, {self.fc1_g.out_features}, {self.fc2.out_features}, "
                f"activation={self.activation!r}, bias={self.fc1_g.bias is not None})")
