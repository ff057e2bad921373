"""Causal depthwise conv1d along the serialized voxel order — the local mixing of Voxel Mamba, LION and Vim-style blocks, and
the conv1d of MinkowskiMamba.  The sequence is the selective scan's (scan_sequence: every instance along the curve `order`,
instance after instance, backwards with `reverse`).  With K taps, weight [D, K] and bias [D]:

    pre[row_p, d] = bias[d] + sum_{j < K} weight[d, K - 1 - j] x[row_{p - j}, d]
    y = act(pre),  act the identity or SiLU

where tap j is dropped when fewer than j positions of the instance precede p: on one instance this is
`torch.nn.functional.conv1d(..., padding=K - 1, groups=D)` cut to its first N outputs.

MinkowskiCausalConv1dFunction runs `CausalConv1d{Forward,Backward}GPU` (both host layers) on the kernels of
csrc/causal_conv1d.hip: float32 and bfloat16 rows, 2 to 4 taps, any channel count, fp32 arithmetic with one rounding at the
store, bitwise reproducible gradients.  `causal_conv1d` dispatches between them and `causal_conv1d_reference`, the same
formula with torch index operations (float64, CPU tensors, other widths)."""
import torch
from torch.autograd import Function

from .common import get_minkowski_function
from .selective_scan import _check_order, scan_sequence

ACTIVATIONS = (None, "silu")


def _check_activation(activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be None or 'silu', not {activation!r}")


def _weight_2d(weight):
    """[D, K] from [D, K] or conv1d's [D, 1, K]"""
    if weight.dim() == 3 and weight.shape[1] == 1:
        return weight[:, 0, :]
    if weight.dim() != 2:
        raise ValueError(f"weight must have the shape [D, K] or [D, 1, K], not {tuple(weight.shape)}")
    return weight


def causal_conv1d_reference(x, weight, bias=None, activation=None, seq_rows=None, starts=None):
    """The formula of the module docstring with torch index operations: K masked gathers that stop at the instance starts.
    In float64 when an operand is float64, else in the dtype of x (bfloat16 rounds after every tap); the result has the
    dtype of x.  seq_rows / starts: see scan_sequence (default: the rows in their own order, one instance)."""
    _check_activation(activation)
    n = x.shape[0]
    weight = _weight_2d(weight)
    k = weight.shape[1]
    if seq_rows is None:
        seq_rows = torch.arange(n, device=x.device)
    if starts is None:
        starts = torch.zeros(n, dtype=torch.bool, device=x.device)
        starts[:1] = True
    ops = [t for t in (x, weight, bias) if t is not None]
    work = torch.float64 if any(t.dtype == torch.float64 for t in ops) else x.dtype
    pos = torch.arange(n, device=x.device)
    rank = pos - torch.cummax(torch.where(starts, pos, torch.zeros_like(pos)), 0).values
    xs = x.to(work)[seq_rows]
    w = weight.to(work)                                                 # tap j back is w[:, k - 1 - j]
    acc = xs * w[:, k - 1]
    for j in range(1, k):
        back = xs[(pos - j).clamp(min=0)]
        acc = acc + torch.where((rank >= j)[:, None], back, torch.zeros_like(back)) * w[:, k - 1 - j]
    if bias is not None:
        acc = acc + bias.to(work)
    if activation == "silu":
        acc = torch.nn.functional.silu(acc)
    return torch.zeros_like(acc).index_copy(0, seq_rows, acc).to(x.dtype)


class MinkowskiCausalConv1dFunction(Function):
    """The causal conv1d on the kernels of csrc/causal_conv1d.hip.  x: (N, D) features on the map `coords_key` (a row view
    with a row stride is taken as it is); weight: (D, K) float32, K in 2..4; bias: (D,) float32 or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, activation, order, reverse, coords_key, coords_manager):
        _check_order(order)
        _check_activation(activation)
        ops = [None if t is None else t.detach() for t in (x, weight, bias)]
        fw_fn = get_minkowski_function("CausalConv1dForward", x, coords_key)
        y = fw_fn(*ops, activation, order, bool(reverse), coords_key, coords_manager._manager)
        ctx.save_for_backward(*ops)
        ctx.misc = (activation, order, bool(reverse), coords_key, coords_manager)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, bias = ctx.saved_tensors
        activation, order, reverse, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("CausalConv1dBackward", grad_out, coords_key)
        grads = bw_fn(x, weight, bias, grad_out, activation, order, reverse, coords_key, coords_manager._manager,
                      list(ctx.needs_input_grad[:3]))
        return (*grads, None, None, None, None, None)


# The kernels were faster than the torch formulation at every measured shape, so no width is left to torch.
def is_fused(x, weight, bias=None):
    """whether causal_conv1d runs these operands on the HIP kernels (else on causal_conv1d_reference)"""
    params = [t for t in (weight, bias) if t is not None]
    return (x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16) and
            all(t.dtype != torch.float64 for t in params) and weight.dim() in (2, 3) and 2 <= weight.shape[-1] <= 4)


def causal_conv1d(x, weight, bias=None, activation=None, order="z", reverse=False, coords_key=None, coords_manager=None,
                  fused=None):
    """The causal depthwise conv1d of the feature matrix x (N, D) that sits on the map `coords_key` of `coords_manager`,
    along the curve `order` of every instance.  weight: (D, K) or conv1d's (D, 1, K), any float dtype; bias: (D,) or None;
    activation: None or "silu".  fused: None picks the kernels where is_fused(...) says so, False forces the torch
    formulation, True makes an operand the kernels do not serve an error."""
    _check_order(order)
    _check_activation(activation)
    weight = _weight_2d(weight)
    if fused is None:
        fused = is_fused(x, weight, bias)
    if fused:                                     # the kernels take fp32 parameters; autograd casts the gradients back
        return MinkowskiCausalConv1dFunction.apply(x, weight.float().contiguous(), None if bias is None else bias.float(),
                                                   activation, order, reverse, coords_key, coords_manager)
    seq_rows, starts = scan_sequence(coords_key, coords_manager, order, reverse)
    return causal_conv1d_reference(x, weight, bias, activation, seq_rows.to(x.device), starts.to(x.device))
