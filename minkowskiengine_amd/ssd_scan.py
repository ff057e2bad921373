"""Mamba-2's state-space-dual scan (SSD; Dao & Gu 2024) over the serialized voxel order: the sequence of selective_scan
(every instance along a space-filling curve, a zero state at every instance start), with ONE decay per head instead of one
per channel and state, which turns a chunk of the recurrence into matrix products.  H heads of width P, S states, G groups;
head h reads group h // (H // G) of B and C:

    dt_t = dt[row_t, h] + dt_bias[h]                                  (softplus of that with dt_softplus)
    h_t  = exp(dt_t A[h]) h_{t-1} + dt_t B[row_t, g] (outer) x[row_t, h]          an S x P state per head
    out[row_t, h] = C[row_t, g] . h_t + D[h] x[row_t, h]

MinkowskiSSDScanFunction runs `SSDScan{Forward,Backward}GPU` (both host layers) on the MFMA kernels of csrc/ssd_scan.hip:
float32 and bfloat16 rows, P of 32 or 64, S of 64 or 128; gradients for all seven operands, bitwise reproducible.
`ssd_scan` dispatches between them and `ssd_scan_reference`, the same formulas written with torch operations position by
position (float64, CPU tensors, other widths: slow, a yardstick).  MinkowskiMamba2 is the Mamba-2 block on a SparseTensor
with the parameters and state dict of `mamba_ssm.Mamba2`."""
import math

import torch
from torch.autograd import Function

from .common import get_minkowski_function
from .selective_scan import _check_order, scan_sequence
from .sparse_tensor import SparseTensor


def ssd_scan_reference(x, dt, A, B, C, D=None, dt_bias=None, dt_softplus=False, headdim=64, ngroups=1, seq_rows=None,
                       starts=None):
    """The formulas of the module docstring with torch operations, one position after the other and with no chunks, in
    float64 when an operand is float64 and in float32 otherwise; the result has the dtype of x.  seq_rows / starts: see
    scan_sequence (default: the rows in their own order, one instance)."""
    n, p, g = x.shape[0], int(headdim), int(ngroups)
    h, s = x.shape[1] // p, B.shape[1] // g
    if seq_rows is None:
        seq_rows = torch.arange(n, device=x.device)
    if starts is None:
        starts = torch.zeros(n, dtype=torch.bool, device=x.device)
    ops = [t for t in (x, dt, A, B, C, D, dt_bias) if t is not None]
    work = torch.float64 if any(t.dtype == torch.float64 for t in ops) else torch.float32
    xw = x.to(work).view(n, h, p)
    Bw = B.to(work).view(n, g, s).repeat_interleave(h // g, 1)
    Cw = C.to(work).view(n, g, s).repeat_interleave(h // g, 1)
    dtw = dt.to(work)
    if dt_bias is not None:
        dtw = dtw + dt_bias.to(work)
    if dt_softplus:
        dtw = torch.nn.functional.softplus(dtw)
    decay = torch.exp(dtw * A.to(work))
    state = xw.new_zeros(h, s, p)
    ys = []
    for r, start in zip(seq_rows.tolist(), starts.tolist()):
        if start:
            state = torch.zeros_like(state)
        state = decay[r, :, None, None] * state + (dtw[r, :, None] * Bw[r])[:, :, None] * xw[r, :, None, :]
        ys.append((Cw[r, :, :, None] * state).sum(1))
    y = torch.zeros_like(xw)
    if n > 0:
        y = y.index_copy(0, seq_rows, torch.stack(ys))
    if D is not None:
        y = y + D.to(work)[:, None] * xw
    return y.reshape(n, h * p).to(x.dtype)


class MinkowskiSSDScanFunction(Function):
    """The SSD scan on the kernels of csrc/ssd_scan.hip.  x: (N, H P) features on the map `coords_key`, dt: (N, H), B, C:
    (N, G S) (row views with a row stride are taken as they are); A, D, dt_bias: (H,) float32; D and dt_bias may be None."""

    @staticmethod
    def forward(ctx, x, dt, A, B, C, D, dt_bias, dt_softplus, headdim, ngroups, order, reverse, coords_key, coords_manager):
        _check_order(order)
        ops = [None if t is None else t.detach() for t in (x, dt, A, B, C, D, dt_bias)]
        fw_fn = get_minkowski_function("SSDScanForward", x, coords_key)
        out, entry = fw_fn(*ops, bool(dt_softplus), int(headdim), int(ngroups), order, bool(reverse), coords_key,
                           coords_manager._manager)
        ctx.save_for_backward(*ops, entry)
        ctx.misc = (bool(dt_softplus), int(headdim), int(ngroups), order, bool(reverse), coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        *ops, entry = ctx.saved_tensors
        dt_softplus, headdim, ngroups, order, reverse, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("SSDScanBackward", grad_out, coords_key)
        grads = bw_fn(*ops, entry, grad_out, dt_softplus, headdim, ngroups, order, reverse, coords_key,
                      coords_manager._manager, list(ctx.needs_input_grad[:7]))
        return (*grads, None, None, None, None, None, None, None)


def is_fused(x, dt, A, B, C, D=None, dt_bias=None, headdim=64, ngroups=1):
    """whether ssd_scan runs these operands on the HIP kernels (else on ssd_scan_reference)"""
    params = [t for t in (A, D, dt_bias) if t is not None]
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and all(t.dtype == x.dtype for t in (dt, B, C)) and
            all(t.dtype == torch.float32 for t in params) and headdim in (32, 64) and x.shape[1] % headdim == 0 and
            B.shape[1] % ngroups == 0 and B.shape[1] // ngroups in (64, 128) and (x.shape[1] // headdim) % ngroups == 0)


def ssd_scan(x, dt, A, B, C, D=None, dt_bias=None, dt_softplus=False, headdim=64, ngroups=1, order="z", reverse=False,
             coords_key=None, coords_manager=None, fused=None):
    """The SSD scan of the feature matrices x (N, H headdim), dt (N, H) and B, C (N, ngroups S) that sit on the map
    `coords_key` of `coords_manager`, along the curve `order` of every instance.  fused: None picks the kernels where
    is_fused(...) says so, False forces the torch formulation, True makes an operand the kernels do not serve an error."""
    if fused is None:
        fused = is_fused(x, dt, A, B, C, D, dt_bias, headdim, ngroups)
    if fused:
        return MinkowskiSSDScanFunction.apply(x, dt, A, B, C, D, dt_bias, dt_softplus, headdim, ngroups, order, reverse,
                                              coords_key, coords_manager)
    seq_rows, starts = scan_sequence(coords_key, coords_manager, order, reverse)
    return ssd_scan_reference(x, dt, A, B, C, D, dt_bias, dt_softplus, headdim, ngroups, seq_rows.to(x.device),
                              starts.to(x.device))


class MinkowskiMamba2(torch.nn.Module):
    r"""The Mamba-2 block (Dao & Gu 2024) on a SparseTensor: the sequence of an instance is its voxels along the curve
    `order` ("z", "z_trans", "hilbert" or "hilbert_trans"); the result sits on the input's coordinate map.  The parameters
    are those of `mamba_ssm.Mamba2` (in_proj, conv1d, dt_bias, A_log, D, norm.weight, out_proj), so a state dict in that
    layout loads strictly.  `bidirectional=True` adds a second scan that walks the same order backwards over the same
    projections and the same conv output; the two results are summed before the gated norm.

    The scan runs on the HIP kernels (headdim 32 or 64, d_state 64 or 128, float32 / bfloat16), the causal conv1d on
    `causal_conv1d`, the norm on the package's RMS norm; `fused = False`, CPU tensors and float64 run the torch formulations
    of all three."""

    def __init__(self, d_model, d_state=128, d_conv=4, expand=2, headdim=64, ngroups=1, order="z", bidirectional=False,
                 bias=False, conv_bias=True, dt_min=0.001, dt_max=0.1, dt_init_floor=1e-4):
        super().__init__()
        from .normalization import MinkowskiRMSNorm
        _check_order(order)
        self.d_model, self.d_state, self.d_conv, self.expand = int(d_model), int(d_state), int(d_conv), int(expand)
        self.headdim, self.ngroups = int(headdim), int(ngroups)
        self.d_inner = self.expand * self.d_model
        assert self.d_inner % self.headdim == 0, "expand * d_model must be a multiple of headdim"
        self.nheads = self.d_inner // self.headdim
        assert self.nheads % self.ngroups == 0, "ngroups must divide the number of heads"
        self.order, self.bidirectional = order, bool(bidirectional)
        self.fused = None               # see ssd_scan
        gs = self.ngroups * self.d_state
        self.in_proj = torch.nn.Linear(self.d_model, 2 * self.d_inner + 2 * gs + self.nheads, bias=bias)
        self.conv1d = torch.nn.Conv1d(self.d_inner + 2 * gs, self.d_inner + 2 * gs, kernel_size=self.d_conv,
                                      groups=self.d_inner + 2 * gs, padding=self.d_conv - 1, bias=conv_bias)
        dt = torch.exp(torch.rand(self.nheads) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
        dt = dt.clamp(min=dt_init_floor)
        self.dt_bias = torch.nn.Parameter(dt + torch.log(-torch.expm1(-dt)))     # the inverse of softplus
        self.dt_bias._no_weight_decay = True
        self.A_log = torch.nn.Parameter(torch.log(torch.empty(self.nheads).uniform_(1, 16)))
        self.A_log._no_weight_decay = True
        self.D = torch.nn.Parameter(torch.ones(self.nheads))
        self.D._no_weight_decay = True
        self.norm = MinkowskiRMSNorm(self.d_inner, eps=1e-5)
        self.out_proj = torch.nn.Linear(self.d_inner, self.d_model, bias=bias)

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.d_model}, d_state={self.d_state}, d_conv={self.d_conv}, "
                f"expand={self.expand}, headdim={self.headdim}, ngroups={self.ngroups}, order={self.order!r}, "
                f"bidirectional={self.bidirectional})")

    def forward(self, input):
        from .causal_conv1d import causal_conv1d
        from .MinkowskiFunctional import rms_norm
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.d_model, f"Channel size mismatch {self.d_model} != {input.shape[1]}"
        key, manager = input.coordinate_map_key, input._manager
        di, gs = self.d_inner, self.ngroups * self.d_state
        zxbcdt = self.in_proj(input.F)
        z, xBC, dt = zxbcdt[:, :di], zxbcdt[:, di:2 * di + 2 * gs], zxbcdt[:, 2 * di + 2 * gs:]
        xBC = causal_conv1d(xBC, self.conv1d.weight, self.conv1d.bias, "silu", self.order, False, key, manager,
                            fused=self.fused)
        x, B, C = xBC[:, :di], xBC[:, di:di + gs], xBC[:, di + gs:]
        A = -torch.exp(self.A_log.float())
        y = None
        for reverse in (False, True) if self.bidirectional else (False,):
            yr = ssd_scan(x, dt, A, B, C, self.D.float(), self.dt_bias.float(), True, self.headdim, self.ngroups, self.order,
                          reverse, key, manager, fused=self.fused)
            y = yr if y is None else y + yr
        y = y * torch.nn.functional.silu(z)
        if self.fused is False or not y.is_cuda or y.dtype == torch.float64:
            y = torch.nn.functional.rms_norm(y, (di,), self.norm.weight.to(y.dtype), 1e-5)
        else:
            y = rms_norm(SparseTensor(y, coordinate_map_key=key, coordinate_manager=manager), self.norm.weight, 1e-5).F
        return SparseTensor(self.out_proj(y), coordinate_map_key=key, coordinate_manager=manager)
