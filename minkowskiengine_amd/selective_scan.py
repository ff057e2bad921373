"""Selective state-space scan (Mamba's S6) over the serialized voxel order — the token mixer of Voxel Mamba, LION,
PointMamba, Mamba3D and Serialized Point Mamba: the voxels of every instance are ordered along a space-filling curve (the
orders of serialized attention) and a linear recurrence with input-dependent step, input and output matrices runs along
that sequence, starting from a zero state in every instance:

    dt_t = delta[row_t] + delta_bias                       (softplus of that with delta_softplus)
    h_t  = exp(dt_t A) h_{t-1} + dt_t B[row_t] u[row_t]    per channel d and state s
    out[row_t] = (C[row_t] . h_t + Dskip u[row_t]) * silu(z[row_t])

MinkowskiSelectiveScanFunction runs `SelectiveScan{Forward,Backward}GPU` (both host layers) on the kernels of
csrc/selective_scan.hip: float32 and bfloat16 rows, 8 or 16 states, any channel count; gradients for all eight operands,
bitwise reproducible.  `selective_scan` dispatches between them and `selective_scan_reference`, the same formulas written
with torch operations position by position (float64, CPU tensors, other state counts, mixed dtypes: slow, a yardstick).
MinkowskiMamba is the Mamba block on a SparseTensor with the parameters and state dict of `mamba_ssm.Mamba`."""
import math

import torch
from torch.autograd import Function

from .common import get_minkowski_function
from .serialized_attention import SERIAL_ORDERS
from .sparse_tensor import SparseTensor


def _check_order(order):
    if order not in SERIAL_ORDERS:
        raise ValueError(f"order must be one of {SERIAL_ORDERS}, not {order!r}")


def scan_sequence(coords_key, coords_manager, order="z", reverse=False):
    """-> (seq_rows int64 [N], starts bool [N]): the row of every sequence position (every instance along the curve `order`,
    instance after instance; the whole list backwards with `reverse`) and whether the position starts an instance."""
    _check_order(order)
    seq_rows = coords_manager._manager._patch_rows(coords_key, 1, order)[1].long()
    if reverse:
        seq_rows = seq_rows.flip(0)
    inst = coords_manager._manager._origin_rows(coords_key).long()[seq_rows]
    starts = torch.ones_like(inst, dtype=torch.bool)
    starts[1:] = inst[1:] != inst[:-1]
    return seq_rows, starts


def selective_scan_reference(u, delta, A, B, C, Dskip=None, z=None, delta_bias=None, delta_softplus=False, seq_rows=None,
                             starts=None):
    """The formulas of the module docstring with torch operations, one position after the other and with no chunks, in
    float64 when an operand is float64 and in float32 otherwise; the result has the dtype of u.  seq_rows / starts: see
    scan_sequence (default: the rows in their own order, one instance)."""
    n, d = u.shape
    if seq_rows is None:
        seq_rows = torch.arange(n, device=u.device)
    if starts is None:
        starts = torch.zeros(n, dtype=torch.bool, device=u.device)
    ops = [t for t in (u, delta, A, B, C, Dskip, z, delta_bias) if t is not None]
    work = torch.float64 if any(t.dtype == torch.float64 for t in ops) else torch.float32
    uw, A, B, C = u.to(work), A.to(work), B.to(work), C.to(work)
    dt = delta.to(work)
    if delta_bias is not None:
        dt = dt + delta_bias.to(work)
    if delta_softplus:
        dt = torch.nn.functional.softplus(dt)
    x = dt * uw
    h = torch.zeros_like(A)
    ys = []
    for r, start in zip(seq_rows.tolist(), starts.tolist()):
        if start:
            h = torch.zeros_like(A)
        h = torch.exp(dt[r, :, None] * A) * h + x[r, :, None] * B[r, None, :]
        ys.append(h @ C[r])
    y = torch.zeros_like(uw)
    if n > 0:
        y = y.index_copy(0, seq_rows, torch.stack(ys))
    if Dskip is not None:
        y = y + Dskip.to(work) * uw
    if z is not None:
        y = y * torch.nn.functional.silu(z.to(work))
    return y.to(u.dtype)


class MinkowskiSelectiveScanFunction(Function):
    """The selective scan on the kernels of csrc/selective_scan.hip.  u, delta, z: (N, D) features on the map `coords_key`
    (row views with a row stride are taken as they are); B, C: (N, S); A: (D, S) float32; Dskip, delta_bias: (D,) float32;
    z, Dskip and delta_bias may be None.  S must be 8 or 16, the rows float32 or bfloat16."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, Dskip, z, delta_bias, delta_softplus, order, reverse, coords_key, coords_manager):
        _check_order(order)
        ops = [None if t is None else t.detach() for t in (u, delta, A, B, C, Dskip, z, delta_bias)]
        fw_fn = get_minkowski_function("SelectiveScanForward", u, coords_key)
        out, entry = fw_fn(*ops, bool(delta_softplus), order, bool(reverse), coords_key, coords_manager._manager)
        ctx.save_for_backward(*ops, entry)
        ctx.misc = (bool(delta_softplus), order, bool(reverse), coords_key, coords_manager)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        *ops, entry = ctx.saved_tensors
        delta_softplus, order, reverse, coords_key, coords_manager = ctx.misc
        bw_fn = get_minkowski_function("SelectiveScanBackward", grad_out, coords_key)
        grads = bw_fn(*ops, entry, grad_out, delta_softplus, order, reverse, coords_key, coords_manager._manager,
                      list(ctx.needs_input_grad[:8]))
        return (*grads, None, None, None, None, None)


def is_fused(u, delta, A, B, C, Dskip=None, z=None, delta_bias=None):
    """whether selective_scan runs these operands on the HIP kernels (else on selective_scan_reference)"""
    rows = [t for t in (u, delta, B, C, z) if t is not None]
    params = [t for t in (A, Dskip, delta_bias) if t is not None]
    return (u.is_cuda and u.dtype in (torch.float32, torch.bfloat16) and all(t.dtype == u.dtype for t in rows) and
            all(t.dtype == torch.float32 for t in params) and A.dim() == 2 and A.shape[1] in (8, 16))


def selective_scan(u, delta, A, B, C, Dskip=None, z=None, delta_bias=None, delta_softplus=False, order="z", reverse=False,
                   coords_key=None, coords_manager=None, fused=None):
    """The selective scan of the feature matrices u, delta, z (N, D) and B, C (N, S) that sit on the map `coords_key` of
    `coords_manager`, along the curve `order` of every instance.  fused: None picks the kernels where is_fused(...) says
    so, False forces the torch formulation, True makes an operand the kernels do not serve an error."""
    if fused is None:
        fused = is_fused(u, delta, A, B, C, Dskip, z, delta_bias)
    if fused:
        return MinkowskiSelectiveScanFunction.apply(u, delta, A, B, C, Dskip, z, delta_bias, delta_softplus, order, reverse,
                                                    coords_key, coords_manager)
    seq_rows, starts = scan_sequence(coords_key, coords_manager, order, reverse)
    return selective_scan_reference(u, delta, A, B, C, Dskip, z, delta_bias, delta_softplus, seq_rows.to(u.device),
                                    starts.to(u.device))


class MinkowskiMamba(torch.nn.Module):
    r"""The Mamba block (Gu & Dao 2023) on a SparseTensor: the sequence of an instance is its voxels along the curve
    `order` ("z", "z_trans", "hilbert" or "hilbert_trans"); the result sits on the input's coordinate map.  The parameters
    and their initialisation are those of `mamba_ssm.Mamba` (in_proj, conv1d, x_proj, dt_proj, A_log, D, out_proj), so a
    state dict in that layout loads strictly.  `bidirectional=True` adds a second scan that walks the same order backwards
    over the same projections; the two results are summed before out_proj.

    The scan runs on the HIP kernels (d_state 8 or 16, float32 / bfloat16), and so does the causal depthwise conv1d with
    its SiLU along the same sequence (`causal_conv1d`, d_conv 2 to 4); one forward-direction conv feeds both scans of a
    bidirectional block.  `fused = False` and float64 run the torch formulations of both."""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", order="z", bidirectional=False, bias=False,
                 conv_bias=True, dt_min=0.001, dt_max=0.1, dt_init_floor=1e-4):
        super().__init__()
        _check_order(order)
        self.d_model, self.d_state, self.d_conv, self.expand = int(d_model), int(d_state), int(d_conv), int(expand)
        self.d_inner = self.expand * self.d_model
        self.dt_rank = math.ceil(self.d_model / 16) if dt_rank == "auto" else int(dt_rank)
        self.order, self.bidirectional = order, bool(bidirectional)
        self.fused = None               # see selective_scan
        self.in_proj = torch.nn.Linear(self.d_model, 2 * self.d_inner, bias=bias)
        self.conv1d = torch.nn.Conv1d(self.d_inner, self.d_inner, kernel_size=self.d_conv, groups=self.d_inner,
                                      padding=self.d_conv - 1, bias=conv_bias)
        self.x_proj = torch.nn.Linear(self.d_inner, self.dt_rank + 2 * self.d_state, bias=False)
        self.dt_proj = torch.nn.Linear(self.dt_rank, self.d_inner, bias=True)
        std = self.dt_rank ** -0.5
        torch.nn.init.uniform_(self.dt_proj.weight, -std, std)
        dt = torch.exp(torch.rand(self.d_inner) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
        dt = dt.clamp(min=dt_init_floor)
        with torch.no_grad():
            self.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))     # the inverse of softplus
        self.dt_proj.bias._no_reinit = True
        A = torch.arange(1, self.d_state + 1, dtype=torch.float32).repeat(self.d_inner, 1)
        self.A_log = torch.nn.Parameter(torch.log(A))
        self.A_log._no_weight_decay = True
        self.D = torch.nn.Parameter(torch.ones(self.d_inner))
        self.D._no_weight_decay = True
        self.out_proj = torch.nn.Linear(self.d_inner, self.d_model, bias=bias)

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.d_model}, d_state={self.d_state}, d_conv={self.d_conv}, "
                f"expand={self.expand}, dt_rank={self.dt_rank}, order={self.order!r}, bidirectional={self.bidirectional})")

    def forward(self, input):
        from .causal_conv1d import causal_conv1d
        if not isinstance(input, SparseTensor):
            raise TypeError(f"{self.__class__.__name__} takes a SparseTensor, not a {type(input).__name__} "
                            "(quantise a TensorField with .sparse() first)")
        assert input.shape[1] == self.d_model, f"Channel size mismatch {self.d_model} != {input.shape[1]}"
        key, manager = input.coordinate_map_key, input._manager
        xz = self.in_proj(input.F)
        x, z = xz[:, :self.d_inner], xz[:, self.d_inner:]
        x = causal_conv1d(x, self.conv1d.weight, self.conv1d.bias, "silu", self.order, False, key, manager, fused=self.fused)
        x_dbl = self.x_proj(x)
        dt = torch.nn.functional.linear(x_dbl[:, :self.dt_rank], self.dt_proj.weight)
        B = x_dbl[:, self.dt_rank:self.dt_rank + self.d_state]
        C = x_dbl[:, self.dt_rank + self.d_state:]
        A = -torch.exp(self.A_log.float())
        y = None
        for reverse in (False, True) if self.bidirectional else (False,):
            yr = selective_scan(x, dt, A, B, C, self.D.float(), z, self.dt_proj.bias.float(), True, self.order, reverse, key,
                                manager, fused=self.fused)
            y = yr if y is None else y + yr
        return SparseTensor(self.out_proj(y), coordinate_map_key=key, coordinate_manager=manager)
