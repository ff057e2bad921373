"""Arithmetic between two sparse tensors on DIFFERENT coordinate maps (reference: MinkowskiTensor._binary_functor,
MinkowskiTensor.py:511-546): the result lives on the union of the two maps.  One fused HIP pass writes every union row
once (csrc/union_arith.hip); the union map and its row tables are built once per ordered pair of keys and kept by the
coordinate manager, so `(a + b).coordinate_map_key == (a - b).coordinate_map_key` (the reference registers a new map
per call: README, drop-in limits)."""
import torch
from torch.autograd import Function

from . import host as _host

_OPS = {torch.add: "add", torch.sub: "sub", torch.mul: "mul", torch.div: "div"}


class MinkowskiUnionArithmeticFunction(Function):
    """out = a (op) b over the union: fn(a, b) on shared rows, a's row where only a holds it, fn(0, b) where only b
    does.  The backward pass is one gather launch per input that needs a gradient."""

    @staticmethod
    def forward(ctx, a_feat, b_feat, op, tables, backend):
        u_of_a, u_of_b, a_of_u, b_of_u = tables
        a_feat, b_feat = a_feat.contiguous(), b_feat.contiguous()
        out = backend.union_arith_fw(a_feat, b_feat, a_of_u, b_of_u, op)
        ctx.op, ctx.tables, ctx.backend = op, tables, backend
        ctx.save_for_backward(a_feat, b_feat)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        a_feat, b_feat = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_a, grad_b = ctx.backend.union_arith_bw(grad_out.contiguous(), a_feat, b_feat, *ctx.tables, ctx.op,
                                                    need_a, need_b)
        return grad_a, grad_b, None, None, None


def union_arithmetic(a, b, op):
    """`a (op) b` for two SparseTensors of one manager whose coordinate map keys differ; op: torch.add / sub / mul /
    div or "add" / "sub" / "mul" / "div"."""
    from .sparse_tensor import SparseTensor
    op = _OPS.get(op, op)
    assert op in _OPS.values(), f"unsupported operator {op!r}"
    assert a._manager is b._manager, "coordinate managers must match"
    assert a.F.is_cuda and b.F.is_cuda, "arithmetic across coordinate maps needs GPU tensors (no CPU path)"
    assert a.F.shape[1] == b.F.shape[1], f"channel counts differ: {a.F.shape[1]} and {b.F.shape[1]}"
    assert a.F.dtype == b.F.dtype, f"feature dtypes differ: {a.F.dtype} and {b.F.dtype}"
    manager = a._manager
    # (the manager checks that both maps exist and share a tensor stride)
    out_key, *tables = manager._manager.union_arith_maps(a.coordinate_map_key, b.coordinate_map_key)
    backend = _host.backend_of(manager)
    out = MinkowskiUnionArithmeticFunction.apply(a.F, b.F, op, tuple(tables), backend)
    return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=manager)
