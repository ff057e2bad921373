"""Sparse matrix products on the deterministic CSR kernels of csrc/field.hip (reference:
MinkowskiEngine/sparse_matrix_functions.py, which runs cuSPARSE coo_spmm).  A COO matrix (rows, cols, vals) of shape
`size` is turned into rows by a stable radix sort (CsrFromCooGPU) and multiplied by a row-stationary gather-sum
(CsrGatherGPU): every row is summed in entry order, without atomics, so results are bitwise reproducible.  The backward
pass multiplies by the transpose, built the same way from the columns."""
import torch
from torch.autograd import Function

from . import host as _host


def _acc(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _check_coo(rows, cols, size, mat):
    """indices in range: a row >= size[0] would break the row pointer, a column >= size[1] read outside mat"""
    assert mat.is_cuda, "mat must be a CUDA (ROCm) tensor: the MI355X path has no CPU implementation"
    assert mat.dim() == 2 and mat.shape[0] == int(size[1]), "mat must be [size[1], C]"
    assert rows.numel() == cols.numel(), "rows and cols must have one entry each"
    for name, t, n in (("rows", rows, int(size[0])), ("cols", cols, int(size[1]))):
        if t.numel():
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= n:
                raise ValueError(f"{name} out of range [0, {n}): [{lo}, {hi}]")


def spmm(rows, cols, vals, size, mat, is_sorted=False, cuda_spmm_alg=1):
    """out [size[0], C] = COO(rows, cols, vals; size) @ mat"""
    assert len(rows) == len(cols) == len(vals), "rows, cols and vals must have one entry each"
    assert mat.is_cuda, "mat must be a CUDA (ROCm) tensor: the MI355X path has no CPU implementation"
    return _host.backend().coo_spmm_int32(rows, cols, vals, int(size[0]), int(size[1]), mat, cuda_spmm_alg, is_sorted)


def spmm_average(rows, cols, size, mat, cuda_spmm_alg=1):
    """(out, COO of the averaging matrix in row order): out[i] = mean of mat[cols] over the entries of row i"""
    assert mat.is_cuda, "mat must be a CUDA (ROCm) tensor: the MI355X path has no CPU implementation"
    out, r, c, v = _host.backend().coo_spmm_average_int32(rows, cols, int(size[0]), int(size[1]), mat, cuda_spmm_alg)
    return out, r, c, v


class MinkowskiSPMMFunction(Function):
    """out = A @ mat for A = COO(rows, cols, vals) of shape size; differentiable with respect to mat"""

    @staticmethod
    def forward(ctx, rows, cols, vals, size, mat, cuda_spmm_alg=1):
        _check_coo(rows, cols, size, mat)
        assert vals.numel() == rows.numel(), "vals must have one entry per (row, col)"
        B = _host.backend()
        vals = vals.to(_acc(mat))
        ctx.misc = (rows, cols, vals, size, B)
        rowptr, c, v = B.CsrFromCooGPU(rows, int(size[0]), cols, vals)
        return B.CsrGatherGPU(mat.contiguous(), rowptr, c, v)

    @staticmethod
    def backward(ctx, grad):
        rows, cols, vals, size, B = ctx.misc
        grad_mat = None
        if ctx.needs_input_grad[4]:
            rowptr, c, v = B.CsrFromCooGPU(cols, int(size[1]), rows, vals)
            grad_mat = B.CsrGatherGPU(grad.contiguous(), rowptr, c, v)
        return None, None, None, None, grad_mat, None


class MinkowskiSPMMAverageFunction(Function):
    """out[i] = mean over the entries (i, j) of mat[j]; differentiable with respect to mat"""

    @staticmethod
    def forward(ctx, rows, cols, size, mat, cuda_spmm_alg=1):
        _check_coo(rows, cols, size, mat)
        B = _host.backend()
        out, r, c, v = B.coo_spmm_average_int32(rows, cols, int(size[0]), int(size[1]), mat.contiguous(),
                                                cuda_spmm_alg)
        ctx.misc = (r, c, v, size, B)
        return out

    @staticmethod
    def backward(ctx, grad):
        r, c, v, size, B = ctx.misc
        grad_mat = None
        if ctx.needs_input_grad[3]:
            rowptr, cc, vv = B.CsrFromCooGPU(c, int(size[1]), r, v)
            grad_mat = B.CsrGatherGPU(grad.contiguous(), rowptr, cc, vv)
        return None, None, None, grad_mat, None
