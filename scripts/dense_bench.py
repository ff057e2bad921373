"""Dense <-> sparse conversion (csrc/dense.hip): time per call of `SparseTensor.dense()` forward and forward + backward,
of `ME.to_sparse` and of `ME.to_sparse_all`, next to the reference's own formulation in torch on the same GPU in the same
process, alternating: `torch.zeros(shape)` + advanced-index assignment and its autograd backward for dense();
`abs().sum(ch)` / `torch.where` / `stack` / index for to_sparse; `permute + reshape` and the numpy mesh-grid upload for
to_sparse_all.  The two movers are also timed alone under each forced policy, for the policy's crossover.

    python scripts/dense_bench.py [--iters 50] [--repeats 3] [--json out.jsonl] [--small]

Shapes: (a) 100k rows x C 64 in 1 x 70^3 (occupancy 0.29); (b) 100k rows x C 64 in 1 x 215^3 (occupancy 0.01; the box is
2.5 GB in fp32); (c) 200k rows x C 96 bf16 in 2 x 128^3; (d) 3 x 4 x 11^4 to_sparse_all; (e) to_sparse of (a)'s box.
Byte model (compulsory traffic, e = bytes per element): cell-stationary rows -> box or box -> rows
e*cells*C + e*N*C + 4*cells (box once, rows once, grid once); the grid build adds 4*cells + 8*N; row-stationary
box -> rows e*N*C twice (the gather's 64-byte sectors are what it really moves).  Fraction of 6.3 TB/s.  Every figure is
the minimum over --repeats rounds of --iters calls; `spread` is (max - min) / min over the rounds of our own call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import backend

HBM = 6.3e12


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def alternate(fns, iters, repeats):
    """{name: [seconds per round]} with the candidates taking turns inside every round"""
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters))
    return out


def cloud(n, extent, batch, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    lin = torch.randperm(batch * extent ** 3, generator=g)[:n]
    c = torch.stack([lin // extent ** 3, (lin // extent ** 2) % extent, (lin // extent) % extent, lin % extent], 1)
    return c.int().to(dev)


def torch_dense(feats, coords, shape):
    out = torch.zeros(shape, dtype=feats.dtype, device=feats.device)
    t = coords[:, 1:].t().long()
    out[(coords[:, 0].long(), slice(None)) + tuple(t)] = feats
    return out


def torch_to_sparse(x):
    b = torch.where(x.abs().sum(1) != 0)
    feats = torch.zeros((len(b[0]), x.size(1)), dtype=x.dtype, device=x.device)
    feats[:] = x[(b[0], slice(None)) + tuple(b[1:])]
    return torch.stack(b, 1).int(), feats


def numpy_coordinates(shape):
    size = [shape[0]] + list(shape[2:])
    return torch.from_numpy(np.stack([s.reshape(-1) for s in np.meshgrid(*(np.linspace(0, s - 1, s) for s in size),
                                                                         indexing="ij")], 1)).int()


def best(ts):
    return min(ts)


def dense_case(name, n, c, batch, extent, dtype, iters, repeats, dev):
    e = torch.empty(0, dtype=dtype).element_size()
    coords = cloud(n, extent, batch, dev)
    shape = torch.Size([batch, c] + [extent] * 3)
    cells = batch * extent ** 3
    feats = torch.randn(n, c, device=dev).to(dtype).requires_grad_(True)
    x = ME.SparseTensor(feats, coords)
    gout = torch.randn(shape, device=dev).to(dtype)
    feats_t = feats.detach().clone().requires_grad_(True)

    def ours_fwd():
        return x.dense(shape=shape, min_coordinate=0)[0]

    def ours_step():
        feats.grad = None
        ours_fwd().backward(gout)

    def torch_step():
        feats_t.grad = None
        torch_dense(feats_t, coords, shape).backward(gout)

    ours_step(), torch_step()
    assert torch.equal(ours_fwd().detach(), torch_dense(feats_t.detach(), coords, shape))
    assert torch.equal(feats.grad, feats_t.grad)
    r = alternate(dict(ours_fwd=ours_fwd, torch_fwd=lambda: torch_dense(feats_t.detach(), coords, shape),
                       ours_step=ours_step, torch_step=torch_step), iters, repeats)
    # the movers alone, each policy forced, on prepared indices
    cell, grid, _ = backend.DenseCellIndexGPU(coords, [0] * 3, [1] * 3, [batch] + [extent] * 3, True)
    f = feats.detach()
    inner = extent ** 3
    k = alternate(dict(
        to_box_cell=lambda: backend.DenseRowsToBoxGPU(f, cell, grid, batch, inner, 2),
        to_box_row=lambda: backend.DenseRowsToBoxGPU(f, cell, None, batch, inner, 1),
        to_rows_cell=lambda: backend.DenseBoxToRowsGPU(gout, cell, grid, n, batch, inner, 2),
        to_rows_row=lambda: backend.DenseBoxToRowsGPU(gout, cell, None, n, batch, inner, 1),
        index_and_grid=lambda: backend.DenseCellIndexGPU(coords, [0] * 3, [1] * 3, [batch] + [extent] * 3, True),
        torch_zeros=lambda: torch.zeros(shape, dtype=dtype, device=dev)), iters, repeats)
    model = e * cells * c + e * n * c + 4 * cells
    row = dict(case=name, dtype=str(dtype).split(".")[-1], n=n, C=c, box=list(shape), occupancy=round(n / cells, 4),
               policy_to_box=backend.DensePolicy(n, cells, c, e, True), policy_to_rows=backend.DensePolicy(n, cells, c, e, False),
               model_MB=round(model / 1e6, 1))
    for key, ts in list(r.items()) + list(k.items()):
        row[key + "_us"] = round(best(ts) * 1e6, 1)
    for key in ("ours_fwd", "ours_step"):
        row[key + "_spread"] = round((max(r[key]) - min(r[key])) / min(r[key]), 3)
    row["to_box_cell_hbm_frac"] = round(model / best(k["to_box_cell"]) / HBM, 3)
    row["to_rows_cell_hbm_frac"] = round(model / best(k["to_rows_cell"]) / HBM, 3)
    row["fwd_ratio_torch_over_ours"] = round(best(r["torch_fwd"]) / best(r["ours_fwd"]), 2)
    row["step_ratio_torch_over_ours"] = round(best(r["torch_step"]) / best(r["ours_step"]), 2)
    return row


def to_sparse_case(name, n, c, batch, extent, dtype, iters, repeats, dev):
    coords = cloud(n, extent, batch, dev)
    shape = torch.Size([batch, c] + [extent] * 3)
    base = torch_dense(torch.randn(n, c, device=dev).to(dtype) + 3, coords, shape)
    x = base.clone().requires_grad_(True)
    xt = base.clone().requires_grad_(True)
    gout = torch.randn(n, c, device=dev).to(dtype)

    def ours_step():
        x.grad = None
        ME.to_sparse(x).F.backward(gout)

    def torch_step():
        xt.grad = None
        co, f = torch_to_sparse(xt)
        ME.SparseTensor(f, co).F.backward(gout)

    ours_step(), torch_step()
    assert torch.equal(x.grad, xt.grad)
    r = alternate(dict(ours_fwd=lambda: ME.to_sparse(x.detach()), ours_step=ours_step,
                       torch_fwd=lambda: ME.SparseTensor(*reversed(torch_to_sparse(xt.detach()))), torch_step=torch_step),
                  iters, repeats)
    row = dict(case=name, dtype=str(dtype).split(".")[-1], n=n, C=c, box=list(shape))
    for key, ts in r.items():
        row[key + "_us"] = round(best(ts) * 1e6, 1)
    for key in ("ours_fwd", "ours_step"):
        row[key + "_spread"] = round((max(r[key]) - min(r[key])) / min(r[key]), 3)
    row["fwd_ratio_torch_over_ours"] = round(best(r["torch_fwd"]) / best(r["ours_fwd"]), 2)
    row["step_ratio_torch_over_ours"] = round(best(r["torch_step"]) / best(r["ours_step"]), 2)
    return row


def to_sparse_all_case(name, shape, iters, repeats, dev):
    x = torch.randn(shape, device=dev, requires_grad=True)
    xt = x.detach().clone().requires_grad_(True)
    d = len(shape) - 2
    gout = torch.randn(x.numel() // shape[1], shape[1], device=dev)

    def torch_fwd(t):
        return ME.SparseTensor(t.permute(0, *range(2, 2 + d), 1).reshape(-1, shape[1]), numpy_coordinates(shape),
                               device=dev)

    def ours_step():
        x.grad = None
        ME.to_sparse_all(x).F.backward(gout)

    def torch_step():
        xt.grad = None
        torch_fwd(xt).F.backward(gout)

    ours_step(), torch_step()
    assert torch.equal(x.grad, xt.grad)
    r = alternate(dict(ours_fwd=lambda: ME.to_sparse_all(x.detach()), ours_step=ours_step,
                       torch_fwd=lambda: torch_fwd(xt.detach()), torch_step=torch_step,
                       ours_coordinates=lambda: ME.dense_coordinates(shape, device=dev),
                       numpy_coordinates=lambda: numpy_coordinates(shape).to(dev)), iters, repeats)
    row = dict(case=name, dtype="float32", box=list(shape))
    for key, ts in r.items():
        row[key + "_us"] = round(best(ts) * 1e6, 1)
    for key in ("ours_fwd", "ours_step"):
        row[key + "_spread"] = round((max(r[key]) - min(r[key])) / min(r[key]), 3)
    row["fwd_ratio_torch_over_ours"] = round(best(r["torch_fwd"]) / best(r["ours_fwd"]), 2)
    row["step_ratio_torch_over_ours"] = round(best(r["torch_step"]) / best(r["ours_step"]), 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", action="store_true", help="(b) with C 16: a 640 MB box")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [dense_case("a_70^3", 100000, 64, 1, 70, torch.float32, args.iters, args.repeats, dev),
            dense_case("b_215^3", 100000, 16 if args.small else 64, 1, 215, torch.float32, max(5, args.iters // 5),
                       args.repeats, dev),
            dense_case("c_2x128^3", 200000, 96, 2, 128, torch.bfloat16, max(5, args.iters // 2), args.repeats, dev),
            to_sparse_all_case("d_3x4x11^4", (3, 4, 11, 11, 11, 11), args.iters, args.repeats, dev),
            to_sparse_case("e_to_sparse_70^3", 100000, 64, 1, 70, torch.float32, max(5, args.iters // 2), args.repeats, dev)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
