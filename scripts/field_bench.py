"""Tensor fields (csrc/field.hip): time per call of the field operators on a ~250k-point field voxelised to a ~200k-voxel
scene, against a byte model and against the same operations written with torch (index_add_ / torch.sparse.mm on the same
maps) on the same GPU.

    python scripts/field_bench.py [--iters 30] [--json out.jsonl]

Operations, each timed whole as the autograd functions run it (CSR builds included; slice backward reuses the voxel
CSR that sparse() built, and is also shown with the CSR built anew): map build (TensorField + sparse()), interpolation
map, forward (map + gather) and backward (transpose + gather), sparse() UNWEIGHTED_AVERAGE forward / backward, slice
forward / backward; C = 20 and 96, fp32 and bf16.  The torch lines run on the precomputed maps.
Byte model of the gather-sum: e*C*(n_rows + n_distinct_cols) + 8*nnz (e = 4 fp32, 2 bf16); fraction of 6.3 TB/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME

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


def scene(dev, n_points=250000, seed=0):
    """points of a ~200k-voxel surface-like scene: 200k voxels of a 3-D grid, 1.25 points per voxel on average"""
    g = torch.Generator().manual_seed(seed)
    vox = torch.unique(torch.randint(0, 120, (int(1.7 * 200000), 3), generator=g), dim=0)[:200000]
    pick = torch.cat([torch.arange(vox.shape[0]), torch.randint(0, vox.shape[0], (n_points - vox.shape[0],), generator=g)])
    pts = vox[pick].double() + torch.rand(n_points, 3, generator=g, dtype=torch.float64)
    return torch.cat([torch.zeros(n_points, 1, dtype=torch.float64), pts], 1).float().to(dev)


def case(coords, C, dtype, iters, dev):
    e = 2 if dtype == torch.bfloat16 else 4
    f = torch.rand(coords.shape[0], C, device=dev).to(dtype).requires_grad_(True)
    B = ME.MinkowskiEngineBackend
    rows = []

    def rec(op, t, nbytes, t_torch=None):
        r = dict(op=op, C=C, dtype=str(dtype).split(".")[-1], us=round(t * 1e6, 1),
                 hbm_frac=round(nbytes / t / HBM, 3) if nbytes else None,
                 torch_us=round(t_torch * 1e6, 1) if t_torch else None)
        rows.append(r)
        print(json.dumps(r), flush=True)

    def build():
        tf = ME.TensorField(f, coordinates=coords)
        return tf, tf.sparse()

    t_build = timed(lambda: build(), max(3, iters // 5))
    tf, s = build()
    rec("map_build(sparse)", t_build, 0)
    mgr = tf.coordinate_manager._manager
    inv = tf.inverse_mapping(s.coordinate_map_key)
    n_p, n_v = coords.shape[0], s.F.shape[0]
    inv32 = inv.int()
    x = f.detach()

    # every timing below is the whole operator as the autograd functions run it, CSR builds included
    def avg_fwd():        # sparse() on a new map: the voxel CSR (stable radix sort), 1 / count, the gather-sum
        rowptr, cols, _ = B.CsrFromCooGPU(inv32, n_v)
        count = (rowptr[1:] - rowptr[:-1]).float()
        return B.CsrGatherGPU(x, rowptr, cols, None, 1.0 / count.clamp_min(1)), rowptr, cols, count

    _, rowptr, cols, count = avg_fwd()
    t = timed(avg_fwd, iters)
    t_t = timed(lambda: torch.zeros(n_v, C, device=dev, dtype=dtype).index_add_(0, inv, x) / count[:, None].to(dtype),
                iters)
    rec("sparse_avg_fwd(csr+gather)", t, e * C * (n_v + n_p) + 8 * n_p, t_t)
    ident = torch.arange(n_p + 1, dtype=torch.int32, device=dev)
    gy = torch.rand(n_v, C, device=dev).to(dtype)
    t = timed(lambda: B.CsrGatherGPU(gy, ident, inv32, None, (1.0 / count.clamp_min(1))[inv]), iters)
    t_t = timed(lambda: gy[inv] / count[inv][:, None].to(dtype), iters)
    rec("sparse_avg_bwd", t, e * C * (n_p + n_v) + 8 * n_p, t_t)
    # slice forward (gather by inverse_mapping); backward on the voxel CSR that sparse() built and the field keeps
    sv = s.F.detach()
    t = timed(lambda: B.CsrGatherGPU(sv, ident, inv32), iters)
    t_t = timed(lambda: sv[inv], iters)
    rec("slice_fwd", t, e * C * (n_p + n_v) + 8 * n_p, t_t)
    gp = torch.rand(n_p, C, device=dev).to(dtype)
    t = timed(lambda: B.CsrGatherGPU(gp, rowptr, cols), iters)
    t_t = timed(lambda: torch.zeros(n_v, C, device=dev, dtype=dtype).index_add_(0, inv, gp), iters)
    rec("slice_bwd(cached csr)", t, e * C * (n_v + n_p) + 8 * n_p, t_t)
    t = timed(lambda: B.CsrGatherGPU(gp, *B.CsrFromCooGPU(inv32, n_v)[:2]), iters)
    rec("slice_bwd(csr+gather)", t, e * C * (n_v + n_p) + 8 * n_p, t_t)
    # interpolation: the map, forward (map + gather, as InterpolationForwardGPU runs), backward (transpose + gather,
    # as InterpolationBackwardGPU runs); torch runs on the precomputed map (it needs the same map first)
    q = coords + 0.25
    t = timed(lambda: mgr._interpolation_map(s.coordinate_map_key, q), max(3, iters // 5))
    rec("interp_map", t, 0)
    im, om, w, rp = mgr._interpolation_map(s.coordinate_map_key, q)
    nnz = im.numel()
    Bh = ME.host.backend_of(mgr)
    t = timed(lambda: Bh.InterpolationForwardGPU(sv, q, s.coordinate_map_key, mgr), iters)
    A = torch.sparse_coo_tensor(torch.stack([om.long(), im.long()]), w, (n_p, n_v)).coalesce()
    t_t = timed(lambda: torch.sparse.mm(A, sv.float()), iters) if dtype == torch.float32 else None
    rec("interp_fwd(map+gather)", t, e * C * (n_p + n_v) + 8 * nnz, t_t)
    t = timed(lambda: B.CsrGatherGPU(sv, rp, im, w), iters)
    rec("interp_fwd(gather)", t, e * C * (n_p + n_v) + 8 * nnz, t_t)
    t = timed(lambda: Bh.InterpolationBackwardGPU(gp, im, om, w, s.coordinate_map_key, mgr), iters)
    t_t = timed(lambda: torch.zeros(n_v, C, device=dev, dtype=dtype).index_add_(0, im.long(), gp[om.long()] *
                                                                               w[:, None].to(dtype)), iters)
    rec("interp_bwd(transpose+gather)", t, e * C * (n_v + n_p) + 8 * nnz, t_t)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    coords = scene(dev)
    all_rows = []
    for C in (20, 96):
        for dt in (torch.float32, torch.bfloat16):
            all_rows += case(coords, C, dt, a.iters, dev)
    if a.json:
        with open(a.json, "w") as fh:
            for r in all_rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
