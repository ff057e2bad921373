"""Generate the tensor-field fixtures (field_*.npz) with the reference's own CPU CoordinateMapManager.

The reference's manager (compiled unmodified into oracle/_ref/_C.so by oracle/build_ref.py, through oracle.ref) gives:
    insert_field(coords.float(), [1] * D)                      the field (MinkowskiTensorField.py __init__)
    field_to_sparse_insert_and_map(field_key, tensor_stride)   the sparse coordinates, unique_index, inverse_mapping
    interpolation_map_weight(queries, sparse_key)              the (in, out, weight) triples of the trilinear map
Each case also holds float64 restatements, over those reference maps, of
    interpolation forward  out[p] = sum_e w_e * x[in_e]  (e with out_e = p) and its backward  dx[r] = sum_e w_e * dy[out_e]
    UNWEIGHTED_AVERAGE sparse()  avg[v] = mean of the field features of voxel v, and its backward dF[i] = dy[v(i)] / n_v
Rows are in the reference's sparse row order; the tests relabel them with helpers.row_mapping.

Run where the reference's source tree is available:
    python tests/golden/make_golden_field.py
The .npz files are committed; tests never need the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref  # noqa: E402


def field_case(name, D, n, extent, batch, tensor_stride, c=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = ref.load()
    b = torch.randint(0, batch, (n, 1), generator=g).float()
    x = (torch.rand(n, D, generator=g) - 0.5) * 2 * extent          # negative coordinates included
    x[: n // 8] = torch.round(x[: n // 8])                          # points exactly on voxel boundaries
    coords = torch.cat([b, x], 1).float().contiguous()
    feats = torch.rand(n, c, generator=g) - 0.5
    mgr = C.CoordinateMapManagerCPU(C.MinkowskiAlgorithm.DEFAULT, 1)
    fkey = mgr.insert_field(coords, [1] * D, "")
    skey, (unique_map, inverse_map) = mgr.field_to_sparse_insert_and_map(fkey, list(tensor_stride), "")
    sparse_coords = mgr.get_coordinates(skey)
    ns = sparse_coords.shape[0]
    # queries: the field points, shifted points (some corners missing at the edges) and far points (no corner present)
    q = torch.cat([coords, coords[: n // 2] + torch.cat([torch.zeros(n // 2, 1), torch.full((n // 2, D), 0.37)], 1),
                   torch.cat([torch.zeros(8, 1), torch.full((8, D), 1000.5)], 1)], 0).contiguous()
    in_map, out_map, weights = mgr.interpolation_map_weight(q, skey)
    in_map, out_map, w = in_map.long().numpy(), out_map.long().numpy(), weights.double().numpy()
    sf = (torch.rand(ns, c, generator=g) - 0.5)
    dq = (torch.rand(q.shape[0], c, generator=g) - 0.5)
    xs, dy = sf.double().numpy(), dq.double().numpy()
    interp_out = np.zeros((q.shape[0], c))
    np.add.at(interp_out, out_map, w[:, None] * xs[in_map])
    interp_grad = np.zeros((ns, c))
    np.add.at(interp_grad, in_map, w[:, None] * dy[out_map])
    inv = inverse_map.long().numpy()
    cnt = np.bincount(inv, minlength=ns).astype(np.float64)
    avg = np.zeros((ns, c))
    np.add.at(avg, inv, feats.double().numpy())
    avg /= cnt[:, None]
    dv = (torch.rand(ns, c, generator=g) - 0.5)
    avg_grad = dv.double().numpy()[inv] / cnt[inv][:, None]
    out = os.path.join(HERE, f"field_{name}.npz")
    np.savez_compressed(
        out, D=D, tensor_stride=np.array(tensor_stride, np.int32), field_coords=coords.numpy(),
        field_feats=feats.numpy(), sparse_coords=sparse_coords.int().numpy(), unique_map=unique_map.long().numpy(),
        inverse_map=inv, queries=q.numpy(), ref_in=in_map, ref_out=out_map, ref_w=weights.numpy(),
        sparse_feats=sf.numpy(), grad_queries=dq.numpy(), interp_out=interp_out, interp_grad=interp_grad,
        avg_feats=avg, grad_sparse=dv.numpy(), avg_grad=avg_grad)
    print(f"{out}: {n} points, {ns} voxels, {len(in_map)} interpolation entries, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    field_case("2d_s1", 2, 1500, 8.0, 2, [1, 1], seed=1)
    field_case("3d_s1", 3, 2000, 5.0, 3, [1, 1, 1], seed=2)
    field_case("3d_s2", 3, 2000, 8.0, 2, [2, 2, 2], seed=3)
    field_case("3d_aniso", 3, 2000, 8.0, 2, [2, 4, 1], seed=4)
    field_case("4d_s1", 4, 1500, 2.0, 1, [1, 1, 1, 1], seed=5)
