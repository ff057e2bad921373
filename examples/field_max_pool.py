"""Per-voxel max of a TensorField (VoxelNet / PointNet-style encoders): quantise the field, then pool the points of each
voxel with MinkowskiDirectMaxPoolingFunction.  `TensorField.sparse(MAX_POOL)` is not wired to the function yet; these
three lines are what that mode does.

    python examples/field_max_pool.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


def voxel_max(field, tensor_stride=1):
    mgr = field.coordinate_manager
    stride = ME.convert_to_int_list(tensor_stride, field.D)
    key, (_, inverse) = mgr.field_to_sparse_insert_and_map(field.coordinate_field_map_key, stride)
    feats = ME.MinkowskiDirectMaxPoolingFunction.apply(torch.arange(len(field), device=field.device), inverse, field.F,
                                                       mgr.size(key))
    return ME.SparseTensor(feats, coordinate_map_key=key, coordinate_manager=mgr)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    coords = torch.cat([torch.randint(0, 2, (5000, 1), generator=g).float(), torch.rand(5000, 3, generator=g) * 12], 1)
    feats = torch.rand(5000, 8, generator=g).to(dev).requires_grad_(True)
    voxels = voxel_max(ME.TensorField(feats, coordinates=coords.to(dev)))
    voxels.F.sum().backward()
    print(f"{len(feats)} points -> {voxels.F.shape[0]} voxels; {int((feats.grad != 0).sum())} winning elements")
