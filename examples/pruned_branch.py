"""A two-branch block of a completion / generative network: one branch keeps every voxel, the other is pruned to the
voxels a classifier keeps and refined there; the pruned branch is then added back onto the dense one.  The two branches
live on different coordinate maps, so the `+` runs on the union of the maps (csrc/union_arith.hip).  The union map and
its row tables are kept per pair of maps: a second operator on the same two branches (the `*` gate below) builds nothing.

    python examples/pruned_branch.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class PrunedBranchBlock(nn.Module):
    def __init__(self, channels, D=3):
        super().__init__()
        self.trunk = nn.Sequential(ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D),
                                   ME.MinkowskiBatchNorm(channels), ME.MinkowskiReLU())
        self.keep = ME.MinkowskiConvolution(channels, 1, kernel_size=1, bias=True, dimension=D)
        self.prune = ME.MinkowskiPruning()
        self.refine = nn.Sequential(ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D),
                                    ME.MinkowskiBatchNorm(channels), ME.MinkowskiGELU())

    def forward(self, x):
        y = self.trunk(x)
        mask = self.keep(y).F.squeeze(1) > 0
        fine = self.refine(self.prune(y, mask))          # fewer voxels than y, a coordinate map of its own
        added = y + fine                                 # rows only y holds pass through unchanged
        gated = y * ME.MinkowskiFunctional.sigmoid(fine)  # (y's map, fine's map) again: the cached union, `added`'s key
        return added + gated                             # one shared map: plain addition of the features


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 40, (30000, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)
    x = ME.SparseTensor(torch.rand(pts.shape[0], 16, generator=g).to(dev), coords)
    block = PrunedBranchBlock(16).to(dev)
    out = block(x)
    out.F.square().mean().backward()
    keys = x.coordinate_manager.get_coordinate_map_keys(1)
    print(f"{len(x)} voxels in, {len(out)} out on {out.coordinate_map_key}; {len(keys)} stride-1 maps: the input, the "
          f"pruned branch, their union")
