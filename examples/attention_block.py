"""The attention block of the coarse levels of a sparse diffusion or completion U-Net: GroupNorm -> multi-head
self-attention -> residual.  At tensor stride 8 or 16 a scene holds a few hundred to a few thousand voxels, and every voxel
attends to the voxels of its own scene (batch index) and to no others.  MinkowskiSelfAttention does that on the rows of the
sparse tensor as they are — scenes of different sizes, rows in any order, no padding and no Python loop over the scenes —
with torch.nn.MultiheadAttention's parameters, and its gradients are bitwise reproducible (csrc/attention.hip, DESIGN
8.11).

    python examples/attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class AttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, groups=8):
        super().__init__()
        self.norm = ME.MinkowskiGroupNorm(groups, channels)
        self.attn = ME.MinkowskiSelfAttention(channels, num_heads)

    def forward(self, x):
        return self.attn(self.norm(x)) + x               # the same coordinate map: plain addition of the features


def coarse_level(x, levels=3, D=3):
    """the tensor-stride-2^levels map of x with averaged features: where a U-Net puts its attention blocks"""
    pool = ME.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=D)
    for _ in range(levels):
        x = pool(x)
    return x


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    scenes = []
    for b, (k, extent) in enumerate(((60000, 96), (20000, 64))):     # two scenes of different sizes
        pts = torch.unique(torch.randint(0, extent, (k, 3), generator=g), dim=0)
        scenes.append(torch.cat([torch.full((pts.shape[0], 1), b, dtype=torch.long), pts], 1))
    coords = torch.cat(scenes, 0).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(dev), coords)
    y = coarse_level(x)                                  # tensor stride 8
    sizes = [int((y.C[:, 0] == b).sum()) for b in range(2)]
    block = AttentionBlock(64, 2).to(dev)
    out = block(y)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels of 2 scenes in, {sizes[0]} + {sizes[1]} voxels at tensor stride {y.tensor_stride[0]}, "
          f"{tuple(out.F.shape)} out; gradient norm of in_proj_weight {float(block.attn.in_proj_weight.grad.norm()):.3e}")
