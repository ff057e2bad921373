"""A residual block of a sparse U-Net for diffusion / completion: convolution -> GroupNorm -> SiLU, twice, with the input
added back, on a branch that was pruned to the voxels a classifier keeps and then up-sampled by a generative transposed
convolution.  Such networks run one to four scenes per GPU, where batch statistics are useless: MinkowskiGroupNorm
normalises every scene (batch index) on its own, per group of channels, whatever the scenes' sizes
(csrc/group_norm.hip).

    python examples/generative_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class ResidualGroupNormBlock(nn.Module):
    def __init__(self, channels, groups=8, D=3):
        super().__init__()
        self.conv1 = ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D)
        self.norm1 = ME.MinkowskiGroupNorm(groups, channels)
        self.conv2 = ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D)
        self.norm2 = ME.MinkowskiGroupNorm(groups, channels)
        self.act = ME.MinkowskiSiLU()

    def forward(self, x):
        y = self.act(self.norm1(self.conv1(x)))
        y = self.norm2(self.conv2(y))
        return self.act(y + x)                           # the same coordinate map: plain addition of the features


class GenerativeStage(nn.Module):
    """coarse voxels -> keep the ones the classifier picks -> residual block there -> 8 children per kept voxel"""

    def __init__(self, channels, out_channels, D=3):
        super().__init__()
        self.keep = ME.MinkowskiConvolution(channels, 1, kernel_size=1, bias=True, dimension=D)
        self.prune = ME.MinkowskiPruning()
        self.block = ResidualGroupNormBlock(channels, D=D)
        self.up = ME.MinkowskiGenerativeConvolutionTranspose(channels, out_channels, kernel_size=2, stride=2, dimension=D)

    def forward(self, x):
        mask = self.keep(x).F.squeeze(1) > 0
        return self.up(self.block(self.prune(x, mask)))


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    scenes = []
    for b, k in enumerate((12000, 5000)):                # two scenes of different sizes at tensor stride 2
        pts = torch.unique(torch.randint(0, 32, (k, 3), generator=g), dim=0) * 2
        scenes.append(torch.cat([torch.full((pts.shape[0], 1), b, dtype=torch.long), pts], 1))
    coords = torch.cat(scenes, 0).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 32, generator=g).to(dev), coords, tensor_stride=2)
    stage = GenerativeStage(32, 16).to(dev)
    out = stage(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels of 2 scenes at stride 2 in, {len(out)} at stride {out.tensor_stride[0]} out; "
          f"GroupNorm weight gradient norm {float(stage.block.norm1.weight.grad.norm()):.3e}")
