"""The transformer block of the fine levels of a sparse U-Net (Fast Point Transformer, Stratified Transformer, Point
Transformer v2, neighbourhood-attention U-Nets): pre-norm local attention and a pre-norm MLP, each with a residual.  Every
voxel attends to the voxels inside a 3x3x3 region around it, so the cost is N * 27 instead of the N^2 of
MinkowskiSelfAttention (examples/attention_block.py) and the block runs on 100k-voxel maps.
MinkowskiLocalSelfAttention materialises nothing of size [N, K, C], has a learned bias per head and kernel offset, and its
gradients are bitwise reproducible (csrc/local_attention.hip).

    python examples/local_attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class LocalAttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, kernel_size=3, groups=8, mlp_ratio=4, D=3):
        super().__init__()
        self.norm1 = ME.MinkowskiGroupNorm(groups, channels)
        self.attn = ME.MinkowskiLocalSelfAttention(channels, num_heads, kernel_size=kernel_size, dimension=D)
        self.norm2 = ME.MinkowskiGroupNorm(groups, channels)
        self.mlp = nn.Sequential(ME.MinkowskiLinear(channels, mlp_ratio * channels), ME.MinkowskiGELU(),
                                 ME.MinkowskiLinear(mlp_ratio * channels, channels))

    def forward(self, x):
        x = self.attn(self.norm1(x)) + x                 # the same coordinate map: plain addition of the features
        return self.mlp(self.norm2(x)) + x


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 96, (120000, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(dev), coords)
    block = LocalAttentionBlock(64, 2).to(dev)
    out = block(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out; gradient norms: in_proj_weight "
          f"{float(block.attn.in_proj_weight.grad.norm()):.3e}, rel_pos_bias {float(block.attn.rel_pos_bias.grad.norm()):.3e}")
