"""A Swin-style stage on one level of a sparse network (SST, DSVT, Swin3D): every block is a submanifold convolution (the
conditional positional encoding), a norm, window attention and a pre-norm MLP, each with a residual.  Space is cut into
boxes of `window_size` voxels per axis and a voxel attends inside its box; the blocks alternate `shift = 0` and
`shift = window_size // 2`, which moves the window borders from layer to layer.  MinkowskiWindowSelfAttention pads nothing,
wraps nothing around and needs no mask, builds its lists once per (map, window size, shift), and its gradients are bitwise
reproducible (csrc/serial_attention.hip).

    python examples/window_attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class WindowAttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, window_size=8, shift=0, groups=8, mlp_ratio=4, D=3):
        super().__init__()
        self.cpe = ME.MinkowskiConvolution(channels, channels, kernel_size=3, bias=True, dimension=D)   # stride 1: submanifold
        self.norm1 = ME.MinkowskiGroupNorm(groups, channels)
        self.attn = ME.MinkowskiWindowSelfAttention(channels, num_heads, window_size=window_size, shift=shift)
        self.norm2 = ME.MinkowskiGroupNorm(groups, channels)
        self.mlp = nn.Sequential(ME.MinkowskiLinear(channels, mlp_ratio * channels), ME.MinkowskiGELU(),
                                 ME.MinkowskiLinear(mlp_ratio * channels, channels))

    def forward(self, x):
        x = self.cpe(x) + x                              # the same coordinate map: plain addition of the features
        x = self.attn(self.norm1(x)) + x
        return self.mlp(self.norm2(x)) + x


class WindowStage(nn.Module):
    """`depth` blocks on one coordinate map; block i has shift 0 for even i and window_size // 2 for odd i"""

    def __init__(self, channels, num_heads, depth=4, window_size=8, D=3):
        super().__init__()
        self.blocks = nn.ModuleList(WindowAttentionBlock(channels, num_heads, window_size,
                                                         (window_size // 2) if i % 2 else 0, D=D) for i in range(depth))

    def forward(self, x):
        for block in self.blocks:
            x = block(x)
        return x


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 96, (120000, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(dev), coords)
    stage = WindowStage(64, 2, depth=4, window_size=8).to(dev)
    out = stage(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out, shifts {[b.attn.shift for b in stage.blocks]}; gradient norm of "
          f"the last in_proj_weight {float(stage.blocks[-1].attn.in_proj_weight.grad.norm()):.3e}")
