"""A window-attention stage whose only positional signal is rotary position embedding (3-D RoPE, as in sparse generative
transformers and the successors of Point Transformer V3): every block is a norm, window attention with `rope=True` and a
pre-norm MLP, each with a residual; there is no convolution in front of the attention.  q and k are rotated by angles taken
from the voxel coordinates, so the score of two voxels depends on their offset and the stage is translation invariant.
The blocks alternate `shift = 0` and `shift = window_size // 2`.  The rotation is one pass of csrc/rope.hip over the
projected [N, 2C] view, on a table the coordinate manager builds once per map.

    python examples/rope_attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class RopeAttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, window_size=8, shift=0, groups=8, mlp_ratio=4, rope_base=10000.0):
        super().__init__()
        self.norm1 = ME.MinkowskiGroupNorm(groups, channels)
        self.attn = ME.MinkowskiWindowSelfAttention(channels, num_heads, window_size=window_size, shift=shift, rope=True,
                                                    rope_base=rope_base)
        self.norm2 = ME.MinkowskiGroupNorm(groups, channels)
        self.mlp = nn.Sequential(ME.MinkowskiLinear(channels, mlp_ratio * channels), ME.MinkowskiGELU(),
                                 ME.MinkowskiLinear(mlp_ratio * channels, channels))

    def forward(self, x):
        x = self.attn(self.norm1(x)) + x                 # the same coordinate map: plain addition of the features
        return self.mlp(self.norm2(x)) + x


class RopeStage(nn.Module):
    """`depth` blocks on one coordinate map; block i has shift 0 for even i and window_size // 2 for odd i"""

    def __init__(self, channels, num_heads, depth=4, window_size=8, rope_base=10000.0):
        super().__init__()
        self.blocks = nn.ModuleList(RopeAttentionBlock(channels, num_heads, window_size, (window_size // 2) if i % 2 else 0,
                                                       rope_base=rope_base) for i in range(depth))

    def forward(self, x):
        for block in self.blocks:
            x = block(x)
        return x


def main(device=None, steps=3, voxels=120000, side=96, quiet=False):
    """a few optimiser steps of the stage on a random scene -> the last loss"""
    dev = torch.device("cuda:0") if device is None else device
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, side, (voxels, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)
    feats = torch.randn(coords.shape[0], 64, generator=g).to(dev)
    stage = RopeStage(64, 2, depth=4, window_size=8).to(dev)
    opt = torch.optim.SGD(stage.parameters(), lr=1e-3)
    loss = None
    for _ in range(steps):
        x = ME.SparseTensor(feats, coords)
        out = stage(x)
        loss = out.F.square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    if not quiet:
        print(f"{coords.shape[0]} voxels, {tuple(out.F.shape)} out, shifts {[b.attn.shift for b in stage.blocks]}, rope "
              f"{[b.attn.rope for b in stage.blocks]}; loss {float(loss):.4e}")
    return float(loss)


if __name__ == "__main__":
    main()
