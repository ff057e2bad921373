"""A Point Transformer v3-style stage on the fine level of a sparse network: every block is a submanifold convolution (the
conditional positional encoding), a norm, serialized patch attention and a pre-norm MLP, each with a residual.  The voxels of
a scene are ordered along a space-filling curve and cut into patches of `patch_size`; a voxel attends inside its patch, so
the cost is N * patch_size on the MFMA kernels of MinkowskiSelfAttention.  The blocks cycle the four orders (z, z_trans,
hilbert, hilbert_trans), which moves the patch borders from layer to layer.  MinkowskiSerializedSelfAttention pads nothing,
borrows no rows, builds its lists once per (map, patch size, order), and its gradients are bitwise reproducible
(csrc/serial_attention.hip).

    python examples/serialized_attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402

ORDERS = ("z", "z_trans", "hilbert", "hilbert_trans")


class SerializedAttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, patch_size=1024, order="z", groups=8, mlp_ratio=4, D=3):
        super().__init__()
        self.cpe = ME.MinkowskiConvolution(channels, channels, kernel_size=3, bias=True, dimension=D)   # stride 1: submanifold
        self.norm1 = ME.MinkowskiGroupNorm(groups, channels)
        self.attn = ME.MinkowskiSerializedSelfAttention(channels, num_heads, patch_size=patch_size, order=order)
        self.norm2 = ME.MinkowskiGroupNorm(groups, channels)
        self.mlp = nn.Sequential(ME.MinkowskiLinear(channels, mlp_ratio * channels), ME.MinkowskiGELU(),
                                 ME.MinkowskiLinear(mlp_ratio * channels, channels))

    def forward(self, x):
        x = self.cpe(x) + x                              # the same coordinate map: plain addition of the features
        x = self.attn(self.norm1(x)) + x
        return self.mlp(self.norm2(x)) + x


class SerializedStage(nn.Module):
    """`depth` blocks on one coordinate map; block i uses ORDERS[i % 4]"""

    def __init__(self, channels, num_heads, depth=4, patch_size=1024, D=3):
        super().__init__()
        self.blocks = nn.ModuleList(SerializedAttentionBlock(channels, num_heads, patch_size, ORDERS[i % len(ORDERS)], D=D)
                                    for i in range(depth))

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
    stage = SerializedStage(64, 2, depth=4, patch_size=1024).to(dev)
    out = stage(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out, orders {[b.attn.order for b in stage.blocks]}; gradient norm of "
          f"the last in_proj_weight {float(stage.blocks[-1].attn.in_proj_weight.grad.norm()):.3e}")
