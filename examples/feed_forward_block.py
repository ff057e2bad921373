"""The pre-norm block of examples/prenorm_block.py with its MLP as one fused operator:

    h = h + attn(LN1(h));   h = h + mlp(LN2(h)),   mlp = MinkowskiFeedForward(C, 4 C)

MinkowskiFeedForward runs fc2(gelu(fc1(x))) on the kernels of csrc/feed_forward.hip: the [N, 4 C] hidden
matrix is never written, forward or backward, and the `mlp.fc1.*` / `mlp.fc2.*` entries of a PTv3 checkpoint load
strictly.  The rest of the block is unchanged:

MinkowskiLayerNorm normalises every voxel over its channels (torch.nn.LayerNorm's parameters, so a PTv3 / SST / Swin3D
checkpoint's `norm1.weight` / `norm1.bias` load strictly), and `forward_residual` takes the residual add in front of a
norm into the norm's launch: `normed, stream = norm.forward_residual(branch, stream)` is `stream = stream + branch;
normed = norm(stream)` bit for bit, with one pass over the features per direction instead of two (csrc/layer_norm.hip,
DESIGN 8.17).  A stage chains the blocks through that call, so only the first norm and the last add stand alone.

    python examples/feed_forward_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402

ORDERS = ("z", "z_trans", "hilbert", "hilbert_trans")


class PreNormBlock(nn.Module):
    def __init__(self, channels, num_heads, patch_size=1024, order="z", mlp_ratio=4):
        super().__init__()
        self.norm1 = ME.MinkowskiLayerNorm(channels)
        self.attn = ME.MinkowskiSerializedSelfAttention(channels, num_heads, patch_size=patch_size, order=order)
        self.norm2 = ME.MinkowskiLayerNorm(channels)
        self.mlp = ME.MinkowskiFeedForward(channels, mlp_ratio * channels)

    def forward(self, stream, branch=None):
        """`branch`: the output of the previous block's MLP, not yet added to `stream`; -> (stream, branch) of this block"""
        normed, stream = (self.norm1(stream), stream) if branch is None else self.norm1.forward_residual(branch, stream)
        normed, stream = self.norm2.forward_residual(self.attn(normed), stream)
        return stream, self.mlp(normed)


class PreNormStage(nn.Module):
    """`depth` blocks on one coordinate map; block i uses ORDERS[i % 4]"""

    def __init__(self, channels, num_heads, depth=4, patch_size=1024):
        super().__init__()
        self.blocks = nn.ModuleList(PreNormBlock(channels, num_heads, patch_size, ORDERS[i % len(ORDERS)])
                                    for i in range(depth))

    def forward(self, x):
        branch = None
        for block in self.blocks:
            x, branch = block(x, branch)
        return x + branch


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 96, (120000, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(dev), coords)
    stage = PreNormStage(64, 2, depth=4, patch_size=1024).to(dev)
    out = stage(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out; gradient norm of the last mlp.fc1.weight "
          f"{float(stage.blocks[-1].mlp.fc1.weight.grad.norm()):.3e}, of the first mlp.fc2.weight "
          f"{float(stage.blocks[0].mlp.fc2.weight.grad.norm()):.3e}; fused: {stage.blocks[0].mlp.is_fused(x)}")
