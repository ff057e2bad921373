"""A LLaMA-style pre-norm block on a sparse tensor: RMSNorm, serialized attention and a SwiGLU MLP as one fused operator:

    h = h + attn(RMS1(h));   h = h + mlp(RMS2(h)),   mlp = MinkowskiGatedFeedForward(C, 8 C / 3 rounded to 32)

MinkowskiGatedFeedForward runs fc2(silu(fc1_g(x)) * fc1_x(x)) on the kernels of csrc/gated_feed_forward.hip:
none of the three [N, hidden] matrices of the unfused form is written, forward or backward, and a timm `SwiGLU` state dict
(`fc1_g`, `fc1_x`, `fc2`) loads strictly; `MinkowskiGatedFeedForward.from_packed` takes a packed `gate_up_proj`.
MinkowskiRMSNorm's `forward_residual` takes the residual add in front of a norm into the norm's launch, as in
examples/feed_forward_block.py.

    python examples/gated_feed_forward_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402

ORDERS = ("z", "z_trans", "hilbert", "hilbert_trans")


class SwiGLUBlock(nn.Module):
    def __init__(self, channels, num_heads, patch_size=1024, order="z"):
        super().__init__()
        hidden = (8 * channels // 3 + 31) // 32 * 32          # LLaMA's 8/3 ratio, rounded up to the kernels' chunk
        self.norm1 = ME.MinkowskiRMSNorm(channels)
        self.attn = ME.MinkowskiSerializedSelfAttention(channels, num_heads, patch_size=patch_size, order=order)
        self.norm2 = ME.MinkowskiRMSNorm(channels)
        self.mlp = ME.MinkowskiGatedFeedForward(channels, hidden, activation="silu", bias=False)

    def forward(self, stream, branch=None):
        """`branch`: the output of the previous block's MLP, not yet added to `stream`; -> (stream, branch) of this block"""
        normed, stream = (self.norm1(stream), stream) if branch is None else self.norm1.forward_residual(branch, stream)
        normed, stream = self.norm2.forward_residual(self.attn(normed), stream)
        return stream, self.mlp(normed)


class SwiGLUStage(nn.Module):
    """`depth` blocks on one coordinate map; block i uses ORDERS[i % 4]"""

    def __init__(self, channels, num_heads, depth=4, patch_size=1024):
        super().__init__()
        self.blocks = nn.ModuleList(SwiGLUBlock(channels, num_heads, patch_size, ORDERS[i % len(ORDERS)])
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
    stage = SwiGLUStage(64, 2, depth=4, patch_size=1024).to(dev)
    out = stage(x)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out; gradient norm of the last mlp.fc1_g.weight "
          f"{float(stage.blocks[-1].mlp.fc1_g.weight.grad.norm()):.3e}, of the first mlp.fc2.weight "
          f"{float(stage.blocks[0].mlp.fc2.weight.grad.norm()):.3e}; fused: {stage.blocks[0].mlp.is_fused(x)}")
