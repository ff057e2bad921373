"""One block of a sparse diffusion transformer (DiT, PixArt, TRELLIS-style flow transformers) with adaLN-Zero
conditioning:

    h = h + gate1[b] * attn(LN(h) * (1 + scale1[b]) + shift1[b])
    h = h + gate2[b] * mlp (LN(h) * (1 + scale2[b]) + shift2[b])

with one (shift, scale, gate) row per scene b from a zero-initialised Linear on the scene's timestep / class embedding.
MinkowskiAdaLayerNorm runs the modulated norm in one launch, and `forward_residual` takes the gated add of the first half
into the second norm's launch (csrc/ada_layer_norm.hip).  The last gated add of a block stays in torch (a
stack of blocks would hand it to the next block's first norm, as examples/prenorm_block.py does for the plain norm).

    python examples/dit_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class DiTBlock(nn.Module):
    def __init__(self, channels, num_heads, cond_features, window_size=8, mlp_ratio=4):
        super().__init__()
        self.norm1 = ME.MinkowskiAdaLayerNorm(channels)
        self.attn = ME.MinkowskiWindowSelfAttention(channels, num_heads, window_size=window_size)
        self.norm2 = ME.MinkowskiAdaLayerNorm(channels)
        self.mlp = ME.MinkowskiFeedForward(channels, mlp_ratio * channels)
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(cond_features, 6 * channels))
        nn.init.zeros_(self.modulation[1].weight)         # adaLN-Zero: the block starts as the identity
        nn.init.zeros_(self.modulation[1].bias)

    def forward(self, h, cond):
        """h: a SparseTensor; cond [scenes, cond_features]: row j for the j-th smallest batch index of h"""
        shift1, scale1, gate1, shift2, scale2, gate2 = self.modulation(cond).chunk(6, dim=1)
        branch = self.attn(self.norm1(h, scale1, shift1))
        normed, h = self.norm2.forward_residual(branch, h, scale2, shift2, gate1)       # h = h + gate1[b] * branch
        branch = self.mlp(normed)
        rows = h.coordinate_manager._manager._origin_rows(h.coordinate_map_key).long()
        return ME.SparseTensor(h.F + gate2[rows].to(h.F.dtype) * branch.F, coordinate_map_key=h.coordinate_map_key,
                               coordinate_manager=h.coordinate_manager)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    scenes = [torch.unique(torch.randint(0, 48, (20000, 3), generator=g), dim=0) for _ in range(2)]
    coords = torch.cat([torch.cat([torch.full((p.shape[0], 1), b), p], 1) for b, p in enumerate(scenes)]).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(dev), coords)
    block = DiTBlock(64, 2, cond_features=32).to(dev)
    with torch.no_grad():                                 # (away from the zero start, so that every gradient is alive)
        block.modulation[1].weight.normal_(0, 0.02)
    cond = torch.randn(2, 32, generator=g).to(dev).requires_grad_()
    out = block(x, cond)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in 2 scenes, {tuple(out.F.shape)} out; gradient norm of the conditioning "
          f"{float(cond.grad.norm()):.3e}, of the modulation weight {float(block.modulation[1].weight.grad.norm()):.3e}")
