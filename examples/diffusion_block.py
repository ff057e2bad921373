"""A residual block of a sparse diffusion U-Net conditioned on a per-scene embedding (a timestep or a class): convolution
-> ConditionalGroupNorm with a fused SiLU, twice, with the input added back.  Every scene (batch index) has its own
embedding; one torch.nn.Linear turns it into a (scale, shift) pair per norm layer, which modulates the normalised
features per channel — AdaGN / FiLM: silu(GroupNorm(x) * (1 + scale[b]) + shift[b]).  MinkowskiConditionalGroupNorm
does that in the passes over the feature matrix of the plain MinkowskiGroupNorm, whatever the scenes' sizes, and the
gradients of scale and shift are fixed-order sums (csrc/group_norm.hip).

    python examples/diffusion_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class ConditionalResidualBlock(nn.Module):
    def __init__(self, channels, emb_channels, groups=8, D=3):
        super().__init__()
        self.channels = channels
        self.conv1 = ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D)
        self.norm1 = ME.MinkowskiConditionalGroupNorm(groups, channels, activation="silu")
        self.conv2 = ME.MinkowskiConvolution(channels, channels, kernel_size=3, dimension=D)
        self.norm2 = ME.MinkowskiConditionalGroupNorm(groups, channels, activation="silu")
        self.to_mod = nn.Linear(emb_channels, 4 * channels)      # (scale, shift) of both norm layers
        nn.init.normal_(self.to_mod.weight, std=0.02)
        nn.init.zeros_(self.to_mod.bias)

    def forward(self, x, emb):
        """emb: [scenes, emb_channels], row j for the j-th smallest batch index of x"""
        scale1, shift1, scale2, shift2 = self.to_mod(emb).split(self.channels, dim=1)
        y = self.norm1(self.conv1(x), scale1, shift1)
        y = self.norm2(self.conv2(y), scale2, shift2)
        return y + x                                     # the same coordinate map: plain addition of the features


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    scenes = []
    for b, k in enumerate((12000, 5000)):                # two scenes of different sizes
        pts = torch.unique(torch.randint(0, 32, (k, 3), generator=g), dim=0)
        scenes.append(torch.cat([torch.full((pts.shape[0], 1), b, dtype=torch.long), pts], 1))
    coords = torch.cat(scenes, 0).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 32, generator=g).to(dev), coords)
    emb = torch.randn(2, 64, generator=g).to(dev)        # one embedding per scene
    block = ConditionalResidualBlock(32, 64).to(dev)
    out = block(x, emb)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels of 2 scenes ({scenes[0].shape[0]} + {scenes[1].shape[0]}) in, {tuple(out.F.shape)} out; "
          f"gradient norm of the conditioning Linear {float(block.to_mod.weight.grad.norm()):.3e}")
