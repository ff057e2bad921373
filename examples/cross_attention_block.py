"""A block of a sparse generative U-Net conditioned twice: on a per-scene embedding (the timestep) through conditional
group normalisation, and on a sequence of context tokens per scene (the text or image tokens of CLIP / DINO) through
cross-attention.  conditional group norm + SiLU -> convolution -> self-attention inside every scene -> cross-attention
from every voxel to the tokens of its scene -> MLP, each with a residual.  The contexts are padded to a common length L
and `context_lengths` masks the padding, as `key_padding_mask` does in torch.  MinkowskiCrossAttention carries the
parameters of torch.nn.MultiheadAttention(kdim=, vdim=); its dK / dV pass is split over the voxels where the context is
short (csrc/attention.hip).

    python examples/cross_attention_block.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class CrossAttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, emb_channels, context_channels, groups=8, mlp_ratio=4, D=3):
        super().__init__()
        self.channels = channels
        self.norm_in = ME.MinkowskiConditionalGroupNorm(groups, channels, activation="silu")
        self.to_mod = nn.Linear(emb_channels, 2 * channels)          # (scale, shift) of norm_in
        self.conv = ME.MinkowskiConvolution(channels, channels, kernel_size=3, bias=True, dimension=D)
        self.norm_self = ME.MinkowskiGroupNorm(groups, channels)
        self.self_attn = ME.MinkowskiSelfAttention(channels, num_heads)
        self.norm_cross = ME.MinkowskiGroupNorm(groups, channels)
        self.cross_attn = ME.MinkowskiCrossAttention(channels, num_heads, kdim=context_channels, vdim=context_channels)
        self.norm_mlp = ME.MinkowskiGroupNorm(groups, channels)
        self.mlp = nn.Sequential(ME.MinkowskiLinear(channels, mlp_ratio * channels), ME.MinkowskiGELU(),
                                 ME.MinkowskiLinear(mlp_ratio * channels, channels))

    def forward(self, x, emb, context, context_lengths=None):
        """emb [scenes, emb_channels] and context [scenes, L, context_channels]: row j for the j-th smallest batch index"""
        scale, shift = self.to_mod(emb).split(self.channels, dim=1)
        x = self.conv(self.norm_in(x, scale, shift)) + x
        x = self.self_attn(self.norm_self(x)) + x
        x = self.cross_attn(self.norm_cross(x), context, context_lengths) + x
        return self.mlp(self.norm_mlp(x)) + x


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    coords = []
    for b in range(2):
        pts = torch.unique(torch.randint(0, 24, (4000, 3), generator=g), dim=0)
        coords.append(torch.cat([torch.full((pts.shape[0], 1), b), pts], 1))
    coords = torch.cat(coords).int().to(dev)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 128, generator=g).to(dev), coords)
    emb = torch.randn(2, 64, generator=g).to(dev)
    context = torch.randn(2, 77, 768, generator=g).to(dev)            # two prompts padded to 77 tokens
    lengths = torch.tensor([77, 12])
    block = CrossAttentionBlock(128, 4, emb_channels=64, context_channels=768).to(dev)
    context.requires_grad_(True)
    out = block(x, emb, context, lengths)
    out.F.square().mean().backward()
    print(f"{len(x)} voxels in, {tuple(out.F.shape)} out; gradient norm of the context {float(context.grad.norm()):.3e}, "
          f"of the masked tokens {float(context.grad[1, 12:].norm()):.1e}")
