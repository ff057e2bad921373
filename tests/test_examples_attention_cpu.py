"""Host-side checks of examples/attention_block.py: the block is built from the package's layers and carries
torch.nn.MultiheadAttention's parameters (the GPU run of the block: tests/test_gpu_attention.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_attention_block_is_group_norm_then_self_attention():
    import attention_block as AB
    import minkowskiengine_amd as ME
    block = AB.AttentionBlock(64, 2, groups=4)
    assert isinstance(block.norm, ME.MinkowskiGroupNorm) and isinstance(block.attn, ME.MinkowskiSelfAttention)
    assert (block.norm.num_groups, block.norm.num_channels) == (4, 64)
    assert (block.attn.embed_dim, block.attn.num_heads) == (64, 2)
    names = sorted(k for k, _ in block.named_parameters())
    assert names == ["attn.in_proj_bias", "attn.in_proj_weight", "attn.out_proj.bias", "attn.out_proj.weight", "norm.bias",
                     "norm.weight"]
    torch.nn.MultiheadAttention(64, 2, batch_first=True).load_state_dict(block.attn.state_dict(), strict=True)
    assert callable(AB.coarse_level)
