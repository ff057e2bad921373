"""Host-side checks of examples/local_attention_block.py: the block is built from the package's layers and carries
MinkowskiSelfAttention's parameters plus the bias table (the GPU run of the block: tests/test_gpu_local_attention.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_local_attention_block_is_pre_norm_attention_and_mlp():
    import local_attention_block as LB
    import minkowskiengine_amd as ME
    block = LB.LocalAttentionBlock(64, 2, groups=4)
    assert isinstance(block.norm1, ME.MinkowskiGroupNorm) and isinstance(block.norm2, ME.MinkowskiGroupNorm)
    assert isinstance(block.attn, ME.MinkowskiLocalSelfAttention)
    assert (block.attn.embed_dim, block.attn.num_heads, block.attn.kernel_generator.kernel_volume) == (64, 2, 27)
    assert isinstance(block.mlp[0], ME.MinkowskiLinear) and isinstance(block.mlp[2], ME.MinkowskiLinear)
    assert (block.mlp[0].linear.out_features, block.mlp[2].linear.out_features) == (256, 64)
    names = sorted(k for k, _ in block.named_parameters() if k.startswith("attn."))
    assert names == ["attn.in_proj_bias", "attn.in_proj_weight", "attn.out_proj.bias", "attn.out_proj.weight",
                     "attn.rel_pos_bias"]
    ME.MinkowskiSelfAttention(64, 2).load_state_dict(
        {k[5:]: v for k, v in block.state_dict().items() if k.startswith("attn.") and k != "attn.rel_pos_bias"}, strict=True)
