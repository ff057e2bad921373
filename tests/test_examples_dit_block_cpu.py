"""Host-side checks of examples/dit_block.py: the block is built from the package's layers and starts as adaLN-Zero (the
GPU run of the layer: tests/test_gpu_ada_layer_norm.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_dit_block_is_ada_norm_window_attention_ada_norm_and_fused_mlp():
    import torch
    import minkowskiengine_amd as ME
    import dit_block as DB
    block = DB.DiTBlock(64, 2, cond_features=32, window_size=6)
    assert isinstance(block.norm1, ME.MinkowskiAdaLayerNorm) and isinstance(block.norm2, ME.MinkowskiAdaLayerNorm)
    assert not list(block.norm1.parameters()) and block.norm1.eps == 1e-6          # DiT's norms carry no parameters
    assert isinstance(block.attn, ME.MinkowskiWindowSelfAttention) and block.attn.window_size == 6
    assert isinstance(block.mlp, ME.MinkowskiFeedForward)
    linear = block.modulation[1]
    assert (linear.in_features, linear.out_features) == (32, 6 * 64)
    assert not linear.weight.any() and not linear.bias.any()
    assert all(not p.any() for p in block.modulation(torch.randn(2, 32)).chunk(6, dim=1))
