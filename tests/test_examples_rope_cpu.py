"""Host-side checks of examples/rope_attention_block.py: the stage is built from the package's layers, its window
attention has rope=True, alternates shift 0 and window_size // 2 over its blocks and carries MinkowskiSelfAttention's
parameters (the GPU run: tests/test_gpu_rope.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_rope_stage_is_norm_rope_window_attention_and_mlp_alternating_the_shift():
    import minkowskiengine_amd as ME
    import rope_attention_block as RB
    stage = RB.RopeStage(64, 2, depth=5, window_size=6, rope_base=100.0)
    assert [b.attn.shift for b in stage.blocks] == [0, 3, 0, 3, 0]
    for block in stage.blocks:
        assert isinstance(block.norm1, ME.MinkowskiGroupNorm) and isinstance(block.norm2, ME.MinkowskiGroupNorm)
        assert isinstance(block.attn, ME.MinkowskiWindowSelfAttention)
        assert (block.attn.embed_dim, block.attn.num_heads, block.attn.window_size) == (64, 2, 6)
        assert block.attn.rope is True and block.attn.rope_base == 100.0
        assert "rope=True, rope_base=100.0" in repr(block.attn)
        assert not any(isinstance(m, ME.MinkowskiConvolution) for m in block.modules())
        assert isinstance(block.mlp[0], ME.MinkowskiLinear) and isinstance(block.mlp[2], ME.MinkowskiLinear)
        assert (block.mlp[0].linear.out_features, block.mlp[2].linear.out_features) == (256, 64)
    block = stage.blocks[1]
    names = sorted(k for k, _ in block.named_parameters() if k.startswith("attn."))
    assert names == ["attn.in_proj_bias", "attn.in_proj_weight", "attn.out_proj.bias", "attn.out_proj.weight"]
    ME.MinkowskiSelfAttention(64, 2).load_state_dict(
        {k[5:]: v for k, v in block.state_dict().items() if k.startswith("attn.")}, strict=True)
    assert callable(RB.main)
