"""MinkowskiFeedForward without a GPU: the torch fallback, the width predicate, state dicts and argument errors."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from minkowskiengine_amd.feed_forward import is_fused


class _Rows:
    """the two attributes feed_forward reads from a sparse tensor, around CPU features"""

    def __init__(self, feats):
        self.F, self.coordinate_field_map_key = feats, "rows"

    def _like(self, feats):
        return _Rows(feats)


@pytest.mark.parametrize("act,fn", [("gelu", F.gelu), ("gelu_tanh", lambda t: F.gelu(t, approximate="tanh")),
                                    ("relu", F.relu), ("silu", F.silu)])
def test_cpu_tensors_take_the_torch_formulation(act, fn):
    torch.manual_seed(0)
    mlp = ME.MinkowskiFeedForward(32, 64, 96, activation=act)
    x = _Rows(torch.randn(9, 32))
    assert not mlp.is_fused(x)
    want = mlp.fc2(fn(mlp.fc1(x.F)))
    assert torch.equal(mlp(x).F, want)
    w = (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)
    assert torch.equal(ME.MinkowskiFunctional.feed_forward(x, *w, activation=act).F, want)


@pytest.mark.parametrize("c,hd,cout,dtype,served,fused", [
    (32, 32, 32, torch.float32, True, True), (64, 4096, 64, torch.float32, True, True),
    (128, 512, 128, torch.float32, True, False), (160, 64, 32, torch.float32, False, False),
    (32, 64, 160, torch.float32, False, False), (128, 512, 128, torch.bfloat16, True, True),
    (256, 1024, 256, torch.bfloat16, True, False), (32, 64, 160, torch.bfloat16, True, False),
    (288, 64, 32, torch.bfloat16, False, False), (48, 64, 64, torch.bfloat16, False, False),
    (64, 48, 64, torch.bfloat16, False, False), (64, 64, 16, torch.float32, False, False),
    (64, 64, 64, torch.float64, False, False), (64, 64, 64, torch.float16, False, False)])
def test_width_rule(c, hd, cout, dtype, served, fused):
    assert backend.feed_forward_supported(c, hd, cout, dtype) == served
    assert backend.feed_forward_fused(c, hd, cout, dtype) == fused
    if dtype in (torch.float32, torch.bfloat16):        # the library's predicate is the same rule
        assert bool(_lib.load().me_ffn_supported(c, hd, cout, torch.finfo(dtype).bits // 8)) == served
    # the module's predicate needs CUDA rows on top of the widths
    w1, w2 = torch.zeros(hd, c, dtype=dtype), torch.zeros(cout, hd, dtype=dtype)
    assert not is_fused(torch.zeros(4, c, dtype=dtype), w1, None, w2, None)


def test_row_splits_are_whole_blocks_without_an_empty_split():
    lib = _lib.load()
    for n in (1, 128, 129, 293, 1000, 120000):
        s = lib.me_ffn_row_splits(n, 64, 256, 64, 2)
        blocks = -(-n // backend.FFN_ROWS)
        assert 1 <= s <= blocks and (s - 1) * -(-blocks // s) < blocks
    assert lib.me_ffn_row_splits(293, 32, 32, 32, 4) == 3
    assert lib.me_ffn_workspace_bytes(293, 32, 32, 32, 4) == 2 * 32 * 32 * 4 + 4 * 3 * (2 * 32 * 32 + 64) * 4


@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly(bias):
    seq = nn.Sequential(nn.Linear(32, 128, bias=bias), nn.GELU(), nn.Linear(128, 32, bias=bias))
    mlp = ME.MinkowskiFeedForward(32, 128, bias=bias)
    assert sorted(mlp.state_dict()) == sorted(f"fc{i}.{p}" for i in (1, 2) for p in (("weight", "bias") if bias else ("weight",)))
    mlp.load_state_dict({k.replace("0.", "fc1.").replace("2.", "fc2."): v for k, v in seq.state_dict().items()}, strict=True)
    x = torch.randn(5, 32)
    assert torch.equal(mlp(_Rows(x)).F, seq(x))


def test_argument_errors():
    with pytest.raises(ValueError, match="activation"):
        ME.MinkowskiFeedForward(32, 64, activation="swiglu")
    mlp = ME.MinkowskiFeedForward(32, 64)
    with pytest.raises(ValueError, match="channel mismatch"):
        mlp(_Rows(torch.randn(4, 64)))
    with pytest.raises(ValueError, match="activation"):
        ME.MinkowskiFunctional.feed_forward(_Rows(torch.randn(4, 32)), mlp.fc1.weight, None, mlp.fc2.weight, None, "tanh")
    with pytest.raises(RuntimeError):                       # mixed dtypes: the torch formulation refuses them
        mlp(_Rows(torch.randn(4, 32).bfloat16()))
    # the operators themselves: no CPU implementation, and the checks of the host layer
    with pytest.raises(ValueError, match="FeedForwardForwardCPU"):
        ME.MinkowskiFeedForwardFunction.apply(torch.randn(4, 32), mlp.fc1.weight, None, mlp.fc2.weight, None, "gelu")
    lib = _lib.load()
    assert lib.me_ffn_forward(None, None, None, None, None, 0, 4, 48, 64, 32, 0, None, None) != 0      # width
    assert lib.me_ffn_forward(None, None, None, None, None, 0, 4, 32, 64, 32, 7, None, None) != 0      # activation
    assert lib.me_ffn_backward(None, None, None, None, None, 1, 4, 32, 64, 32, 0, 1, 1, 1, None, None, None, None, None,
                               None, 0, None) != 0                                                     # outputs missing
