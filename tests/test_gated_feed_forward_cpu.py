"""MinkowskiGatedFeedForward without a GPU: the torch fallback, the width predicate, state dicts, argument errors and the
host-side checks of me_glu_*."""
import pytest
import torch
import torch.nn.functional as F

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from minkowskiengine_amd.feed_forward import ACTIVATIONS


class _Rows:
    """the two attributes gated_feed_forward reads from a sparse tensor, around CPU features"""

    def __init__(self, feats):
        self.F, self.coordinate_field_map_key = feats, "rows"

    def _like(self, feats):
        return _Rows(feats)


@pytest.mark.parametrize("act", sorted(ACTIVATIONS))
@pytest.mark.parametrize("bias", [True, False])
def test_cpu_tensors_take_the_torch_formulation(act, bias):
    torch.manual_seed(0)
    mlp = ME.MinkowskiGatedFeedForward(32, 64, 96, activation=act, bias=bias)
    names = [f"{m}.{p}" for m in ("fc1_g", "fc1_x", "fc2") for p in (("weight", "bias") if bias else ("weight",))]
    assert sorted(mlp.state_dict()) == sorted(names)                      # timm SwiGLU's names
    x = _Rows(torch.randn(9, 32))
    assert not mlp.is_fused(x)
    want = mlp.fc2(ACTIVATIONS[act](mlp.fc1_g(x.F)) * mlp.fc1_x(x.F))
    assert torch.equal(mlp(x).F, want)
    w = (mlp.fc1_g.weight, mlp.fc1_g.bias, mlp.fc1_x.weight, mlp.fc1_x.bias, mlp.fc2.weight, mlp.fc2.bias)
    assert torch.equal(ME.MinkowskiFunctional.gated_feed_forward(x, *w, activation=act).F, want)
    # a packed first layer by its halves, either one as the gate
    for halves, gate_first in (((0, 2), True), ((2, 0), False)):
        packed = ME.MinkowskiGatedFeedForward.from_packed(
            torch.cat([w[halves[0]], w[halves[1]]]), torch.cat([w[halves[0] + 1], w[halves[1] + 1]]) if bias else None,
            w[4], w[5], activation=act, gate_first=gate_first)
        assert torch.equal(packed(x).F, want)


@pytest.mark.parametrize("c,hd,cout,dtype,served", [
    (32, 32, 32, torch.float32, True), (64, 4096, 64, torch.float32, True), (96, 64, 32, torch.float32, False),
    (32, 64, 96, torch.float32, False), (128, 352, 128, torch.bfloat16, True), (160, 64, 32, torch.bfloat16, False),
    (32, 64, 160, torch.bfloat16, False), (48, 64, 64, torch.bfloat16, False), (64, 48, 64, torch.bfloat16, False),
    (64, 64, 16, torch.float32, False), (64, 64, 64, torch.float64, False), (64, 64, 64, torch.float16, False)])
def test_width_rule(c, hd, cout, dtype, served):
    assert backend.gated_feed_forward_supported(c, hd, cout, dtype) == served
    assert backend.gated_feed_forward_fused(c, hd, cout, dtype) == served      # the rule starts at the kernels' widths
    if dtype in (torch.float32, torch.bfloat16):        # the library's predicate is the same rule
        assert bool(_lib.load().me_glu_supported(c, hd, cout, torch.finfo(dtype).bits // 8)) == served


def test_row_splits_and_workspace():
    lib = _lib.load()
    for c, hd, cout, elem in ((64, 256, 64, 2), (128, 352, 32, 2), (32, 32, 32, 4)):
        last = 0
        for n in (1, 128, 129, 293, 1000, 120000):
            s = lib.me_glu_row_splits(n, c, hd, cout, elem)
            blocks = -(-n // backend.FFN_ROWS)
            assert 1 <= s <= blocks and (s - 1) * -(-blocks // s) < blocks        # whole blocks, no empty split
            ws = lib.me_glu_workspace_bytes(n, c, hd, cout, elem)
            assert ws >= last                                                      # monotone in n
            last = ws
    assert lib.me_glu_row_splits(293, 32, 32, 32, 4) == 3
    assert lib.me_glu_workspace_bytes(293, 32, 32, 32, 4) == 3 * 32 * 32 * 4 + 4 * 3 * (3 * 32 * 32 + 96) * 4
    assert lib.me_version() >= 350


def test_argument_errors():
    with pytest.raises(ValueError, match="activation"):
        ME.MinkowskiGatedFeedForward(32, 64, activation="swiglu")
    mlp = ME.MinkowskiGatedFeedForward(32, 64)
    with pytest.raises(ValueError, match="channel mismatch"):
        mlp(_Rows(torch.randn(4, 64)))
    w = (mlp.fc1_g.weight, None, mlp.fc1_x.weight, None, mlp.fc2.weight, None)
    with pytest.raises(ValueError, match="activation"):
        ME.MinkowskiFunctional.gated_feed_forward(_Rows(torch.randn(4, 32)), *w, "tanh")
    with pytest.raises(ValueError, match="packed"):
        ME.MinkowskiGatedFeedForward.from_packed(torch.zeros(96, 32), None, torch.zeros(32, 64), None)
    with pytest.raises(RuntimeError):                       # mixed dtypes: the torch formulation refuses them
        mlp(_Rows(torch.randn(4, 32).bfloat16()))
    # the operators themselves: no CPU implementation
    with pytest.raises(ValueError, match="GatedFeedForwardForwardCPU"):
        ME.MinkowskiGatedFeedForwardFunction.apply(torch.randn(4, 32), *w, "silu")
    # the host-side checks of the library: nothing is launched
    lib, nul = _lib.load(), (None,) * 7
    assert lib.me_glu_forward(*nul, 0, 4, 48, 64, 32, 3, None, None) != 0                      # width
    assert lib.me_glu_forward(*nul, 0, 4, 96, 64, 32, 3, None, None) != 0                      # fp32 beyond its limit
    assert lib.me_glu_forward(*nul, 0, 4, 32, 64, 32, 7, None, None) != 0                      # activation
    assert lib.me_glu_forward(*nul, 0, -1, 32, 64, 32, 3, None, None) != 0                     # n
    assert lib.me_glu_forward(*nul, 0, 4, 32, 64, 32, 3, None, None) != 0                      # operands missing
    assert lib.me_glu_forward(*nul, 0, 0, 32, 64, 32, 3, None, None) == 0                      # n = 0: nothing to do
    assert lib.me_glu_backward(*nul, 1, 4, 32, 64, 32, 3, 1, 1, 1, *nul, None, 0, None) != 0   # outputs missing
    assert lib.me_glu_backward(*nul, 1, 4, 32, 64, 32, 3, 0, 0, 0, *nul, None, 0, None) == 0   # nothing wanted
    assert lib.me_ffn_forward(None, None, None, None, None, 0, 4, 32, 64, 32, 7, None, None) != 0   # 7 stays an error
