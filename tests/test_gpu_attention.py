"""GPU tests of MinkowskiSelfAttention, MinkowskiAttentionFunction and MinkowskiFunctional.scaled_dot_product_attention
(the kernels of csrc/attention.hip through the operators of both host layers).

Yardstick of the module: torch.nn.MultiheadAttention (batch_first, no mask, no dropout) with the same state dict, applied
to the rows of every instance as one sequence in float64.  Bound, as in test_gpu_attention_kernels.py: E_torch is the
maximum absolute error of that torch module run in the dtype under test on the same rows; the layer must stay within
FACTOR * E_torch per tensor (output, input gradient, every parameter gradient).  Figures are printed before the assertion."""
import math
import os
import sys

import pytest
import torch

import minkowskiengine_amd as ME
from test_gpu_attention_kernels import BK, FACTOR, draw, make_tensor, reference, torch_attention

pytestmark = pytest.mark.gpu


def _mha_per_instance(state, dtype, feats, dout, batch, embed_dim, heads, bias):
    """torch.nn.MultiheadAttention in `dtype` with the parameters `state` on the rows of every instance -> (out, grads)"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    mha = torch.nn.MultiheadAttention(embed_dim, heads, bias=bias, batch_first=True).to(feats.device).to(dtype)
    mha.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=True)
    x = feats.detach().to(dtype).requires_grad_()
    out = torch.zeros_like(x)
    with sdpa_kernel(SDPBackend.MATH):
        for b in torch.unique(batch).tolist():
            m = (batch == b).nonzero().reshape(-1)
            xb = x[m][None]
            out = out.index_copy(0, m, mha(xb, xb, xb, need_weights=False)[0][0])
        out.backward(dout.to(dtype))
    grads = {k: p.grad for k, p in mha.named_parameters()}
    grads["input"] = x.grad
    return out.detach(), grads


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_module_equals_multihead_attention_per_instance(device, host_layer, dtype, bias):
    embed_dim, heads = 64, 2
    x, batch = make_tensor([BK + 1, 37, 1, 2 * BK + 2], device, shuffle=True, seed=4)
    n = batch.numel()
    torch.manual_seed(11)
    layer = ME.MinkowskiSelfAttention(embed_dim, heads, bias=bias).to(device).to(dtype)
    if bias:
        with torch.no_grad():                            # the biases start at 0: give them something to do
            layer.in_proj_bias.normal_(std=0.3)
            layer.out_proj.bias.normal_(std=0.3)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    feats, dout = draw(n, embed_dim, dtype, device, 1), draw(n, embed_dim, dtype, device, 2)
    f = feats.clone().requires_grad_()
    xin = ME.SparseTensor(f, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    out = layer(xin)
    assert out.coordinate_map_key == x.coordinate_map_key and out.F.dtype == dtype
    out.F.backward(dout)
    ours = {k: p.grad for k, p in layer.named_parameters()}
    ours["input"] = f.grad
    ref_out, ref = _mha_per_instance(state, torch.float64, feats, dout, batch, embed_dim, heads, bias)
    their_out, theirs = _mha_per_instance(state, dtype, feats, dout, batch, embed_dim, heads, bias)
    bad = []
    for name, a, b, r in [("out", out.F.detach(), their_out, ref_out)] + [(k, ours[k], theirs[k], ref[k]) for k in ref]:
        assert a is not None and torch.isfinite(a.float()).all(), name
        e, et = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"module {dtype} bias={bias} {host_layer} {name}: E_layer {e:.3e}  E_torch {et:.3e}  ratio {e / et if et else math.inf:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"beyond {FACTOR} x E_torch: {bad}"


def test_gradcheck_of_the_function_in_float64(device, host_layer):
    """2 instances of 3 and 5 query rows, H = 2, d = 4; q on the stride-2 map, k and v on the stride-1 map"""
    x, _ = make_tensor([6, 10], device, shuffle=True, seed=2)
    xq = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    bq = xq.C[:, 0]
    assert sorted([int((bq == 0).sum()), int((bq == 1).sum())]) == [3, 5]
    g = torch.Generator().manual_seed(3)
    q = torch.randn(xq.F.shape[0], 8, generator=g, dtype=torch.float64).to(device).requires_grad_()
    k = torch.randn(x.F.shape[0], 8, generator=g, dtype=torch.float64).to(device).requires_grad_()
    v = torch.randn(x.F.shape[0], 8, generator=g, dtype=torch.float64).to(device).requires_grad_()
    fn = ME.MinkowskiAttentionFunction

    def f(q_, k_, v_):
        return fn.apply(q_, k_, v_, 2, None, xq.coordinate_map_key, x.coordinate_map_key, None, x.coordinate_manager)
    assert torch.autograd.gradcheck(f, (q, k, v), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    ref = reference(q, k, v, torch.ones_like(q), bq.long(), x.C[:, 0].long(), 2)
    assert float((f(q, k, v).detach() - ref["out"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_functional_on_two_maps(device, host_layer, dtype):
    heads, d = 2, 32
    x, b1 = make_tensor([BK + 7, 2 * BK - 3], device, shuffle=True, seed=6)
    c = heads * d
    feats = draw(b1.numel(), c, dtype, device, 1)
    x = ME.SparseTensor(feats, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    xq = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    xv = ME.SparseTensor(draw(b1.numel(), c, dtype, device, 2), coordinate_map_key=x.coordinate_map_key,
                         coordinate_manager=x.coordinate_manager)
    y = ME.MinkowskiFunctional.scaled_dot_product_attention(xq, x, xv, heads)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == xq.coordinate_map_key
    assert tuple(y.F.shape) == tuple(xq.F.shape) and y.F.dtype == dtype
    bq = xq.C[:, 0].long()
    dout = torch.zeros_like(xq.F)
    ref = reference(xq.F, x.F, xv.F, dout, bq, b1, heads)
    theirs = torch_attention(xq.F, x.F, xv.F, dout, bq, b1, heads)
    e = float((y.F.double() - ref["out"]).abs().max())
    et = float((theirs["out"].double() - ref["out"]).abs().max())
    print(f"functional {dtype} {host_layer}: E_layer {e:.3e}  E_torch {et:.3e}")
    assert e <= FACTOR * et
    with pytest.raises(ValueError, match="share a coordinate map"):
        ME.MinkowskiFunctional.scaled_dot_product_attention(xq, x, xq, heads)


def test_bad_head_counts_raise_before_a_launch(device, host_layer):
    x, b = make_tensor([20, 9], device, seed=1)
    for c, heads, what in ((64, 3, "multiple of num_heads"), (96, 2, "head dimension")):
        t = ME.SparseTensor(torch.randn(b.numel(), c, device=device), coordinate_map_key=x.coordinate_map_key,
                            coordinate_manager=x.coordinate_manager)
        with pytest.raises(ValueError, match=what):
            ME.MinkowskiFunctional.scaled_dot_product_attention(t, t, t, heads)
    layer = ME.MinkowskiSelfAttention(96, 2).to(device)                          # head dimension 48 in fp32
    t = ME.SparseTensor(torch.randn(b.numel(), 96, device=device), coordinate_map_key=x.coordinate_map_key,
                        coordinate_manager=x.coordinate_manager)
    with pytest.raises(ValueError, match="head dimension"):
        layer(t)
    torch.cuda.synchronize(device)


def test_a_tensor_field_raises_a_clear_error(device, host_layer):
    coords = torch.tensor([[0, 0.2, 0.1, 0.0], [0, 1.4, 0.3, 0.2], [1, 0.1, 2.2, 0.5]])
    field = ME.TensorField(torch.randn(3, 64), coordinates=coords, device=device)
    with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
        ME.MinkowskiSelfAttention(64, 2).to(device)(field)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.scaled_dot_product_attention(field, field, field, 2)


def test_the_examples_block_runs(device, host_layer):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import attention_block as AB
    g = torch.Generator().manual_seed(0)
    scenes = []
    for b, (k, extent) in enumerate(((3000, 32), (900, 24))):                    # two scenes of different sizes
        pts = torch.unique(torch.randint(0, extent, (k, 3), generator=g), dim=0)
        scenes.append(torch.cat([torch.full((pts.shape[0], 1), b, dtype=torch.long), pts], 1))
    coords = torch.cat(scenes, 0).int().to(device)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(device), coords)
    y = AB.coarse_level(x, levels=2)
    assert y.tensor_stride[0] == 4
    block = AB.AttentionBlock(64, 2).to(device)
    out = block(y)
    assert tuple(out.F.shape) == tuple(y.F.shape)
    out.F.square().mean().backward()
    norm = float(block.attn.in_proj_weight.grad.norm())
    assert math.isfinite(norm) and norm > 0.0
