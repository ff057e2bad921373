"""GPU tests of MinkowskiLocalSelfAttention, MinkowskiLocalAttentionFunction and MinkowskiFunctional.local_attention (the
kernels of csrc/local_attention.hip through the operators of both host layers).

Yardstick of the module: the same block built from torch.nn.functional.linear and the gather formulation
(test_gpu_local_attention_kernels.yardstick's arithmetic, written here with autograd through the parameters) in float64.
Bound, as in test_gpu_local_attention_kernels.py: E_torch is the maximum absolute error of that torch block run in the dtype
under test; the layer must stay within FACTOR * E_torch per tensor (output, input gradient, every parameter gradient).
Figures are printed before the assertion."""
import math
import os
import sys

import pytest
import torch

import minkowskiengine_amd as ME
from test_gpu_local_attention_kernels import FACTOR, Scene, batched, draw, scattered, two_instances, yardstick

pytestmark = pytest.mark.gpu


def _torch_block(state, dtype, feats, dout, nbr, heads):
    """linear -> gather attention -> linear in `dtype` with the parameters `state` -> (out, grads by parameter name)"""
    p = {k: v.detach().to(dtype).requires_grad_() for k, v in state.items()}
    x = feats.detach().to(dtype).requires_grad_()
    n, c = x.shape
    d, vol = c // heads, nbr.shape[0]
    qkv = torch.nn.functional.linear(x, p["in_proj_weight"], p.get("in_proj_bias"))
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    idx, hole = nbr.clamp(min=0).t(), (nbr < 0).t()
    s = torch.einsum("nhd,nkhd->nhk", q.reshape(n, heads, d), k[idx].view(n, vol, heads, d)) / math.sqrt(d)
    if "rel_pos_bias" in p:
        s = s + p["rel_pos_bias"][None]
    w = torch.softmax(s.masked_fill(hole[:, None, :], -math.inf), -1)          # the centre offset is always present
    attn = torch.einsum("nhk,nkhd->nhd", w, v[idx].view(n, vol, heads, d)).reshape(n, c)
    out = torch.nn.functional.linear(attn, p["out_proj.weight"], p.get("out_proj.bias"))
    out.backward(dout.to(dtype))
    grads = {k: t.grad for k, t in p.items()}
    grads["input"] = x.grad
    return out.detach(), grads


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_module_equals_the_torch_block(device, host_layer, dtype, bias):
    embed_dim, heads = 64, 2
    sc = two_instances(device)
    torch.manual_seed(11)
    layer = ME.MinkowskiLocalSelfAttention(embed_dim, heads, bias=bias, rel_pos_bias=bias, dimension=3).to(device).to(dtype)
    with torch.no_grad():                                # the biases start at 0: give them something to do
        for name, p in layer.named_parameters():
            if "bias" in name:
                p.normal_(std=0.3)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    feats, dout = draw(sc.n_in, embed_dim, dtype, device, 1), draw(sc.n_in, embed_dim, dtype, device, 2)
    f = feats.clone().requires_grad_()
    out = layer(ME.SparseTensor(f, coordinate_map_key=sc.kv_key, coordinate_manager=sc.mgr))
    assert out.coordinate_map_key == sc.kv_key and out.F.dtype == dtype
    out.F.backward(dout)
    ours = {k: p.grad for k, p in layer.named_parameters()}
    ours["input"] = f.grad
    nbr = sc.table()
    ref_out, ref = _torch_block(state, torch.float64, feats, dout, nbr, heads)
    their_out, theirs = _torch_block(state, dtype, feats, dout, nbr, heads)
    assert set(ref) == set(ours)
    bad = []
    for name, a, b, r in [("out", out.F.detach(), their_out, ref_out)] + [(k, ours[k], theirs[k], ref[k]) for k in ref]:
        assert a is not None and a.dtype == dtype and torch.isfinite(a.float()).all(), name
        e, et = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"module {dtype} bias={bias} {host_layer} {name}: E_layer {e:.3e}  E_torch {et:.3e}  ratio {e / et if et else math.inf:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"beyond {FACTOR} x E_torch: {bad}"


def test_gradcheck_of_the_function_in_float64(device, host_layer):
    """10 rows, H = 2, d = 4, a bias table; the kernel-3 region on one map"""
    sc = Scene(batched(scattered(10, 3, 2)), device, kernel_size=3)
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(10, 8, generator=g, dtype=torch.float64).to(device).requires_grad_() for _ in range(3))
    bias = torch.randn(2, 27, generator=g, dtype=torch.float64).to(device).requires_grad_()

    def f(q_, k_, v_, b_):
        return ME.MinkowskiLocalAttentionFunction.apply(q_, k_, v_, b_, 2, None, sc.gen, sc.q_key, sc.kv_key, sc.mgr)
    assert torch.autograd.gradcheck(f, (q, k, v, bias), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    ref = yardstick(q, k, v, None, sc.table(), 2, bias)
    assert float((f(q, k, v, bias).detach() - ref["out"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_functional_on_two_maps(device, host_layer, dtype):
    """the query on the stride-2 map of the keys' manager: attention pooling over a 3x3x3 region"""
    heads, d = 2, 32
    c = heads * d
    sc = Scene(batched(scattered(300, 8, 9)), device, stride=2, kernel_size=3)
    xk = ME.SparseTensor(draw(sc.n_in, c, dtype, device, 1), coordinate_map_key=sc.kv_key, coordinate_manager=sc.mgr)
    xv = ME.SparseTensor(draw(sc.n_in, c, dtype, device, 2), coordinate_map_key=sc.kv_key, coordinate_manager=sc.mgr)
    xq = ME.SparseTensor(draw(sc.n_out, c, dtype, device, 3), coordinate_map_key=sc.q_key, coordinate_manager=sc.mgr)
    bias = draw(heads, 27, torch.float32, device, 4)
    y = ME.MinkowskiFunctional.local_attention(xq, xk, xv, heads, kernel_size=3, rel_pos_bias=bias)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == sc.q_key
    assert tuple(y.F.shape) == tuple(xq.F.shape) and y.F.dtype == dtype
    nbr = sc.table()
    ref = yardstick(xq.F, xk.F, xv.F, None, nbr, heads, bias)
    theirs = yardstick(xq.F, xk.F, xv.F, None, nbr, heads, bias, dtype=dtype)
    e = float((y.F.double() - ref["out"]).abs().max())
    et = float((theirs["out"].double() - ref["out"]).abs().max())
    print(f"functional {dtype} {host_layer}: E_layer {e:.3e}  E_torch {et:.3e}")
    assert e <= FACTOR * et
    same = ME.MinkowskiFunctional.local_attention(xk, xk, xv, heads)             # one map: stride 1, no bias
    assert same.coordinate_map_key == sc.kv_key and tuple(same.F.shape) == (sc.n_in, c)


def test_bad_head_counts_and_a_value_on_another_map_raise_before_a_launch(device, host_layer):
    sc = Scene(batched(scattered(60, 6, 1)), device, stride=2, kernel_size=3)

    def tensor(c, key=None, n=None):
        return ME.SparseTensor(torch.randn(n or sc.n_in, c, device=device), coordinate_map_key=key or sc.kv_key,
                               coordinate_manager=sc.mgr)
    for c, heads, what in ((64, 3, "multiple of num_heads"), (96, 2, "head dimension"), (8, 2, "head dimension")):
        t = tensor(c)
        with pytest.raises(ValueError, match=what):
            ME.MinkowskiFunctional.local_attention(t, t, t, heads)
    with pytest.raises(ValueError, match="head dimension"):
        ME.MinkowskiLocalSelfAttention(96, 2, dimension=3).to(device)(tensor(96))   # head dimension 48 in fp32
    t = tensor(64)
    with pytest.raises(ValueError, match="share a coordinate map"):
        ME.MinkowskiFunctional.local_attention(t, t, tensor(64, sc.q_key, sc.n_out), 2)
    with pytest.raises(ValueError, match="rel_pos_bias"):
        ME.MinkowskiFunctional.local_attention(t, t, t, 2, rel_pos_bias=torch.zeros(2, 26, device=device))
    torch.cuda.synchronize(device)


def test_a_tensor_field_raises_a_clear_error(device, host_layer):
    coords = torch.tensor([[0, 0.2, 0.1, 0.0], [0, 1.4, 0.3, 0.2], [1, 0.1, 2.2, 0.5]])
    field = ME.TensorField(torch.randn(3, 64), coordinates=coords, device=device)
    with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
        ME.MinkowskiLocalSelfAttention(64, 2, dimension=3).to(device)(field)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.local_attention(field, field, field, 2)


def test_the_examples_block_runs(device, host_layer):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import local_attention_block as LB
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 24, (3000, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(device)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(device), coords)
    block = LB.LocalAttentionBlock(64, 2).to(device)
    out = block(x)
    assert out.coordinate_map_key == x.coordinate_map_key and tuple(out.F.shape) == tuple(x.F.shape)
    out.F.square().mean().backward()
    for p in (block.attn.in_proj_weight, block.attn.rel_pos_bias, block.mlp[0].linear.weight):
        norm = float(p.grad.norm())
        assert math.isfinite(norm) and norm > 0.0
