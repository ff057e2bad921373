"""Rotary position embedding on the GPU, through both host layers: the autograd function, the manager's table cache, the
module and functional forms, and the `rope=True` argument of the three self-attention modules.

The yardstick is the float64 numpy definition of tests/test_rope_cpu.py; the fp32 bound per pair, 2^-21 hypot(x0, x1), is
the one derived in tests/test_gpu_rope_kernels.py (coordinates here stay far below 2^20 cells)."""
import gc
import weakref

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from test_gpu_attention_kernels import draw
from test_gpu_rope_kernels import apply as abi_apply, pair_excess
from test_gpu_window_attention import _equal, random_scene, scene_of
from test_rope_cpu import rope_angles, rope_apply, rope_table
from test_window_attention_cpu import WINDOW, edges_scene

pytestmark = pytest.mark.gpu
FN = ME.MinkowskiRotaryEmbeddingFunction


def rotate(x, feats, heads, base=10000.0, unit=None):
    return FN.apply(feats, heads, base, unit, x.coordinate_map_key, x.coordinate_manager)


def _f64(t):
    return t.detach().cpu().double().numpy()


# ---- the function ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_two_calls_and_two_hosts_are_bitwise_equal_and_backward_is_the_negative_sign(device, dtype):
    heads, d = 3, 32
    coords = random_scene((150, 90), (0, 2), 3, 1, seed=1, lo=-400, hi=400)
    results = []
    prev = ME.get_host()
    try:
        for layer in ("python", "native", "python"):
            ME.set_host(layer)
            x = scene_of(coords, device)
            feats, dout = draw(240, heads * d, dtype, device, 1), draw(240, heads * d, dtype, device, 2)
            for _ in range(2):
                f = feats.clone().requires_grad_()
                y = rotate(x, f, heads)
                assert y.is_contiguous() and y.dtype == dtype
                y.backward(dout)
                results.append((y.detach(), f.grad))
            table = x.coordinate_manager.rope_table(x.coordinate_map_key, d, dtype=torch.float64 if dtype == torch.float64
                                                    else torch.float32)
            results.append((abi_apply(feats, heads, d, table, 1), abi_apply(dout, heads, d, table, -1)))
    finally:
        ME.set_host(prev)
    for y, dx in results[1:]:
        assert _equal(results[0][0], y) and _equal(results[0][1], dx)
    if dtype == torch.float32:
        x64 = _f64(feats)
        assert pair_excess(_f64(results[0][0]), rope_apply(x64, coords, heads), x64, 2.0 ** -21) <= 1.0
        g64 = _f64(dout)
        assert pair_excess(_f64(results[0][1]), rope_apply(g64, coords, heads, sign=-1), g64, 2.0 ** -21) <= 1.0


def test_gradient_through_a_strided_input_view(device, host_layer):
    """x = the first 2C columns of a [n, 3C] leaf: its gradient is the output gradient rotated back, zero in the rest"""
    heads, d = 2, 32
    c = heads * d
    coords = random_scene((100, 60), (0, 1), 3, 1, seed=2)
    x = scene_of(coords, device)
    qkv = draw(160, 3 * c, torch.float32, device, 3).requires_grad_()
    dout = draw(160, 2 * c, torch.float32, device, 4)
    y = rotate(x, qkv[:, :2 * c], 2 * heads)
    y.backward(dout)
    x64, g64 = _f64(qkv)[:, :2 * c], _f64(dout)
    assert pair_excess(_f64(y), rope_apply(x64, coords, 2 * heads), x64, 2.0 ** -21) <= 1.0
    assert pair_excess(_f64(qkv.grad[:, :2 * c]), rope_apply(g64, coords, 2 * heads, sign=-1), g64, 2.0 ** -21) <= 1.0
    assert not qkv.grad[:, 2 * c:].any()
    contiguous = rotate(x, qkv.detach()[:, :2 * c].contiguous(), 2 * heads)
    assert _equal(contiguous, y.detach())


def test_gradcheck_of_the_function_in_float64(device, host_layer):
    """12 rows, D = 3, 2 heads of 6: one pair per axis at frequency 1"""
    coords = random_scene((7, 5), (0, 1), 3, 1, seed=3, lo=-6, hi=7)
    x = scene_of(coords, device)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(12, 12, generator=g, dtype=torch.float64).to(device).requires_grad_()
    assert torch.autograd.gradcheck(lambda f: rotate(x, f, 2), (feats,), eps=1e-6, atol=1e-8, rtol=1e-6, nondet_tol=0.0)
    assert np.abs(_f64(rotate(x, feats, 2)) - rope_apply(_f64(feats), coords, 2)).max() <= 1e-14
    assert torch.autograd.gradcheck(lambda f: rotate(x, f, 2, 50.0, (1, 2, 3)), (feats,), eps=1e-6, atol=1e-8, rtol=1e-6,
                                    nondet_tol=0.0)


def test_strided_and_pruned_maps_and_units(device, host_layer):
    """the default unit is the tensor stride of the map; unit= overrides it; a pruned map keeps its rows' angles"""
    heads, d = 2, 20
    x = scene_of(random_scene((150, 90, 60), (0, 1, 2), 3, 1, seed=5), device)
    y = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    assert y.tensor_stride[0] == 2
    z = ME.MinkowskiPruning()(x, x.C[:, 0] != 1)
    assert z.F.shape[0] == 210
    for t, default in ((x, 1), (y, 2), (z, 1)):
        n = t.F.shape[0]
        feats = draw(n, heads * d, torch.float32, device, 7)
        x64, c = _f64(feats), t.C.cpu().numpy()
        for unit, want_unit in ((None, default), (1, 1), (3, 3), ((1, 2, 4), (1, 2, 4))):
            got = _f64(rotate(t, feats, heads, unit=unit))
            assert pair_excess(got, rope_apply(x64, c, heads, unit=want_unit), x64, 2.0 ** -21) <= 1.0, (default, unit)
        got = _f64(rotate(t, feats, heads, base=100.0))
        assert pair_excess(got, rope_apply(x64, c, heads, base=100.0, unit=default), x64, 2.0 ** -21) <= 1.0
    feats = draw(y.F.shape[0], heads * d, torch.float32, device, 7)
    assert not _equal(rotate(y, feats, heads), rotate(y, feats, heads, unit=1))


def test_module_and_functional_forms(device, host_layer):
    coords = random_scene((80, 40), (0, 1), 3, 1, seed=8)
    x = scene_of(coords, device)
    feats = draw(120, 64, torch.float32, device, 9)
    xin = ME.SparseTensor(feats, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    want = rotate(x, feats, 2, 500.0, (1, 2, 1))
    out = ME.MinkowskiRotaryEmbedding(2, base=500.0, unit=(1, 2, 1))(xin)
    assert isinstance(out, ME.SparseTensor) and out.coordinate_map_key == x.coordinate_map_key and _equal(out.F, want)
    out = ME.MinkowskiFunctional.rotary_embedding(xin, 2, base=500.0, unit=(1, 2, 1))
    assert out.coordinate_map_key == x.coordinate_map_key and _equal(out.F, want)
    assert _equal(ME.MinkowskiFunctional.rotary_embedding(xin, 2).F, rotate(x, feats, 2))
    with pytest.raises(ValueError, match="multiple of num_heads"):
        rotate(x, feats, 3)
    with pytest.raises(ValueError, match="even"):
        rotate(x, feats[:, :10], 2)
    with pytest.raises(ValueError, match="per spatial axis"):
        rotate(x, feats[:, :8], 2)                                      # heads of 4: two pairs for three axes
    with pytest.raises(ValueError, match="per spatial axis"):
        rotate(x, feats, 2, unit=(1, 1))
    with pytest.raises(RuntimeError, match="Invalid x size"):
        rotate(x, feats[:100], 2)
    torch.cuda.synchronize(device)


# ---- the cache -------------------------------------------------------------------------------------------------------------
def test_cached_tables(device, host_layer):
    x = scene_of(random_scene((150, 90), (0, 1), 3, 1, seed=6), device)
    cm, key = x.coordinate_manager, x.coordinate_map_key
    got = cm.rope_table(key, 32)
    assert got.shape == (240, 16, 2) and got.dtype == torch.float32
    assert np.abs(_f64(got) - rope_table(x.C.cpu().numpy(), 32)).max() <= 2.0 ** -24
    for same in (cm.rope_table(key, 32), cm.rope_table(key, 32, 10000.0, None, torch.float32), cm.rope_table(key, 32, unit=1),
                 cm.rope_table(key, 32, unit=(1, 1, 1))):
        assert same.data_ptr() == got.data_ptr()
    others = [cm.rope_table(key, 64), cm.rope_table(key, 32, base=100.0), cm.rope_table(key, 32, unit=2),
              cm.rope_table(key, 32, unit=(1, 1, 2)), cm.rope_table(key, 32, dtype=torch.float64)]
    assert len({t.data_ptr() for t in others + [got]}) == 6
    assert others[4].dtype == torch.float64 and others[0].shape == (240, 32, 2)
    _, t_abs = rope_angles(x.C.cpu().numpy(), 32)
    assert (np.abs(_f64(others[4]) - rope_table(x.C.cpu().numpy(), 32)) <= 2.0 ** -52 + t_abs[..., None] * 2.0 ** -51).all()
    rotate(x, draw(240, 64, torch.float32, device, 1), 2)             # the function takes the entry of d = 32
    with pytest.raises(ValueError, match="float32 or float64"):
        cm.rope_table(key, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="even"):
        cm.rope_table(key, 7)
    if host_layer == "python":
        mgr = cm._manager
        assert len(mgr._rope_table_cache) == 6
        assert all(any(t is h for h in mgr.device_tensors()) for t in others + [got])
        ref = weakref.ref(mgr)
        del mgr, cm, x, got, same, others
        gc.collect()
        assert ref() is None


# ---- the self-attention modules ------------------------------------------------------------------------------------------------
def _attention(kind, q, k, v, heads, key, cm):
    if kind == "instance":
        return ME.MinkowskiAttentionFunction.apply(q, k, v, heads, None, key, key, None, cm)
    if kind == "serialized":
        return ME.MinkowskiSerializedAttentionFunction.apply(q, k, v, heads, None, 128, "z", key, cm)
    return ME.MinkowskiWindowAttentionFunction.apply(q, k, v, heads, None, WINDOW, (4, 0, 4), key, cm)


def _module(kind, embed_dim, heads, **kw):
    if kind == "instance":
        return ME.MinkowskiSelfAttention(embed_dim, heads, **kw)
    if kind == "serialized":
        return ME.MinkowskiSerializedSelfAttention(embed_dim, heads, patch_size=128, order="z", **kw)
    return ME.MinkowskiWindowSelfAttention(embed_dim, heads, window_size=WINDOW, shift=(4, 0, 4), **kw)


KINDS = ("instance", "serialized", "window")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_rope_modules_equal_the_manual_composition(device, host_layer, kind, dtype):
    """two instances, 64 channels in 2 heads, windows of 1 to 150 rows: linear -> the rotary function on qkv[:, :2C] with 2H
    heads -> the module's attention function -> output projection, bit for bit, the parameter gradients included"""
    embed_dim, heads = 64, 2
    c = embed_dim
    x = scene_of(edges_scene(), device)
    n, key, cm = x.F.shape[0], x.coordinate_map_key, x.coordinate_manager
    torch.manual_seed(11)
    layer = _module(kind, embed_dim, heads, rope=True, rope_base=100.0).to(device).to(dtype)
    with torch.no_grad():
        layer.in_proj_bias.normal_(std=0.3)
        layer.out_proj.bias.normal_(std=0.3)
    feats, dout = draw(n, embed_dim, dtype, device, 1), draw(n, embed_dim, dtype, device, 2)

    f = feats.clone().requires_grad_()
    out = layer(ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=cm))
    out.F.backward(dout)
    ours = {k: p.grad.clone() for k, p in layer.named_parameters()}
    ours["input"] = f.grad

    layer.zero_grad(set_to_none=True)
    f2 = feats.clone().requires_grad_()
    qkv = torch.nn.functional.linear(f2, layer.in_proj_weight, layer.in_proj_bias)
    qk = FN.apply(qkv[:, :2 * c], 2 * heads, 100.0, None, key, cm)
    attn = _attention(kind, qk[:, :c], qk[:, c:], qkv[:, 2 * c:], heads, key, cm)
    manual = torch.nn.functional.linear(attn, layer.out_proj.weight, layer.out_proj.bias)
    manual.backward(dout)
    theirs = {k: p.grad for k, p in layer.named_parameters()}
    theirs["input"] = f2.grad

    assert _equal(out.F.detach(), manual.detach())
    for name in ours:
        assert ours[name] is not None and _equal(ours[name], theirs[name]), name
    plain = _module(kind, embed_dim, heads).to(device).to(dtype)
    plain.load_state_dict(layer.state_dict(), strict=True)
    other = plain(ME.SparseTensor(feats, coordinate_map_key=key, coordinate_manager=cm)).F.detach()
    assert float((other.float() - out.F.detach().float()).abs().max()) > 1e-3


@pytest.mark.parametrize("kind", KINDS)
def test_rope_modules_are_translation_invariant_in_float64(device, host_layer, kind):
    """the same scene moved by (1000, -2048, 512) cells (multiples of the window, so the windows hold the same rows; the
    serialized patches hold whole instances) in a fresh manager: the rows keep their order, so row i answers row i"""
    embed_dim, heads = 64, 2
    coords = edges_scene()
    moved = coords + np.array([0, 1000, -2048, 512])
    torch.manual_seed(5)
    kw = {"patch_size": 1024} if kind == "serialized" else {}
    cls = {"instance": ME.MinkowskiSelfAttention, "serialized": ME.MinkowskiSerializedSelfAttention,
           "window": ME.MinkowskiWindowSelfAttention}[kind]
    rope = cls(embed_dim, heads, rope=True, **kw).to(device).double()
    plain = cls(embed_dim, heads, **kw).to(device).double()
    plain.load_state_dict(rope.state_dict(), strict=True)
    feats = draw(coords.shape[0], embed_dim, torch.float64, device, 3)
    outs = []
    for rows in (coords, moved):
        x = scene_of(rows, device)
        xin = ME.SparseTensor(feats, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
        outs.append((rope(xin).F.detach(), plain(xin).F.detach()))
    scale = float(outs[0][0].abs().max())
    diff = float((outs[0][0] - outs[1][0]).abs().max())
    print(f"{kind} {host_layer}: translated |diff| / max |out| = {diff / scale:.3e}")
    assert diff <= 1e-9 * scale
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 1e-9 * scale       # (without rope the layer never saw positions)
    assert float((outs[0][0] - outs[0][1]).abs().max()) > 1e-3 * scale        # rope changes the result by far more


def test_the_examples_stage_runs(device, host_layer):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import rope_attention_block
    finally:
        sys.path.pop(0)
    loss = rope_attention_block.main(device=device, steps=2, voxels=20000, side=48, quiet=True)
    assert loss == loss and loss < float("inf")
