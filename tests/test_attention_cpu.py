"""MinkowskiSelfAttention without a GPU: the public names, the parameters and their torch.nn.MultiheadAttention-shaped
state dict, the C ABI (header, ctypes table, exports, version, workspace size, host-only argument errors) and the operators
of both host layers."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("me_attn_workspace_bytes", "me_attn_forward", "me_attn_backward", "me_attn_forward_f64", "me_attn_backward_f64")
OPERATORS = ("AttentionForwardGPU", "AttentionBackwardGPU")
TABLE = 64   # a non-NULL table "pointer": the host-side checks never dereference it, and they fail before any launch


def _calls(lib, c=64, heads=2, stride=None, tables=TABLE, big=1 << 30, bf16=0):
    """the four launching entry points with every data pointer NULL: only the host-side checks can run"""
    s = c if stride is None else stride
    t = (tables,) * 4
    return (
        lambda: lib.me_attn_forward(None, None, None, bf16, s, s, s, *t, 10, 10, 2, c, heads, 0.125, None, s, None, None),
        lambda: lib.me_attn_backward(None, None, None, None, None, None, bf16, s, s, s, s, s, *t, 10, 10, 2, c, heads,
                                     0.125, None, s, None, s, None, s, None, big, None),
        lambda: lib.me_attn_forward_f64(None, None, None, s, s, s, *t, 10, 10, 2, c, heads, 0.125, None, s, None, None),
        lambda: lib.me_attn_backward_f64(None, None, None, None, None, None, s, s, s, s, s, *t, 10, 10, 2, c, heads, 0.125,
                                         None, s, None, s, None, s, None))


def test_names_are_exported():
    assert issubclass(ME.MinkowskiSelfAttention, torch.nn.Module)
    assert issubclass(ME.MinkowskiAttentionFunction, torch.autograd.Function)
    assert callable(ME.MinkowskiFunctional.scaled_dot_product_attention)
    assert "scaled_dot_product_attention" in ME.MinkowskiFunctional.__all__


@pytest.mark.parametrize("bias", [True, False])
def test_parameters_shapes_and_defaults(bias):
    layer = ME.MinkowskiSelfAttention(64, 2, bias=bias)
    assert (layer.embed_dim, layer.num_heads, layer.head_dim) == (64, 2, 32)
    named = {k: tuple(v.shape) for k, v in layer.named_parameters()}
    want = {"in_proj_weight": (192, 64), "out_proj.weight": (64, 64)}
    if bias:
        want.update({"in_proj_bias": (192,), "out_proj.bias": (64,)})
    assert named == want
    assert all(p.dtype == torch.float32 for p in layer.parameters())
    assert ME.MinkowskiSelfAttention(64, 2).in_proj_bias is not None            # bias defaults to True
    assert layer.double().in_proj_weight.dtype == torch.float64
    assert layer.bfloat16().out_proj.weight.dtype == torch.bfloat16


@pytest.mark.parametrize("bias", [True, False])
def test_initialisation_is_multihead_attentions(bias):
    torch.manual_seed(7)
    theirs = torch.nn.MultiheadAttention(64, 2, bias=bias, batch_first=True)
    torch.manual_seed(7)
    ours = ME.MinkowskiSelfAttention(64, 2, bias=bias)
    mine, other = ours.state_dict(), theirs.state_dict()
    assert list(mine) == list(other)
    for k in mine:
        assert torch.equal(mine[k], other[k]), k


@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly_in_both_directions(bias):
    theirs = torch.nn.MultiheadAttention(96, 3, bias=bias, batch_first=True)
    ours = ME.MinkowskiSelfAttention(96, 3, bias=bias)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    for k, t in theirs.state_dict().items():
        assert torch.equal(ours.state_dict()[k], t), k
    with torch.no_grad():
        for p in ours.parameters():
            p.add_(1.0)
    back = torch.nn.MultiheadAttention(96, 3, bias=bias, batch_first=True)
    back.load_state_dict(ours.state_dict(), strict=True)
    for k, t in ours.state_dict().items():
        assert torch.equal(back.state_dict()[k], t), k
    with pytest.raises(RuntimeError):                                           # strict: the other bias setting does not load
        ME.MinkowskiSelfAttention(96, 3, bias=not bias).load_state_dict(theirs.state_dict(), strict=True)


def test_repr():
    assert repr(ME.MinkowskiSelfAttention(64, 2)) == "MinkowskiSelfAttention(64, 2, bias=True)"
    assert repr(ME.MinkowskiSelfAttention(256, 8, bias=False)) == "MinkowskiSelfAttention(256, 8, bias=False)"


def test_embed_dim_must_divide_into_heads():
    with pytest.raises(ValueError):
        ME.MinkowskiSelfAttention(100, 3)
    with pytest.raises(ValueError):
        ME.MinkowskiSelfAttention(64, 0)


def test_module_and_functional_take_sparse_tensors_only():
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiSelfAttention(64, 2)(torch.zeros(4, 64))
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.scaled_dot_product_attention(torch.zeros(4, 64), torch.zeros(4, 64), torch.zeros(4, 64), 2)


def test_cpu_tensors_have_no_operator():
    for name in OPERATORS:
        assert hasattr(backend, name), name
    with pytest.raises(ValueError, match="AttentionForwardCPU"):
        ME.get_minkowski_function("AttentionForward", torch.zeros(1))
    with pytest.raises(ValueError, match="AttentionBackwardCPU"):
        ME.get_minkowski_function("AttentionBackward", torch.zeros(1))


def test_c_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/me_amd.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.me_version() >= 270
    assert re.search(r"1\.17 \(270\)\s+round 17:", header)


def test_workspace_bytes_are_monotone():
    lib = _lib.load()
    ns = (0, 1, 100, 5000, 100000, 10 ** 7)
    sizes = [lib.me_attn_workspace_bytes(n, n, 2, 4) for n in ns]
    assert sizes == sorted(sizes) and sizes[1] < sizes[-1]
    for n, size in zip(ns, sizes):
        assert size >= n * 4 * 4                                                # delta [n_q, heads] fp32
    by_batch = [lib.me_attn_workspace_bytes(5000, 5000, b, 4) for b in (1, 2, 16, 1000)]
    assert by_batch == sorted(by_batch)
    by_heads = [lib.me_attn_workspace_bytes(5000, 5000, 2, h) for h in (1, 2, 8)]
    assert by_heads == sorted(by_heads) and by_heads[0] < by_heads[-1]


@pytest.mark.parametrize("c,heads", [(64, 3), (100, 8), (64, 0), (64, -1)])
def test_channels_must_divide_into_heads_host_side(c, heads):
    """checked before anything touches a device: every data pointer is NULL and no GPU is needed"""
    lib = _lib.load()
    for call in _calls(lib, c=c, heads=heads):
        assert call() != 0
        assert "head" in lib.me_last_error().decode()


@pytest.mark.parametrize("c,heads", [(96, 2), (16, 1), (512, 2), (40, 1)])
def test_a_bad_head_dimension_is_a_host_side_error(c, heads):
    lib = _lib.load()
    for bf16 in (0, 1):
        for call in _calls(lib, c=c, heads=heads, bf16=bf16)[:2]:
            assert call() != 0
            assert "head dimension must be 32, 64 or 128" in lib.me_last_error().decode()
    forward_f64 = _calls(lib, c=c, heads=heads)[2]                              # float64: any head dimension; the next check fires
    assert forward_f64() != 0
    assert "null data pointer" in lib.me_last_error().decode()


def test_a_misaligned_or_short_stride_is_a_host_side_error():
    lib = _lib.load()
    for stride, bf16 in ((66, 0), (68, 1), (63, 0), (32, 1)):                   # 66 floats / 68 bf16: no multiple of 16 bytes
        for call in _calls(lib, stride=stride, bf16=bf16)[:2]:
            assert call() != 0
            assert "row stride" in lib.me_last_error().decode()
    for call in _calls(lib, stride=68, bf16=0)[:1] + _calls(lib, stride=72, bf16=1)[:1]:   # aligned: past the stride check
        assert call() != 0
        assert "null data pointer" in lib.me_last_error().decode()
    for call in _calls(lib, stride=63)[2:]:                                     # float64: only stride >= c
        assert call() != 0
        assert "row stride" in lib.me_last_error().decode()


def test_a_short_workspace_is_a_host_side_error():
    lib = _lib.load()
    need = lib.me_attn_workspace_bytes(10, 10, 2, 2)
    assert need > 0
    backward = _calls(lib, big=need - 1)[1]
    assert backward() != 0
    assert "workspace too small" in lib.me_last_error().decode()


def test_a_missing_table_pointer_is_a_host_side_error():
    lib = _lib.load()
    for call in _calls(lib, tables=None):
        assert call() != 0
        assert "table pointer" in lib.me_last_error().decode()


def test_both_host_layers_expose_the_operators():
    for name in OPERATORS:
        assert callable(getattr(backend, name))
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in OPERATORS:
        assert hasattr(native, name), name
