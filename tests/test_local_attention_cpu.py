"""MinkowskiLocalSelfAttention without a GPU: the public names, the parameters and their MinkowskiSelfAttention-shaped state
dict, the C ABI (header, ctypes table, exports, version, workspace size, host-only argument errors), the operators of both
host layers, and the yardstick of the GPU tests (tests/test_gpu_local_attention_kernels.py `yardstick`) on the CPU in
float64 against a plain Python loop over a coordinate dictionary."""
import itertools
import math
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("me_local_attn_workspace_bytes", "me_local_attn_forward", "me_local_attn_backward",
           "me_local_attn_forward_f64", "me_local_attn_backward_f64")
OPERATORS = ("LocalAttentionForwardGPU", "LocalAttentionBackwardGPU")
TABLE = 64   # a non-NULL table "pointer": the host-side checks never dereference it, and they fail before any launch


def _calls(lib, c=64, heads=2, stride=None, tables=TABLE, big=1 << 30, bf16=0, volume=27):
    """the four launching entry points with every data pointer NULL: only the host-side checks can run"""
    s = c if stride is None else stride
    return (
        lambda: lib.me_local_attn_forward(None, None, None, bf16, s, s, s, tables, 10, 10, volume, c, heads, 0.125, None,
                                          None, s, None, None, None),
        lambda: lib.me_local_attn_backward(None, None, None, None, None, None, None, bf16, s, s, s, s, s, tables, tables, 10,
                                           10, volume, c, heads, 0.125, None, None, s, None, s, None, s, None, None, big,
                                           None),
        lambda: lib.me_local_attn_forward_f64(None, None, None, s, s, s, tables, 10, 10, volume, c, heads, 0.125, None, None,
                                              s, None, None),
        lambda: lib.me_local_attn_backward_f64(None, None, None, None, None, None, s, s, s, s, s, tables, tables, 10, 10,
                                               volume, c, heads, 0.125, None, None, s, None, s, None, s, None, None))


def test_names_are_exported():
    assert issubclass(ME.MinkowskiLocalSelfAttention, torch.nn.Module)
    assert issubclass(ME.MinkowskiLocalAttentionFunction, torch.autograd.Function)
    assert callable(ME.MinkowskiFunctional.local_attention)
    assert "local_attention" in ME.MinkowskiFunctional.__all__


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rel", [True, False])
def test_parameters_shapes_defaults_and_initialisation(bias, rel):
    layer = ME.MinkowskiLocalSelfAttention(64, 2, bias=bias, rel_pos_bias=rel, dimension=3)
    assert (layer.embed_dim, layer.num_heads, layer.head_dim) == (64, 2, 32)
    assert layer.kernel_generator.kernel_size == [3, 3, 3] and layer.kernel_generator.kernel_dilation == [1, 1, 1]
    named = {k: tuple(v.shape) for k, v in layer.named_parameters()}
    want = {"in_proj_weight": (192, 64), "out_proj.weight": (64, 64)}
    if bias:
        want.update({"in_proj_bias": (192,), "out_proj.bias": (64,)})
    if rel:
        want["rel_pos_bias"] = (2, 27)
        assert torch.count_nonzero(layer.rel_pos_bias) == 0                     # initialised to zero
    assert named == want
    assert all(p.dtype == torch.float32 for p in layer.parameters())
    default = ME.MinkowskiLocalSelfAttention(64, 2, dimension=3)
    assert default.in_proj_bias is not None and default.rel_pos_bias is not None
    assert tuple(ME.MinkowskiLocalSelfAttention(32, 4, kernel_size=5, dilation=2, dimension=2).rel_pos_bias.shape) == (4, 25)
    torch.manual_seed(7)
    theirs = ME.MinkowskiSelfAttention(64, 2, bias=bias)
    torch.manual_seed(7)
    ours = ME.MinkowskiLocalSelfAttention(64, 2, bias=bias, rel_pos_bias=rel, dimension=3)
    for k, t in theirs.state_dict().items():
        assert torch.equal(ours.state_dict()[k], t), k
    assert layer.double().in_proj_weight.dtype == torch.float64
    assert layer.bfloat16().out_proj.weight.dtype == torch.bfloat16


def test_a_custom_kernel_generator_sets_the_bias_width():
    gen = ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=[[0, 0, 0], [1, 0, 0], [0, 2, 1]], dimension=3)
    layer = ME.MinkowskiLocalSelfAttention(32, 2, kernel_generator=gen)
    assert tuple(layer.rel_pos_bias.shape) == (2, 3) and layer.dimension == 3
    with pytest.raises(ValueError, match="stride"):
        ME.MinkowskiLocalSelfAttention(32, 2, kernel_generator=ME.KernelGenerator(kernel_size=3, stride=2, dimension=3))


@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_to_and_from_the_global_layer(bias):
    glob = ME.MinkowskiSelfAttention(96, 3, bias=bias)
    plain = ME.MinkowskiLocalSelfAttention(96, 3, bias=bias, rel_pos_bias=False, dimension=3)
    plain.load_state_dict(glob.state_dict(), strict=True)                       # the same names without the bias table
    assert list(plain.state_dict()) == list(glob.state_dict())
    local = ME.MinkowskiLocalSelfAttention(96, 3, bias=bias, dimension=3)
    with pytest.raises(RuntimeError, match="rel_pos_bias"):
        local.load_state_dict(glob.state_dict(), strict=True)
    missing = local.load_state_dict(glob.state_dict(), strict=False)
    assert missing.missing_keys == ["rel_pos_bias"] and missing.unexpected_keys == []
    for k, t in glob.state_dict().items():
        assert torch.equal(local.state_dict()[k], t), k
    back = ME.MinkowskiSelfAttention(96, 3, bias=bias)
    extra = back.load_state_dict(local.state_dict(), strict=False)
    assert extra.unexpected_keys == ["rel_pos_bias"] and extra.missing_keys == []


def test_repr():
    assert repr(ME.MinkowskiLocalSelfAttention(64, 2, dimension=3)) == \
        "MinkowskiLocalSelfAttention(64, 2, kernel_size=[3, 3, 3], dilation=[1, 1, 1], bias=True, rel_pos_bias=True)"
    assert repr(ME.MinkowskiLocalSelfAttention(256, 8, kernel_size=5, dilation=2, bias=False, rel_pos_bias=False, dimension=2)) \
        == "MinkowskiLocalSelfAttention(256, 8, kernel_size=[5, 5], dilation=[2, 2], bias=False, rel_pos_bias=False)"


def test_embed_dim_must_divide_into_heads():
    with pytest.raises(ValueError):
        ME.MinkowskiLocalSelfAttention(100, 3, dimension=3)
    with pytest.raises(ValueError):
        ME.MinkowskiLocalSelfAttention(64, 0, dimension=3)


def test_module_and_functional_take_sparse_tensors_only():
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiLocalSelfAttention(64, 2, dimension=3)(torch.zeros(4, 64))
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.local_attention(torch.zeros(4, 64), torch.zeros(4, 64), torch.zeros(4, 64), 2)


def test_cpu_tensors_have_no_operator():
    for name in OPERATORS:
        assert hasattr(backend, name), name
    with pytest.raises(ValueError, match="LocalAttentionForwardCPU"):
        ME.get_minkowski_function("LocalAttentionForward", torch.zeros(1))
    with pytest.raises(ValueError, match="LocalAttentionBackwardCPU"):
        ME.get_minkowski_function("LocalAttentionBackward", torch.zeros(1))


def test_c_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/me_amd.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype"
        assert hasattr(lib, s), f"{s} is not exported"
        declared = re.search(r"\b" + s + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[s][1]), f"{s}: the prototype and the header disagree"
    assert lib.me_version() >= 280
    assert re.search(r"1\.18 \(280\)\s+round 18:", header)


def test_workspace_bytes_are_monotone():
    lib = _lib.load()
    ns = (0, 1, 100, 5000, 100000, 10 ** 7)
    for with_bias in (0, 1):
        sizes = [lib.me_local_attn_workspace_bytes(n, 4, 27, with_bias) for n in ns]
        assert sizes == sorted(sizes) and sizes[1] < sizes[-1]
        for n, size in zip(ns, sizes):
            assert size >= n * 4 * 4                                            # delta [n_out, heads] fp32
        by_heads = [lib.me_local_attn_workspace_bytes(5000, h, 27, with_bias) for h in (1, 2, 8)]
        assert by_heads == sorted(by_heads) and by_heads[0] < by_heads[-1]
        by_volume = [lib.me_local_attn_workspace_bytes(5000, 4, k, with_bias) for k in (1, 8, 27, 125)]
        assert by_volume == sorted(by_volume)
        assert with_bias == 0 or by_volume[0] < by_volume[-1]                   # only the bias sums grow with the volume
    assert lib.me_local_attn_workspace_bytes(5000, 4, 27, 1) > lib.me_local_attn_workspace_bytes(5000, 4, 27, 0)


@pytest.mark.parametrize("c,heads", [(64, 3), (100, 8), (64, 0), (64, -1)])
def test_channels_must_divide_into_heads_host_side(c, heads):
    """checked before anything touches a device: every data pointer is NULL and no GPU is needed"""
    lib = _lib.load()
    for call in _calls(lib, c=c, heads=heads):
        assert call() != 0
        assert "head" in lib.me_last_error().decode()


@pytest.mark.parametrize("c,heads", [(96, 2), (4, 1), (512, 2), (40, 1), (24, 2)])
def test_a_bad_head_dimension_is_a_host_side_error(c, heads):
    lib = _lib.load()
    for bf16 in (0, 1):
        for call in _calls(lib, c=c, heads=heads, bf16=bf16)[:2]:
            assert call() != 0
            assert "head dimension must be a power of two from 8 to 128" in lib.me_last_error().decode()
    forward_f64 = _calls(lib, c=c, heads=heads)[2]                              # float64: any head dimension; the next check fires
    assert forward_f64() != 0
    assert "null data pointer" in lib.me_last_error().decode()


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_every_head_dimension_of_the_rule_passes_the_host_checks(d):
    lib = _lib.load()
    for bf16 in (0, 1):
        forward = _calls(lib, c=3 * d, heads=3, bf16=bf16)[0]
        assert forward() != 0
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
    need = lib.me_local_attn_workspace_bytes(10, 2, 27, 0)
    assert need > 0
    backward = _calls(lib, big=need - 1)[1]
    assert backward() != 0
    assert "workspace too small" in lib.me_last_error().decode()


def test_a_missing_table_pointer_is_a_host_side_error():
    lib = _lib.load()
    for call in _calls(lib, tables=None):
        assert call() != 0
        assert "table pointer" in lib.me_last_error().decode()


@pytest.mark.parametrize("volume", [0, -1, (1 << 20) + 1])
def test_a_volume_out_of_range_is_a_host_side_error(volume):
    lib = _lib.load()
    for call in _calls(lib, volume=volume):
        assert call() != 0
        assert "volume out of range" in lib.me_last_error().decode()


def test_both_host_layers_expose_the_operators():
    for name in OPERATORS:
        assert callable(getattr(backend, name))
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in OPERATORS:
        assert hasattr(native, name), name


# ---- the yardstick of the GPU tests against a plain Python loop ------------------------------------------------------------
def _python_loop(coords_q, coords_kv, offsets, q, k, v, bias, heads, scale):
    """out and lse row by row, head by head, offset by offset, through a dictionary coordinate -> row"""
    rows = {tuple(c): j for j, c in enumerate(coords_kv)}
    d = q.shape[1] // heads
    out = torch.zeros_like(q)
    lse = torch.full((len(coords_q), heads), -math.inf, dtype=torch.float64)
    nbr = torch.full((len(offsets), len(coords_q)), -1, dtype=torch.int64)
    for i, u in enumerate(coords_q):
        for kk, off in enumerate(offsets):
            nbr[kk, i] = rows.get(tuple(a + b for a, b in zip(u, off)), -1)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            terms = [(scale * float(q[i, sl] @ k[j, sl]) + float(bias[h, kk]), j)
                     for kk, j in enumerate(nbr[:, i].tolist()) if j >= 0]
            if not terms:
                continue
            total = sum(math.exp(s) for s, _ in terms)
            lse[i, h] = math.log(total)
            for s, j in terms:
                out[i, sl] += math.exp(s) / total * v[j, sl]
    return nbr, out, lse


def test_the_yardstick_of_the_gpu_tests_matches_a_plain_python_loop():
    from test_gpu_local_attention_kernels import yardstick
    g = torch.Generator().manual_seed(3)
    pts = torch.unique(torch.randint(0, 5, (60, 3), generator=g), dim=0)
    coords_kv = [tuple(p) for p in pts.tolist()]
    coords_q = coords_kv[::2] + [(40, 40, 40)]                                  # the last query has no neighbour
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 1, 0)]
    heads, d = 2, 3
    q = torch.randn(len(coords_q), heads * d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(len(coords_kv), heads * d, generator=g, dtype=torch.float64) for _ in range(2))
    bias = torch.randn(heads, len(offsets), generator=g, dtype=torch.float64)
    dout = torch.randn(len(coords_q), heads * d, generator=g, dtype=torch.float64)
    scale = 0.7
    nbr, out, lse = _python_loop(coords_q, coords_kv, offsets, q, k, v, bias, heads, scale)
    assert int((nbr[:, -1] >= 0).sum()) == 0 and int((nbr >= 0).sum()) > 100
    got = yardstick(q, k, v, dout, nbr, heads, bias, scale)
    assert float((got["out"] - out).abs().max()) < 1e-12
    assert torch.equal(torch.isfinite(got["lse"]), torch.isfinite(lse)) and got["lse"][-1, 0] == -math.inf
    finite = torch.isfinite(lse)
    assert float((got["lse"][finite] - lse[finite]).abs().max()) < 1e-12
    assert torch.count_nonzero(got["out"][-1]) == 0 and torch.count_nonzero(got["dq"][-1]) == 0
    # the gradients of the loop by autograd through the same loop arithmetic on the dense formulation: finite differences
    eps = 1e-6
    for name, t in (("dq", q), ("dk", k), ("dv", v), ("dbias", bias)):
        flat = t.view(-1)
        for pos in (0, flat.numel() // 2, flat.numel() - 1 - (heads * d if name == "dq" else 0)):
            keep = float(flat[pos])
            flat[pos] = keep + eps
            up = float((_python_loop(coords_q, coords_kv, offsets, q, k, v, bias, heads, scale)[1] * dout).sum())
            flat[pos] = keep - eps
            down = float((_python_loop(coords_q, coords_kv, offsets, q, k, v, bias, heads, scale)[1] * dout).sum())
            flat[pos] = keep
            assert abs((up - down) / (2 * eps) - float(got[name].view(-1)[pos])) < 1e-6, (name, pos)
