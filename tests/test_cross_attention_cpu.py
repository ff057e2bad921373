"""Host-side checks of cross-attention to a dense context (no GPU): the module against torch.nn.MultiheadAttention
(parameters, initialisation, state dicts), the errors raised before any launch, the ABI 1.20 symbols, the workspace
size, the policy me_attn_kv_splits and the host-side errors of the entry points, called with null data pointers."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

import minkowskiengine_amd as ME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

MAX_SPLITS = 32                 # ME_ATTN_MAX_KV_SPLITS
IMAGE_CAP = 64 << 20            # the documented cap on the partial images: 2 * S * n_kv * c * 4 bytes
SYMBOLS = ("me_attn_context_lists", "me_attn_kv_splits", "me_attn_split_workspace_bytes", "me_attn_backward_split",
           "me_attn_backward_split_f64")
DIMS = [dict(), dict(kdim=96, vdim=48), dict(kdim=64, vdim=80)]


def _torch_mha(embed, heads, bias=True, **kw):
    return torch.nn.MultiheadAttention(embed, heads, bias=bias, batch_first=True, **kw)


# ---- the module -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", DIMS, ids=["same", "kdim96_vdim48", "kdim64_vdim80"])
@pytest.mark.parametrize("bias", [True, False])
def test_parameters_have_torchs_names_and_shapes(kw, bias):
    ours, theirs = ME.MinkowskiCrossAttention(64, 2, bias=bias, **kw), _torch_mha(64, 2, bias=bias, **kw)
    a = {k: tuple(v.shape) for k, v in ours.named_parameters()}
    b = {k: tuple(v.shape) for k, v in theirs.named_parameters()}
    assert a == b
    assert ("in_proj_weight" in a) == (not kw) and ("k_proj_weight" in a) == bool(kw)


@pytest.mark.parametrize("kw", DIMS[:2], ids=["same", "kdim96_vdim48"])
def test_initialisation_statistics_are_torchs(kw):
    """xavier_uniform_ on every projection weight (bound sqrt(6 / (fan_in + fan_out))), zero biases, torch's Linear
    initialisation of out_proj.weight: the bound holds exactly, and the standard deviation within 5 % over >= 4096 draws"""
    torch.manual_seed(0)
    ours, theirs = ME.MinkowskiCrossAttention(128, 4, **kw), _torch_mha(128, 4, **kw)
    for (name, p), (_, t) in zip(sorted(ours.named_parameters()), sorted(theirs.named_parameters())):
        if name.endswith("bias"):
            assert float(p.detach().abs().max()) == 0.0 and float(t.detach().abs().max()) == 0.0, name
            continue
        if name != "out_proj.weight":
            bound = math.sqrt(6.0 / (p.shape[0] + p.shape[1]))
            assert float(p.detach().abs().max()) <= bound and float(p.detach().abs().max()) > 0.95 * bound, name
        assert abs(float(p.detach().std()) / float(t.detach().std()) - 1.0) < 0.05, name
        assert abs(float(p.detach().mean())) < 0.05 * float(p.detach().std()) + 1e-3, name


@pytest.mark.parametrize("kw", DIMS, ids=["same", "kdim96_vdim48", "kdim64_vdim80"])
@pytest.mark.parametrize("bias", [True, False])
def test_state_dicts_load_strictly_in_both_directions(kw, bias):
    torch.manual_seed(1)
    ours, theirs = ME.MinkowskiCrossAttention(64, 2, bias=bias, **kw), _torch_mha(64, 2, bias=bias, **kw)
    assert sorted(ours.state_dict()) == sorted(theirs.state_dict())
    theirs.load_state_dict(ours.state_dict(), strict=True)
    for k, v in ours.state_dict().items():
        assert torch.equal(v, theirs.state_dict()[k])
    back = ME.MinkowskiCrossAttention(64, 2, bias=bias, **kw)
    back.load_state_dict(theirs.state_dict(), strict=True)
    for k, v in back.state_dict().items():
        assert torch.equal(v, ours.state_dict()[k])


def test_repr():
    assert repr(ME.MinkowskiCrossAttention(64, 2)) == "MinkowskiCrossAttention(64, 2, kdim=64, vdim=64, bias=True)"
    m = ME.MinkowskiCrossAttention(128, 4, kdim=768, vdim=512, bias=False)
    assert repr(m) == "MinkowskiCrossAttention(128, 4, kdim=768, vdim=512, bias=False)"
    assert m.head_dim == 32


def test_constructor_errors():
    for args, kw in (((64, 3), {}), ((0, 1), {}), ((64, 0), {}), ((64, 2), dict(kdim=0)), ((64, 2), dict(vdim=-1))):
        with pytest.raises(ValueError):
            ME.MinkowskiCrossAttention(*args, **kw)


def test_package_exports():
    for name in ("MinkowskiCrossAttention", "MinkowskiCrossAttentionFunction"):
        assert hasattr(ME, name)
    assert callable(ME.MinkowskiFunctional.cross_attention)
    assert "cross_attention" in ME.MinkowskiFunctional.__all__


# ---- errors that need no device -----------------------------------------------------------------------------------------------
def test_a_plain_tensor_or_a_tensor_field_as_the_query_raises_type_error():
    m = ME.MinkowskiCrossAttention(64, 2)
    ctx = torch.zeros(1, 5, 64)
    with pytest.raises(TypeError, match="SparseTensor"):
        m(torch.zeros(3, 64), ctx)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.cross_attention(torch.zeros(3, 64), ctx, ctx, 2)
    field = object.__new__(ME.TensorField)         # the type alone decides: nothing of the field is read
    with pytest.raises(TypeError, match="TensorField"):
        m(field, ctx)
    with pytest.raises(TypeError, match="TensorField"):
        ME.MinkowskiFunctional.cross_attention(field, ctx, ctx, 2)


class _FakeManager:
    def __init__(self, instances):
        self.instances = instances

    def origin_map_size(self):
        return self.instances


def _apply(q, k, v, lengths=None, heads=2, instances=2):
    return ME.MinkowskiCrossAttentionFunction.apply(q, k, v, lengths, heads, None, None, _FakeManager(instances))


def test_value_errors_come_before_any_launch():
    q, k = torch.zeros(6, 64), torch.zeros(2, 5, 64)
    with pytest.raises(ValueError, match="instances, tokens, channels"):
        _apply(q, k.reshape(10, 64), k.reshape(10, 64))                       # not 3-D
    with pytest.raises(ValueError, match="instances, tokens, channels"):
        _apply(q, k, torch.zeros(2, 4, 64))                                   # keys and values of different lengths
    with pytest.raises(ValueError, match="dtype and device"):
        _apply(q, k.double(), k.double())
    with pytest.raises(ValueError, match="dtype and device"):
        _apply(q, k, k.to("meta"))
    with pytest.raises(ValueError, match="2 instances"):
        _apply(q, torch.zeros(3, 5, 64), torch.zeros(3, 5, 64))               # a wrong B
    with pytest.raises(ValueError, match="head dimension"):
        _apply(torch.zeros(6, 48), torch.zeros(2, 5, 48), torch.zeros(2, 5, 48))   # d = 24
    with pytest.raises(ValueError, match="multiple of num_heads"):
        _apply(q, k, k, heads=3)
    with pytest.raises(ValueError, match="channels of the queries"):
        _apply(q, torch.zeros(2, 5, 128), torch.zeros(2, 5, 128))
    with pytest.raises(ValueError, match="context_lengths"):
        _apply(q, k, k, lengths=torch.tensor([5, 5, 5]))
    with pytest.raises(ValueError, match="context_lengths"):
        _apply(q, k, k, lengths=torch.tensor([5.0, 5.0]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_prototyped_and_exported():
    from minkowskiengine_amd import _lib, backend, host
    lib = _lib.load()
    assert lib.me_version() >= 300
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    assert re.search(r"1\.20 \(300\)", header) and "#define ME_ATTN_MAX_KV_SPLITS 32" in header
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes is not None, name
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in ("CrossAttentionForwardGPU", "CrossAttentionBackwardGPU"):
        assert callable(getattr(backend, name)) and hasattr(native, name), name
    assert hasattr(backend.CoordinateMapManagerGPU_c10, "_context_rows") and \
        hasattr(native.CoordinateMapManagerGPU_c10, "_context_rows")


def test_workspace_bytes_are_monotone_and_hold_delta_and_both_images():
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    base = dict(n_q=1000, n_kv=154, n_batch=2, c=256, heads=8, kv_splits=4)
    order = ("n_q", "n_kv", "n_batch", "c", "heads", "kv_splits")

    def ws(**kw):
        a = dict(base, **kw)
        return lib.me_attn_split_workspace_bytes(*(a[k] for k in order))
    for name, bigger in (("n_q", 4000), ("n_kv", 300), ("n_batch", 8), ("c", 512), ("heads", 16), ("kv_splits", 9)):
        assert ws(**{name: bigger}) >= ws(), name
    for name, bigger in (("n_q", 4000), ("n_kv", 300), ("c", 512), ("heads", 16), ("kv_splits", 9)):
        assert ws(**{name: bigger}) > ws(), name
    for s in (1, 2, 3, 8, 32):
        for n_q, n_kv, c, heads in ((1000, 154, 256, 8), (271, 231, 64, 2), (40000, 2748, 256, 4), (0, 0, 32, 1)):
            got = lib.me_attn_split_workspace_bytes(n_q, n_kv, 2, c, heads, s)
            assert got >= lib.me_attn_workspace_bytes(n_q, n_kv, 2, heads) + 2 * s * n_kv * c * 4, (s, n_q, n_kv)


def _policy_shapes():
    for n_q in (0, 1, 500, 2048, 5000, 20000, 40000, 200000, 2000000):
        for n_kv in (1, 77, 154, 616, 2748, 10992, 100000):
            for n_batch in (1, 2, 8, 64):
                for c, heads in ((32, 1), (128, 4), (256, 4), (256, 8), (1024, 8)):
                    yield n_q, n_kv, n_batch, c, heads


def test_the_policy_stays_in_range_and_under_the_image_cap():
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    seen = set()
    for n_q, n_kv, n_batch, c, heads in _policy_shapes():
        s = lib.me_attn_kv_splits(n_q, n_kv, n_batch, c, heads)
        assert 1 <= s <= MAX_SPLITS, (n_q, n_kv, n_batch, c, heads, s)
        assert s == lib.me_attn_kv_splits(n_q, n_kv, n_batch, c, heads)          # a pure function
        if s > 1:
            assert 2 * s * n_kv * c * 4 <= IMAGE_CAP, (n_q, n_kv, n_batch, c, heads, s)
            assert n_q // n_batch // s >= 256                                    # the documented queries per slice
            assert s * (-(-n_kv // 64) + n_batch) * heads <= 512                 # the slices add no second round
        seen.add(s)
    assert 1 in seen and MAX_SPLITS in seen and len(seen) > 4


def test_the_policy_keeps_every_self_attention_shape_of_the_benchmark_at_one():
    import attention_bench
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    for name, sizes, c, heads in attention_bench.SHAPES:
        n = sum(sizes)
        assert lib.me_attn_kv_splits(n, n, len(sizes), c, heads) == 1, name


# ---- host-side errors, called with null data pointers -------------------------------------------------------------------------
def _backward_split(lib, c=64, heads=2, stride=64, ws_bytes=None, kv_splits=2, n_q=100, n_kv=77, n_batch=1):
    one = ctypes.c_void_p(16)
    if ws_bytes is None:
        ws_bytes = lib.me_attn_split_workspace_bytes(n_q, n_kv, n_batch, c, heads, max(kv_splits, 1))
    return lib.me_attn_backward_split(None, None, None, None, None, None, 0, stride, stride, stride, stride, stride, one, one,
                                      one, one, None, None, n_q, n_kv, n_batch, c, heads, 0.125, None, stride, None, stride,
                                      None, stride, None, ws_bytes, kv_splits, None)


def test_the_c_abi_refuses_bad_arguments_without_a_gpu():
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    for bad in (0, -1, MAX_SPLITS + 1):
        assert _backward_split(lib, kv_splits=bad) != 0
        assert b"kv_splits" in lib.me_last_error()
    need = lib.me_attn_split_workspace_bytes(100, 77, 1, 64, 2, 2)
    assert _backward_split(lib, ws_bytes=need - 1) != 0 and b"workspace too small" in lib.me_last_error()
    assert _backward_split(lib, ws_bytes=lib.me_attn_workspace_bytes(100, 77, 1, 2)) != 0      # delta alone is not enough
    assert _backward_split(lib, c=48) != 0 and b"head dimension" in lib.me_last_error()        # d = 24
    assert _backward_split(lib, c=64, heads=3) != 0
    assert _backward_split(lib, stride=62) != 0 and b"row stride" in lib.me_last_error()
    assert _backward_split(lib, stride=32) != 0
    assert _backward_split(lib) == 0        # valid arguments, every gradient pointer null: nothing to do, nothing launched
    one = ctypes.c_void_p(16)
    assert lib.me_attn_context_lists(2, 0, None, one, one, one, None) != 0 and b"tokens" in lib.me_last_error()
    assert lib.me_attn_context_lists(-1, 5, None, one, one, one, None) != 0 and b"n_batch" in lib.me_last_error()
    assert lib.me_attn_context_lists(1 << 20, 1 << 12, None, one, one, one, None) != 0          # 2^32 rows
    assert lib.me_attn_context_lists(2, 5, None, None, one, one, None) != 0


# ---- the example --------------------------------------------------------------------------------------------------------------
def test_examples_cross_attention_block_is_built_from_the_packages_layers():
    import cross_attention_block as CB
    block = CB.CrossAttentionBlock(128, 4, emb_channels=64, context_channels=768)
    assert isinstance(block.norm_in, ME.MinkowskiConditionalGroupNorm) and block.to_mod.out_features == 256
    assert isinstance(block.conv, ME.MinkowskiConvolution) and block.conv.kernel_generator.kernel_volume == 27
    assert isinstance(block.self_attn, ME.MinkowskiSelfAttention)
    assert isinstance(block.cross_attn, ME.MinkowskiCrossAttention)
    assert (block.cross_attn.embed_dim, block.cross_attn.num_heads, block.cross_attn.kdim, block.cross_attn.vdim) == \
        (128, 4, 768, 768)
    names = sorted(k for k, _ in block.named_parameters() if k.startswith("cross_attn."))
    assert names == ["cross_attn.in_proj_bias", "cross_attn.k_proj_weight", "cross_attn.out_proj.bias",
                     "cross_attn.out_proj.weight", "cross_attn.q_proj_weight", "cross_attn.v_proj_weight"]
    torch.nn.MultiheadAttention(128, 4, kdim=768, vdim=768, batch_first=True).load_state_dict(
        {k[len("cross_attn."):]: v for k, v in block.state_dict().items() if k.startswith("cross_attn.")}, strict=True)
