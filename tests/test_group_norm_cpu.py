"""MinkowskiGroupNorm without a GPU: the public names, the parameters and their torch.nn.GroupNorm-shaped state dict, the
C ABI (header, ctypes table, exports, version, workspace size, host-only argument errors) and the operators of both host
layers."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GNORM_SYMBOLS = ("me_gnorm_workspace_bytes", "me_gnorm_stats", "me_gnorm_apply", "me_gnorm_backward",
                 "me_gnorm_stats_f64", "me_gnorm_apply_f64", "me_gnorm_backward_f64")
OPERATORS = ("GroupNormForwardGPU", "GroupNormBackwardGPU")


def test_names_are_exported():
    assert issubclass(ME.MinkowskiGroupNorm, torch.nn.Module)
    assert issubclass(ME.MinkowskiGroupNormFunction, torch.autograd.Function)
    assert callable(ME.MinkowskiFunctional.group_norm)


def test_parameters_and_defaults():
    layer = ME.MinkowskiGroupNorm(4, 16)
    assert (layer.num_groups, layer.num_channels, layer.eps, layer.affine) == (4, 16, 1e-5, True)
    named = dict(layer.named_parameters())
    assert sorted(named) == ["bias", "weight"]
    for p in named.values():
        assert tuple(p.shape) == (16,) and p.dtype == torch.float32
    assert torch.equal(layer.weight.detach(), torch.ones(16)) and torch.equal(layer.bias.detach(), torch.zeros(16))
    with torch.no_grad():
        layer.weight.fill_(3.0)
        layer.bias.fill_(-2.0)
    layer.reset_parameters()
    assert torch.equal(layer.weight.detach(), torch.ones(16)) and torch.equal(layer.bias.detach(), torch.zeros(16))
    assert layer.double().weight.dtype == torch.float64


def test_affine_false_has_no_parameters():
    layer = ME.MinkowskiGroupNorm(2, 6, affine=False)
    assert layer.weight is None and layer.bias is None
    assert list(layer.parameters()) == [] and list(layer.state_dict()) == []
    layer.reset_parameters()
    torch.nn.GroupNorm(2, 6, affine=False).load_state_dict(layer.state_dict(), strict=True)


def test_state_dicts_move_between_torch_and_the_module():
    theirs = torch.nn.GroupNorm(4, 16)
    with torch.no_grad():
        theirs.weight.copy_(torch.arange(16.0))
        theirs.bias.copy_(-torch.arange(16.0))
    ours = ME.MinkowskiGroupNorm(4, 16)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert torch.equal(ours.weight.detach(), theirs.weight.detach()) and torch.equal(ours.bias.detach(), theirs.bias.detach())
    assert sorted(ours.state_dict()) == ["bias", "weight"]
    back = torch.nn.GroupNorm(4, 16)
    back.load_state_dict(ours.state_dict(), strict=True)
    assert torch.equal(back.weight.detach(), theirs.weight.detach()) and torch.equal(back.bias.detach(), theirs.bias.detach())


def test_repr():
    assert repr(ME.MinkowskiGroupNorm(4, 16)) == "MinkowskiGroupNorm(4, 16, eps=1e-05, affine=True)"
    assert repr(ME.MinkowskiGroupNorm(1, 3, eps=1e-3, affine=False)) == "MinkowskiGroupNorm(1, 3, eps=0.001, affine=False)"


def test_channels_must_divide_into_groups():
    with pytest.raises(ValueError):
        ME.MinkowskiGroupNorm(4, 10)
    ME.MinkowskiGroupNorm(5, 10)


def test_module_and_functional_take_sparse_tensors_only():
    with pytest.raises(AssertionError):
        ME.MinkowskiGroupNorm(1, 3)(torch.zeros(4, 3))
    with pytest.raises(AssertionError):
        ME.MinkowskiFunctional.group_norm(torch.zeros(4, 3), 1)


def test_cpu_tensors_have_no_operator():
    with pytest.raises(ValueError, match="GroupNormForwardCPU"):
        ME.get_minkowski_function("GroupNormForward", torch.zeros(1))
    with pytest.raises(ValueError, match="GroupNormBackwardCPU"):
        ME.get_minkowski_function("GroupNormBackward", torch.zeros(1))


def test_c_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for s in GNORM_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/me_amd.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.me_version() >= 250


def test_workspace_bytes():
    lib = _lib.load()
    sizes = [lib.me_gnorm_workspace_bytes(n, 2, 64, 8) for n in (0, 1, 100, 5000, 100000, 10 ** 7)]
    assert sizes[0] > 0
    assert sizes == sorted(sizes) and sizes[1] < sizes[-1]
    # the partials of every (chunk, instance, channel) at the 512-chunk cap, as instance norm's workspace
    assert sizes[-1] >= 2 * 512 * 2 * 64 * 4
    assert lib.me_gnorm_workspace_bytes(100, 2, 64, 8) >= lib.me_inorm_workspace_bytes(100, 2, 64)


def test_both_host_layers_expose_the_operators():
    for name in OPERATORS:
        assert callable(getattr(backend, name))
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in OPERATORS:
        assert hasattr(native, name), name


@pytest.mark.parametrize("c,groups", [(8, 0), (8, -2), (8, 3), (12, 5)])
def test_bad_groups_are_host_side_errors(c, groups):
    """checked before anything touches a device: every pointer is NULL and no GPU is needed"""
    lib = _lib.load()
    big = 1 << 30
    calls = (
        lambda: lib.me_gnorm_stats(None, 0, None, 10, 2, c, groups, 1e-5, None, None, None, big, None),
        lambda: lib.me_gnorm_apply(None, 0, None, 10, 2, c, groups, None, None, None, None, None, None),
        lambda: lib.me_gnorm_backward(None, None, 0, None, 10, 2, c, groups, None, None, None, None, None, None, None,
                                      big, None),
        lambda: lib.me_gnorm_stats_f64(None, None, 10, 2, c, groups, 1e-5, None, None, None),
        lambda: lib.me_gnorm_apply_f64(None, None, 10, 2, c, groups, None, None, None, None, None, None),
        lambda: lib.me_gnorm_backward_f64(None, None, None, 10, 2, c, groups, None, None, None, None, None, None, None,
                                          big, None))
    for call in calls:
        assert call() != 0
        assert "groups" in lib.me_last_error().decode()
