"""MinkowskiConditionalGroupNorm without a GPU: the public names, the parameters and their torch.nn.GroupNorm-shaped state
dict, the activation argument, the C ABI (header, ctypes table, exports, version, workspace size, host-only argument
errors) and the operators of both host layers."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("me_gnorm_cond_workspace_bytes", "me_gnorm_cond_apply", "me_gnorm_cond_backward", "me_gnorm_cond_apply_f64",
           "me_gnorm_cond_backward_f64")
OPERATORS = ("ConditionalGroupNormForwardGPU", "ConditionalGroupNormBackwardGPU")


def _calls(lib, c, groups, act, big=1 << 30):
    """the four launching entry points with every pointer NULL: only the host-side checks can run"""
    return (
        lambda: lib.me_gnorm_cond_apply(None, 0, None, 10, 2, c, groups, None, None, None, None, None, None, act, None,
                                        None, big, None),
        lambda: lib.me_gnorm_cond_backward(None, None, 0, None, 10, 2, c, groups, None, None, None, None, None, None, act,
                                           None, None, None, None, None, None, big, None),
        lambda: lib.me_gnorm_cond_apply_f64(None, None, 10, 2, c, groups, None, None, None, None, None, None, act, None,
                                            None),
        lambda: lib.me_gnorm_cond_backward_f64(None, None, None, 10, 2, c, groups, None, None, None, None, None, None, act,
                                               None, None, None, None, None, None, big, None))


def test_names_are_exported():
    assert issubclass(ME.MinkowskiConditionalGroupNorm, torch.nn.Module)
    assert issubclass(ME.MinkowskiConditionalGroupNormFunction, torch.autograd.Function)
    assert callable(ME.MinkowskiFunctional.conditional_group_norm)
    assert "conditional_group_norm" in ME.MinkowskiFunctional.__all__


def test_parameters_and_defaults():
    layer = ME.MinkowskiConditionalGroupNorm(4, 16)
    assert (layer.num_groups, layer.num_channels, layer.eps, layer.affine, layer.activation) == (4, 16, 1e-5, True, None)
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
    assert ME.MinkowskiConditionalGroupNorm(4, 16, activation="silu").activation == "silu"


def test_affine_false_has_no_parameters():
    layer = ME.MinkowskiConditionalGroupNorm(2, 6, affine=False, activation="silu")
    assert layer.weight is None and layer.bias is None
    assert list(layer.parameters()) == [] and list(layer.state_dict()) == []
    layer.reset_parameters()
    torch.nn.GroupNorm(2, 6, affine=False).load_state_dict(layer.state_dict(), strict=True)


def test_state_dicts_move_between_torch_and_the_module():
    theirs = torch.nn.GroupNorm(4, 16)
    with torch.no_grad():
        theirs.weight.copy_(torch.arange(16.0))
        theirs.bias.copy_(-torch.arange(16.0))
    ours = ME.MinkowskiConditionalGroupNorm(4, 16, activation="silu")
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert torch.equal(ours.weight.detach(), theirs.weight.detach()) and torch.equal(ours.bias.detach(), theirs.bias.detach())
    assert sorted(ours.state_dict()) == ["bias", "weight"]
    back = torch.nn.GroupNorm(4, 16)
    back.load_state_dict(ours.state_dict(), strict=True)
    assert torch.equal(back.weight.detach(), theirs.weight.detach()) and torch.equal(back.bias.detach(), theirs.bias.detach())
    ME.MinkowskiGroupNorm(4, 16).load_state_dict(ours.state_dict(), strict=True)


def test_repr():
    assert repr(ME.MinkowskiConditionalGroupNorm(4, 16)) == \
        "MinkowskiConditionalGroupNorm(4, 16, eps=1e-05, affine=True, activation=None)"
    assert repr(ME.MinkowskiConditionalGroupNorm(1, 3, eps=1e-3, affine=False, activation="silu")) == \
        "MinkowskiConditionalGroupNorm(1, 3, eps=0.001, affine=False, activation='silu')"


def test_channels_must_divide_into_groups():
    with pytest.raises(ValueError):
        ME.MinkowskiConditionalGroupNorm(4, 10)
    ME.MinkowskiConditionalGroupNorm(5, 10)


@pytest.mark.parametrize("activation", ["relu", "SiLU", 1, True, ""])
def test_a_bad_activation_raises(activation):
    with pytest.raises(ValueError, match="activation"):
        ME.MinkowskiConditionalGroupNorm(4, 16, activation=activation)


def test_module_and_functional_take_sparse_tensors_only():
    with pytest.raises(AssertionError):
        ME.MinkowskiConditionalGroupNorm(1, 3)(torch.zeros(4, 3))
    with pytest.raises(AssertionError):
        ME.MinkowskiFunctional.conditional_group_norm(torch.zeros(4, 3), 1)


def test_cpu_tensors_have_no_operator():
    for name in OPERATORS:                             # the GPU operators exist; only their CPU names do not
        assert hasattr(backend, name), name
    with pytest.raises(ValueError, match="ConditionalGroupNormForwardCPU"):
        ME.get_minkowski_function("ConditionalGroupNormForward", torch.zeros(1))
    with pytest.raises(ValueError, match="ConditionalGroupNormBackwardCPU"):
        ME.get_minkowski_function("ConditionalGroupNormBackward", torch.zeros(1))


def test_c_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/me_amd.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype"
        assert hasattr(lib, s), f"{s} is not exported"
    assert lib.me_version() >= 260


def test_workspace_bytes():
    lib = _lib.load()
    ns = (0, 1, 100, 5000, 100000, 10 ** 7)
    sizes = [lib.me_gnorm_cond_workspace_bytes(n, 2, 64, 8) for n in ns]
    assert sizes[0] > 0
    assert sizes == sorted(sizes) and sizes[1] < sizes[-1]
    for n, size in zip(ns, sizes):
        # group norm's workspace plus ge and be [n_batch, c], wide enough for the float64 entry points
        assert size >= lib.me_gnorm_workspace_bytes(n, 2, 64, 8) + 2 * 2 * 64 * 8
    assert lib.me_gnorm_cond_workspace_bytes(100, 0, 64, 8) == 0 and lib.me_gnorm_cond_workspace_bytes(100, 2, 64, 0) == 0


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
    for call in _calls(lib, c, groups, 1):
        assert call() != 0
        assert "groups" in lib.me_last_error().decode()


@pytest.mark.parametrize("act", [2, -1, 17])
def test_an_unknown_act_is_a_host_side_error(act):
    lib = _lib.load()
    for call in _calls(lib, 8, 2, act):
        assert call() != 0
        assert "act must be 0 (identity) or 1 (SiLU)" in lib.me_last_error().decode()


def test_too_many_channels_and_a_short_workspace_are_host_side_errors():
    lib = _lib.load()
    need = lib.me_gnorm_cond_workspace_bytes(10, 2, 8, 2)
    apply_, backward = _calls(lib, 3226, 2, 1)[:2]
    for call in (apply_, backward):
        assert call() != 0
        assert "channel count too large" in lib.me_last_error().decode()
    for call in (_calls(lib, 8, 2, 1, big=need - 1)[i] for i in (0, 1, 3)):
        assert call() != 0
        assert "workspace too small" in lib.me_last_error().decode()
