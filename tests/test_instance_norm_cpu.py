"""MinkowskiInstanceNorm / MinkowskiStableInstanceNorm without a GPU: the public names, the parameters and their
reference-shaped state dict, the C ABI (header and ctypes table), the operators of both host layers, and the fixtures
recorded from the reference (tests/golden/make_golden_instance_norm.py)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "instance_norm_*.npz")))
INORM_SYMBOLS = ("me_inorm_workspace_bytes", "me_inorm_stats", "me_inorm_apply", "me_inorm_backward",
                 "me_inorm_stats_f64", "me_inorm_apply_f64", "me_inorm_backward_f64")


def test_names_are_exported():
    assert issubclass(ME.MinkowskiInstanceNorm, torch.nn.Module)
    assert issubclass(ME.MinkowskiStableInstanceNorm, torch.nn.Module)
    assert issubclass(ME.MinkowskiInstanceNormFunction, torch.autograd.Function)


@pytest.mark.parametrize("cls,eps", [("MinkowskiInstanceNorm", 1e-8), ("MinkowskiStableInstanceNorm", 1e-6)])
def test_parameters_repr_and_state_dict(cls, eps):
    layer = getattr(ME, cls)(7)
    assert layer.eps == eps
    assert repr(layer) == f"{cls}(nchannels=7)"
    named = dict(layer.named_parameters())
    assert sorted(named) == ["bias", "weight"]
    for p in named.values():
        assert tuple(p.shape) == (1, 7) and p.dtype == torch.float32
    assert torch.equal(layer.weight.detach(), torch.ones(1, 7)) and torch.equal(layer.bias.detach(), torch.zeros(1, 7))
    # a reference-shaped state dict (MinkowskiNormalization.py:318-319, 374-375: two (1, C) parameters, no buffers)
    state = {"weight": torch.full((1, 7), 2.0), "bias": torch.full((1, 7), -1.0)}
    layer.load_state_dict(state, strict=True)
    assert sorted(layer.state_dict()) == ["bias", "weight"]
    assert torch.equal(layer.weight.detach(), state["weight"]) and torch.equal(layer.bias.detach(), state["bias"])
    layer.reset_parameters()
    assert torch.equal(layer.weight.detach(), torch.ones(1, 7)) and torch.equal(layer.bias.detach(), torch.zeros(1, 7))
    assert layer.double().weight.dtype == torch.float64


def test_modules_take_sparse_tensors_only():
    with pytest.raises(AssertionError):
        ME.MinkowskiInstanceNorm(3)(torch.zeros(4, 3))
    with pytest.raises(AssertionError):
        ME.MinkowskiStableInstanceNorm(3)(torch.zeros(4, 3))


def test_c_abi_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for s in INORM_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/me_amd.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes prototype"
        assert hasattr(lib, s)
    assert lib.me_version() >= 190
    # host-only entry point: the workspace covers the partials of every (chunk, instance, channel) and never shrinks
    small, large = lib.me_inorm_workspace_bytes(100, 2, 8), lib.me_inorm_workspace_bytes(100000, 4, 64)
    assert 0 < small < large
    assert large >= 2 * 512 * 4 * 64 * 4


def test_both_host_layers_expose_the_operators():
    for name in ("InstanceNormForwardGPU", "InstanceNormBackwardGPU"):
        assert callable(getattr(backend, name))
    native = host.native_module()
    assert native is not None, host.native_error()
    for name in ("InstanceNormForwardGPU", "InstanceNormBackwardGPU"):
        assert hasattr(native, name), name


def test_cpu_tensors_have_no_operator():
    with pytest.raises(ValueError, match="InstanceNormForwardCPU"):
        ME.get_minkowski_function("InstanceNormForward", torch.zeros(1))


def test_fixture_set_is_complete():
    names = [os.path.basename(p) for p in GOLDEN]
    assert names == ["instance_norm_2d_b4_c3.npz", "instance_norm_3d_b2_c64_offsets.npz", "instance_norm_3d_b2_c8.npz",
                     "instance_norm_3d_b2_interleaved_c5.npz", "instance_norm_3d_b3_sizes_c16.npz",
                     "instance_norm_4d_b2_c17.npz"]
    for p in GOLDEN:
        assert os.path.getsize(p) < (1 << 20), p


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_fixtures_are_consistent(path):
    d = np.load(path)
    n, c = d["feats"].shape
    assert d["coords"].shape[0] == n and d["coords"].dtype == np.int32
    assert d["feats"].dtype == np.float32 and d["grad_out"].dtype == np.float32
    for k in ("grad_out", "out", "grad_in"):
        assert d[k].shape == (n, c), k
    for k in ("weight", "bias", "grad_weight", "grad_bias"):
        assert d[k].shape == (1, c), k
    for k in ("out", "grad_in", "grad_weight", "grad_bias"):
        assert d[k].dtype == np.float64, k
    # properties of the formula: grad_bias = sum grad_out; the input gradient of every instance sums to zero
    assert np.abs(d["grad_bias"] - d["grad_out"].astype(np.float64).sum(0, keepdims=True)).max() <= 1e-9
    batch = d["coords"][:, 0]
    for b in np.unique(batch):
        assert np.abs(d["grad_in"][batch == b].sum(0)).max() <= 1e-9, b
    # the recorded output is the plain formula (x - mean_b) / sqrt(var_b + 1e-8) * w + b
    x = d["feats"].astype(np.float64)
    for b in np.unique(batch):
        m = batch == b
        mu, var = x[m].mean(0), x[m].var(0)
        assert np.abs(d["out"][m] - ((x[m] - mu) / np.sqrt(var + 1e-8) * d["weight"] + d["bias"])).max() <= 1e-12


def test_fixtures_cover_the_cases_they_are_named_for():
    sizes = np.load(os.path.join(ROOT, "tests", "golden", "instance_norm_3d_b3_sizes_c16.npz"))
    counts = np.bincount(sizes["coords"][:, 0])
    assert counts.tolist() == [700, 40, 1]
    one = sizes["coords"][:, 0] == 2     # one row: variance 0, normalised value 0 -> out = bias, gradient exactly 0
    assert np.array_equal(sizes["out"][one], sizes["bias"].astype(np.float64))
    assert np.all(sizes["grad_in"][one] == 0.0)
    mixed = np.load(os.path.join(ROOT, "tests", "golden", "instance_norm_3d_b2_interleaved_c5.npz"))["coords"][:, 0]
    assert np.count_nonzero(np.diff(mixed)) > 100          # the two instances are interleaved row by row
    off = np.load(os.path.join(ROOT, "tests", "golden", "instance_norm_3d_b2_c64_offsets.npz"))["feats"]
    assert np.median(np.abs(off.mean(0)) / off.std(0)) > 3  # channel means several times the spread
