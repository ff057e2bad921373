"""MinkowskiLayerNorm / MinkowskiRMSNorm without a GPU: the public names, torch's parameters and state dicts, the C ABI
of csrc/layer_norm.hip (declared, prototyped, exported; version 1.23), its host-side policy functions and argument
errors (all reachable with NULL data pointers), and the operators of both host layers."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "me_amd.h")).read()
SYMBOLS = ("me_lnorm_chunks", "me_lnorm_workspace_bytes", "me_lnorm_forward", "me_lnorm_backward", "me_lnorm_forward_f64",
           "me_lnorm_backward_f64")


def test_names_are_exported():
    for name in ("MinkowskiLayerNorm", "MinkowskiRMSNorm", "MinkowskiLayerNormFunction"):
        assert hasattr(ME, name), name
    for name in ("layer_norm", "rms_norm"):
        assert callable(getattr(ME.MinkowskiFunctional, name)) and name in ME.MinkowskiFunctional.__all__
    for name in ("LayerNormForwardGPU", "LayerNormBackwardGPU"):
        assert callable(getattr(backend, name))
        native = ME.host.native_module()
        assert native is not None and callable(getattr(native, name)), ME.host.native_error()


@pytest.mark.parametrize("affine,bias", [(True, True), (True, False), (False, True)])
def test_layer_norm_parameters_are_torchs(affine, bias):
    ours, ref = ME.MinkowskiLayerNorm(12, eps=1e-6, elementwise_affine=affine, bias=bias), \
        torch.nn.LayerNorm(12, eps=1e-6, elementwise_affine=affine, bias=bias)
    assert ours.normalized_shape == ref.normalized_shape == ME.MinkowskiLayerNorm((12,)).normalized_shape
    assert {k: (v.shape, v.dtype) for k, v in ours.state_dict().items()} == \
        {k: (v.shape, v.dtype) for k, v in ref.state_dict().items()}
    for k, v in ours.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k                       # ones / zeros
    with torch.no_grad():
        for p in ref.parameters():
            p.uniform_(-1, 1)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in ours.state_dict().items())
    assert all(p.dtype == torch.float64 for p in ours.double().parameters())
    assert repr(ours) == f"MinkowskiLayerNorm(12, eps=1e-06, elementwise_affine={affine}, bias={affine and bias})"


@pytest.mark.parametrize("affine", [True, False])
def test_rms_norm_parameters_are_torchs(affine):
    ours, ref = ME.MinkowskiRMSNorm((12,), elementwise_affine=affine), torch.nn.RMSNorm(12, elementwise_affine=affine)
    assert ours.eps is None and list(ours.state_dict()) == list(ref.state_dict())
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert repr(ours) == f"MinkowskiRMSNorm(12, eps=None, elementwise_affine={affine})"
    with pytest.raises(ValueError):
        ME.MinkowskiRMSNorm((3, 4))


def test_abi_is_declared_prototyped_and_exported():
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", HEADER)
        assert decl, f"{name} is not declared in include/me_amd.h"
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
        assert getattr(lib, name) is not None
    assert lib.me_version() >= 330
    assert re.search(r"1\.23 \(330\)\s+round 23:", HEADER)


def test_chunks_and_workspace_are_pure_and_monotone():
    lib = _lib.load()
    for c, e in ((8, 2), (64, 2), (512, 4), (2048, 4), (7, 4)):
        prev = 0
        for n in (0, 1, 2, 63, 64, 1000, 4097, 100_000, 1_000_000, (1 << 31) - 1):
            g = lib.me_lnorm_chunks(n, c, e)
            assert g == lib.me_lnorm_chunks(n, c, e) and 1 <= g <= 1024 and g <= max(n, 1) and g >= prev, (n, c, e, g)
            assert lib.me_lnorm_workspace_bytes(n, c, e) == g * 2 * c * 4
            prev = g
    assert lib.me_lnorm_chunks(100_000, 64, 2) == 782 and lib.me_lnorm_chunks(100_000, 512, 2) == 1024


FAKE = 4096      # an address that is never dereferenced: the checks come before any launch


def _forward(lib, n=4, c=8, xs=None, ys=None, res=None, sout=None, rs=8, ss=8, f64=False):
    xs, ys = c if xs is None else xs, c if ys is None else ys
    if f64:
        return lib.me_lnorm_forward_f64(None, res, sout, xs, rs, ss, n, c, 0, None, None, 1e-5, None, ys, None, None, None)
    return lib.me_lnorm_forward(None, res, sout, 0, xs, rs, ss, n, c, 0, None, None, 1e-5, None, ys, None, None, None)


def _backward(lib, n=4, c=8, xs=None, dys=None, gg=None, ws=None, ws_bytes=0, f64=False):
    xs, dys = c if xs is None else xs, c if dys is None else dys
    if f64:
        return lib.me_lnorm_backward_f64(None, None, None, xs, dys, 0, n, c, 0, None, None, None, None, c, gg, None, None)
    return lib.me_lnorm_backward(None, None, None, 0, xs, dys, 0, n, c, 0, None, None, None, None, c, gg, None, ws, ws_bytes,
                                 None)


@pytest.mark.parametrize("call,kwargs,message", [
    (_forward, dict(c=0), "channel count"), (_backward, dict(c=0), "channel count"),
    (_forward, dict(c=0, f64=True), "channel count"), (_backward, dict(c=0, f64=True), "channel count"),
    (_forward, dict(c=2049), "ME_LNORM_MAX_C"), (_backward, dict(c=2049), "ME_LNORM_MAX_C"),
    (_forward, dict(xs=7), "stride"), (_forward, dict(ys=7), "stride"), (_forward, dict(xs=7, f64=True), "stride"),
    (_forward, dict(res=FAKE, sout=FAKE, rs=7), "stride"), (_forward, dict(res=FAKE, sout=FAKE, ss=7), "stride"),
    (_backward, dict(dys=7), "stride"), (_backward, dict(xs=7, f64=True), "stride"),
    (_forward, dict(n=-1), "row count"), (_forward, dict(n=1 << 31), "row count"),
    (_backward, dict(n=-1), "row count"), (_backward, dict(n=1 << 31, f64=True), "row count"),
    (_backward, dict(gg=FAKE), "workspace"), (_backward, dict(gg=FAKE, ws=FAKE, ws_bytes=63), "workspace"),
    (_forward, dict(res=FAKE), "stream_out"), (_forward, dict(res=FAKE, f64=True), "stream_out"),
])
def test_argument_errors_come_before_any_launch(call, kwargs, message):
    lib = _lib.load()
    assert call(lib, **kwargs) != 0
    assert message in lib.me_last_error().decode(), lib.me_last_error()


def test_an_empty_matrix_is_legal():
    lib = _lib.load()
    assert _forward(lib, n=0) == 0 and _forward(lib, n=0, f64=True) == 0 and _backward(lib, n=0) == 0
    assert _forward(lib, n=0, c=4096, f64=True) == 0            # the float64 twins take any width


def test_cpu_tensors_and_plain_tensors_raise():
    x = torch.rand(2, 8)
    for call in (lambda: ME.get_minkowski_function("LayerNormForward", x),
                 lambda: ME.MinkowskiLayerNormFunction.apply(x, None, None, None, 1e-5, False),
                 lambda: ME.MinkowskiLayerNormFunction.apply(x, x, None, None, 1e-5, True)):
        with pytest.raises(ValueError, match="LayerNormForwardCPU"):
            call()
    for call in (ME.MinkowskiLayerNorm(8), ME.MinkowskiRMSNorm(8), ME.MinkowskiFunctional.layer_norm,
                 ME.MinkowskiFunctional.rms_norm, lambda t: ME.MinkowskiLayerNorm(8).forward_residual(t, t)):
        with pytest.raises(TypeError):
            call(x)
