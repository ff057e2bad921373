"""MinkowskiAdaLayerNorm without a GPU: the public names, torch's parameters and state dicts, the C ABI of
csrc/ada_layer_norm.hip (declared, prototyped, exported; version 1.26), its argument errors (all reachable with NULL data
pointers) and the operators of both host layers."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "me_amd.h")).read()
SYMBOLS = ("me_adaln_chunks", "me_adaln_workspace_bytes", "me_adaln_forward", "me_adaln_backward", "me_adaln_forward_f64",
           "me_adaln_backward_f64")


def test_names_are_exported_on_both_hosts():
    for name in ("MinkowskiAdaLayerNorm", "MinkowskiAdaLayerNormFunction"):
        assert hasattr(ME, name), name
    assert callable(ME.MinkowskiFunctional.ada_layer_norm) and "ada_layer_norm" in ME.MinkowskiFunctional.__all__
    native = ME.host.native_module()
    for name in ("AdaLayerNormForwardGPU", "AdaLayerNormBackwardGPU"):
        assert callable(getattr(backend, name))
        assert native is not None and callable(getattr(native, name)), ME.host.native_error()


@pytest.mark.parametrize("rms", [False, True])
def test_parameters_are_the_plain_layers(rms):
    plain = ME.MinkowskiRMSNorm(12) if rms else ME.MinkowskiLayerNorm(12)
    ref = torch.nn.RMSNorm(12) if rms else torch.nn.LayerNorm(12)
    ours = ME.MinkowskiAdaLayerNorm((12,), elementwise_affine=True, rms=rms)
    with torch.no_grad():
        for p in ref.parameters():
            p.uniform_(-1, 1)
    for other in (ref, plain):
        other.load_state_dict(ref.state_dict(), strict=True)
        ours.load_state_dict(other.state_dict(), strict=True)
        other.load_state_dict(ours.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in ours.state_dict().items())
    assert all(p.dtype == torch.float64 for p in ours.double().parameters())
    assert repr(ours) == f"MinkowskiAdaLayerNorm(12, eps=1e-06, elementwise_affine=True, bias={not rms}, rms={rms})"
    bare = ME.MinkowskiAdaLayerNorm(12)
    assert not bare.state_dict() and bare.weight is None
    assert repr(bare) == "MinkowskiAdaLayerNorm(12, eps=1e-06, elementwise_affine=False, bias=False, rms=False)"


def test_constructor_and_input_errors():
    for shape in ((3, 4), 0):
        with pytest.raises(ValueError):
            ME.MinkowskiAdaLayerNorm(shape)
    x = torch.rand(2, 8)
    with pytest.raises(ValueError, match="AdaLayerNormForwardCPU"):
        ME.MinkowskiAdaLayerNormFunction.apply(x, None, None, None, None, None, None, 1e-6, False, None, None)
    layer = ME.MinkowskiAdaLayerNorm(8)
    for call in (layer, ME.MinkowskiFunctional.ada_layer_norm, lambda t: layer.forward_residual(t, t)):
        with pytest.raises(TypeError):
            call(x)

    class Field:                                # anything that is not a SparseTensor, a TensorField included
        F = x
        coordinate_field_map_key = None
    with pytest.raises(TypeError):
        layer(Field())


def test_abi_is_declared_prototyped_and_exported():
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", HEADER)
        assert decl, f"{name} is not declared in include/me_amd.h"
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
        assert getattr(lib, name) is not None
    assert lib.me_version() >= 360
    assert re.search(r"1\.26 \(360\)\s+round 26:", HEADER)
    for n, nb, c, e in ((0, 0, 8, 2), (1000, 3, 64, 2), (100_000, 8, 512, 4)):
        g = lib.me_adaln_chunks(n, nb, c, e)
        assert g == lib.me_lnorm_chunks(n, c, e) + nb
        assert lib.me_adaln_workspace_bytes(n, nb, c, e) == (3 * g + 2 * nb) * c * 4


FAKE = 4096      # an address that is never dereferenced: the checks come before any launch


def _forward(lib, n=4, c=8, nb=1, xs=None, ys=None, res=None, sout=None, gate=None, f64=False):
    xs, ys = c if xs is None else xs, c if ys is None else ys
    mods = (None, nb, None, None, None, None, gate)
    if f64:
        return lib.me_adaln_forward_f64(None, res, sout, xs, c, c, n, c, 0, *mods, 1e-6, None, ys, None, None, None)
    return lib.me_adaln_forward(None, res, sout, 0, xs, c, c, n, c, 0, *mods, 1e-6, None, ys, None, None, None)


def _backward(lib, n=4, c=8, nb=1, dy=FAKE, dys=None, gate=None, inp=None, gg=None, gsc=None, ws=None, ws_bytes=0, f64=False):
    dys = c if dys is None else dys
    if f64:
        return lib.me_adaln_backward_f64(None, dy, None, inp, c, dys, c, c, n, c, 0, None, None, None, nb, None, None, None,
                                         gate, None, None, None, c, None, c, gg, None, gsc, None, None, None)
    return lib.me_adaln_backward(None, dy, None, inp, 0, c, dys, c, c, n, c, 0, None, None, nb, None, None, None, gate, None,
                                 None, c, None, c, gg, None, gsc, None, None, ws, ws_bytes, None)


@pytest.mark.parametrize("call,kwargs,message", [
    (_forward, dict(c=0), "channel count"), (_backward, dict(c=0), "channel count"),
    (_forward, dict(c=0, f64=True), "channel count"), (_backward, dict(c=0, f64=True), "channel count"),
    (_forward, dict(c=2049), "ME_LNORM_MAX_C"), (_backward, dict(c=2049), "ME_LNORM_MAX_C"),
    (_forward, dict(n=-1), "row count"), (_backward, dict(n=1 << 31, f64=True), "row count"),
    (_forward, dict(nb=0), "instance"), (_backward, dict(nb=0), "instance"),
    (_forward, dict(xs=7), "stride"), (_forward, dict(ys=7, f64=True), "stride"), (_backward, dict(dys=7), "stride"),
    (_forward, dict(res=FAKE), "stream_out"), (_forward, dict(gate=FAKE), "a gate needs a residual"),
    (_forward, dict(gate=FAKE, f64=True), "a gate needs a residual"),
    (_backward, dict(gate=FAKE), "given together"), (_backward, dict(inp=FAKE, f64=True), "given together"),
    (_backward, dict(dy=None, gg=FAKE), "need dy"),
    (_backward, dict(gg=FAKE), "workspace"), (_backward, dict(gsc=FAKE, ws=FAKE, ws_bytes=63), "workspace"),
    (_forward, dict(), "must be given"), (_backward, dict(), "must be given"), (_backward, dict(f64=True), "must be given"),
])
def test_argument_errors_come_before_any_launch(call, kwargs, message):
    lib = _lib.load()
    assert call(lib, **kwargs) != 0
    assert message in lib.me_last_error().decode(), lib.me_last_error()


def test_an_empty_matrix_is_legal():
    lib = _lib.load()
    assert _forward(lib, n=0, nb=0) == 0 and _forward(lib, n=0, nb=0, f64=True) == 0
    assert _backward(lib, n=0, nb=0) == 0 and _backward(lib, n=0, nb=0, f64=True) == 0
    assert _forward(lib, n=0, nb=0, c=4096, f64=True) == 0            # the float64 twins take any width
