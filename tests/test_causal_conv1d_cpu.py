"""The causal conv1d without a GPU: the public names, the C ABI of csrc/causal_conv1d.hip (declared, prototyped, exported;
version 1.28), its argument errors (all reachable with NULL or fake pointers), the torch formulation against
torch.nn.functional.conv1d per instance, and MinkowskiMamba's state dict."""
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from minkowskiengine_amd.causal_conv1d import causal_conv1d_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "me_amd.h")).read()
SYMBOLS = ("me_cconv_supported", "me_cconv_chunk", "me_cconv_workspace_bytes", "me_cconv_forward", "me_cconv_backward")
FAKE = 4096      # an address that is never dereferenced: the checks come before any launch


def test_names_are_exported_on_both_hosts():
    for name in ("MinkowskiCausalConv1dFunction", "causal_conv1d", "causal_conv1d_reference"):
        assert hasattr(ME, name), name
    assert callable(ME.MinkowskiFunctional.causal_conv1d) and "causal_conv1d" in ME.MinkowskiFunctional.__all__
    native = ME.host.native_module()
    for name in ("CausalConv1dForwardGPU", "CausalConv1dBackwardGPU"):
        assert callable(getattr(backend, name))
        assert native is not None and callable(getattr(native, name)), ME.host.native_error()


def test_abi_is_declared_prototyped_and_exported():
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", HEADER)
        assert decl, f"{name} is not declared in include/me_amd.h"
        args = 0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == args, name
        assert getattr(lib, name) is not None
    assert lib.me_version() >= 380
    assert lib.me_cconv_supported(1, 2, 0) == 1 and lib.me_cconv_supported(96, 4, 1) == 1
    assert lib.me_cconv_supported(64, 1, 0) == 0 and lib.me_cconv_supported(64, 5, 0) == 0
    assert lib.me_cconv_supported(0, 4, 0) == 0
    assert lib.me_cconv_chunk() > 0
    assert lib.me_cconv_workspace_bytes(1000, 96, 4, 1) >= 5 * 96 * 4
    assert backend.CCONV_MAX_RUNS == int(re.search(r"#define ME_CCONV_MAX_RUNS (\d+)", HEADER).group(1))


def _forward(lib, n=4, d=8, k=4, xs=None, x=None):
    return lib.me_cconv_forward(x, 0, d if xs is None else xs, None, None, 1, None, None, 0, n, d, k, None, d, None)


def _backward(lib, n=4, d=8, k=4, xs=None, db=None, full=False):
    p = FAKE if full else None                      # full: every data pointer given, only the workspace is missing
    return lib.me_cconv_backward(p, p, 0, d if xs is None else xs, d, p, None, 1, p, p, 0, n, d, k, None, d, None, db, None, 0,
                                 None)


@pytest.mark.parametrize("call,kwargs,message", [
    (_forward, dict(d=0), "k = 2, 3 or 4"), (_forward, dict(k=1), "k = 2, 3 or 4"), (_backward, dict(k=5), "k = 2, 3 or 4"),
    (_forward, dict(n=-1), "2^31"), (_backward, dict(n=1 << 31), "2^31"),
    (_forward, dict(xs=7), "stride"), (_backward, dict(xs=7), "stride"),
    (_backward, dict(db=FAKE), "needs bias"),
    (_forward, dict(), "must be given"), (_forward, dict(x=FAKE), "must be given"), (_backward, dict(), "must be given"),
    (_backward, dict(full=True), "workspace is smaller"),
])
def test_argument_errors_come_before_any_launch(call, kwargs, message):
    lib = _lib.load()
    assert call(lib, **kwargs) != 0
    assert message in lib.me_last_error().decode(), lib.me_last_error()


def test_an_empty_matrix_is_legal():
    lib = _lib.load()
    assert _forward(lib, n=0) == 0 and _backward(lib, n=0) == 0


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("activation,with_bias", [(None, True), ("silu", True), ("silu", False)])
def test_the_torch_formulation_is_conv1d_per_instance(reverse, activation, with_bias):
    g = torch.Generator().manual_seed(0)
    n, d, k = 7, 3, 4
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    weight = torch.randn(d, 1, k, generator=g, dtype=torch.float64)
    bias = torch.randn(d, generator=g, dtype=torch.float64) if with_bias else None
    seq = torch.tensor([4, 0, 6, 2, 5, 1, 3])           # two instances: positions 0..2 and 3..6
    starts = torch.tensor([True, False, False, True, False, False, False])
    if reverse:                                         # the same list walked backwards: positions 0..3 and 4..6
        seq, starts = seq.flip(0), torch.tensor([True, False, False, False, True, False, False])
    want = torch.zeros(n, d, dtype=torch.float64)
    for rows in (seq[:4], seq[4:]) if reverse else (seq[:3], seq[3:]):
        out = torch.nn.functional.conv1d(x[rows].t()[None], weight, bias, padding=k - 1, groups=d)[0, :, :len(rows)].t()
        want[rows] = torch.nn.functional.silu(out) if activation else out
    got = causal_conv1d_reference(x, weight, bias, activation, seq, starts)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_mamba_keeps_its_state_dict():
    keys = {"A_log", "D", "in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias",
            "out_proj.weight"}
    sd = ME.MinkowskiMamba(32, d_state=16, d_conv=4, expand=2).state_dict()
    assert set(sd) == keys and tuple(sd["conv1d.weight"].shape) == (64, 1, 4) and tuple(sd["conv1d.bias"].shape) == (64,)
