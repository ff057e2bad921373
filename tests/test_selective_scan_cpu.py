"""The selective scan without a GPU: the public names, the C ABI of csrc/selective_scan.hip (declared, prototyped, exported;
version 1.27), its argument errors (all reachable with NULL data pointers), the torch formulation against a loop written
out by hand, and MinkowskiMamba's state dict."""
import math
import os
import re

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from minkowskiengine_amd.selective_scan import selective_scan_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "me_amd.h")).read()
SYMBOLS = ("me_sscan_supported", "me_sscan_chunk", "me_sscan_workspace_bytes", "me_sscan_forward", "me_sscan_backward")
FAKE = 4096      # an address that is never dereferenced: the checks come before any launch


def test_names_are_exported_on_both_hosts():
    for name in ("MinkowskiMamba", "MinkowskiSelectiveScanFunction", "selective_scan"):
        assert hasattr(ME, name), name
    assert callable(ME.MinkowskiFunctional.selective_scan) and "selective_scan" in ME.MinkowskiFunctional.__all__
    native = ME.host.native_module()
    for name in ("SelectiveScanForwardGPU", "SelectiveScanBackwardGPU"):
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
    assert lib.me_version() >= 370
    assert re.search(r"1\.27 \(370\)\s+round 27:", HEADER)
    assert lib.me_sscan_supported(1, 16, 0) == 1 and lib.me_sscan_supported(96, 8, 1) == 1
    assert lib.me_sscan_supported(64, 12, 0) == 0 and lib.me_sscan_supported(0, 16, 0) == 0
    assert lib.me_sscan_chunk() > 0
    assert lib.me_sscan_workspace_bytes(1000, 96, 16, 1) > lib.me_sscan_workspace_bytes(1000, 96, 16, 0) > 0


def _forward(lib, n=4, d=8, s=16, us=None, bs=None, ws=None, ws_bytes=0):
    us, bs = d if us is None else us, s if bs is None else bs
    return lib.me_sscan_forward(None, None, None, None, None, 0, us, d, d, bs, s, None, None, None, 1, None, None, 0, n, d, s,
                                None, d, None, ws, ws_bytes, None)


def _backward(lib, n=4, d=8, s=16, us=None, dz=None, dd=None, db=None):
    us = d if us is None else us
    return lib.me_sscan_backward(None, None, None, None, None, None, 0, us, d, d, s, s, d, None, None, None, 1, None, None, 0,
                                 n, d, s, None, None, None, dz, None, None, None, dd, db, None, 0, None)


@pytest.mark.parametrize("call,kwargs,message", [
    (_forward, dict(d=0), "s = 8 or 16"), (_backward, dict(s=12), "s = 8 or 16"),
    (_forward, dict(n=-1), "2^31"), (_backward, dict(n=1 << 31), "2^31"),
    (_forward, dict(us=7), "stride"), (_forward, dict(bs=15), "stride"), (_backward, dict(us=7), "stride"),
    (_backward, dict(dz=FAKE), "dz needs z"), (_backward, dict(dd=FAKE), "needs Dskip"),
    (_backward, dict(db=FAKE), "needs delta_bias"),
    (_forward, dict(), "must be given"), (_backward, dict(), "must be given"),
])
def test_argument_errors_come_before_any_launch(call, kwargs, message):
    lib = _lib.load()
    assert call(lib, **kwargs) != 0
    assert message in lib.me_last_error().decode(), lib.me_last_error()


def test_an_empty_matrix_is_legal():
    lib = _lib.load()
    assert _forward(lib, n=0) == 0 and _backward(lib, n=0) == 0


def test_the_torch_formulation_is_the_loop_written_out():
    g = torch.Generator().manual_seed(0)
    n, d, s = 7, 3, 4
    u, delta, z = (torch.randn(n, d, generator=g, dtype=torch.float64) for _ in range(3))
    B, C = (torch.randn(n, s, generator=g, dtype=torch.float64) for _ in range(2))
    A = -torch.rand(d, s, generator=g, dtype=torch.float64) - 0.1
    Dskip, bias = (torch.randn(d, generator=g, dtype=torch.float64) for _ in range(2))
    seq = torch.tensor([4, 0, 6, 2, 5, 1, 3])           # two instances: positions 0..2 and 3..6
    starts = torch.tensor([True, False, False, True, False, False, False])
    want = torch.zeros(n, d, dtype=torch.float64)
    for ch in range(d):
        h = [0.0] * s
        for p in range(n):
            r = int(seq[p])
            if starts[p]:
                h = [0.0] * s
            x = float(delta[r, ch] + bias[ch])
            dt = x if x > 20 else math.log1p(math.exp(x))
            y = float(Dskip[ch] * u[r, ch])
            for k in range(s):
                h[k] = math.exp(dt * float(A[ch, k])) * h[k] + dt * float(B[r, k]) * float(u[r, ch])
                y += float(C[r, k]) * h[k]
            zz = float(z[r, ch])
            want[r, ch] = y * zz / (1 + math.exp(-zz))
    got = selective_scan_reference(u, delta, A, B, C, Dskip, z, bias, True, seq, starts)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    plain = selective_scan_reference(u, delta.abs(), A, B, C, seq_rows=seq, starts=starts)
    assert plain.shape == (n, d) and not torch.equal(plain, got)


@pytest.mark.parametrize("bias", [False, True])
def test_mamba_has_the_state_dict_of_mamba_ssm(bias):
    m = ME.MinkowskiMamba(32, d_state=16, d_conv=4, expand=2, bias=bias)
    keys = {"A_log", "D", "in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias",
            "out_proj.weight"} | ({"in_proj.bias", "out_proj.bias"} if bias else set())
    sd = m.state_dict()
    assert set(sd) == keys
    shapes = {"A_log": (64, 16), "D": (64,), "in_proj.weight": (128, 32), "conv1d.weight": (64, 1, 4), "x_proj.weight": (34, 64),
              "dt_proj.weight": (64, 2), "out_proj.weight": (32, 64)}
    assert all(tuple(sd[k].shape) == v for k, v in shapes.items())
    assert torch.equal(sd["A_log"][5], torch.log(torch.arange(1, 17.0))) and torch.equal(sd["D"], torch.ones(64))
    dt = torch.nn.functional.softplus(sd["dt_proj.bias"])
    assert float(dt.min()) >= 0.9e-3 and float(dt.max()) <= 0.11
    other = ME.MinkowskiMamba(32, bias=bias, order="hilbert", bidirectional=True)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    with pytest.raises(ValueError):
        ME.MinkowskiMamba(32, order="snake")
