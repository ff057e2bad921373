"""What the SSD scan and MinkowskiMamba2 promise without a GPU: the exported names, the torch formulation against explicit
loops, the parameter layout of the block and its CPU / float64 path."""
import math

import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import backend
from minkowskiengine_amd.ssd_scan import ssd_scan_reference

KEYS = {"in_proj.weight": (2 * 128 + 2 * 2 * 64 + 4, 64), "conv1d.weight": (128 + 2 * 2 * 64, 1, 4),
        "conv1d.bias": (128 + 2 * 2 * 64,), "dt_bias": (4,), "A_log": (4,), "D": (4,), "norm.weight": (128,),
        "out_proj.weight": (64, 128)}            # MinkowskiMamba2(64, d_state=64, headdim=32, ngroups=2)


def test_names_are_exported():
    for name in ("MinkowskiMamba2", "MinkowskiSSDScanFunction", "ssd_scan", "ssd_scan_reference"):
        assert hasattr(ME, name), name
    assert callable(ME.MinkowskiFunctional.ssd_scan) and "ssd_scan" in ME.MinkowskiFunctional.__all__
    assert callable(backend.SSDScanForwardGPU) and callable(backend.SSDScanBackwardGPU)


def test_reference_equals_explicit_loops():
    g = torch.Generator().manual_seed(0)
    n, h, p, s, grp = 7, 2, 3, 4, 2
    x, dt, B, C = (torch.randn(n, w, generator=g, dtype=torch.float64) for w in (h * p, h, grp * s, grp * s))
    A, D, bias = -torch.rand(h, generator=g).double(), torch.randn(h, generator=g).double(), torch.randn(h, generator=g).double()
    seq, starts = torch.randperm(n, generator=g), torch.tensor([True, False, False, True, False, False, False])
    got = ssd_scan_reference(x, dt, A, B, C, D, bias, True, p, grp, seq, starts)
    want = torch.zeros(n, h * p, dtype=torch.float64)
    for i in range(h):
        state = [[0.0] * p for _ in range(s)]
        for r, start in zip(seq.tolist(), starts.tolist()):
            step = math.log1p(math.exp(float(dt[r, i] + bias[i])))
            for j in range(s):
                for k in range(p):
                    state[j][k] = (0.0 if start else math.exp(step * float(A[i])) * state[j][k]) + \
                        step * float(B[r, i * s + j]) * float(x[r, i * p + k])       # h // (h / grp) = i: one head a group
            for k in range(p):
                want[r, i * p + k] = sum(float(C[r, i * s + j]) * state[j][k] for j in range(s)) + float(D[i] * x[r, i * p + k])
    assert float((got - want).abs().max()) < 1e-12


def test_mamba2_has_the_state_dict_of_mamba_ssm():
    layer = ME.MinkowskiMamba2(64, d_state=64, headdim=32, ngroups=2)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == KEYS
    layer.load_state_dict({k: torch.randn(shape) for k, shape in KEYS.items()}, strict=True)
    fresh = ME.MinkowskiMamba2(64, d_state=64, headdim=32, ngroups=2)
    assert torch.all(fresh.D == 1) and torch.all(fresh.A_log >= 0) and torch.all(fresh.A_log <= math.log(16))
    step = torch.nn.functional.softplus(fresh.dt_bias)
    assert torch.all(step >= 1e-4 - 1e-7) and torch.all(step <= 0.1 + 1e-6)


class _Line:
    """a stand-in for the GPU coordinate manager (there is no CPU map): six rows, instances of 4 and 2 rows"""
    _manager = property(lambda self: self)
    _patch_rows = lambda self, key, size, order: (None, torch.tensor([2, 0, 3, 1, 5, 4], dtype=torch.int32))
    _origin_rows = lambda self, key: torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.int32)


def test_cpu_and_float64_operands_run_the_torch_formulation_and_backpropagate():
    """the path MinkowskiMamba2 takes for CPU tensors and float64: ssd_scan picks ssd_scan_reference by itself"""
    g = torch.Generator().manual_seed(1)
    x, dt, B, C = (torch.randn(6, w, generator=g, dtype=torch.float64, requires_grad=True) for w in (8, 2, 8, 8))
    A = -torch.rand(2, generator=g).double().requires_grad_()
    seq, starts = torch.tensor([2, 0, 3, 1, 5, 4]), torch.tensor([True, False, False, False, True, False])
    outs = [ME.ssd_scan(x, dt, A, B, C, None, None, True, 4, 2, "z", rev, None, _Line()) for rev in (False, True)]
    assert torch.equal(outs[0], ssd_scan_reference(x, dt, A, B, C, None, None, True, 4, 2, seq, starts))
    assert torch.equal(outs[1], ssd_scan_reference(x, dt, A, B, C, None, None, True, 4, 2, seq.flip(0),
                                                   torch.tensor([True, False, True, False, False, False])))
    grads = torch.autograd.grad(outs[0].sum() + outs[1].sum(), (x, dt, A, B, C))
    assert all(torch.isfinite(v).all() and v.abs().sum() > 0 for v in grads)
