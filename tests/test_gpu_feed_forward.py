"""MinkowskiFeedForward on the kernels of csrc/feed_forward.hip against the torch formulation linear -> act -> linear.
Exactness: on inputs from {-1, 0, 1} with relu every intermediate is a small integer, so all six outputs equal the float64
reference bit for bit, whatever the tiling.  Accuracy: per tensor E_ours <= 4 E_torch with E the largest absolute error
against float64 on the CPU and E_torch that of torch's same-dtype GPU path; where E_torch is 0 the floor is
finfo(dtype).eps * max|reference| (the bound of tests/test_gpu_layer_norm.py)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import minkowskiengine_amd as ME
from minkowskiengine_amd import backend
from minkowskiengine_amd.feed_forward import ACTIVATIONS

pytestmark = pytest.mark.gpu
FACTOR = 4.0
DTYPES = (torch.float32, torch.bfloat16)
NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2")
ROWS = backend.FFN_ROWS


def _split_n(c, hd, cout, dtype):
    """the smallest row count with at least three row splits of the weight-gradient kernel and a ragged last one"""
    return next(n for n in range(2 * ROWS + 37, 40 * ROWS, ROWS) if backend.feed_forward_row_splits(n, c, hd, cout, dtype) >= 3)


def _inputs(n, c, hd, cout, dtype, device, integer, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda *s: torch.randint(-1, 2, s, generator=g).float()) if integer else (lambda *s: torch.randn(*s, generator=g))
    s1, s2 = (1.0, 1.0) if integer else (c ** -0.5, hd ** -0.5)
    t = {"x": rnd(n, c), "w1": s1 * rnd(hd, c), "b1": rnd(hd), "w2": s2 * rnd(cout, hd), "b2": rnd(cout), "dy": rnd(n, cout)}
    return {k: v.to(dtype).to(device) for k, v in t.items()}


def _grads(t, mlp):
    leaf = {k: t[k].clone().requires_grad_() for k in ("x", "w1", "b1", "w2", "b2")}
    y = mlp(*leaf.values())
    gs = torch.autograd.grad(y, list(leaf.values()), t["dy"])
    return dict(zip(NAMES, (y.detach(),) + tuple(gs)))


def _ours(t, act):
    return _grads(t, lambda x, w1, b1, w2, b2: ME.MinkowskiFeedForwardFunction.apply(x, w1, b1, w2, b2, act))


def _torch(t, act, dtype=None, device=None):
    t = {k: v.to(device=device or v.device, dtype=dtype or v.dtype) for k, v in t.items()}
    return _grads(t, lambda x, w1, b1, w2, b2: F.linear(ACTIVATIONS[act](F.linear(x, w1, b1)), w2, b2))


def _widths(kind, dtype):
    top = backend.FFN_MAX_WIDTH[dtype]
    return {"32": (32, 32, 32), "96-96-64": (96, 96, 64), "64-160-96": (64, 160, 96), "max-in": (top, 64, 32),
            "max-out": (32, 64, top)}[kind]


@pytest.mark.parametrize("rows", ["1", "31", "33", "block+1", "splits"])
@pytest.mark.parametrize("widths", ["32", "96-96-64", "64-160-96", "max-in", "max-out"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_integer_inputs_are_exact(device, dtype, widths, rows):
    c, hd, cout = _widths(widths, dtype)
    n = {"1": 1, "31": 31, "33": 33, "block+1": ROWS + 1}.get(rows) or _split_n(c, hd, cout, dtype)
    t = _inputs(n, c, hd, cout, dtype, device, integer=True)
    cpu = {k: v.double().cpu() for k, v in t.items()}
    z = cpu["x"] @ cpu["w1"].T + cpu["b1"]
    dh = cpu["dy"] @ cpu["w2"]
    ref = _torch(cpu, "relu")
    assert z.abs().max() <= 256 and dh.abs().max() <= 256                   # exact in bf16
    assert all(v.abs().max() < 2 ** 24 for v in ref.values())               # every sum exact in fp32
    ours = _ours(t, "relu")
    for name in NAMES:
        assert torch.equal(ours[name].cpu(), ref[name].to(dtype)), name


@pytest.mark.parametrize("mode", ["no-bias", "in", "fc1", "fc2"])
@pytest.mark.parametrize("rows", ["33", "block+1"])
@pytest.mark.parametrize("widths", ["32", "64-160-96"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_integer_inputs_are_exact_without_biases_and_per_gradient(device, dtype, widths, rows, mode):
    """The operators called directly on the inputs of test_integer_inputs_are_exact: with every bias None, and with
    each need_grad_* flag alone (an output that is not wanted is None)."""
    c, hd, cout = _widths(widths, dtype)
    n = {"33": 33, "block+1": ROWS + 1}[rows]
    t = _inputs(n, c, hd, cout, dtype, device, integer=True)
    bias = mode != "no-bias"
    cpu = {k: v.double().cpu() * (1.0 if bias or k not in ("b1", "b2") else 0.0) for k, v in t.items()}
    z = cpu["x"] @ cpu["w1"].T + cpu["b1"]
    dh = cpu["dy"] @ cpu["w2"]
    ref = _torch(cpu, "relu")
    assert z.abs().max() <= 256 and dh.abs().max() <= 256                   # exact in bf16
    assert all(v.abs().max() < 2 ** 24 for v in ref.values())               # every sum exact in fp32
    b1, b2 = (t["b1"], t["b2"]) if bias else (None, None)
    need = {"no-bias": (True, True, True), "in": (True, False, False), "fc1": (False, True, False),
            "fc2": (False, False, True)}[mode]
    y = backend.FeedForwardForwardGPU(t["x"], t["w1"], b1, t["w2"], b2, "relu")
    grads = backend.FeedForwardBackwardGPU(t["x"], t["dy"], t["w1"], b1, t["w2"], "relu", *need)
    wanted = dict(zip(NAMES[1:], (need[0], need[1], need[1] and bias, need[2], need[2])))
    assert torch.equal(y.cpu(), ref["y"].to(dtype))
    for name, g in zip(NAMES[1:], grads):
        if wanted[name]:
            assert torch.equal(g.cpu(), ref[name].to(dtype)), name
        else:
            assert g is None, name


@pytest.mark.parametrize("shape", [(133, 64, 128, 64), (128, 32, 96, 64)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", sorted(ACTIVATIONS))
def test_matches_float64_within_torchs_error(device, host_layer, act, dtype, shape):
    t = _inputs(*shape, dtype, device, integer=False)
    ref, ours, base = _torch(t, act, torch.float64, "cpu"), _ours(t, act), _torch(t, act)
    for name in NAMES:
        err = lambda a: float((a.double().cpu() - ref[name]).abs().max())
        e_ours, e_torch = err(ours[name]), err(base[name])
        floor = torch.finfo(dtype).eps * float(ref[name].abs().max())
        print(f"{act} {dtype} {shape} {name}: E_ours {e_ours:.3e} E_torch {e_torch:.3e} floor {floor:.3e}")
        assert e_ours <= FACTOR * (e_torch if e_torch > 0 else floor), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_host_layers_and_reruns_give_the_same_bits(device, dtype):
    t = _inputs(ROWS + 5, 64, 160, 96, dtype, device, integer=False)
    results = {}
    for host in ("python", "native"):
        ME.set_host(host)
        try:
            results[host] = _ours(t, "gelu")
            again = _ours(t, "gelu")
        finally:
            ME.set_host("python")
        for name in NAMES:
            assert torch.equal(results[host][name], again[name]), (host, name)
    for name in NAMES:
        assert torch.equal(results["python"][name], results["native"][name]), name


def test_module(device, host_layer):
    n, c, hd = 70, 64, 256
    g = torch.Generator().manual_seed(3)
    seq = nn.Sequential(nn.Linear(c, hd), nn.GELU(), nn.Linear(hd, c)).to(device)
    mlp = ME.MinkowskiFeedForward(c, hd).to(device)
    mlp.load_state_dict({k.replace("0.", "fc1.").replace("2.", "fc2."): v for k, v in seq.state_dict().items()}, strict=True)
    coords = torch.cat([torch.zeros(n, 1), torch.arange(n)[:, None], torch.zeros(n, 2)], 1).int().to(device)
    feats = torch.randn(n, c, generator=g).to(device)
    field = ME.TensorField(feats, coordinates=coords.float() + 0.25)
    assert mlp.is_fused(field)
    out = mlp(field)
    assert isinstance(out, ME.TensorField) and out.coordinate_field_map_key == field.coordinate_field_map_key
    ref = nn.Sequential(nn.Linear(c, hd), nn.GELU(), nn.Linear(hd, c)).double()
    ref.load_state_dict(seq.state_dict())
    want = ref(feats.double().cpu()).detach()
    e_ours = float((out.F.detach().double().cpu() - want).abs().max())
    e_torch = float((seq(feats).detach().double().cpu() - want).abs().max())
    print(f"module: E_ours {e_ours:.3e} E_torch {e_torch:.3e}")
    assert e_ours <= FACTOR * e_torch
    # a frozen fc1: no gradient comes back for it
    mlp.fc1.requires_grad_(False)
    x = ME.SparseTensor(feats.clone().requires_grad_(), coords)
    mlp(x).F.sum().backward()
    assert mlp.fc1.weight.grad is None and mlp.fc1.bias.grad is None
    assert mlp.fc2.weight.grad is not None and x.F.grad is not None
    w = [p.detach() for p in (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight)]
    grads = ME.get_minkowski_function("FeedForwardBackward", feats)(feats, feats, *w, "gelu", need_grad_fc1=False)
    assert grads[1] is None and grads[2] is None and all(grads[i] is not None for i in (0, 3, 4))
    assert not ME.MinkowskiFeedForward(256, 512).to(device).bfloat16().is_fused(feats.bfloat16().repeat(1, 4))
    # outside the width rule: the torch formulation, exactly
    for width, dtype in ((48, torch.float32), (64, torch.float64)):
        other = ME.MinkowskiFeedForward(width, 2 * width, activation="silu").to(device).to(dtype)
        xs = ME.SparseTensor(torch.randn(n, width, generator=g).to(dtype).to(device), coords)
        assert not other.is_fused(xs)
        assert torch.equal(other(xs).F, other.fc2(F.silu(other.fc1(xs.F))))
