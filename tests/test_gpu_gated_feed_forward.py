"""MinkowskiGatedFeedForward on the kernels of csrc/gated_feed_forward.hip against the torch formulation
fc2(act(fc1_g(x)) * fc1_x(x)).  Exactness: rows of x and dy with at most four entries from {-1, 1}, parameters from
{-1, 0, 1} and relu keep every intermediate a small integer (|Zg|, |Zu| <= 5, |H| <= 25, |dH| <= 4, |dZg|, |dZu| <= 20:
exact in bf16), so all eight outputs equal the float64 reference bit for bit, whatever the tiling.  Accuracy: per tensor
E_ours <= 4 E_torch with E the largest absolute error against float64 on the CPU and E_torch that of torch's same-dtype
GPU path; where E_torch is 0 the floor is finfo(dtype).eps * max|reference| (the bound of tests/test_gpu_feed_forward.py)."""
import pytest
import torch
import torch.nn.functional as F

import minkowskiengine_amd as ME
from minkowskiengine_amd import backend
from minkowskiengine_amd.feed_forward import ACTIVATIONS

pytestmark = pytest.mark.gpu
FACTOR = 4.0
DTYPES = (torch.float32, torch.bfloat16)
LEAVES = ("x", "wg", "bg", "wu", "bu", "w2", "b2")
NAMES = ("y", "dx", "dwg", "dbg", "dwu", "dbu", "dw2", "db2")
ROWS = backend.FFN_ROWS


def _inputs(n, c, hd, cout, dtype, device, integer, seed=0):
    g = torch.Generator().manual_seed(seed)
    if integer:
        rnd = lambda *s: torch.randint(-1, 2, s, generator=g).float()
        sparse = lambda m, k: torch.zeros(m, k).scatter_(1, torch.randint(0, k, (m, 4), generator=g),
                                                         torch.randint(0, 2, (m, 4), generator=g) * 2.0 - 1.0)
        t = {"x": sparse(n, c), "wg": rnd(hd, c), "bg": rnd(hd), "wu": rnd(hd, c), "bu": rnd(hd), "w2": rnd(cout, hd),
             "b2": rnd(cout), "dy": sparse(n, cout)}
    else:
        rnd = lambda *s: torch.randn(*s, generator=g)
        t = {"x": rnd(n, c), "wg": c ** -0.5 * rnd(hd, c), "bg": rnd(hd), "wu": c ** -0.5 * rnd(hd, c), "bu": rnd(hd),
             "w2": hd ** -0.5 * rnd(cout, hd), "b2": rnd(cout), "dy": rnd(n, cout)}
    return {k: v.to(dtype).to(device) for k, v in t.items()}


def _grads(t, mlp):
    leaf = [t[k].clone().requires_grad_() for k in LEAVES]
    y = mlp(*leaf)
    return dict(zip(NAMES, (y.detach(),) + torch.autograd.grad(y, leaf, t["dy"])))


def _ours(t, act):
    return _grads(t, lambda *w: ME.MinkowskiGatedFeedForwardFunction.apply(*w, act))


def _torch(t, act, dtype=None, device=None):
    t = {k: v.to(device=device or v.device, dtype=dtype or v.dtype) for k, v in t.items()}
    return _grads(t, lambda x, wg, bg, wu, bu, w2, b2: F.linear(ACTIVATIONS[act](F.linear(x, wg, bg)) * F.linear(x, wu, bu),
                                                                 w2, b2))


def _widths(kind, dtype):
    top = backend.GLU_MAX_WIDTH[dtype]
    return {"32": (32, 32, 32), "64-160-96": (64, 160, 96 if top >= 96 else 32), "max-in": (top, 64, 32),
            "max-out": (32, 64, top)}[kind]


@pytest.mark.parametrize("rows", ["1", "33", "block+1", "splits"])
@pytest.mark.parametrize("widths", ["32", "64-160-96", "max-in", "max-out"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_integer_inputs_are_exact(device, dtype, widths, rows):
    c, hd, cout = _widths(widths, dtype)
    # "splits": the smallest ragged row count with at least three row splits of the weight-gradient kernel
    n = {"1": 1, "33": 33, "block+1": ROWS + 1}.get(rows) or next(
        m for m in range(2 * ROWS + 37, 40 * ROWS, ROWS) if backend.gated_feed_forward_row_splits(m, c, hd, cout, dtype) >= 3)
    t = _inputs(n, c, hd, cout, dtype, device, integer=True)
    cpu = {k: v.double().cpu() for k, v in t.items()}
    zg, zu = cpu["x"] @ cpu["wg"].T + cpu["bg"], cpu["x"] @ cpu["wu"].T + cpu["bu"]
    dh = cpu["dy"] @ cpu["w2"]
    ref = _torch(cpu, "relu")
    top = lambda v: float(v.abs().max())
    assert top(zg) <= 5 and top(zu) <= 5 and top(F.relu(zg) * zu) <= 25 and top(dh) <= 4          # exact in bf16
    assert top(dh * zu * (zg > 0)) <= 20 and top(dh * F.relu(zg)) <= 20
    assert all(top(v) < 2 ** 24 for v in ref.values())                                            # every sum exact in fp32
    ours = _ours(t, "relu")
    for name in NAMES:
        assert torch.equal(ours[name].cpu(), ref[name].to(dtype)), name


@pytest.mark.parametrize("mode", ["no-bias", "in", "fc1", "fc2"])
@pytest.mark.parametrize("rows", ["33", "block+1"])
@pytest.mark.parametrize("widths", ["32", "64-160-96"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_integer_inputs_are_exact_without_biases_and_per_gradient(device, dtype, widths, rows, mode):
    """The operators called directly on the inputs of test_integer_inputs_are_exact: with every bias None, and with
    each need_grad_* flag alone (an output that is not wanted is None).  The bounds that keep the float64 reference exact
    in bf16 are asserted again, on the inputs as this test uses them."""
    c, hd, cout = _widths(widths, dtype)
    n = {"33": 33, "block+1": ROWS + 1}[rows]
    t = _inputs(n, c, hd, cout, dtype, device, integer=True)
    bias = mode != "no-bias"
    cpu = {k: v.double().cpu() * (1.0 if bias or k not in ("bg", "bu", "b2") else 0.0) for k, v in t.items()}
    zg, zu = cpu["x"] @ cpu["wg"].T + cpu["bg"], cpu["x"] @ cpu["wu"].T + cpu["bu"]
    dh = cpu["dy"] @ cpu["w2"]
    ref = _torch(cpu, "relu")
    top = lambda v: float(v.abs().max())
    assert top(zg) <= 5 and top(zu) <= 5 and top(F.relu(zg) * zu) <= 25 and top(dh) <= 4          # exact in bf16
    assert top(dh * zu * (zg > 0)) <= 20 and top(dh * F.relu(zg)) <= 20
    assert all(top(v) < 2 ** 24 for v in ref.values())                                            # every sum exact in fp32
    bg, bu, b2 = (t["bg"], t["bu"], t["b2"]) if bias else (None, None, None)
    need = {"no-bias": (True, True, True), "in": (True, False, False), "fc1": (False, True, False),
            "fc2": (False, False, True)}[mode]
    y = backend.GatedFeedForwardForwardGPU(t["x"], t["wg"], bg, t["wu"], bu, t["w2"], b2, "relu")
    grads = backend.GatedFeedForwardBackwardGPU(t["x"], t["dy"], t["wg"], bg, t["wu"], bu, t["w2"], "relu", *need)
    fc1b = need[1] and bias
    wanted = dict(zip(NAMES[1:], (need[0], need[1], fc1b, need[1], fc1b, need[2], need[2])))
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
    """Largest E_ours / E_torch seen on one MI355X over all cases: see DESIGN 8.19."""
    t = _inputs(*shape, dtype, device, integer=False)
    ref, ours, base = _torch(t, act, torch.float64, "cpu"), _ours(t, act), _torch(t, act)
    for name in NAMES:
        err = lambda a: float((a.double().cpu() - ref[name]).abs().max())
        e_ours, e_torch = err(ours[name]), err(base[name])
        floor = torch.finfo(dtype).eps * float(ref[name].abs().max())
        print(f"{act} {dtype} {shape} {name}: E_ours {e_ours:.3e} E_torch {e_torch:.3e} floor {floor:.3e} "
              f"ratio {e_ours / (e_torch if e_torch > 0 else floor):.2f}")
        assert e_ours <= FACTOR * (e_torch if e_torch > 0 else floor), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_host_layers_and_reruns_give_the_same_bits(device, dtype):
    t = _inputs(ROWS + 5, 64, 160, 64, dtype, device, integer=False)
    results = {}
    for host in ("python", "native"):
        ME.set_host(host)
        try:
            results[host] = _ours(t, "silu")
            again = _ours(t, "silu")
        finally:
            ME.set_host("python")
        for name in NAMES:
            assert torch.equal(results[host][name], again[name]), (host, name)
    for name in NAMES:
        assert torch.equal(results["python"][name], results["native"][name]), name


def test_module(device, host_layer):
    n, c, hd = 70, 64, 160
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(device)
    timm = {"fc1_g.weight": rnd(hd, c) * c ** -0.5, "fc1_g.bias": rnd(hd), "fc1_x.weight": rnd(hd, c) * c ** -0.5,
            "fc1_x.bias": rnd(hd), "fc2.weight": rnd(c, hd) * hd ** -0.5, "fc2.bias": rnd(c)}     # timm SwiGLU's names
    mlp = ME.MinkowskiGatedFeedForward(c, hd).to(device)
    mlp.load_state_dict(timm, strict=True)
    coords = torch.cat([torch.zeros(n, 1), torch.arange(n)[:, None], torch.zeros(n, 2)], 1).int().to(device)
    feats = rnd(n, c)
    field = ME.TensorField(feats, coordinates=coords.float() + 0.25)
    assert mlp.is_fused(field)
    out = mlp(field)
    assert isinstance(out, ME.TensorField) and out.coordinate_field_map_key == field.coordinate_field_map_key
    # a packed first layer, either half as the gate: the bits of the separate one
    for first, second, gate_first in (("fc1_g", "fc1_x", True), ("fc1_x", "fc1_g", False)):
        packed = ME.MinkowskiGatedFeedForward.from_packed(
            torch.cat([timm[first + ".weight"], timm[second + ".weight"]]), torch.cat([timm[first + ".bias"], timm[second + ".bias"]]),
            timm["fc2.weight"], timm["fc2.bias"], gate_first=gate_first)
        assert packed.is_fused(field) and torch.equal(packed(field).F, out.F)
    # frozen fc1_g / fc1_x: no gradient comes back for them
    mlp.fc1_g.requires_grad_(False)
    mlp.fc1_x.requires_grad_(False)
    x = ME.SparseTensor(feats.clone().requires_grad_(), coords)
    mlp(x).F.sum().backward()
    assert all(p.grad is None for p in list(mlp.fc1_g.parameters()) + list(mlp.fc1_x.parameters()))
    assert mlp.fc2.weight.grad is not None and mlp.fc2.bias.grad is not None and x.F.grad is not None
    # outside the width rule: the torch formulation, exactly
    for width, dtype in ((48, torch.float32), (64, torch.float64), (128, torch.float32)):
        other = ME.MinkowskiGatedFeedForward(width, 2 * width, activation="gelu").to(device).to(dtype)
        xs = ME.SparseTensor(torch.randn(n, width, generator=g).to(dtype).to(device), coords)
        assert not other.is_fused(xs)
        assert torch.equal(other(xs).F, other.fc2(F.gelu(other.fc1_g(xs.F)) * other.fc1_x(xs.F)))
