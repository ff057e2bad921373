"""MinkowskiLayerNorm / MinkowskiRMSNorm on the GPU (csrc/layer_norm.hip) against torch.nn.functional.layer_norm / rms_norm
in float64 on the CPU, on the inputs as stored (bf16 inputs are up-cast).  The bound is the project's for fused kernels:
per tensor E_ours <= 4 E_torch with E the largest absolute error and E_torch that of torch's same-dtype GPU path (add +
norm); where E_torch is 0 the floor is finfo(dtype).eps * max|reference|.

The bitwise checks on views compare y, stream and dx: every row sum is one balanced tree over the channel index whatever
piece width and lane team serve the row.  The parameter gradients of a view are NOT asserted bit-equal to those of its
copy: the rows a lane sums depend on the team width (they are bitwise reproducible per layout, which is asserted)."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib

pytestmark = pytest.mark.gpu
FACTOR = 4.0
KINDS, DTYPES = ("layer", "rms"), (torch.float32, torch.bfloat16)
SHAPES = [(1, 8), (257, 8), (130, 96), (67, 520), (5, 2048), (33, 7), (33, 12), (40, 1), ("uneven", 64)]
NAMES = ("y", "stream", "dx", "dr", "dw", "db")


def _eps(kind, dtype):
    return 1e-5 if kind == "layer" else torch.finfo(dtype).eps          # eps=None of torch.nn.RMSNorm


def _uneven_n(c, elem):
    """the smallest n >= 200 with n = G k + 1 for G = me_lnorm_chunks(n, c, elem) >= 2: chunks of unequal length"""
    lib = _lib.load()
    return next(n for n in range(200, 4000) if lib.me_lnorm_chunks(n, c, elem) >= 2 and n % lib.me_lnorm_chunks(n, c, elem) == 1)


def _inputs(n, c, dtype, device, residual, seed=0, x=None):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    t = {"x": (rnd(n, c) if x is None else x).to(dtype), "r": rnd(n, c).to(dtype) if residual else None,
         "w": 1 + 0.1 * rnd(c), "b": 0.1 * rnd(c), "dy": rnd(n, c).to(dtype), "ds": rnd(n, c).to(dtype) if residual else None}
    return {k: None if v is None else v.to(device) for k, v in t.items()}


def _grads(kind, t, norm):
    """y, stream and the gradients of (x, r, w, b) under the output gradients (dy, ds); `norm(x, r, w, b) -> y | (y, stream)`"""
    leaf = {k: None if t[k] is None or (k == "b" and kind == "rms") else t[k].clone().requires_grad_() for k in "xrwb"}
    out = norm(leaf["x"], leaf["r"], leaf["w"], leaf["b"])
    y, stream = out if leaf["r"] is not None else (out, None)
    ins = [v for v in leaf.values() if v is not None]
    outs, gos = ([y, stream], [t["dy"], t["ds"]]) if stream is not None else ([y], [t["dy"]])
    gs = dict(zip([k for k, v in leaf.items() if v is not None], torch.autograd.grad(outs, ins, gos)))
    return dict(zip(NAMES, (y, stream, gs["x"], gs.get("r"), gs.get("w"), gs.get("b"))))


def _ours(kind, t, eps):
    return _grads(kind, t, lambda x, r, w, b: ME.MinkowskiLayerNormFunction.apply(x, r, w, b, eps, kind == "rms"))


def _torch(kind, t, eps, dtype=None, device=None):
    """the unfused torch formulation in `dtype` on `device` (default: as stored)"""
    t = {k: None if v is None else v.to(device=device or v.device, dtype=dtype or t["x"].dtype) for k, v in t.items()}

    def norm(x, r, w, b):
        s = x if r is None else r + x
        y = F.rms_norm(s, s.shape[1:], w, eps) if kind == "rms" else F.layer_norm(s, s.shape[1:], w, b, eps)
        return y if r is None else (y, s)
    return _grads(kind, t, norm)


def _assert_bound(kind, t, dtype):
    eps = _eps(kind, dtype)
    ref, ours, base = _torch(kind, t, eps, torch.float64, "cpu"), _ours(kind, t, eps), _torch(kind, t, eps)
    for name in NAMES:
        if ref[name] is None:
            continue
        err = lambda a: float((a.detach().double().cpu() - ref[name]).abs().max()) if a.numel() else 0.0
        e_ours, e_torch = err(ours[name]), err(base[name])
        floor = torch.finfo(dtype).eps * float(ref[name].abs().max()) if ref[name].numel() else 0.0
        print(f"{kind} {dtype} {tuple(t['x'].shape)} {name}: E_ours {e_ours:.3e} E_torch {e_torch:.3e} floor {floor:.3e}")
        assert e_ours <= FACTOR * (e_torch if e_torch > 0 else floor), name
    assert ours["dr"] is None or ours["dr"].data_ptr() == ours["dx"].data_ptr()       # one tensor, returned twice


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_matches_the_yardstick_within_torchs_error(device, host_layer, kind, dtype, residual, shape):
    n, c = shape
    if n == "uneven":
        n = _uneven_n(c, torch.finfo(dtype).bits // 8)
    _assert_bound(kind, _inputs(n, c, dtype, device, residual), dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_two_pass_variance_on_a_large_offset(device, host_layer, kind):
    g = torch.Generator().manual_seed(1)
    x = 1e4 + 1e-2 * torch.randn(130, 96, generator=g)
    _assert_bound(kind, _inputs(130, 96, torch.float32, device, False, x=x), torch.float32)


def _equal(a, b, names):
    for name in names:
        assert (a[name] is None) == (b[name] is None) and (a[name] is None or torch.equal(a[name], b[name])), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_bitwise_equalities(device, kind, dtype):
    n, c, eps = 130, 96, _eps(kind, dtype)
    t = _inputs(n, c, dtype, device, True)
    results = {}
    for host in ("python", "native"):
        ME.set_host(host)
        try:
            fused = _ours(kind, t, eps)
            _equal(fused, _ours(kind, t, eps), NAMES)                                      # two runs
            # the unfused ME addition followed by the plain call, on sparse tensors of one map
            coords = torch.cat([torch.zeros(n, 1), torch.arange(n)[:, None], torch.zeros(n, 2)], 1).int().to(device)
            mod = (ME.MinkowskiRMSNorm(c) if kind == "rms" else ME.MinkowskiLayerNorm(c)).to(device)
            with torch.no_grad():
                mod.weight.copy_(t["w"])
                if kind == "layer":
                    mod.bias.copy_(t["b"])
            grads = {}
            for form in ("unfused", "fused"):
                xs = ME.SparseTensor(t["x"].clone().requires_grad_(), coords)
                rs = ME.SparseTensor(t["r"].clone().requires_grad_(), coordinate_map_key=xs.coordinate_map_key,
                                     coordinate_manager=xs.coordinate_manager)
                if form == "unfused":
                    stream = rs + xs
                    y = mod(stream)
                else:
                    y, stream = mod.forward_residual(xs, rs)
                mod.zero_grad()
                torch.autograd.backward([y.F, stream.F], [t["dy"], t["ds"]])
                grads[form] = dict(zip(NAMES, (y.F, stream.F, xs.F.grad, rs.F.grad, mod.weight.grad.clone(),
                                               mod.bias.grad.clone() if kind == "layer" else None)))
            _equal(grads["fused"], grads["unfused"], NAMES)
            _equal(grads["fused"], fused, NAMES)
            # a column view and a misaligned view against their contiguous copies
            for col in (8, 1):
                view = dict(t)
                for k in ("x", "r", "dy", "ds"):
                    big = torch.zeros(n, c + 16, dtype=dtype, device=device)
                    big[:, col:col + c] = t[k]
                    view[k] = big[:, col:col + c]
                    assert not view[k].is_contiguous()
                _equal(_ours(kind, view, eps), fused, ("y", "stream", "dx", "dr"))
            results[host] = fused
        finally:
            ME.set_host("python")
    _equal(results["python"], results["native"], NAMES)


@pytest.mark.parametrize("kind", KINDS)
def test_constant_and_zero_rows_are_exact(device, host_layer, kind):
    for dtype in DTYPES:
        t = _inputs(33, 96, dtype, device, False)
        t["x"][3] = 0.0 if kind == "rms" else 2.71875
        y = _ours(kind, t, _eps(kind, dtype))["y"]
        want = torch.zeros(96, device=device) if kind == "rms" else t["b"]
        assert torch.equal(y[3], want.to(dtype))


@pytest.mark.parametrize("c", [8, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_a_poisoned_row_stays_in_its_team(device, host_layer, kind, c):
    t = _inputs(64, c, torch.bfloat16, device, False)
    clean = _ours(kind, t, _eps(kind, torch.bfloat16))
    t["x"] = t["x"].clone()
    t["x"][5, c // 2] = float("nan")
    t["x"][40, 3] = float("inf")
    bad = _ours(kind, t, _eps(kind, torch.bfloat16))
    keep = torch.ones(64, dtype=torch.bool, device=device)
    keep[[5, 40]] = False
    for name in ("y", "dx"):
        assert torch.equal(bad[name][keep], clean[name][keep]), name
    assert bad["y"][5].isnan().all() and bad["y"][40].isnan().any()
    assert kind == "rms" or bad["y"][40].isnan().all()


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_matrix(device, host_layer, kind):
    out = _ours(kind, _inputs(0, 12, torch.float32, device, True), 1e-5)
    assert out["y"].shape == out["stream"].shape == out["dx"].shape == (0, 12)
    assert torch.equal(out["dw"], torch.zeros(12, device=device))
    assert kind == "rms" or torch.equal(out["db"], torch.zeros(12, device=device))


@pytest.mark.parametrize("kind", KINDS)
def test_float64_twins_and_gradcheck(device, host_layer, kind):
    for n, c in ((33, 12), (5, 2100)):
        t = {k: None if v is None else v.double() for k, v in _inputs(n, c, torch.float32, device, True).items()}
        ours, ref = _ours(kind, t, 1e-5), _torch(kind, t, 1e-5, torch.float64, "cpu")
        for name in NAMES:
            assert ref[name] is None or float((ours[name].cpu() - ref[name]).abs().max()) <= 1e-10, name
    t = {k: None if v is None else v.double().requires_grad_() for k, v in _inputs(7, 5, torch.float32, device, True).items()}
    args = (t["x"], t["r"], t["w"]) + ((t["b"],) if kind == "layer" else ())
    fn = lambda x, r, w, b=None: ME.MinkowskiLayerNormFunction.apply(x, r, w, b, 1e-5, kind == "rms")
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-3)


def _scene(device, n=1500, c=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.unique(torch.randint(0, 24, (2 * n, 3), generator=g), dim=0)[:n]
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(device)
    return torch.randn(pts.shape[0], c, generator=g).to(device), coords


def test_modules_on_tensors_and_fields(device, host_layer):
    feats, coords = _scene(device)
    ref = torch.nn.LayerNorm(64)
    with torch.no_grad():
        ref.weight.uniform_(0.5, 1.5)
        ref.bias.uniform_(-1, 1)
    mod = ME.MinkowskiLayerNorm(64).to(device)
    mod.load_state_dict(ref.state_dict(), strict=True)
    want = ref.double()(feats.double().cpu())
    y = mod(ME.SparseTensor(feats, coords))
    base = F.layer_norm(feats, (64,), mod.weight, mod.bias, 1e-5)
    e_ours, e_torch = (float((a.detach().double().cpu() - want).abs().max()) for a in (y.F, base))
    print(f"module: E_ours {e_ours:.3e} E_torch {e_torch:.3e}")
    assert e_ours <= FACTOR * e_torch
    field = ME.TensorField(feats, coordinates=coords.float() + 0.25)
    for out in (mod(field), ME.MinkowskiRMSNorm(64).to(device)(field), ME.MinkowskiFunctional.layer_norm(field),
                *mod.forward_residual(field, field)):
        assert isinstance(out, ME.TensorField) and out.coordinate_field_map_key == field.coordinate_field_map_key
        assert out._manager is field._manager and out.F.shape == feats.shape
    assert torch.equal(mod(field).F, y.F)
    # rows wider than the kernels serve take torch's path and still match
    wide = ME.SparseTensor(torch.randn(9, 2100, device=device), coords[:9])
    for m, fn in ((ME.MinkowskiLayerNorm(2100), F.layer_norm), (ME.MinkowskiRMSNorm(2100, eps=1e-6), F.rms_norm)):
        got, stream = m.to(device).forward_residual(wide, wide)
        assert torch.equal(stream.F, wide.F + wide.F)
        torch.testing.assert_close(got.F, fn((2 * wide.F).double(), (2100,), eps=m.eps).float(), rtol=1e-5, atol=1e-5)


def test_the_prenorm_example_runs(device, host_layer):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "prenorm_block.py")
    spec = importlib.util.spec_from_file_location("prenorm_block", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    feats, coords = _scene(device)
    stage = example.PreNormStage(64, 2, depth=2, patch_size=256).to(device)
    out = stage(ME.SparseTensor(feats, coords))
    out.F.square().mean().backward()
    for grad in (stage.blocks[-1].attn.in_proj_weight.grad, stage.blocks[0].norm1.weight.grad):
        assert grad.isfinite().all() and float(grad.abs().max()) > 0
