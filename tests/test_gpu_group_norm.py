"""GPU tests of MinkowskiGroupNorm (csrc/group_norm.hip through the operators of both host layers).

Expectation: float64 on the CPU, torch.nn.functional.group_norm on every instance's [1, C, n_b] tensor with autograd for
the three gradients (the reference has no group norm, so there is no recorded fixture); computed once per case and
shared by the tests and host layers that use it.

Bounds, the project's own as tests/test_gpu_instance_norm.py states them.  fp32: helpers.assert_close at its defaults,
1e-4 + 1e-4 |b| per element.  float64: 1e-10.  bf16: the expectation is evaluated on the bf16-rounded inputs; the kernels
compute in fp32 and round once at the store (half an ulp of an 8-bit significand = 2^-8 relative), so out and grad_in get
1e-4 + 2^-8 |b|; the parameter gradients are fp32 sums and keep the fp32 bound."""
import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

from helpers import assert_close, make_cloud

pytestmark = pytest.mark.gpu
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)     # MinkowskiEngine/utils/gradcheck.py:37-39
NAMES = ("out", "grad_in", "grad_weight", "grad_bias")
EPS = 1e-5

# (instance row counts, C, G, D, interleaved)
FP32_CASES = {
    "sizes700_40_1_c16_g4": ((700, 40, 1), 16, 4, 3, False),        # cg = the piece width; a one-row instance with cg > 1
    "c12_g4_straddle": ((300, 257), 12, 4, 3, False),               # 4-float pieces straddle the groups of 3
    "c6_g2_scalar": ((300, 257), 6, 2, 3, False),                   # c % 4 != 0: one element per piece
    "c5_g1_scalar": ((90, 10), 5, 1, 3, False),
    "interleaved_c24_g3": ((400, 400), 24, 3, 3, True),             # the two instances alternate row by row
    "c1024_g32_capped": ((2500, 2500), 1024, 32, 3, False),         # one row lane, 512 chunks; one chunk holds the boundary
    "one_instance_c96_g3": ((3000,), 96, 3, 3, False),
    "4d_c8_g2": ((200, 100), 8, 2, 4, False),
}
BF16_CASES = {
    "sizes700_40_1_c16_g4": ((700, 40, 1), 16, 4, 3, False),
    "c24_g4_straddle": ((300, 257), 24, 4, 3, False),               # cg = 6: 8-element pieces straddle the groups
}
_cache = {}


def _scene(sizes, D, interleaved, seed):
    parts = []
    for b, k in enumerate(sizes):
        extent = max(4, int(np.ceil((4 * k) ** (1.0 / D))))         # a quarter of the cells at the most
        pts = make_cloud(k, extent, D, seed=seed + b)
        assert pts.shape[0] == k
        pts[:, 0] = b
        parts.append(pts)
    if interleaved:
        assert len(set(sizes)) == 1
        return torch.stack(parts, 1).reshape(-1, D + 1).contiguous()
    return torch.cat(parts, 0)


def _expect(feats, batch, groups, weight, bias, dy, eps=EPS):
    """float64 on the CPU -> (out, grad_in, grad_weight, grad_bias) as numpy arrays"""
    x = feats.detach().double().cpu().requires_grad_(True)
    w = weight.detach().double().cpu().requires_grad_(True)
    b = bias.detach().double().cpu().requires_grad_(True)
    batch = batch.cpu().long()
    out = torch.zeros_like(x)
    for i in torch.unique(batch):
        m = (batch == i).nonzero().reshape(-1)
        o = torch.nn.functional.group_norm(x[m].t()[None], groups, w, b, eps)[0].t()
        out = out.index_copy(0, m, o)
    out.backward(dy.detach().double().cpu())
    return out.detach().numpy(), x.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def _case(name, table=FP32_CASES, bf16=False, feats_fn=None):
    """the inputs of a case and its expectation, built once"""
    key = (name, bf16, feats_fn)
    if key not in _cache:
        sizes, c, groups, D, interleaved = table[name]
        seed = sum(sizes) + 31 * c + groups
        coords = _scene(sizes, D, interleaved, seed)
        g = torch.Generator().manual_seed(seed)
        n = coords.shape[0]
        feats = torch.randn(n, c, generator=g) if feats_fn is None else feats_fn(n, c, g)
        dy = torch.rand(n, c, generator=g) - 0.5
        if bf16:
            feats, dy = feats.bfloat16().float(), dy.bfloat16().float()
        z = dict(coords=coords, feats=feats, grad_out=dy, weight=torch.rand(c, generator=g) + 0.5,
                 bias=torch.rand(c, generator=g) - 0.5, groups=groups)
        z["want"] = _expect(feats, coords[:, 0], groups, z["weight"], z["bias"], dy)
        _cache[key] = z
    return _cache[key]


def _layer(ME, device, z, dtype, **kw):
    layer = ME.MinkowskiGroupNorm(z["groups"], z["feats"].shape[1], **kw)
    if dtype == torch.float64:
        layer = layer.double()
    layer = layer.to(device)
    if layer.weight is not None:
        with torch.no_grad():
            layer.weight.copy_(z["weight"])
            layer.bias.copy_(z["bias"])
    return layer


def _run(ME, device, z, dtype, perm=None):
    """module forward + backward -> (out, grad_in, grad_weight, grad_bias, layer, x)"""
    layer = _layer(ME, device, z, dtype)
    feats, coords, dy = z["feats"], z["coords"], z["grad_out"]
    if perm is not None:
        feats, coords, dy = feats[perm], coords[perm], dy[perm]
    x = ME.SparseTensor(feats.to(dtype).to(device), coords.to(device), requires_grad=True)
    assert torch.equal(x.C.cpu(), coords), "rows keep the order they were given in"
    y = layer(x)
    assert y.F.dtype == dtype and y.coordinate_map_key == x.coordinate_map_key
    assert y.coordinate_manager is x.coordinate_manager
    y.F.backward(dy.to(dtype).to(device))
    return y.F.detach(), x.F.grad, layer.weight.grad, layer.bias.grad, layer, x


@pytest.mark.parametrize("name", list(FP32_CASES))
def test_fp32_parity(device, host_layer, name):
    import minkowskiengine_amd as ME
    z = _case(name)
    got = _run(ME, device, z, torch.float32)
    assert got[2].dtype == torch.float32 and tuple(got[2].shape) == (z["feats"].shape[1],)
    for g, w, what in zip(got, z["want"], NAMES):
        assert bool(torch.isfinite(g).all()), what
        assert_close(g, w, what=what)


def _offset_feats(n, c, g):
    return 100.0 + torch.randn(n, c, generator=g) + 3.0 * torch.randn(1, c, generator=g)


def test_offset_stability(device, host_layer):
    """rows at 100 + N(0, 1) plus per-channel offsets of 3 N(0, 1): E[x^2] - E[x]^2 in fp32 loses the digits the bound
    asks for (x^2 is 1e4 with an ulp of 1e-3 against a variance of about 10); shifted sums and Chan merges do not"""
    import minkowskiengine_amd as ME
    z = _case("offset", {"offset": ((5000, 700), 64, 8, 3, False)}, feats_fn=_offset_feats)
    assert float(z["feats"].mean()) > 90
    got = _run(ME, device, z, torch.float32)
    for g, w, what in zip(got, z["want"], NAMES):
        assert_close(g, w, what=what)


def test_one_group_per_channel_is_instance_norm(device, host_layer):
    import minkowskiengine_amd as ME
    z = dict(_case("sizes700_40_1_c16_g4"))
    c = z["feats"].shape[1]
    z["groups"] = c
    got = _run(ME, device, z, torch.float32)
    inorm = ME.MinkowskiInstanceNorm(c).to(device)
    inorm.eps = got[4].eps = EPS
    assert got[4].eps == inorm.eps
    with torch.no_grad():
        inorm.weight.copy_(z["weight"].reshape(1, c))
        inorm.bias.copy_(z["bias"].reshape(1, c))
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
    y = inorm(x)
    y.F.backward(z["grad_out"].to(device))
    want = (y.F.detach(), x.F.grad, inorm.weight.grad.reshape(-1), inorm.bias.grad.reshape(-1))
    for g, w, what in zip(got, want, NAMES):
        assert_close(g, w.cpu().numpy(), what=what)
    # the one-row instance: variance 0, normalised value 0 -> out = bias and a gradient of exactly 0
    one = z["coords"][:, 0] == 2
    assert int(one.sum()) == 1
    assert torch.equal(got[0].cpu()[one], z["bias"].reshape(1, c))
    assert bool((got[1].cpu()[one] == 0).all())


def test_row_order_and_bitwise_reproducibility(device):
    """shuffled rows change nothing beyond fp32 reassociation; every run is bitwise reproducible and the two host layers
    agree bit for bit"""
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    perm = torch.randperm(z["feats"].shape[0], generator=torch.Generator().manual_seed(3))
    prev = ME.get_host()
    try:
        runs = {}
        for order, p in (("sorted", None), ("shuffled", perm)):
            for host in ("python", "native", "python", "native", "python", "native"):
                ME.set_host(host)
                runs.setdefault(order, []).append(_run(ME, device, z, torch.float32, perm=p)[:4])
            for r in runs[order][1:]:
                for a, b, what in zip(runs[order][0], r, NAMES):
                    assert torch.equal(a, b), (order, what)
    finally:
        ME.set_host(prev)
    base, shuf = runs["sorted"][0], runs["shuffled"][0]
    assert_close(shuf[0], base[0].cpu()[perm], what="out")
    assert_close(shuf[1], base[1].cpu()[perm], what="grad_in")
    assert_close(shuf[2], base[2], what="grad_weight")
    assert_close(shuf[3], base[3], what="grad_bias")
    assert_close(shuf[0], z["want"][0][perm.numpy()], what="out vs the expectation")
    assert_close(shuf[1], z["want"][1][perm.numpy()], what="grad_in vs the expectation")


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_bf16(device, host_layer, name):
    import minkowskiengine_amd as ME
    z = _case(name, BF16_CASES, bf16=True)
    out, gi, gw, gb, layer, _ = _run(ME, device, z, torch.bfloat16)
    assert out.dtype == torch.bfloat16 and gi.dtype == torch.bfloat16
    assert layer.weight.dtype == torch.float32 and gw.dtype == torch.float32 and gb.dtype == torch.float32
    w_out, w_gi, w_gw, w_gb = z["want"]
    assert_close(out, w_out, atol=1e-4, rtol=2.0 ** -8, what="out")
    assert_close(gi, w_gi, atol=1e-4, rtol=2.0 ** -8, what="grad_in")
    assert_close(gw, w_gw, what="grad_weight")
    assert_close(gb, w_gb, what="grad_bias")


def test_float64_parity(device, host_layer):
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    got = _run(ME, device, z, torch.float64)
    for g, w, what in zip(got, z["want"], NAMES):
        g = g.cpu().numpy()
        assert g.dtype == np.float64
        err = float(np.abs(g - w).max())
        print(what, "max abs err", err)
        assert err <= 1e-10, f"{what}: {err}"


def test_float64_gradcheck(device, host_layer):
    import minkowskiengine_amd as ME
    c0 = [[0, 0], [0, 1], [1, 0], [1, 1], [2, 1], [3, 2], [0, 3]]
    c1 = [[1, 0], [0, 2], [2, 2], [3, 0], [1, 3]]
    coords = ME.utils.batched_coordinates([torch.IntTensor(c0), torch.IntTensor(c1)]).to(device)
    g = torch.Generator().manual_seed(0)
    assert coords.shape[0] == 12
    feats = torch.rand(12, 6, generator=g, dtype=torch.float64).to(device).requires_grad_()
    x = ME.SparseTensor(feats, coords)
    key, cm = x.coordinate_map_key, x.coordinate_manager
    layer = ME.MinkowskiGroupNorm(2, 6).double().to(device)
    with torch.no_grad():
        layer.weight.copy_(torch.rand(6, generator=g, dtype=torch.float64) + 0.5)
        layer.bias.copy_(torch.rand(6, generator=g, dtype=torch.float64))
    assert gradcheck(lambda f, w, b: ME.MinkowskiGroupNormFunction.apply(f, 2, w, b, EPS, key, None, cm),
                     (x.F, layer.weight, layer.bias), **GC)
    wrap = lambda f: ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=cm)      # noqa: E731
    assert gradcheck(lambda f: layer(wrap(f)).F, (x.F,), **GC)
    assert gradcheck(lambda f, w, b: ME.MinkowskiFunctional.group_norm(wrap(f), 2, w, b).F,
                     (x.F, layer.weight, layer.bias), **GC)
    assert gradcheck(lambda f: ME.MinkowskiFunctional.group_norm(wrap(f), 3).F, (x.F,), **GC)


def test_affine_false_and_the_functional_form(device, host_layer):
    import minkowskiengine_amd as ME
    z = dict(_case("c12_g4_straddle"))
    c = z["feats"].shape[1]
    z["weight"], z["bias"] = torch.ones(c), torch.zeros(c)
    base = _run(ME, device, z, torch.float32)

    def go(fn):
        x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
        y = fn(x)
        assert y.coordinate_map_key == x.coordinate_map_key and y.coordinate_manager is x.coordinate_manager
        y.F.backward(z["grad_out"].to(device))
        return y.F.detach(), x.F.grad

    plain = _layer(ME, device, z, torch.float32, affine=False)
    assert list(plain.parameters()) == []
    for out, gi in (go(plain), go(lambda x: ME.MinkowskiFunctional.group_norm(x, z["groups"]))):
        assert torch.equal(out, base[0]) and torch.equal(gi, base[1])
    # the functional form with parameters is the module
    w = z["weight"].to(device).requires_grad_(True)
    b = z["bias"].to(device).requires_grad_(True)
    out, gi = go(lambda x: ME.MinkowskiFunctional.group_norm(x, z["groups"], w, b, EPS))
    assert torch.equal(out, base[0]) and torch.equal(gi, base[1])
    assert torch.equal(w.grad, base[2]) and torch.equal(b.grad, base[3])


def test_non_default_stream(device, host_layer):
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    base = _run(ME, device, z, torch.float32)[:4]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        got = _run(ME, device, z, torch.float32)[:4]
    side.synchronize()
    for a, b, what in zip(base, got, NAMES):
        assert torch.equal(a, b), what


def test_non_contiguous_grad_out(device, host_layer):
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    c = z["feats"].shape[1]
    layer = _layer(ME, device, z, torch.float32)
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
    wide = torch.zeros(x.F.shape[0], 2 * c + 1, device=device)
    wide[:, 1:c + 1] = z["grad_out"].to(device)
    dy = wide[:, 1:c + 1]
    assert not dy.is_contiguous()
    layer(x).F.backward(dy)
    for g, w, what in zip((x.F.grad, layer.weight.grad, layer.bias.grad), z["want"][1:], NAMES[1:]):
        assert_close(g, w, what=what)


def test_api_errors(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(300, 10, 3, seed=5, batch=2).to(device)
    x = ME.SparseTensor(torch.rand(coords.shape[0], 6, device=device), coords)
    with pytest.raises(AssertionError, match="Channel size mismatch"):
        ME.MinkowskiGroupNorm(1, 5).to(device)(x)
    with pytest.raises(ValueError, match="GroupNormForwardCPU"):          # as the other layers: no CPU operator
        ME.MinkowskiGroupNormFunction.apply(x.F.cpu(), 2, None, None, EPS, x.coordinate_map_key, None,
                                            x.coordinate_manager)
    with pytest.raises(RuntimeError, match="num_groups"):                  # the operators check the groups themselves
        ME.MinkowskiFunctional.group_norm(x, 4)
    with pytest.raises(RuntimeError):                                      # parameters left on the CPU
        ME.MinkowskiGroupNorm(2, 6)(x)
    with pytest.raises(RuntimeError):                                      # float64 features need a .double() module
        ME.MinkowskiGroupNorm(2, 6).to(device)(ME.SparseTensor(x.F.double(), coordinate_map_key=x.coordinate_map_key,
                                                               coordinate_manager=x.coordinate_manager))


def test_composition_on_a_pruned_generative_branch(device, host_layer):
    """conv -> MinkowskiGroupNorm -> MinkowskiSiLU -> pruning -> generative transposed convolution, forward and backward"""
    import minkowskiengine_amd as ME
    coords = make_cloud(1000, 14, 3, seed=17, batch=2)
    g = torch.Generator().manual_seed(17)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 4, generator=g).to(device), coords.to(device), requires_grad=True)
    conv = ME.MinkowskiConvolution(4, 12, kernel_size=2, stride=2, dimension=3).to(device)
    norm = ME.MinkowskiGroupNorm(3, 12).to(device)
    up = ME.MinkowskiGenerativeConvolutionTranspose(12, 6, kernel_size=2, stride=2, dimension=3).to(device)
    h = conv(x)
    hn = norm(h)
    assert hn.coordinate_map_key == h.coordinate_map_key and hn.coordinate_manager is h.coordinate_manager
    assert hn.F.shape == h.F.shape
    act = ME.MinkowskiSiLU()(hn)
    keep = torch.rand(act.F.shape[0], generator=g) < 0.6
    assert 0 < int(keep.sum()) < keep.numel()
    y = up(ME.MinkowskiPruning()(act, keep.to(device)))
    assert y.F.shape[0] == 8 * int(keep.sum()) and y.F.shape[1] == 6
    (y.F ** 2).sum().backward()
    for name, t in (("input", x.F.grad), ("conv", conv.kernel.grad), ("weight", norm.weight.grad),
                    ("bias", norm.bias.grad), ("up", up.kernel.grad)):
        assert t is not None and bool(torch.isfinite(t).all()), name
        assert float(t.abs().max()) > 0, name
