"""GPU tests of MinkowskiConditionalGroupNorm (the k_gnc_* kernels of csrc/group_norm.hip through the operators of both
host layers).

Expectation: float64 on the CPU, torch.nn.functional.group_norm on every instance's [1, C, n_b] tensor, then the
modulation `* (1 + scale[b]) + shift[b]`, then silu, with autograd for all six results (out, grad_in and the gradients of
weight, bias, scale and shift); computed once per case and shared by the tests and host layers that use it.

Bounds, the project's own as tests/test_gpu_group_norm.py states them.  fp32: helpers.assert_close at its defaults,
1e-4 + 1e-4 |b| per element.  float64: 1e-10.  bf16: the expectation is evaluated on the bf16-rounded inputs; the kernels
compute in fp32 and round once at the store, so out and grad_in get 1e-4 + 2^-8 |b|; the four parameter gradients are fp32
sums and keep the fp32 bound."""
import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

from helpers import assert_close, make_cloud

pytestmark = pytest.mark.gpu
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)     # MinkowskiEngine/utils/gradcheck.py:37-39
NAMES = ("out", "grad_in", "grad_weight", "grad_bias", "grad_scale", "grad_shift")
EPS = 1e-5
MANY = tuple(3 + (7 * b) % 38 for b in range(70))

# (instance row counts, C, G, D, interleaved)
FP32_CASES = {
    "sizes700_40_1_c16_g4": ((700, 40, 1), 16, 4, 3, False),        # a one-row instance
    "c12_g4_straddle": ((300, 257), 12, 4, 3, False),               # 4-float pieces straddle the groups of 3
    "c6_g2_scalar": ((300, 257), 6, 2, 3, False),                   # c % 4 != 0: one element per piece
    "interleaved_c24_g3": ((400, 400), 24, 3, 3, True),             # the two instances alternate row by row
    "70_instances_c8_g2": (MANY, 8, 2, 3, False),                   # a thread's rows span several instances
    "c1024_g32_capped": ((2500, 2500), 1024, 32, 3, False),         # one row lane, capped chunks
    "4d_c8_g2": ((200, 100), 8, 2, 4, False),
}
BF16_CASES = {
    "sizes700_40_1_c16_g4": ((700, 40, 1), 16, 4, 3, False),
    "c24_g4_straddle": ((300, 257), 24, 4, 3, False),               # cg = 6: 8-element pieces straddle the groups
}
PARITY = [(name, "silu") for name in FP32_CASES] + [("sizes700_40_1_c16_g4", None)]
_cache = {}


def _scene(sizes, D, interleaved, seed, batch_ids=None):
    parts = []
    for b, k in enumerate(sizes):
        extent = max(4, int(np.ceil((4 * k) ** (1.0 / D))))         # a quarter of the cells at the most
        pts = make_cloud(k, extent, D, seed=seed + b)
        assert pts.shape[0] == k
        pts[:, 0] = b if batch_ids is None else batch_ids[b]
        parts.append(pts)
    if interleaved:
        assert len(set(sizes)) == 1
        return torch.stack(parts, 1).reshape(-1, D + 1).contiguous()
    return torch.cat(parts, 0)


def _group_norm(xb, groups, w, b, eps):
    """torch.nn.functional.group_norm on the [1, C, n_b] tensor of one instance.  torch refuses a group of one value (one
    row with one channel per group); that group is written out: mean = the value, biased variance 0"""
    if xb.shape[0] * (xb.shape[1] // groups) > 1:
        return torch.nn.functional.group_norm(xb.t()[None], groups, w, b, eps)[0].t()
    xg = xb.reshape(xb.shape[0], groups, -1)
    mu = xg.mean(dim=(0, 2), keepdim=True)
    var = ((xg - mu) ** 2).mean(dim=(0, 2), keepdim=True)
    return ((xg - mu) / torch.sqrt(var + eps)).reshape(xb.shape) * w + b


def _expect(feats, batch, groups, weight, bias, scale, shift, dy, activation, eps=EPS, rows_of=None):
    """float64 on the CPU -> the six results as numpy arrays.  Row j of scale / shift belongs to the j-th smallest batch
    index, or to the batch index rows_of[j] when the tensor has lost an instance."""
    x = feats.detach().double().cpu().requires_grad_(True)
    w = weight.detach().double().cpu().requires_grad_(True)
    b = bias.detach().double().cpu().requires_grad_(True)
    sc = scale.detach().double().cpu().requires_grad_(True)
    sh = shift.detach().double().cpu().requires_grad_(True)
    batch = batch.cpu().long()
    ids = torch.unique(batch).tolist() if rows_of is None else list(rows_of)
    out = torch.zeros_like(x)
    for j, i in enumerate(ids):
        m = (batch == i).nonzero().reshape(-1)
        if m.numel() == 0:
            continue
        o = _group_norm(x[m], groups, w, b, eps)
        o = o * (1 + sc[j]) + sh[j]
        out = out.index_copy(0, m, torch.nn.functional.silu(o) if activation == "silu" else o)
    out.backward(dy.detach().double().cpu())
    return tuple(t.numpy() for t in (out.detach(), x.grad, w.grad, b.grad, sc.grad, sh.grad))


def _case(name, table=FP32_CASES, bf16=False, activation="silu", groups=None, batch_ids=None, zero_mod=False):
    """the inputs of a case and its expectation, built once"""
    key = (name, bf16, activation, groups, batch_ids, zero_mod)
    if key not in _cache:
        sizes, c, g_, D, interleaved = table[name]
        groups = g_ if groups is None else groups
        seed = sum(sizes) + 31 * c + g_
        coords = _scene(sizes, D, interleaved, seed, batch_ids)
        g = torch.Generator().manual_seed(seed)
        n, nb = coords.shape[0], len(sizes)
        feats = torch.randn(n, c, generator=g)
        dy = torch.rand(n, c, generator=g) - 0.5
        if bf16:
            feats, dy = feats.bfloat16().float(), dy.bfloat16().float()
        z = dict(coords=coords, feats=feats, grad_out=dy, weight=torch.rand(c, generator=g) + 0.5,
                 bias=torch.rand(c, generator=g) - 0.5, scale=0.5 * torch.randn(nb, c, generator=g),
                 shift=torch.randn(nb, c, generator=g), groups=groups, activation=activation)
        if zero_mod:
            z["scale"], z["shift"] = torch.zeros(nb, c), torch.zeros(nb, c)
        z["want"] = _expect(feats, coords[:, 0], groups, z["weight"], z["bias"], z["scale"], z["shift"], dy, activation)
        _cache[key] = z
    return _cache[key]


def _layer(ME, device, z, dtype, cls=None, **kw):
    if cls is None:
        layer = ME.MinkowskiConditionalGroupNorm(z["groups"], z["feats"].shape[1], activation=z["activation"], **kw)
    else:
        layer = cls(z["groups"], z["feats"].shape[1], **kw)
    if dtype == torch.float64:
        layer = layer.double()
    layer = layer.to(device)
    if layer.weight is not None:
        with torch.no_grad():
            layer.weight.copy_(z["weight"])
            layer.bias.copy_(z["bias"])
    return layer


def _run(ME, device, z, dtype, perm=None, modulate=True):
    """module forward + backward -> (out, grad_in, grad_weight, grad_bias, grad_scale, grad_shift, layer, x)"""
    layer = _layer(ME, device, z, dtype)
    feats, coords, dy = z["feats"], z["coords"], z["grad_out"]
    if perm is not None:
        feats, coords, dy = feats[perm], coords[perm], dy[perm]
    x = ME.SparseTensor(feats.to(dtype).to(device), coords.to(device), requires_grad=True)
    assert torch.equal(x.C.cpu(), coords), "rows keep the order they were given in"
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    sc = z["scale"].to(pd).to(device).requires_grad_(True) if modulate else None
    sh = z["shift"].to(pd).to(device).requires_grad_(True) if modulate else None
    y = layer(x, sc, sh)
    assert y.F.dtype == dtype and y.coordinate_map_key == x.coordinate_map_key
    assert y.coordinate_manager is x.coordinate_manager
    y.F.backward(dy.to(dtype).to(device))
    return (y.F.detach(), x.F.grad, layer.weight.grad, layer.bias.grad, sc.grad if modulate else None,
            sh.grad if modulate else None, layer, x)


@pytest.mark.parametrize("name,activation", PARITY)
def test_fp32_parity(device, host_layer, name, activation):
    import minkowskiengine_amd as ME
    z = _case(name, activation=activation)
    got = _run(ME, device, z, torch.float32)
    c, nb = z["feats"].shape[1], z["scale"].shape[0]
    assert got[2].dtype == torch.float32 and tuple(got[2].shape) == (c,)
    assert got[4].dtype == torch.float32 and tuple(got[4].shape) == (nb, c) and tuple(got[5].shape) == (nb, c)
    for g, w, what in zip(got, z["want"], NAMES):
        assert bool(torch.isfinite(g).all()), what
        assert_close(g, w, what=what)


# plain against conditional group norm: (table, dtype); the bf16 case has 8-element pieces that straddle the groups of 6
SPECIAL_CASES = {
    "c12_g4_straddle": (FP32_CASES, torch.float32),
    "sizes700_40_1_c24_g4_bf16": ({"sizes700_40_1_c24_g4_bf16": ((700, 40, 1), 24, 4, 3, False)}, torch.bfloat16),
}


@pytest.mark.parametrize("name", list(SPECIAL_CASES))
def test_plain_group_norm_is_a_special_case(device, host_layer, name):
    """without an activation and without (or with a zero) modulation the layer is MinkowskiGroupNorm bit for bit"""
    import minkowskiengine_amd as ME
    table, dtype = SPECIAL_CASES[name]
    z = _case(name, table, bf16=dtype == torch.bfloat16, activation=None, zero_mod=True)
    plain = _layer(ME, device, z, dtype, cls=ME.MinkowskiGroupNorm)
    x = ME.SparseTensor(z["feats"].to(dtype).to(device), z["coords"].to(device), requires_grad=True)
    y = plain(x)
    y.F.backward(z["grad_out"].to(dtype).to(device))
    want = (y.F.detach(), x.F.grad, plain.weight.grad, plain.bias.grad)
    none = _run(ME, device, z, dtype, modulate=False)
    zero = _run(ME, device, z, dtype)
    for got in (none, zero):
        for g, w, what in zip(got, want, NAMES):
            assert g.dtype == w.dtype and torch.equal(g, w), what
    assert none[4] is None and none[5] is None
    assert_close(zero[4], z["want"][4], what="grad_scale")
    assert_close(zero[5], z["want"][5], what="grad_shift")


def test_one_group_per_channel_and_a_one_row_instance(device, host_layer):
    """G = C: the one-row instance has variance 0 and a normalised value of 0 -> out = silu(be) and a gradient of exactly 0"""
    import minkowskiengine_amd as ME
    z = _case("sizes700_40_1_c16_g4", groups=16)
    got = _run(ME, device, z, torch.float32)
    for g, w, what in zip(got, z["want"], NAMES):
        assert_close(g, w, what=what)
    one = z["coords"][:, 0] == 2
    assert int(one.sum()) == 1
    be = z["bias"].double() * (1 + z["scale"][2].double()) + z["shift"][2].double()
    assert_close(got[0].cpu()[one], torch.nn.functional.silu(be).reshape(1, -1).numpy(), what="out of the one-row instance")
    assert bool((got[1].cpu()[one] == 0).all())


def test_batch_indices_with_gaps(device, host_layer):
    """batch indices 0, 3, 7: row j of scale / shift belongs to the j-th smallest index"""
    import minkowskiengine_amd as ME
    z = _case("sizes700_40_1_c16_g4", batch_ids=(0, 3, 7))
    assert sorted(set(z["coords"][:, 0].tolist())) == [0, 3, 7]
    got = _run(ME, device, z, torch.float32)
    assert tuple(got[4].shape) == (3, 16) and tuple(got[5].shape) == (3, 16)
    for g, w, what in zip(got, z["want"], NAMES):
        assert_close(g, w, what=what)
    # the same rows with indices 0, 1, 2 are the same computation
    base = _run(ME, device, _case("sizes700_40_1_c16_g4"), torch.float32)
    for a, b, what in zip(got[:6], base[:6], NAMES):
        assert torch.equal(a, b), what


def test_an_instance_without_rows(device, host_layer):
    """every row of batch index 1 pruned away: its rows of grad_scale / grad_shift are exactly 0 and written"""
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    c = z["feats"].shape[1]
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device))
    keep = (z["coords"][:, 0] == 0).to(device)
    xp = ME.MinkowskiPruning()(x, keep)
    assert xp.F.shape[0] == 300 and bool((xp.C[:, 0] == 0).all())
    feats = xp.F.detach().clone().requires_grad_(True)
    xq = ME.SparseTensor(feats, coordinate_map_key=xp.coordinate_map_key, coordinate_manager=xp.coordinate_manager)
    layer = _layer(ME, device, z, torch.float32)
    sc = z["scale"].to(device).requires_grad_(True)
    sh = z["shift"].to(device).requires_grad_(True)
    dy = z["grad_out"][:300].to(device)
    y = layer(xq, sc, sh)
    y.F.backward(dy)
    assert tuple(sc.grad.shape) == (2, c) and tuple(sh.grad.shape) == (2, c)
    assert bool((sc.grad[1] == 0).all()) and bool((sh.grad[1] == 0).all())
    want = _expect(feats, xp.C[:, 0], z["groups"], z["weight"], z["bias"], z["scale"], z["shift"], dy, "silu",
                   rows_of=(0, 1))
    for g, w, what in zip((y.F, feats.grad, layer.weight.grad, layer.bias.grad, sc.grad, sh.grad), want, NAMES):
        assert_close(g, w, what=what)


def test_composition_with_group_norm_and_torch(device, host_layer):
    """silu(MinkowskiGroupNorm(x).F * (1 + scale[b]) + shift[b]) written in torch on the GPU"""
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    got = _run(ME, device, z, torch.float32)
    plain = _layer(ME, device, z, torch.float32, cls=ME.MinkowskiGroupNorm)
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
    sc = z["scale"].to(device).requires_grad_(True)
    sh = z["shift"].to(device).requires_grad_(True)
    b = z["coords"][:, 0].long().to(device)
    out = torch.nn.functional.silu(plain(x).F * (1 + sc[b]) + sh[b])
    out.backward(z["grad_out"].to(device))
    want = (out.detach(), x.F.grad, plain.weight.grad, plain.bias.grad, sc.grad, sh.grad)
    for g, w, what in zip(got, want, NAMES):
        assert_close(g, w.cpu().numpy(), what=what)


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
                runs.setdefault(order, []).append(_run(ME, device, z, torch.float32, perm=p)[:6])
            for r in runs[order][1:]:
                for a, b, what in zip(runs[order][0], r, NAMES):
                    assert torch.equal(a, b), (order, what)
    finally:
        ME.set_host(prev)
    base, shuf = runs["sorted"][0], runs["shuffled"][0]
    assert_close(shuf[0], base[0].cpu()[perm], what="out")
    assert_close(shuf[1], base[1].cpu()[perm], what="grad_in")
    for i in (2, 3, 4, 5):
        assert_close(shuf[i], base[i], what=NAMES[i])
    assert_close(shuf[0], z["want"][0][perm.numpy()], what="out vs the expectation")
    assert_close(shuf[1], z["want"][1][perm.numpy()], what="grad_in vs the expectation")


def test_non_default_stream(device, host_layer):
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    base = _run(ME, device, z, torch.float32)[:6]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        got = _run(ME, device, z, torch.float32)[:6]
    side.synchronize()
    for a, b, what in zip(base, got, NAMES):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_bf16(device, host_layer, name):
    import minkowskiengine_amd as ME
    z = _case(name, BF16_CASES, bf16=True)
    out, gi, gw, gb, gsc, gsh, layer, _ = _run(ME, device, z, torch.bfloat16)
    assert out.dtype == torch.bfloat16 and gi.dtype == torch.bfloat16
    assert layer.weight.dtype == torch.float32
    for g in (gw, gb, gsc, gsh):
        assert g.dtype == torch.float32
    w_out, w_gi, w_gw, w_gb, w_gsc, w_gsh = z["want"]
    assert_close(out, w_out, atol=1e-4, rtol=2.0 ** -8, what="out")
    assert_close(gi, w_gi, atol=1e-4, rtol=2.0 ** -8, what="grad_in")
    assert_close(gw, w_gw, what="grad_weight")
    assert_close(gb, w_gb, what="grad_bias")
    assert_close(gsc, w_gsc, what="grad_scale")
    assert_close(gsh, w_gsh, what="grad_shift")


def test_bf16_scale_and_shift_get_bf16_gradients(device, host_layer):
    """the module converts scale / shift to the parameter dtype with .to(): the gradients flow back in the caller's dtype"""
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    layer = _layer(ME, device, z, torch.float32)
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
    sc = z["scale"].bfloat16().to(device).requires_grad_(True)
    sh = z["shift"].bfloat16().to(device).requires_grad_(True)
    y = layer(x, sc, sh)
    assert y.F.dtype == torch.float32
    y.F.backward(z["grad_out"].to(device))
    assert sc.grad.dtype == torch.bfloat16 and sh.grad.dtype == torch.bfloat16
    assert tuple(sc.grad.shape) == tuple(sc.shape)
    zr = dict(z, scale=sc.detach().float().cpu(), shift=sh.detach().float().cpu())
    ref = _run(ME, device, zr, torch.float32)
    assert torch.equal(y.F.detach(), ref[0]) and torch.equal(x.F.grad, ref[1])
    assert torch.equal(sc.grad, ref[4].bfloat16()) and torch.equal(sh.grad, ref[5].bfloat16())


def test_non_contiguous_grad_out(device, host_layer):
    import minkowskiengine_amd as ME
    z = _case("c12_g4_straddle")
    c = z["feats"].shape[1]
    layer = _layer(ME, device, z, torch.float32)
    x = ME.SparseTensor(z["feats"].to(device), z["coords"].to(device), requires_grad=True)
    sc = z["scale"].to(device).requires_grad_(True)
    sh = z["shift"].to(device).requires_grad_(True)
    wide = torch.zeros(x.F.shape[0], 2 * c + 1, device=device)
    wide[:, 1:c + 1] = z["grad_out"].to(device)
    dy = wide[:, 1:c + 1]
    assert not dy.is_contiguous()
    layer(x, sc, sh).F.backward(dy)
    for g, w, what in zip((x.F.grad, layer.weight.grad, layer.bias.grad, sc.grad, sh.grad), z["want"][1:], NAMES[1:]):
        assert_close(g, w, what=what)


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
    layer = ME.MinkowskiConditionalGroupNorm(2, 6, activation="silu").double().to(device)
    with torch.no_grad():
        layer.weight.copy_(torch.rand(6, generator=g, dtype=torch.float64) + 0.5)
        layer.bias.copy_(torch.rand(6, generator=g, dtype=torch.float64))
    sc = (0.5 * torch.randn(2, 6, generator=g, dtype=torch.float64)).to(device).requires_grad_()
    sh = torch.randn(2, 6, generator=g, dtype=torch.float64).to(device).requires_grad_()
    fn = ME.MinkowskiConditionalGroupNormFunction
    assert gradcheck(lambda f, w, b, s, t: fn.apply(f, 2, w, b, s, t, "silu", EPS, key, None, cm),
                     (x.F, layer.weight, layer.bias, sc, sh), **GC)
    assert gradcheck(lambda f, s, t: fn.apply(f, 2, None, None, s, t, None, EPS, key, None, cm), (x.F, sc, sh), **GC)
    wrap = lambda f: ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=cm)      # noqa: E731
    assert gradcheck(lambda f, s, t: layer(wrap(f), s, t).F, (x.F, sc, sh), **GC)
    assert gradcheck(lambda f, w, b, s, t: ME.MinkowskiFunctional.conditional_group_norm(
        wrap(f), 2, w, b, s, t, "silu").F, (x.F, layer.weight, layer.bias, sc, sh), **GC)
    assert gradcheck(lambda f, t: ME.MinkowskiFunctional.conditional_group_norm(wrap(f), 3, shift=t, activation="silu").F,
                     (x.F, sh), **GC)


def test_a_nan_stays_in_its_instance_and_group(device, host_layer):
    import minkowskiengine_amd as ME
    z = dict(_case("c12_g4_straddle"))
    feats = z["feats"].clone()
    row, ch = 310, 7                                    # instance 1, group 2 (channels 6..8)
    assert int(z["coords"][row, 0]) == 1
    feats[row, ch] = float("nan")
    z["feats"] = feats
    out = _run(ME, device, z, torch.float32)[0].cpu()
    want = torch.zeros_like(out, dtype=torch.bool)
    want[z["coords"][:, 0] == 1, 6:9] = True
    assert torch.equal(torch.isnan(out), want)
    assert_close(out[~want], z["want"][0][~want.numpy()], what="out outside the NaN's instance and group")


def test_a_very_negative_v_stays_finite(device, host_layer):
    """v = -100: exp(-v) overflows fp32 on the way to the sigmoid; out and the gradient stay finite (about 0)"""
    import minkowskiengine_amd as ME
    z = dict(_case("c12_g4_straddle"))
    c = z["feats"].shape[1]
    z["weight"], z["bias"] = torch.zeros(c), torch.full((c,), -100.0)
    z["scale"], z["shift"] = torch.zeros(2, c), torch.zeros(2, c)
    got = _run(ME, device, z, torch.float32)
    for g, what in zip(got[:6], NAMES):
        assert bool(torch.isfinite(g).all()), what
    assert float(got[0].abs().max()) < 1e-30 and float(got[1].abs().max()) < 1e-30


def test_api_errors(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(300, 10, 3, seed=5, batch=2).to(device)
    x = ME.SparseTensor(torch.rand(coords.shape[0], 6, device=device), coords)
    layer = ME.MinkowskiConditionalGroupNorm(2, 6, activation="silu").to(device)
    good = torch.zeros(2, 6, device=device)
    layer(x, good, good)
    with pytest.raises(AssertionError, match="Channel size mismatch"):
        ME.MinkowskiConditionalGroupNorm(1, 5).to(device)(x)
    with pytest.raises(RuntimeError, match="scale"):                       # one row too many
        layer(x, torch.zeros(3, 6, device=device), good)
    with pytest.raises(RuntimeError, match="scale"):                       # one channel too many
        layer(x, torch.zeros(2, 7, device=device), good)
    with pytest.raises(RuntimeError, match="shift"):
        layer(x, good, torch.zeros(12, device=device))
    with pytest.raises(RuntimeError, match="scale"):                       # scale left on the CPU
        layer(x, torch.zeros(2, 6), good)
    with pytest.raises(ValueError, match="ConditionalGroupNormForwardCPU"):          # as the other layers: no CPU operator
        ME.MinkowskiConditionalGroupNormFunction.apply(x.F.cpu(), 2, None, None, None, None, None, EPS,
                                                       x.coordinate_map_key, None, x.coordinate_manager)
    with pytest.raises(RuntimeError, match="num_groups"):                  # the operators check the groups themselves
        ME.MinkowskiFunctional.conditional_group_norm(x, 4)
    with pytest.raises(RuntimeError, match="activation"):                  # and the activation
        ME.MinkowskiFunctional.conditional_group_norm(x, 2, activation="relu")
    with pytest.raises(RuntimeError):                                      # float64 features need a .double() module
        layer(ME.SparseTensor(x.F.double(), coordinate_map_key=x.coordinate_map_key,
                              coordinate_manager=x.coordinate_manager))
