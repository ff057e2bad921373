"""GPU tests of MinkowskiInstanceNorm / MinkowskiStableInstanceNorm (csrc/instance_norm.hip through the operators of both
host layers): the fixtures recorded from the reference's own module in float64
(tests/golden/make_golden_instance_norm.py), the float64 twins and gradcheck, bf16, bitwise agreement of repeated runs
and of the two hosts, row order, the composed formulation on this package's existing pooling / broadcast kernels, the
reference's own Python package on those kernels, and the API's error paths.

Bounds.  fp32: helpers.assert_close at its defaults, 1e-4 + 1e-4 |b| per element (the project's fp32 bar; outputs are
O(1), gradients O(|dy| / sigma)).  float64: 1e-10.  bf16: the expectation is the float64 formula on the bf16-rounded
inputs; the kernels compute in fp32 and round once at the store, and one round-to-nearest to an 8-bit significand is at
most half an ulp = 2^-8 relative, so out and grad_in get 1e-4 + 2^-8 |b|; the parameter gradients are fp32 sums of exactly
widened bf16 values and keep the fp32 bar."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

from helpers import GOLDEN_DIR, assert_close, make_cloud
from oracle import ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "instance_norm_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)     # MinkowskiEngine/utils/gradcheck.py:37-39
NAMES = ("out", "grad_in", "grad_weight", "grad_bias")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(ref.reference_root(), "MinkowskiEngine")),
                               reason="needs the reference package (its source tree or oracle/_ref/reference_tree)")


def _formula(x, batch, w, b, dy, eps):
    """float64 on the CPU: (out, grad_in, grad_weight, grad_bias) of out = (x - mean_b) / sqrt(var_b + eps) * w + b"""
    x = x.detach().double().cpu().requires_grad_(True)
    w = w.detach().double().cpu().reshape(1, -1).requires_grad_(True)
    b = b.detach().double().cpu().reshape(1, -1).requires_grad_(True)
    batch = batch.cpu().long()
    out = torch.zeros_like(x)
    for i in torch.unique(batch):
        m = (batch == i).nonzero().reshape(-1)
        xi = x[m]
        mu = xi.mean(0, keepdim=True)
        var = ((xi - mu) ** 2).mean(0, keepdim=True)
        out = out.index_copy(0, m, (xi - mu) / torch.sqrt(var + eps) * w + b)
    out.backward(dy.detach().double().cpu())
    return out.detach().numpy(), x.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def _run(ME, device, z, dtype, cls="MinkowskiInstanceNorm", perm=None):
    """module forward + backward on a fixture's inputs -> (out, grad_in, grad_weight, grad_bias, layer, x)"""
    c = z["feats"].shape[1]
    layer = getattr(ME, cls)(c)
    if dtype == torch.float64:
        layer = layer.double()
    layer = layer.to(device)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(z["weight"]))
        layer.bias.copy_(torch.from_numpy(z["bias"]))
    feats, coords, dy = torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"]), torch.from_numpy(z["grad_out"])
    if perm is not None:
        feats, coords, dy = feats[perm], coords[perm], dy[perm]
    x = ME.SparseTensor(feats.to(dtype).to(device), coords.to(device), requires_grad=True)
    assert torch.equal(x.C.cpu(), coords), "rows keep the order they were given in"
    y = layer(x)
    assert y.F.dtype == dtype and y.coordinate_map_key == x.coordinate_map_key
    assert y.coordinate_manager is x.coordinate_manager
    y.F.backward(dy.to(dtype).to(device))
    return y.F.detach(), x.F.grad, layer.weight.grad, layer.bias.grad, layer, x


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fp32_matches_the_reference_fixture(device, host_layer, path):
    import minkowskiengine_amd as ME
    z = np.load(path)
    got = _run(ME, device, z, torch.float32)
    assert got[2].dtype == torch.float32 and tuple(got[2].shape) == (1, z["feats"].shape[1])
    for g, what in zip(got, NAMES):
        assert_close(g, z[what], what=what)


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_float64_matches_the_reference_fixture(device, host_layer, path):
    import minkowskiengine_amd as ME
    z = np.load(path)
    got = _run(ME, device, z, torch.float64)
    for g, what in zip(got, NAMES):
        g = g.cpu().numpy()
        assert g.dtype == np.float64
        err = float(np.abs(g - z[what]).max())
        print(what, "max abs err", err)
        assert err <= 1e-10, f"{what}: {err}"


def test_one_row_instance_is_exactly_zero(device, host_layer):
    """variance 0: the normalised value is 0 (out = bias) and the input gradient is exactly 0, as in the reference —
    under either eps"""
    import minkowskiengine_amd as ME
    z = np.load(os.path.join(GOLDEN_DIR, "instance_norm_3d_b3_sizes_c16.npz"))
    one = torch.from_numpy(z["coords"][:, 0] == 2)
    for cls in ("MinkowskiInstanceNorm", "MinkowskiStableInstanceNorm"):
        out, gi, _, _, layer, _ = _run(ME, device, z, torch.float32, cls)
        assert torch.equal(out.cpu()[one], layer.bias.detach().cpu().expand(int(one.sum()), -1))
        assert torch.all(gi.cpu()[one] == 0)


def test_float64_gradcheck(device, host_layer):
    import minkowskiengine_amd as ME
    from minkowskiengine_amd.normalization import _InstanceNormAffineFunction
    c0 = [[0, 0], [0, 1], [1, 0], [1, 1], [2, 1], [3, 2], [0, 3]]
    c1 = [[1, 0], [0, 2], [2, 2], [3, 0], [1, 3]]
    coords = ME.utils.batched_coordinates([torch.IntTensor(c0), torch.IntTensor(c1)]).to(device)
    g = torch.Generator().manual_seed(0)
    feats = torch.rand(coords.shape[0], 3, generator=g, dtype=torch.float64).to(device).requires_grad_()
    x = ME.SparseTensor(feats, coords)
    key, cm = x.coordinate_map_key, x.coordinate_manager
    for cls in (ME.MinkowskiInstanceNorm, ME.MinkowskiStableInstanceNorm):
        layer = cls(3).double().to(device)
        with torch.no_grad():
            layer.weight.copy_(torch.rand(1, 3, generator=g, dtype=torch.float64) + 0.5)
            layer.bias.copy_(torch.rand(1, 3, generator=g, dtype=torch.float64))
        assert gradcheck(lambda f, w, b: _InstanceNormAffineFunction.apply(f, w, b, layer.eps, key, None, cm),
                         (x.F, layer.weight, layer.bias), **GC)
        assert gradcheck(lambda f: layer(ME.SparseTensor(f, coordinate_map_key=key, coordinate_manager=cm)).F,
                         (x.F,), **GC)
    # the reference-shaped Function: no affine map, eps = 1e-8
    assert gradcheck(lambda f: ME.MinkowskiInstanceNormFunction.apply(f, key, None, cm), (x.F,), **GC)


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_bf16(device, host_layer, path):
    import minkowskiengine_amd as ME
    z = dict(np.load(path))
    # inputs rounded to bf16 first: the expectation is the float64 formula on exactly what the kernels read
    for k in ("feats", "grad_out"):
        z[k] = torch.from_numpy(z[k]).bfloat16().float().numpy()
    out, gi, gw, gb, layer, x = _run(ME, device, z, torch.bfloat16)
    assert layer.weight.dtype == torch.float32 and gw.dtype == torch.float32 and gi.dtype == torch.bfloat16
    w_out, w_gi, w_gw, w_gb = _formula(torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"][:, 0]),
                                       torch.from_numpy(z["weight"]), torch.from_numpy(z["bias"]),
                                       torch.from_numpy(z["grad_out"]), 1e-8)
    assert_close(out, w_out, atol=1e-4, rtol=2.0 ** -8, what="out")
    assert_close(gi, w_gi, atol=1e-4, rtol=2.0 ** -8, what="grad_in")
    assert_close(gw, w_gw, what="grad_weight")
    assert_close(gb, w_gb, what="grad_bias")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_runs_and_hosts_are_bit_identical(device, dtype):
    import minkowskiengine_amd as ME
    prev = ME.get_host()
    try:
        for path in CASES:
            z = np.load(path)
            results = []
            for host in ("python", "native", "python", "native"):
                ME.set_host(host)
                results.append(_run(ME, device, z, dtype)[:4])
            for r in results[1:]:
                for a, b, what in zip(results[0], r, NAMES):
                    assert torch.equal(a, b), (os.path.basename(path), what)
    finally:
        ME.set_host(prev)


def test_large_instances_with_channel_offsets(device, host_layer):
    """the 64-channel fixture's construction at 2 x 3000 rows (the fixture itself is capped by the size of a committed
    file): tens of chunks per instance, channel means up to 13 spreads from zero, where E[x^2] - E[x]^2 in fp32 loses
    the digits the bar asks for; against the float64 formula that the generator asserts for the fixtures"""
    import minkowskiengine_amd as ME
    coords = make_cloud(3000, 24, 3, seed=7, batch=2)
    g = torch.Generator().manual_seed(7)
    n, c = coords.shape[0], 64
    z = dict(coords=coords.numpy(),
             feats=((torch.rand(1, c, generator=g) * 8 - 4) + 0.3 * torch.randn(n, c, generator=g)).numpy(),
             weight=(torch.rand(1, c, generator=g) + 0.5).numpy(), bias=(torch.rand(1, c, generator=g) - 0.5).numpy(),
             grad_out=(torch.rand(n, c, generator=g) - 0.5).numpy())
    got = _run(ME, device, z, torch.float32)
    want = _formula(torch.from_numpy(z["feats"]), coords[:, 0], torch.from_numpy(z["weight"]),
                    torch.from_numpy(z["bias"]), torch.from_numpy(z["grad_out"]), 1e-8)
    for g_, w, what in zip(got, want, NAMES):
        assert_close(g_, w, what=what)


def test_row_order(device, host_layer):
    """shuffling the rows of the input permutes the output and changes nothing beyond fp32 reassociation"""
    import minkowskiengine_amd as ME
    z = np.load(os.path.join(GOLDEN_DIR, "instance_norm_3d_b2_c8.npz"))
    perm = torch.randperm(z["feats"].shape[0], generator=torch.Generator().manual_seed(3))
    base = _run(ME, device, z, torch.float32)
    shuf = _run(ME, device, z, torch.float32, perm=perm)
    assert_close(shuf[0], base[0].cpu()[perm], what="out")
    assert_close(shuf[1], base[1].cpu()[perm], what="grad_in")
    assert_close(shuf[2], base[2], what="grad_weight")
    assert_close(shuf[3], base[3], what="grad_bias")
    assert_close(shuf[0], z["out"][perm.numpy()], what="out vs fixture")
    assert_close(shuf[1], z["grad_in"][perm.numpy()], what="grad_in vs fixture")


def _inputs(coords, c, seed):
    """the fixtures' construction: per-(instance, channel) offsets in [-4, 4] + 0.3 randn, dy in [-0.5, 0.5]"""
    g = torch.Generator().manual_seed(seed)
    n, nb = coords.shape[0], int(coords[:, 0].max()) + 1
    offset = torch.rand(nb, c, generator=g) * 8 - 4
    return dict(coords=coords.numpy(), feats=(offset[coords[:, 0].long()] + 0.3 * torch.randn(n, c, generator=g)).numpy(),
                weight=(torch.rand(1, c, generator=g) + 0.5).numpy(), bias=(torch.rand(1, c, generator=g) - 0.5).numpy(),
                grad_out=(torch.rand(n, c, generator=g) - 0.5).numpy())


def test_an_instance_pruned_away(device, host_layer):
    """MinkowskiPruning removes every row of instance 1 of 3: the pruned map still has 3 instances on its origin map, one
    of them without rows (mean 0, rstd 1 / sqrt(eps), no contribution to any gradient).  Output and all four gradients
    against the float64 formula on the surviving rows; the removed rows get a zero gradient."""
    import minkowskiengine_amd as ME
    z = _inputs(make_cloud(400, 12, 3, seed=21, batch=3), 8, 21)
    coords, feats = torch.from_numpy(z["coords"]), torch.from_numpy(z["feats"])
    keep = coords[:, 0] != 1
    assert 0 < int(keep.sum()) < coords.shape[0] and set(coords[keep][:, 0].tolist()) == {0, 2}
    layer = ME.MinkowskiInstanceNorm(8).to(device)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(z["weight"]))
        layer.bias.copy_(torch.from_numpy(z["bias"]))
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
    pruned = ME.MinkowskiPruning()(x, keep.to(device))
    assert torch.equal(pruned.C.cpu(), coords[keep])
    y = layer(pruned)
    # the statistics keep a row for the instance that lost its rows: the origin map comes from the unpruned map
    assert x.coordinate_manager.origin_map_size() == 3
    assert y.F.shape == (int(keep.sum()), 8)
    dy = torch.from_numpy(z["grad_out"])[keep]
    y.F.backward(dy.to(device))
    want = _formula(feats[keep], coords[keep][:, 0], torch.from_numpy(z["weight"]), torch.from_numpy(z["bias"]), dy, 1e-8)
    got = (y.F.detach(), x.F.grad[keep.to(device)], layer.weight.grad, layer.bias.grad)
    for g_, w, what in zip(got, want, NAMES):
        assert bool(torch.isfinite(g_).all()), what
        assert_close(g_, w, what=what)
    assert bool((x.F.grad[~keep.to(device)] == 0).all())


def test_many_small_instances(device, host_layer):
    """40 instances of 5 - 60 points, c = 12: tens of batch indices in every chunk of the statistics kernels"""
    import minkowskiengine_amd as ME
    sizes = torch.randint(5, 61, (40,), generator=torch.Generator().manual_seed(40)).tolist()
    assert min(sizes) >= 5 and max(sizes) <= 60
    parts = []
    for b, k in enumerate(sizes):
        pts = make_cloud(k, 8, 3, seed=100 + b)
        pts[:, 0] = b
        parts.append(pts)
    z = _inputs(torch.cat(parts, 0), 12, 40)
    got = _run(ME, device, z, torch.float32)
    want = _formula(torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"][:, 0]), torch.from_numpy(z["weight"]),
                    torch.from_numpy(z["bias"]), torch.from_numpy(z["grad_out"]), 1e-8)
    for g_, w, what in zip(got, want, NAMES):
        assert_close(g_, w, what=what)


def test_shuffled_rows_over_several_chunks(device, host_layer):
    """3 x 3000 points, c = 32 (R = 32: 36 chunks of 256 rows), the rows randomly permuted before the tensor is built, so
    that every chunk mixes the three instances: against the float64 formula and, row by row, against the unpermuted
    run, as test_row_order"""
    import minkowskiengine_amd as ME
    z = _inputs(make_cloud(3000, 24, 3, seed=13, batch=3), 32, 13)
    n = z["feats"].shape[0]
    assert n == 9000
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13))
    assert len(set(z["coords"][perm.numpy()][:256, 0].tolist())) == 3
    base = _run(ME, device, z, torch.float32)
    shuf = _run(ME, device, z, torch.float32, perm=perm)
    want = _formula(torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"][:, 0]), torch.from_numpy(z["weight"]),
                    torch.from_numpy(z["bias"]), torch.from_numpy(z["grad_out"]), 1e-8)
    p = perm.numpy()
    for i, what in enumerate(NAMES):
        assert_close(base[i], want[i], what=what + " (sorted rows)")
    assert_close(shuf[0], want[0][p], what="out vs formula")
    assert_close(shuf[1], want[1][p], what="grad_in vs formula")
    assert_close(shuf[2], want[2], what="grad_weight vs formula")
    assert_close(shuf[3], want[3], what="grad_bias vs formula")
    assert_close(shuf[0], base[0].cpu()[perm], what="out")
    assert_close(shuf[1], base[1].cpu()[perm], what="grad_in")
    assert_close(shuf[2], base[2], what="grad_weight")
    assert_close(shuf[3], base[3], what="grad_bias")


def _composed(ME, x, weight, bias, eps):
    """the reference's operator chain (MinkowskiNormalization.py:204-251, 387-393) on this package's existing
    GlobalPoolingForwardGPU / BroadcastForwardGPU"""
    feat, key, cm = x.F, x.coordinate_map_key, x.coordinate_manager
    gkey = ME.CoordinateMapKey(key.get_coordinate_size())
    gpool = ME.get_minkowski_function("GlobalPoolingForward", feat, key)
    bcast = ME.get_minkowski_function("BroadcastForward", feat, key)
    mode = ME.PoolingMode.GLOBAL_AVG_POOLING_KERNEL
    mean, _ = gpool(feat, mode, key, gkey, cm._manager)
    centered = bcast(feat, -mean, ME.BroadcastMode.ELEMENTWISE_ADDITON, key, gkey, cm._manager)
    var, _ = gpool(centered ** 2, mode, key, gkey, cm._manager)
    inv_std = 1 / (var + eps).sqrt()
    norm = bcast(centered, inv_std, ME.BroadcastMode.ELEMENTWISE_MULTIPLICATION, key, gkey, cm._manager)
    return norm * weight + bias


def test_fused_agrees_with_the_composed_formulation(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(5000, 40, 3, seed=11, batch=4)
    g = torch.Generator().manual_seed(11)
    c = 32
    feats = torch.rand(coords.shape[0], c, generator=g) - 0.3
    x = ME.SparseTensor(feats.to(device), coords.to(device))
    assert x.F.shape[0] == 20000
    layer = ME.MinkowskiInstanceNorm(c).to(device)
    with torch.no_grad():
        layer.weight.copy_(torch.rand(1, c, generator=g) + 0.5)
        layer.bias.copy_(torch.rand(1, c, generator=g) - 0.5)
    fused = layer(x).F.detach()
    assert_close(fused, _composed(ME, x, layer.weight.detach(), layer.bias.detach(), 1e-8), what="fused vs composed")
    plain = ME.MinkowskiInstanceNormFunction.apply(x.F, x.coordinate_map_key, None, x.coordinate_manager)
    assert_close(plain, _composed(ME, x, 1.0, 0.0, 1e-8), what="Function vs composed")


def test_stable_instance_norm(device, host_layer):
    import minkowskiengine_amd as ME
    z = np.load(os.path.join(GOLDEN_DIR, "instance_norm_3d_b2_c8.npz"))
    got = _run(ME, device, z, torch.float32, "MinkowskiStableInstanceNorm")
    assert got[4].eps == 1e-6
    want = _formula(torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"][:, 0]), torch.from_numpy(z["weight"]),
                    torch.from_numpy(z["bias"]), torch.from_numpy(z["grad_out"]), 1e-6)
    for g, w, what in zip(got, want, NAMES):
        assert_close(g, w, what=what)
    out64 = _run(ME, device, z, torch.float64, "MinkowskiStableInstanceNorm")[0].cpu().numpy()
    assert float(np.abs(out64 - want[0]).max()) <= 1e-10
    # eps is the only difference to MinkowskiInstanceNorm: small, and visible in float64
    plain64 = _run(ME, device, z, torch.float64)[0].cpu().numpy()
    assert 0 < float(np.abs(out64 - plain64).max()) < 1e-3


def test_api_errors(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(300, 10, 3, seed=5, batch=2).to(device)
    x = ME.SparseTensor(torch.rand(coords.shape[0], 6, device=device), coords)
    with pytest.raises(AssertionError, match="Channel size mismatch"):
        ME.MinkowskiInstanceNorm(5).to(device)(x)
    with pytest.raises(ValueError, match="InstanceNormForwardCPU"):       # as the other layers: no CPU operator
        ME.MinkowskiInstanceNormFunction.apply(x.F.cpu(), x.coordinate_map_key, None, x.coordinate_manager)
    with pytest.raises(RuntimeError):                                      # parameters left on the CPU
        ME.MinkowskiInstanceNorm(6)(x)
    with pytest.raises(RuntimeError):                                      # float64 features need a .double() module
        ME.MinkowskiInstanceNorm(6).to(device)(ME.SparseTensor(x.F.double(), coordinate_map_key=x.coordinate_map_key,
                                                               coordinate_manager=x.coordinate_manager))


def test_strided_map_uses_its_own_rows(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(2000, 16, 3, seed=9, batch=3).to(device)
    x = ME.SparseTensor(torch.rand(coords.shape[0], 8, device=device), coords)
    y = ME.MinkowskiConvolution(8, 12, kernel_size=2, stride=2, dimension=3).to(device)(x)
    assert y.F.shape[0] < x.F.shape[0]
    layer = ME.MinkowskiInstanceNorm(12).to(device)
    out = layer(y)
    assert out.coordinate_map_key == y.coordinate_map_key and out.F.shape == y.F.shape
    want = _formula(y.F, y.C[:, 0], layer.weight, layer.bias, torch.zeros(y.F.shape), 1e-8)
    assert_close(out.F, want[0], what="out on the strided map")


_REF = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
import torch
import minkowskiengine_amd as OURS
import MinkowskiEngineBackend._C as C
from oracle import ref
from helpers import make_cloud, assert_close
ME = ref.import_reference_package(backend=C)          # the reference's Python, our pooling / broadcast kernels
dev = torch.device("cuda:0")
coords = make_cloud(3000, 16, 3, seed=2, batch=3)
g = torch.Generator().manual_seed(0)
feats = torch.rand(coords.shape[0], 16, generator=g)
w, b = torch.rand(1, 16, generator=g) + 0.5, torch.rand(1, 16, generator=g) - 0.5
dy = torch.rand(coords.shape[0], 16, generator=g) - 0.5
theirs, ours = ME.MinkowskiInstanceNorm(16).to(dev), OURS.MinkowskiInstanceNorm(16).to(dev)
with torch.no_grad():
    for layer in (theirs, ours):
        layer.weight.copy_(w); layer.bias.copy_(b)
x = ME.SparseTensor(feats.to(dev), coords.to(dev), requires_grad=True)
ox = OURS.SparseTensor(feats.to(dev), coords.to(dev), requires_grad=True)
y, oy = theirs(x), ours(ox)
assert torch.equal(y.C, oy.C)
assert_close(oy.F, y.F, what="out")
y.F.backward(dy.to(dev)); oy.F.backward(dy.to(dev))
assert_close(ox.F.grad, x.F.grad, what="grad_in")
assert_close(ours.weight.grad, theirs.weight.grad, what="grad_weight")
assert_close(ours.bias.grad, theirs.bias.grad, what="grad_bias")
print("INORM_OK")
"""


@needs_ref
@pytest.mark.parametrize("host", ["python", "native"])
def test_reference_package_instance_norm_agrees(device, host):
    """the reference's own MinkowskiInstanceNorm, run by its unmodified Python package on this package's pooling and
    broadcast kernels, against the fused layer"""
    env = dict(os.environ, ME_AMD_HOST=host)
    out = subprocess.run([sys.executable, "-c", _REF.format(root=ROOT)], capture_output=True, text=True, timeout=900,
                         env=env)
    assert "INORM_OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
