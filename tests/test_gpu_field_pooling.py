"""GPU tests of the origin maps of fields and of global pooling / broadcast over a TensorField (both host layers)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (0, 2, 5)


def _me():
    import minkowskiengine_amd as ME
    return ME


def _clouds(device, dtype=torch.float32, c=6, sizes=(37, 101, 60), seed=0, integer=False):
    """3 clouds of unequal size, batch indices {0, 2, 5}, rows interleaved"""
    g = torch.Generator().manual_seed(seed)
    b = torch.cat([torch.full((n,), float(bi)) for n, bi in zip(sizes, BATCHES)])
    n = len(b)
    if integer:        # distinct integer coordinates
        x = torch.stack([torch.arange(n) % 11, (torch.arange(n) // 11) % 11, torch.arange(n) // 121], 1).float()
    else:
        x = (torch.rand(n, 3, generator=g) - 0.5) * 20
    perm = torch.randperm(n, generator=g)
    coords = torch.cat([b[:, None], x], 1)[perm].contiguous()
    feats = (torch.rand(n, c, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    return coords.to(device), feats.to(device)


def _per_cloud(coords, feats, fn):
    b = coords[:, 0].cpu().numpy().round().astype(np.int64)
    f = feats.detach().double().cpu().numpy()
    return np.stack([fn(f[b == bi]) for bi in BATCHES]), b


def test_origin_field_on_a_field_only_manager(host_layer, device):
    ME = _me()
    coords, feats = _clouds(device)
    tf = ME.TensorField(feats, coordinates=coords)
    mgr = tf.coordinate_manager
    okey = mgr.origin_field()
    assert okey.get_key() == ([0, 0, 0], "")
    oc = mgr.get_coordinates(okey)
    assert oc.cpu().tolist() == [[b, 0, 0, 0] for b in BATCHES]
    assert mgr.origin() == okey
    m = mgr.origin_field_map(tf.coordinate_field_map_key)
    assert list(m.keys()) == [0]
    t = m[0]
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, len(feats))
    assert torch.equal(t[0].cpu(), torch.arange(len(feats), dtype=torch.int32))
    b = coords[:, 0].cpu().numpy().round().astype(np.int64)
    assert np.array_equal(t[1].cpu().numpy(), np.searchsorted(np.array(BATCHES), b))
    rows = tf._batchwise_row_indices
    assert [r.cpu().tolist() for r in rows] == [np.nonzero(b == bi)[0].tolist() for bi in BATCHES]
    assert [len(x) for x in tf.decomposed_features] == [37, 101, 60]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_global_pooling_of_a_field(dtype, host_layer, device):
    ME = _me()
    coords, feats = _clouds(device, dtype=dtype)
    feats.requires_grad_(True)
    tf = ME.TensorField(feats, coordinates=coords)
    # max: bit-equal, gradient on the argmax row
    y = ME.MinkowskiGlobalMaxPooling()(tf)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key.get_key() == ([0, 0, 0], "")
    want, b = _per_cloud(coords, feats, lambda v: v.max(0))
    assert np.array_equal(y.F.detach().double().cpu().numpy(), want)
    gy = torch.rand(y.F.shape, device=device).to(dtype)
    (g,) = torch.autograd.grad(y.F, feats, gy)
    f = feats.detach().double().cpu().numpy()
    wg = np.zeros_like(f)
    for k, bi in enumerate(BATCHES):
        rows = np.nonzero(b == bi)[0]
        wg[rows[f[rows].argmax(0)], np.arange(f.shape[1])] = gy[k].double().cpu().numpy()
    assert np.array_equal(g.double().cpu().numpy(), wg)
    # sum / avg: 1e-4 in fp32 (the project's feature tolerance), the bf16 tolerance of tests/test_gpu_pooling.py
    tol = dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=0.05, rtol=0.02)
    for mod, fn in ((ME.MinkowskiGlobalSumPooling(), lambda v: v.sum(0)), (ME.MinkowskiGlobalAvgPooling(), lambda v: v.mean(0)),
                    (ME.MinkowskiGlobalPooling(), lambda v: v.mean(0))):
        y = mod(tf)
        want, _ = _per_cloud(coords, feats, fn)
        np.testing.assert_allclose(y.F.detach().double().cpu().numpy(), want, **tol)
        (g,) = torch.autograd.grad(y.F, feats, torch.ones_like(y.F))
        cnt = np.array([(b == bi).sum() for bi in BATCHES], np.float64)
        wg = np.ones_like(f) if isinstance(mod, ME.MinkowskiGlobalSumPooling) else \
            (1.0 / cnt)[np.searchsorted(np.array(BATCHES), b)][:, None] * np.ones_like(f)
        np.testing.assert_allclose(g.double().cpu().numpy(), wg, **tol)


def test_global_pooling_of_a_field_gradcheck(host_layer, device):
    ME = _me()
    coords, feats = _clouds(device, dtype=torch.float64, c=3, sizes=(5, 9, 7))
    feats.requires_grad_(True)
    for mod in (ME.MinkowskiGlobalMaxPooling(), ME.MinkowskiGlobalSumPooling(), ME.MinkowskiGlobalAvgPooling()):
        fn = lambda x: mod(ME.TensorField(x, coordinates=coords)).F   # noqa: E731
        assert torch.autograd.gradcheck(fn, (feats,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_field_equals_sparse_tensor_on_distinct_integer_points(host_layer, device):
    """global pooling of SparseTensors is pinned against the reference by tests/test_gpu_pooling.py"""
    ME = _me()
    coords, feats = _clouds(device, integer=True)
    tf = ME.TensorField(feats, coordinates=coords)
    st = ME.SparseTensor(feats, coordinates=coords.int())
    assert torch.equal(st.C, coords.int())                 # same rows in the same order
    for mod in (ME.MinkowskiGlobalMaxPooling(), ME.MinkowskiGlobalSumPooling(), ME.MinkowskiGlobalAvgPooling()):
        a, b = mod(tf), mod(st)
        assert torch.equal(a.C, b.C)
        assert torch.equal(a.F, b.F)


def test_broadcast_onto_a_field(host_layer, device):
    ME = _me()
    from minkowskiengine_amd.broadcast import MinkowskiBroadcastFunction
    coords, feats = _clouds(device)
    feats.requires_grad_(True)
    tf = ME.TensorField(feats, coordinates=coords)
    glob = ME.MinkowskiGlobalAvgPooling()(tf)
    gf = glob.F.detach().clone().requires_grad_(True)
    row = np.searchsorted(np.array(BATCHES), coords[:, 0].cpu().numpy().round().astype(np.int64))
    f, gl = feats.detach().double().cpu().numpy(), gf.detach().double().cpu().numpy()
    for op, fw in ((ME.BroadcastMode.ELEMENTWISE_ADDITON, lambda: f + gl[row]),
                   (ME.BroadcastMode.ELEMENTWISE_MULTIPLICATION, lambda: f * gl[row])):
        out = MinkowskiBroadcastFunction.apply(feats, gf, op, tf.coordinate_field_map_key, glob.coordinate_map_key,
                                               tf.coordinate_manager)
        np.testing.assert_allclose(out.detach().double().cpu().numpy(), fw(), atol=1e-6, rtol=1e-6)
        go = torch.rand_like(out)
        g_in, g_glob = torch.autograd.grad(out, (feats, gf), go)
        gon = go.double().cpu().numpy()
        mult = op == ME.BroadcastMode.ELEMENTWISE_MULTIPLICATION
        np.testing.assert_allclose(g_in.double().cpu().numpy(), gon * gl[row] if mult else gon, atol=1e-6, rtol=1e-6)
        wgg = np.zeros_like(gl)
        np.add.at(wgg, row, gon * f if mult else gon)
        np.testing.assert_allclose(g_glob.double().cpu().numpy(), wgg, atol=1e-4, rtol=1e-4)


def test_field_with_a_batch_index_outside_the_origin_map(host_layer, device):
    ME = _me()
    coords, feats = _clouds(device, integer=True)
    st = ME.SparseTensor(feats, coordinates=coords.int())
    ME.MinkowskiGlobalSumPooling()(st)                       # the origin map now holds {0, 2, 5}
    other = coords[:-3].clone()          # (a row count of its own: the field key equals the sparse key ([1, 1, 1], ""))
    other[0, 0] = 7.0
    tf = ME.TensorField(feats[:-3], coordinates=other, coordinate_manager=st.coordinate_manager)
    with pytest.raises(RuntimeError, match="does not contain every batch index"):
        ME.MinkowskiGlobalMaxPooling()(tf)


_REF_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import MinkowskiEngineBackend._C as C
from oracle import ref
RME = ref.import_reference_package(backend=C)
import torch
import minkowskiengine_amd as ME
g = torch.Generator().manual_seed(0)
n = 300
coords = torch.cat([torch.tensor([0.0, 2.0, 5.0])[torch.randint(0, 3, (n, 1), generator=g)],
                    (torch.rand(n, 3, generator=g) - 0.5) * 10], 1).cuda()
feats = torch.rand(n, 5, generator=g).cuda()
a = RME.MinkowskiGlobalMaxPooling()(RME.TensorField(feats, coordinates=coords))
b = ME.MinkowskiGlobalMaxPooling()(ME.TensorField(feats, coordinates=coords))
assert isinstance(a, RME.SparseTensor)
assert torch.equal(a.F, b.F), (a.F, b.F)
assert torch.equal(a.C, b.C), (a.C, b.C)
print("REF-FIELD-POOL-OK")
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref.reference_root(), "MinkowskiEngine")),
                    reason="needs the reference package (its source tree or the staged copy)")
def test_reference_package_pools_a_field_over_this_backend(device):
    r = subprocess.run([sys.executable, "-c", _REF_SCRIPT.format(root=ROOT)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "REF-FIELD-POOL-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_pointnet_example(device):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import pointnet
    finally:
        sys.path.pop(0)
    loss = pointnet.main(["--points", "256", "--batch", "3"])
    assert math.isfinite(loss)
