"""GPU tests of TensorField (csrc/field.hip through both host layers): sparse() against the existing quantisation path,
slice / cat_slice, strided inverse mappings, spmm, float64 gradcheck, determinism across runs and hosts, bf16, channel
counts, views, empty fields and a per-point training step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)
SQM = None


def _me():
    import minkowskiengine_amd as ME
    return ME


def _points(n=3000, D=3, extent=12.0, batch=2, seed=0, dtype=torch.float32, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, batch, (n, 1), generator=g).double()
    x = (torch.rand(n, D, generator=g, dtype=torch.float64) - 0.5) * 2 * extent
    x[: n // 10] = torch.round(x[: n // 10])            # points exactly on voxel boundaries
    return torch.cat([b, x], 1).to(dtype).to(dev)


def test_sparse_matches_existing_quantisation(host_layer, device):
    ME = _me()
    c = _points(dev=device)
    f = torch.rand(c.shape[0], 7, device=device)
    for mode in (ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE, ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM,
                 ME.SparseTensorQuantizationMode.RANDOM_SUBSAMPLE):
        tf = ME.TensorField(f, coordinates=c, quantization_mode=mode)
        s = tf.sparse()
        ref = ME.SparseTensor(f, coordinates=c.floor().int(), quantization_mode=mode)
        assert torch.equal(s.C, ref.C)
        assert torch.equal(tf.inverse_mapping(s.coordinate_map_key), ref.inverse_mapping)
        torch.testing.assert_close(s.F, ref.F, rtol=1e-6, atol=1e-6)


def test_sparse_average_gradient_float64(host_layer, device):
    ME = _me()
    c = _points(n=500, dtype=torch.float64, dev=device)
    f = torch.rand(c.shape[0], 3, device=device, dtype=torch.float64, requires_grad=True)
    tf = ME.TensorField(f, coordinates=c)
    s = tf.sparse()
    inv = tf.inverse_mapping(s.coordinate_map_key).long()
    n = s.F.shape[0]
    cnt = torch.zeros(n, dtype=torch.float64, device=device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float64))
    ref = torch.zeros(n, 3, dtype=torch.float64, device=device).index_add(0, inv, f) / cnt[:, None]
    torch.testing.assert_close(s.F, ref)
    gy = torch.rand_like(ref)
    (g,) = torch.autograd.grad(s.F, f, gy)
    (gr,) = torch.autograd.grad(ref, f, gy)
    torch.testing.assert_close(g, gr)


def test_slice_and_cat_slice(host_layer, device):
    ME = _me()
    c = _points(dev=device)
    f = torch.rand(c.shape[0], 5, device=device)
    tf = ME.TensorField(f, coordinates=c)
    s = tf.sparse()
    y = s * 2.0
    out = y.slice(tf)
    assert isinstance(out, ME.TensorField) and out.F.shape == (c.shape[0], 5)
    inv = tf.inverse_mapping(s.coordinate_map_key).long()
    assert torch.equal(out.F, y.F[inv])
    cs = y.cat_slice(tf)
    assert torch.equal(cs.F, torch.cat([y.F[inv], f], 1))
    # a strided key resolves through stride_map
    pool = ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3)
    z = pool(s)
    o2 = z.slice(tf)
    _, smap = tf.coordinate_manager.stride_map(s.coordinate_map_key, z.coordinate_map_key)
    assert torch.equal(o2.F, z.F[smap[inv]])
    # slicing by a SparseTensor X
    st = ME.SparseTensor(f, coordinates=c.floor().int(), quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE)
    o3 = st.slice(st)
    assert torch.equal(o3.F, st.F[st.inverse_mapping])
    o4 = (st * 2.0).cat_slice(st)                          # one row per point: sliced features, then X's own
    assert torch.equal(o4.F, torch.cat([st.F[st.inverse_mapping] * 2.0, st.F[st.inverse_mapping]], 1))


def test_gradcheck_sparse_slice_spmm(host_layer, device):
    ME = _me()
    c = _points(n=60, extent=2.0, dtype=torch.float64, dev=device)
    f = torch.rand(c.shape[0], 2, device=device, dtype=torch.float64, requires_grad=True)

    def through(ff):
        tf = ME.TensorField(ff, coordinates=c)
        s = tf.sparse()
        return (s * 3.0).slice(tf).F

    assert torch.autograd.gradcheck(through, (f,), **GC)
    rows = torch.tensor([0, 2, 2, 1, 0, 2], dtype=torch.int32, device=device)
    cols = torch.tensor([1, 0, 3, 3, 2, 1], dtype=torch.int32, device=device)
    vals = torch.rand(6, dtype=torch.float64, device=device)
    mat = torch.rand(4, 3, dtype=torch.float64, device=device, requires_grad=True)
    size = torch.Size([3, 4])
    assert torch.autograd.gradcheck(lambda m: ME.MinkowskiSPMMFunction.apply(rows, cols, vals, size, m), (mat,), **GC)
    assert torch.autograd.gradcheck(lambda m: ME.MinkowskiSPMMAverageFunction.apply(rows, cols, size, m), (mat,), **GC)
    dense = torch.zeros(3, 4, dtype=torch.float64, device=device).index_put_((rows.long(), cols.long()), vals,
                                                                              accumulate=True)
    torch.testing.assert_close(ME.spmm(rows, cols, vals, size, mat.detach()), dense @ mat.detach())


def _run(ME, c, f, gy):
    ff = f.clone().requires_grad_(True)
    tf = ME.TensorField(ff, coordinates=c)
    s = tf.sparse()
    out = s.slice(tf).F * 1.5 + s.features_at_coordinates(c + 0.3)
    (g,) = torch.autograd.grad(out, ff, gy)
    return out.detach(), g


def test_deterministic_across_runs_and_hosts(device):
    ME = _me()
    c = _points(n=20000, extent=6.0, dev=device)
    f = torch.rand(c.shape[0], 20, device=device)
    gy = torch.rand(c.shape[0], 20, device=device)
    res = []
    for host in ("python", "native", "native"):
        prev = ME.get_host()
        ME.set_host(host)
        try:
            res.append(_run(ME, c, f, gy))
        finally:
            ME.set_host(prev)
    for o, g in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(g, res[0][1])


@pytest.mark.parametrize("C", [1, 3, 20, 96, 130])
def test_channels_bf16_views(host_layer, device, C):
    ME = _me()
    c = _points(n=2000, dev=device)
    wide = torch.rand(c.shape[0], C + 3, device=device)
    f = wide[:, 1:C + 1]                                   # a non-contiguous view
    tf = ME.TensorField(f, coordinates=c)
    s = tf.sparse()
    inv = tf.inverse_mapping(s.coordinate_map_key).long()
    n = s.F.shape[0]
    cnt = torch.zeros(n, device=device).index_add_(0, inv, torch.ones(inv.numel(), device=device))
    ref = torch.zeros(n, C, device=device).index_add(0, inv, f) / cnt[:, None]
    torch.testing.assert_close(s.F, ref, rtol=1e-5, atol=1e-6)
    tb = ME.TensorField(f.bfloat16(), coordinates=c)
    sb = tb.sparse()
    assert sb.F.dtype == torch.bfloat16
    torch.testing.assert_close(sb.F.float(), ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(sb.slice(tb).F.float(), ref[inv], rtol=2e-2, atol=2e-2)


def test_empty_field(host_layer, device):
    ME = _me()
    c = torch.empty(0, 4, device=device)
    f = torch.empty(0, 4, device=device)
    tf = ME.TensorField(f, coordinates=c)
    s = tf.sparse()
    assert s.F.shape == (0, 4)
    assert s.slice(tf).F.shape == (0, 4)


def test_max_pool_raises(device):
    ME = _me()
    c = _points(n=10, dev=device)
    tf = ME.TensorField(torch.rand(10, 2, device=device), coordinates=c,
                        quantization_mode=ME.SparseTensorQuantizationMode.MAX_POOL)
    with pytest.raises(NotImplementedError, match="MinkowskiDirectMaxPoolingFunction"):
        tf.sparse()


class _Net(torch.nn.Module):
    """field: Linear + BatchNorm + ReLU -> sparse() -> stride-2 and stride-4 convolutions -> slices of both levels back
    onto the field -> ME.cat -> sparse() -> slice -> per-point classifier (classification_modelnet40.py:189-215)"""

    def __init__(self, ME, cin, classes):
        super().__init__()
        self.lin = ME.MinkowskiLinear(cin, 8)
        self.bn = ME.MinkowskiBatchNorm(8)
        self.relu = ME.MinkowskiReLU()
        self.down2 = ME.MinkowskiConvolution(8, 16, kernel_size=2, stride=2, dimension=3)
        self.down4 = ME.MinkowskiConvolution(16, 16, kernel_size=2, stride=2, dimension=3)
        self.head = torch.nn.Linear(32, classes)

    def forward(self, ME, tf):
        x = self.relu(self.bn(self.lin(tf)))
        s = x.sparse()
        d2 = self.down2(s)
        d4 = self.down4(d2)
        cat = ME.cat(d2.slice(x), d4.slice(x))
        s2 = cat.sparse()
        self.maps = (x, s, d2, d4, cat, s2)
        return self.head(s2.slice(cat).F)


def _restate(net, f, maps):
    """the network in float64 torch on the maps the forward built"""
    x, s, d2, d4, cat, s2 = maps
    cm = x.coordinate_manager
    P = {n: p.detach().double().requires_grad_(True) for n, p in net.named_parameters()}

    def avg(h, inv, n):
        cnt = torch.zeros(n, dtype=torch.float64, device=h.device).index_add_(0, inv, torch.ones_like(inv, dtype=h.dtype))
        return torch.zeros(n, h.shape[1], dtype=h.dtype, device=h.device).index_add(0, inv, h) / cnt[:, None]

    def conv(h, w, a, b, n):
        km = cm.kernel_map(a.coordinate_map_key, b.coordinate_map_key, stride=2, kernel_size=2)
        out = torch.zeros(n, w.shape[2], dtype=h.dtype, device=h.device)
        for k, pairs in km.items():
            i, o = pairs[0].long(), pairs[1].long()
            out = out.index_add(0, o, h[i] @ w[int(k)])
        return out

    h = f.double() @ P["lin.linear.weight"].t() + P["lin.linear.bias"]
    mu, var = h.mean(0), h.var(0, unbiased=False)
    h = torch.relu((h - mu) / torch.sqrt(var + net.bn.bn.eps) * P["bn.bn.weight"] + P["bn.bn.bias"])
    inv1 = x.inverse_mapping(s.coordinate_map_key).long()
    h1 = avg(h, inv1, len(s))
    h2 = conv(h1, P["down2.kernel"], s, d2, len(d2))
    h4 = conv(h2, P["down4.kernel"], d2, d4, len(d4))
    hc = torch.cat([h2[x.inverse_mapping(d2.coordinate_map_key).long()],
                    h4[x.inverse_mapping(d4.coordinate_map_key).long()]], 1)
    inv2 = cat.inverse_mapping(s2.coordinate_map_key).long()
    out = avg(hc, inv2, len(s2))[inv2] @ P["head.weight"].t() + P["head.bias"]
    return out, P


def test_training_step_gradients_and_loss(host_layer, device):
    ME = _me()
    torch.manual_seed(0)
    c = _points(n=4000, extent=8.0, dev=device)
    f = torch.rand(c.shape[0], 4, device=device)
    labels = (c[:, 1] > 0).long()
    net = _Net(ME, 4, 2).to(device)
    # every parameter gradient of one step against the float64 restatement on the same maps
    tf = ME.TensorField(f, coordinates=c)
    loss = torch.nn.functional.cross_entropy(net(ME, tf), labels)
    loss.backward()
    out64, P = _restate(net, f, net.maps)
    loss64 = torch.nn.functional.cross_entropy(out64, labels)
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item()) + 1e-5
    for name, p in net.named_parameters():
        g64 = P[name].grad
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.double(), g64, rtol=2e-3, atol=2e-3 * float(g64.abs().max()) + 1e-7,
                                   msg=lambda m: f"{name}: {m}")
    # the loss falls over a few SGD steps
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        tf = ME.TensorField(f, coordinates=c)
        loss = torch.nn.functional.cross_entropy(net(ME, tf), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
