"""GPU tests of MinkowskiChannelwiseConvolution (csrc/conv_channelwise.hip through the C ABI, both host layers and the
reference-shaped module): the reference-derived fixtures, a float64 torch restatement of the reference's formula
(MinkowskiChannelwiseConvolution.py:184-189) over cm.kernel_map, bitwise agreement of the hosts and of repeated runs,
bf16, float64 gradcheck, rows without neighbours, tight feature views, empty maps and one training step."""
import glob
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, make_cloud, row_mapping

pytestmark = pytest.mark.gpu
CW_CASES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "channelwise_*.npz")))
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)     # MinkowskiEngine/utils/gradcheck.py:37-39


def _close(a, b, rtol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.allclose(a, b, rtol=rtol, atol=rtol * scale), float(np.abs(a - b).max())


def _restate(x, kernel, bias, kmap, n_out):
    """the reference's forward (one gather, multiply and index_add per kernel offset) in torch, differentiable"""
    out = x.new_zeros((n_out, x.shape[1]))
    for k, pairs in kmap.items():
        i, o = pairs[0].long().to(x.device), pairs[1].long().to(x.device)
        out = out.index_add(0, o, x[i] * kernel[int(k)])
    if bias is not None:
        out = out + bias
    return out


def _pairs_of(kmap):
    return {int(k): sorted(map(tuple, v.cpu().numpy().T.tolist())) for k, v in kmap.items() if v.shape[1] > 0}


@pytest.mark.parametrize("path", CW_CASES, ids=[os.path.basename(p)[:-4] for p in CW_CASES])
def test_channelwise_vs_reference_fixture(device, host_layer, path):
    import minkowskiengine_amd as ME
    z = np.load(path)
    D = z["in_coords"].shape[1] - 1
    layer = ME.MinkowskiChannelwiseConvolution(z["feats"].shape[1], kernel_size=z["kernel_size"].tolist(),
                                               stride=z["stride"].tolist(), dilation=z["dilation"].tolist(), bias=True,
                                               dimension=D).to(device)
    with torch.no_grad():
        layer.kernel.copy_(torch.from_numpy(z["kernel"]))
        layer.bias.copy_(torch.from_numpy(z["bias"]))
    x = ME.SparseTensor(torch.from_numpy(z["feats"]).to(device), torch.from_numpy(z["in_coords"]).to(device),
                        requires_grad=True)
    y = layer(x)
    m = row_mapping(y.C.cpu().numpy(), z["out_coords"])           # our row i == fixture row m[i]
    # the kernel map is the reference's: same (in, out) pairs per offset once the output rows are relabelled
    km = x.coordinate_manager.kernel_map(x.coordinate_map_key, y.coordinate_map_key, z["stride"].tolist(),
                                         z["kernel_size"].tolist(), z["dilation"].tolist())
    ours = {k: sorted((i, int(m[o])) for i, o in v) for k, v in _pairs_of(km).items()}
    offs = np.concatenate([[0], np.cumsum(z["kmap_n"])])
    theirs = {int(k): sorted(map(tuple, z["kmap_pairs"][:, offs[j]:offs[j + 1]].T.tolist()))
              for j, k in enumerate(z["kmap_k"])}
    assert ours == theirs
    _close(y.F.detach().cpu().numpy(), z["out"][m])
    y.F.backward(torch.from_numpy(z["grad_out"][m]).to(device))
    _close(x.F.grad.cpu().numpy(), z["grad_in"])
    _close(layer.kernel.grad.cpu().numpy(), z["grad_kernel"])
    _close(layer.bias.grad.cpu().numpy(), z["grad_bias"])


MATRIX = [  # (D, kernel size, stride, dilation, region, C, bias, need dx)
    (3, 3, 1, 1, "cube", 64, True, True),
    (3, 3, 2, 1, "cube", 16, False, True),
    (3, 2, 2, 1, "cube", 8, True, True),
    (3, 5, 1, 1, "cube", 3, True, True),        # volume 125: four k-groups, one-channel pieces
    (3, 5, 1, 1, "cube", 96, False, False),     # volume 125, 4-channel pieces, no dx
    (3, 5, 2, 2, "cube", 96, True, True),       # volume 125: dx by the separate pass
    (3, 1, 1, 1, "cube", 17, True, True),
    (3, 1, 2, 1, "cube", 5, True, False),
    (3, 3, 1, 2, "cube", 256, True, True),
    (3, 3, 1, 1, "cube", 257, True, True),      # more than 256 pieces per row
    (2, 3, 1, 1, "cube", 1, True, True),
    (2, 5, 2, 2, "cube", 5, True, True),
    (2, 2, 1, 1, "cube", 256, False, True),
    (4, 3, 1, 1, "cube", 17, True, True),       # volume 81: three k-groups
    (4, 3, 2, 1, "cube", 8, True, False),
    (4, 2, 1, 1, "cube", 64, False, True),
    (4, 3, 1, 2, "cube", 96, True, True),
    (3, 3, 1, 1, "cross", 8, True, True),
    (3, 5, 1, 2, "cross", 96, True, True),
    (2, 3, 2, 1, "cross", 256, False, False),
    (4, 5, 1, 1, "cross", 5, True, True),
]


def _layer(ME, D, ks, st, dl, region, C, bias, device, dtype=torch.float32):
    kg = ME.KernelGenerator(kernel_size=ks, stride=st, dilation=dl, dimension=D,
                            region_type=ME.RegionType.HYPER_CROSS if region == "cross" else ME.RegionType.HYPER_CUBE)
    layer = ME.MinkowskiChannelwiseConvolution(C, bias=bias, kernel_generator=kg, dimension=D).to(device)
    with torch.no_grad():
        if bias:
            layer.bias.uniform_(-0.5, 0.5)
    return layer.to(dtype) if dtype == torch.float64 else layer


@pytest.mark.parametrize("D,ks,st,dl,region,C,bias,need_dx", MATRIX,
                         ids=[f"{d}d_k{k}s{s}d{l}_{r}_c{c}{'_b' if b else ''}{'' if n else '_nodx'}"
                              for d, k, s, l, r, c, b, n in MATRIX])
def test_channelwise_vs_restatement(device, host_layer, D, ks, st, dl, region, C, bias, need_dx):
    import minkowskiengine_amd as ME
    n = {2: 500, 3: 600, 4: 400}[D]
    coords = make_cloud(n, {2: 30, 3: 11, 4: 6}[D], D, seed=C + 7 * ks, batch=2)
    g = torch.Generator().manual_seed(C)
    feats = torch.rand(coords.shape[0], C, generator=g) - 0.5
    layer = _layer(ME, D, ks, st, dl, region, C, bias, device)
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=need_dx)
    y = layer(x)
    gy = torch.rand(y.F.shape, generator=g) - 0.5
    y.F.backward(gy.to(device))
    cm = x.coordinate_manager
    rt = layer.kernel_generator.region_type
    km = cm.kernel_map(x.coordinate_map_key, y.coordinate_map_key, st, ks, dl, region_type=rt)
    x64 = feats.double().to(device).requires_grad_(True)
    w64 = layer.kernel.detach().double().requires_grad_(True)
    b64 = layer.bias.detach().double().requires_grad_(True) if bias else None
    ref = _restate(x64, w64, b64, km, y.F.shape[0])
    ref.backward(gy.double().to(device))
    _close(y.F.detach().cpu(), ref.detach().cpu())
    _close(layer.kernel.grad.cpu(), w64.grad.cpu())
    if bias:
        _close(layer.bias.grad.cpu(), b64.grad.cpu())
    if need_dx:
        _close(x.F.grad.cpu(), x64.grad.cpu())
    else:
        assert x.F.grad is None


def _run(host, coords, feats, kernel, bias, gy, ks, st, device):
    import minkowskiengine_amd as ME
    prev = ME.get_host()
    ME.set_host(host)
    try:
        layer = ME.MinkowskiChannelwiseConvolution(feats.shape[1], kernel_size=ks, stride=st, bias=True,
                                                   dimension=coords.shape[1] - 1).to(device)
        with torch.no_grad():
            layer.kernel.copy_(kernel)
            layer.bias.copy_(bias)
        x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
        y = layer(x)
        y.F.backward(gy.to(device, y.F.dtype))
        return [t.detach().cpu().clone() for t in (y.F, x.F.grad, layer.kernel.grad, layer.bias.grad)]
    finally:
        ME.set_host(prev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ks,st", [(64, 3, 1), (17, 3, 2), (96, 5, 1)])
def test_channelwise_hosts_and_runs_bitwise_equal(device, dtype, C, ks, st):
    from minkowskiengine_amd import host
    if host.native_module() is None:
        pytest.fail(f"native host layer not available: {host.native_error()}")
    coords = make_cloud(20000, 40, 3, seed=3, batch=2)
    g = torch.Generator().manual_seed(5)
    feats = (torch.rand(coords.shape[0], C, generator=g) - 0.5).to(dtype)
    volume = ks ** 3
    kernel = torch.rand(volume, C, generator=g) - 0.5
    bias = torch.rand(1, C, generator=g) - 0.5
    n_out = coords.shape[0] if st == 1 else None
    if n_out is None:
        import minkowskiengine_amd as ME
        x = ME.SparseTensor(feats.float().to(device), coords.to(device))
        n_out = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, stride=st, dimension=3).to(device)(x).F.shape[0]
    gy = torch.rand(n_out, C, generator=g) - 0.5
    a = _run("python", coords, feats, kernel, bias, gy, ks, st, device)
    b = _run("native", coords, feats, kernel, bias, gy, ks, st, device)
    c = _run("native", coords, feats, kernel, bias, gy, ks, st, device)
    for name, u, v, w in zip(("out", "grad_in", "grad_kernel", "grad_bias"), a, b, c):
        assert torch.equal(u, v), f"{name}: the Python and the native host differ"
        assert torch.equal(v, w), f"{name}: two runs differ"


# (kernel size 2: volume 8, one k-group of 4-channel pieces — the fused bf16 backward with dx)
@pytest.mark.parametrize("C,ks", [(8, 3), (17, 3), (64, 3), (64, 2)], ids=["8", "17", "64", "64-k2"])
def test_channelwise_bf16(device, host_layer, C, ks):
    import minkowskiengine_amd as ME
    coords = make_cloud(3000, 16, 3, seed=11, batch=2)
    g = torch.Generator().manual_seed(C)
    feats = (torch.rand(coords.shape[0], C, generator=g) - 0.5).bfloat16()
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, bias=True, dimension=3).to(device)
    with torch.no_grad():
        layer.bias.uniform_(-0.5, 0.5)
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
    y = layer(x)
    assert y.F.dtype == torch.bfloat16
    gy = (torch.rand(y.F.shape, generator=g) - 0.5).bfloat16()
    y.F.backward(gy.to(device))
    assert layer.kernel.grad.dtype == torch.float32 and layer.bias.grad.dtype == torch.float32
    km = x.coordinate_manager.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 1, ks, 1)
    x64 = feats.double().to(device).requires_grad_(True)
    w64 = layer.kernel.detach().double().requires_grad_(True)
    b64 = layer.bias.detach().double().requires_grad_(True)
    ref = _restate(x64, w64, b64, km, y.F.shape[0])
    ref.backward(gy.double().to(device))
    # out: within one bf16 rounding (2^-8 relative) of the float64 result on the bf16 inputs
    r = ref.detach().cpu().numpy()
    o = y.F.detach().float().cpu().numpy()
    assert (np.abs(o - r) <= np.abs(r) * 2.0 ** -8 + 1e-6).all()
    _close(layer.kernel.grad.cpu(), w64.grad.cpu(), rtol=1e-5)
    _close(layer.bias.grad.cpu(), b64.grad.cpu(), rtol=1e-5)
    gi = x.F.grad.float().cpu().numpy()
    rg = x64.grad.cpu().numpy()
    assert (np.abs(gi - rg) <= np.abs(rg) * 2.0 ** -8 + 1e-6).all()


def test_channelwise_f64_gradcheck(device, host_layer):
    import minkowskiengine_amd as ME
    from torch.autograd import gradcheck
    coords = make_cloud(60, 5, 3, seed=2, batch=2)
    layer = ME.MinkowskiChannelwiseConvolution(3, kernel_size=3, stride=2, bias=True, dimension=3).double().to(device)
    x = ME.SparseTensor(torch.rand(coords.shape[0], 3, dtype=torch.float64).to(device), coords.to(device))
    y = layer(x)
    assert y.F.dtype == torch.float64
    f = ME.MinkowskiChannelwiseConvolutionFunction
    feats = x.F.detach().clone().requires_grad_(True)
    kernel = layer.kernel.detach().clone().requires_grad_(True)
    bias = layer.bias.detach().clone().requires_grad_(True)
    assert gradcheck(lambda a, w, b: f.apply(a, w, b, layer.kernel_generator, x.coordinate_map_key,
                                             y.coordinate_map_key, x.coordinate_manager),
                     (feats, kernel, bias), **GC)


@pytest.mark.parametrize("bias", [True, False])
def test_channelwise_rows_without_neighbours(device, host_layer, bias):
    import minkowskiengine_amd as ME
    coords = make_cloud(800, 10, 3, seed=4, batch=2)
    far = coords.clone()
    far[:, 1:] += 1000                                # no input voxel within the kernel of these
    out_coords = torch.cat([coords[:300], far[300:]], 0)
    C = 24
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=3, bias=bias, dimension=3).to(device)
    x = ME.SparseTensor((torch.rand(coords.shape[0], C) - 0.5).to(device), coords.to(device))
    nan = torch.full((out_coords.shape[0], C), float("nan"), device=device)   # hands NaN memory to the allocator
    del nan
    y = layer(x, out_coords.to(device))
    assert torch.isfinite(y.F).all()
    yc = y.C.cpu()
    lonely = (yc[:, 1:] >= 900).all(1)
    assert int(lonely.sum()) == out_coords.shape[0] - 300
    want = layer.bias.detach().expand(int(lonely.sum()), C) if bias else torch.zeros(int(lonely.sum()), C,
                                                                                      device=device)
    assert torch.equal(y.F[lonely.to(device)], want)


@pytest.mark.parametrize("C", [3, 17, 8])      # (8: 4-channel pieces by c, one channel by the address)
def test_channelwise_tight_feature_view(device, host_layer, C):
    """features and output gradient are views that end exactly at the end of their storage"""
    import minkowskiengine_amd as ME
    coords = make_cloud(700, 10, 3, seed=6, batch=2)
    n = coords.shape[0]
    g = torch.Generator().manual_seed(C)
    base = torch.rand(n * C + 1, generator=g).to(device) - 0.5
    feats = base[1:].view(n, C)
    assert feats.data_ptr() + feats.numel() * 4 == base.data_ptr() + base.numel() * 4
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=3, bias=True, dimension=3).to(device)
    x = ME.SparseTensor(feats, coords.to(device))
    assert x.F.data_ptr() == feats.data_ptr()
    y = layer(x)
    gbase = torch.rand(y.F.shape[0] * C + 1, generator=g).to(device) - 0.5
    gy = gbase[1:].view(y.F.shape[0], C)
    y.F.backward(gy)
    km = x.coordinate_manager.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 1, 3, 1)
    x64 = feats.detach().double().requires_grad_(True)
    w64 = layer.kernel.detach().double().requires_grad_(True)
    b64 = layer.bias.detach().double().requires_grad_(True)
    ref = _restate(x64, w64, b64, km, y.F.shape[0])
    ref.backward(gy.double())
    _close(y.F.detach().cpu(), ref.detach().cpu())
    _close(layer.kernel.grad.cpu(), w64.grad.cpu())
    _close(layer.bias.grad.cpu(), b64.grad.cpu())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_channelwise_empty_map(device, host_layer, dtype):
    from minkowskiengine_amd import host
    B = host.backend()
    mgr = B.CoordinateMapManagerGPU_c10()
    key, _ = mgr.insert_and_map(torch.zeros((0, 4), dtype=torch.int32, device=device), [1, 1, 1], "e")
    out_key = B.CoordinateMapKey(4)
    C = 8
    wt = torch.float64 if dtype == torch.float64 else torch.float32
    feats = torch.zeros((0, C), dtype=dtype, device=device)
    kernel = torch.rand(27, C, dtype=wt, device=device)
    bias = torch.rand(C, dtype=wt, device=device)
    args = ([3, 3, 3], [1, 1, 1], [1, 1, 1], B.RegionType.HYPER_CUBE, torch.IntTensor())
    out = B.ChannelwiseConvolutionForwardGPU(feats, kernel, bias, *args, key, out_key, mgr)
    assert tuple(out.shape) == (0, C) and out.dtype == dtype
    gi, gw, gb = B.ChannelwiseConvolutionBackwardGPU(feats, out, kernel, *args, key, out_key, mgr)
    torch.cuda.synchronize()
    assert tuple(gi.shape) == (0, C)
    assert tuple(gw.shape) == (27, C) and not gw.any()
    assert tuple(gb.shape) == (C,) and not gb.any()


def test_channelwise_network_training_step(device, host_layer):
    """Conv -> Channelwise -> BN -> ReLU, one step: every parameter gradient equals that of the same network with the
    channelwise layer replaced by the torch restatement"""
    import minkowskiengine_amd as ME
    coords = make_cloud(3000, 16, 3, seed=8, batch=2)
    feats = torch.rand(coords.shape[0], 4) - 0.5
    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(4, 32, kernel_size=3, dimension=3).to(device)
    cw = ME.MinkowskiChannelwiseConvolution(32, kernel_size=3, stride=2, bias=True, dimension=3).to(device)
    bn = ME.MinkowskiBatchNorm(32).to(device)
    relu = ME.MinkowskiReLU()
    x = ME.SparseTensor(feats.to(device), coords.to(device))
    h = conv(x)
    y = relu(bn(cw(h)))
    loss = (y.F ** 2).mean()
    loss.backward()
    grads = {n: p.grad.detach().clone() for mod in (conv, cw, bn) for n, p in mod.named_parameters(prefix=str(id(mod)))}
    for mod in (conv, cw, bn):
        mod.zero_grad()
    # the same network with the channelwise layer restated in torch (fp32, on the same kernel map)
    h2 = conv(x)
    km = x.coordinate_manager.kernel_map(h2.coordinate_map_key, y.coordinate_map_key, 2, 3, 1)
    f = _restate(h2.F, cw.kernel, cw.bias, km, y.F.shape[0])
    y2 = relu(bn(ME.SparseTensor(f, coordinate_map_key=y.coordinate_map_key, coordinate_manager=x.coordinate_manager)))
    loss2 = (y2.F ** 2).mean()
    loss2.backward()
    assert torch.allclose(loss, loss2, rtol=1e-5, atol=1e-7)
    for mod in (conv, cw, bn):
        for n, p in mod.named_parameters(prefix=str(id(mod))):
            a, b = grads[n], p.grad
            assert torch.allclose(a, b, rtol=1e-4, atol=max(1e-5 * float(b.abs().max()), 1e-6)), n
