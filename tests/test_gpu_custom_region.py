"""RegionType.CUSTOM on the GPU, on both host layers: kernel maps against numpy (exact pair sets per offset), equivalence
with the built-in regions, the cache key, convolution / pooling / channel-wise operators and the generative layer
against the oracle's feature arithmetic on the numpy-built map, recipe replay and the geometry shortcuts.

Tap k of a CUSTOM layer looks up u + offsets[k] * dilation * tensor_stride, so the expected pairs of tap k are
O.find(in_coords, out_coords + offsets[k] * step).  Tolerances are those the existing tests apply to the same dtype
against the same oracle functions: helpers.assert_close at its default 1e-4 + 1e-4 |want| for fp32
(tests/test_gpu_conv.py:92-95) and, for bf16 features, assert_bf16_close for outputs and input gradients with
assert_close for the fp32 weight gradient (tests/test_gpu_bf16.py:37-42 and :99-103)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import me_oracle as O
from helpers import assert_close, make_cloud
from test_gpu_bf16 import assert_bf16_close, bf16_round

pytestmark = pytest.mark.gpu

SHIFT = [[2, 0, -1]]
# asymmetric, reach +-5 on every axis, no origin
SEVEN = [[5, 0, 0], [-5, 1, 0], [0, 2, -1], [1, 1, 1], [0, -5, 0], [2, 0, 5], [-1, -1, -5]]
SEVEN_B = [[-v for v in row] for row in SEVEN]
FIVE = [[0, 0, 0], [1, 0, 0], [0, 1, 1], [-1, 2, 0], [3, -1, -2]]
CUBE2 = [[x, y, z] for z, y, x in itertools.product((0, 1), repeat=3)]                 # axis 0 fastest
CUBE3 = [[x, y, z] for z, y, x in itertools.product((-1, 0, 1), repeat=3)]
CROSS3 = [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]


def hybrid29():
    import minkowskiengine_amd as ME
    cube, cross = ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS
    return ME.hybrid_region_offsets([cube, cube, cube, cross], 3, 4).tolist()


def expected_kmap(in_c, out_c, offsets, step=1):
    """{k: int32 [2, n_k]} from the oracle's find: tap k pairs out row u with the in row at out_c[u] + offsets[k] * step"""
    km = {}
    step = np.broadcast_to(np.asarray(step, np.int64), (in_c.shape[1] - 1,))
    for k, off in enumerate(np.asarray(offsets, np.int64)):
        q = np.asarray(out_c, np.int64).copy()
        q[:, 1:] += off * step
        rows = O.find(in_c, q.astype(np.int32))
        outs = np.nonzero(rows >= 0)[0]
        if outs.size:
            km[k] = np.stack((rows[outs], outs)).astype(np.int32)
    return km


def transposed(km):
    return {k: np.stack((v[1], v[0])) for k, v in km.items()}


def generator(ME, offsets, D=3, **kw):
    return ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=D, **kw)


def cloud(name):
    return {"one": lambda: make_cloud(1, 4, 3, seed=3, negative=True),
            "130": lambda: make_cloud(130, 7, 3, seed=4, negative=True),
            "3000": lambda: make_cloud(3000, 14, 3, seed=5, batch=2, negative=True),
            "4d": lambda: make_cloud(3000, 8, 4, seed=6, batch=2, negative=True)}[name]()


def n_kernel_maps(cm):
    return repr(cm._manager).count("gpu_kernel_map")        # one line per entry of the kernel-map cache, either host


# ---- 1. kernel map vs numpy / oracle ---------------------------------------------------------------------------------------
KMAP_CASES = [(c, o) for c in ("one", "130", "3000") for o in ("shift", "seven")] + [("4d", "hybrid")]


@pytest.mark.parametrize("ts", [1, 2])
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("cloud_name,offs_name", KMAP_CASES, ids=[f"{c}-{o}" for c, o in KMAP_CASES])
def test_kernel_map_matches_numpy(device, host_layer, cloud_name, offs_name, dil, ts):
    import minkowskiengine_amd as ME
    offsets = {"shift": SHIFT, "seven": SEVEN, "hybrid": hybrid29()}[offs_name]
    coords = cloud(cloud_name)
    D = coords.shape[1] - 1
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=device), coords.to(device))
    cm, key = x.coordinate_manager, x.coordinate_map_key
    if ts == 2:                                       # the strided map of the same cloud: steps are offset * dil * 2
        key = cm.stride(key, 2)
    map_c = cm.get_coordinates(key).cpu().numpy()
    # (offsets may live on the GPU and have any integer dtype)
    offs_t = (torch.tensor(offsets, dtype=torch.int64, device=device) if dil == 2
              else torch.tensor(offsets, dtype=torch.int32))
    got = cm.kernel_map(key, key, stride=1, kernel_size=-1, dilation=dil, region_type=ME.RegionType.CUSTOM,
                        region_offset=offs_t)
    want = expected_kmap(map_c, map_c, offsets, dil * ts)
    O.assert_same_kernel_map(got, want)
    if cloud_name in ("3000", "4d"):                                  # (the case is not vacuous)
        assert sum(v.shape[1] for v in want.values()) > (1000 if dil * ts == 1 else 0)
    # pairs of every tap come sorted by out row, as for the built-in regions
    for k, v in got.items():
        assert bool((v[1][1:] > v[1][:-1]).all()), k


# ---- 2. equivalence with the built-in regions --------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets,builtin,ks,stride", [(CUBE3, "HYPER_CUBE", 3, 1), (CROSS3, "HYPER_CROSS", 3, 1),
                                                       (CUBE2, "HYPER_CUBE", 2, 2)], ids=["cube3", "cross3", "cube2s2"])
def test_custom_lists_of_the_builtin_regions_give_their_maps(device, host_layer, offsets, builtin, ks, stride):
    import minkowskiengine_amd as ME
    coords = cloud("3000")
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=device), coords.to(device))
    cm, key = x.coordinate_manager, x.coordinate_map_key
    okey = cm.stride(key, stride) if stride > 1 else key             # fine -> coarse
    want = cm.kernel_map(key, okey, stride=stride, kernel_size=ks, region_type=getattr(ME.RegionType, builtin))
    got = cm.kernel_map(key, okey, stride=stride, kernel_size=-1, region_type=ME.RegionType.CUSTOM,
                        region_offset=torch.tensor(offsets))
    assert len(want) == len(offsets)
    O.assert_same_kernel_map(got, want)


# ---- 3. two lists, one pair of maps ----------------------------------------------------------------------------------------
def _conv(ME, cin, cout, offsets, device, D=3, bias=False, transpose=False, seed=0, **kw):
    cls = ME.MinkowskiConvolutionTranspose if transpose else ME.MinkowskiConvolution
    conv = cls(cin, cout, bias=bias, kernel_generator=generator(ME, offsets, D, **kw), dimension=D)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        conv.kernel.copy_(torch.rand(conv.kernel.shape, generator=g) - 0.5)
        if bias:
            conv.bias.copy_(torch.rand(conv.bias.shape, generator=g) - 0.5)
    return conv.to(device)


def test_two_offset_lists_on_the_same_maps_do_not_share_a_kernel_map(device, host_layer):
    import minkowskiengine_amd as ME
    coords = cloud("3000")
    feats = torch.rand(coords.shape[0], 3, generator=torch.Generator().manual_seed(1))
    x = ME.SparseTensor(feats.to(device), coords.to(device))
    before = n_kernel_maps(x.coordinate_manager)
    for i, offsets in enumerate((SEVEN, SEVEN_B)):
        conv = _conv(ME, 3, 5, offsets, device, seed=i)
        y = conv(x)
        km = expected_kmap(coords.numpy(), coords.numpy(), offsets)
        assert_close(y.F, O.conv_forward(feats.numpy(), conv.kernel.detach().cpu().numpy(), km, coords.shape[0]),
                     what=f"layer {i}")
    assert n_kernel_maps(x.coordinate_manager) == before + 2
    if host_layer == "python":      # the key of a CUSTOM map carries the offsets as a tuple of tuples behind the eight entries
        keys = [k for k in x.coordinate_manager._manager._kernel_maps if len(k) == 9]
        assert sorted(k[8] for k in keys) == sorted([tuple(map(tuple, SEVEN)), tuple(map(tuple, SEVEN_B))])


# ---- 4. convolution forward and backward vs oracle ----------------------------------------------------------------------------
def _check_conv(ME, device, coords, offsets, cin, cout, bf16=False):
    D = coords.shape[1] - 1
    g = torch.Generator().manual_seed(7)
    feats = torch.rand(coords.shape[0], cin, generator=g) - 0.3
    # (bf16: no bias.  The module adds it to the ROUNDED convolution output and rounds again; the bf16 bound of
    # tests/test_gpu_bf16.py is that of one rounding of the convolution's fp32 sum, which is what it is applied to there)
    conv = _conv(ME, cin, cout, offsets, device, D, bias=not bf16)
    if bf16:
        feats = bf16_round(feats)
        with torch.no_grad():
            conv.kernel.copy_(bf16_round(conv.kernel))
    x = ME.SparseTensor(feats.to(device).to(torch.bfloat16 if bf16 else torch.float32), coords.to(device),
                        requires_grad=True)
    y = conv(x)
    assert np.array_equal(y.C.cpu().numpy(), coords.numpy())
    gy = torch.rand(y.F.shape, generator=g) - 0.5
    if bf16:
        gy = bf16_round(gy)
    y.F.backward(gy.to(device).to(y.F.dtype))
    km = expected_kmap(coords.numpy(), coords.numpy(), offsets)
    w = conv.kernel.detach().float().cpu().numpy()
    b = conv.bias.detach().float().cpu().numpy().astype(np.float64) if conv.bias is not None else 0.0
    ref = O.conv_forward(feats.numpy(), w, km, coords.shape[0]) + b
    gi, gw = O.conv_backward(feats.numpy(), gy.numpy(), w, km)
    gb = gy.numpy().astype(np.float64).sum(0, keepdims=True)
    if bf16:
        assert y.F.dtype == torch.bfloat16 and x.F.grad.dtype == torch.bfloat16
        assert_bf16_close(y.F.detach().float().cpu().numpy(), ref, "forward")
        assert_bf16_close(x.F.grad.float().cpu().numpy(), gi, "grad_in")
    else:
        assert_close(y.F, ref, what="forward")
        assert_close(x.F.grad, gi, what="grad_in")
    assert_close(conv.kernel.grad, gw, what="grad_kernel")
    if conv.bias is not None:
        assert_close(conv.bias.grad, gb, what="grad_bias")


@pytest.mark.parametrize("case", ["seven", "hybrid"])
def test_conv_forward_backward_vs_oracle(device, host_layer, case):
    import minkowskiengine_amd as ME
    if case == "seven":
        _check_conv(ME, device, cloud("3000"), SEVEN, 3, 5)
    else:
        _check_conv(ME, device, cloud("4d"), hybrid29(), 3, 5)


def test_bf16_conv_on_the_hybrid_kernel_vs_oracle(device, host_layer):
    """K = 29 is odd and no multiple of 4: the packed weight image and the batching of offsets see a ragged tail"""
    import minkowskiengine_amd as ME
    _check_conv(ME, device, cloud("4d"), hybrid29(), 16, 32, bf16=True)


def test_strided_conv_and_its_transpose_vs_oracle(device, host_layer):
    """{0,1}^3 at stride 2 (fine -> coarse, steps of the fine stride), then the transposed layer back to stride 1: its map
    is built coarse -> fine with the finer stride and swapped"""
    import minkowskiengine_amd as ME
    coords = cloud("3000")
    fine = coords.numpy()
    g = torch.Generator().manual_seed(11)
    feats = torch.rand(coords.shape[0], 3, generator=g) - 0.3
    down = _conv(ME, 3, 5, CUBE2, device, bias=True, stride=2)
    up = _conv(ME, 5, 3, CUBE2, device, bias=True, transpose=True, seed=1, stride=2)
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
    y = down(x)
    assert y.tensor_stride == [2, 2, 2]
    coarse = y.C.cpu().numpy()
    assert np.array_equal(coarse, O.stride_map(fine, [2] * 3)[0])
    z = up(y)
    assert z.coordinate_map_key == x.coordinate_map_key
    gz = torch.rand(z.F.shape, generator=g) - 0.5
    z.F.backward(gz.to(device))

    km = expected_kmap(fine, coarse, CUBE2)                       # in = fine rows, out = coarse rows
    wd, bd = down.kernel.detach().cpu().numpy(), down.bias.detach().cpu().numpy().astype(np.float64)
    wu, bu = up.kernel.detach().cpu().numpy(), up.bias.detach().cpu().numpy().astype(np.float64)
    y_ref = O.conv_forward(feats.numpy(), wd, km, len(coarse)) + bd
    assert_close(y.F, y_ref, what="down forward")
    z_ref = O.conv_forward(y_ref, wu, transposed(km), len(fine)) + bu
    assert_close(z.F, z_ref, what="up forward")
    gy, gwu = O.conv_backward(y_ref, gz.numpy(), wu, transposed(km))
    gx, gwd = O.conv_backward(feats.numpy(), gy, wd, km)
    assert_close(up.kernel.grad, gwu, what="up grad_kernel")
    assert_close(up.bias.grad, gz.numpy().astype(np.float64).sum(0, keepdims=True), what="up grad_bias")
    assert_close(down.kernel.grad, gwd, what="down grad_kernel")
    assert_close(down.bias.grad, gy.sum(0, keepdims=True), what="down grad_bias")
    assert_close(x.F.grad, gx, what="grad_in")


# ---- 5. pooling and channel-wise convolution -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "max"])
def test_local_pooling_vs_oracle(device, host_layer, mode):
    """forward bit-exact (same offsets, same order), gradients within rtol 1e-5 / atol 1e-6: tests/test_gpu_pooling.py:104-109"""
    import minkowskiengine_amd as ME
    coords = make_cloud(500, 9, 3, seed=8, batch=2, negative=True)
    g = torch.Generator().manual_seed(5)
    feats = torch.rand(coords.shape[0], 4, generator=g) - 0.5
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
    cls = {"sum": ME.MinkowskiSumPooling, "max": ME.MinkowskiMaxPooling}[mode]
    y = cls(kernel_size=-1, kernel_generator=generator(ME, SEVEN), dimension=3)(x)
    km = expected_kmap(coords.numpy(), coords.numpy(), SEVEN)
    ref, aux = O.pool_forward(feats.numpy(), km, coords.shape[0], mode)
    assert np.array_equal(y.F.detach().cpu().numpy(), ref)
    gy = torch.rand(y.F.shape, generator=g)
    y.F.backward(gy.to(device))
    assert np.allclose(x.F.grad.cpu().numpy(), O.pool_backward(gy.numpy(), km, coords.shape[0], mode, aux),
                       rtol=1e-5, atol=1e-6)


def test_channelwise_convolution_vs_numpy(device, host_layer):
    """out_u = bias + sum_k W_k * x_{u + offset_k} in float64 on the numpy-built map; rtol 1e-5 of the largest magnitude:
    tests/test_gpu_channelwise.py:19-23"""
    import minkowskiengine_amd as ME
    coords = cloud("3000")
    n, C = coords.shape[0], 5
    g = torch.Generator().manual_seed(9)
    feats = torch.rand(n, C, generator=g) - 0.5
    layer = ME.MinkowskiChannelwiseConvolution(C, bias=True, kernel_generator=generator(ME, SEVEN), dimension=3).to(device)
    with torch.no_grad():
        layer.bias.uniform_(-0.5, 0.5)
    x = ME.SparseTensor(feats.to(device), coords.to(device), requires_grad=True)
    y = layer(x)
    gy = torch.rand(y.F.shape, generator=g) - 0.5
    y.F.backward(gy.to(device))
    km = expected_kmap(coords.numpy(), coords.numpy(), SEVEN)
    f64, w, g64 = feats.numpy().astype(np.float64), layer.kernel.detach().cpu().numpy().astype(np.float64), gy.numpy().astype(np.float64)
    out = np.zeros((n, C)) + layer.bias.detach().cpu().numpy().astype(np.float64)
    gi, gw = np.zeros((n, C)), np.zeros_like(w)
    for k, (i, o) in km.items():
        np.add.at(out, o, f64[i] * w[k])
        np.add.at(gi, i, g64[o] * w[k])
        gw[k] = (f64[i] * g64[o]).sum(0)

    def close(a, b, what):
        a = a.detach().cpu().numpy().astype(np.float64)
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-5, atol=1e-5 * np.abs(b).max()), what

    close(y.F, out, "forward")
    close(x.F.grad, gi, "grad_in")
    close(layer.kernel.grad, gw, "grad_kernel")
    close(layer.bias.grad, g64.sum(0, keepdims=True), "grad_bias")


# ---- 6. generative layer ---------------------------------------------------------------------------------------------------
def test_generative_transposed_convolution(device, host_layer):
    import minkowskiengine_amd as ME
    coords = make_cloud(200, 8, 3, seed=12, negative=True)
    coords[:, 1:] *= 2                                            # a map at tensor stride 2
    in_c = coords.numpy()
    g = torch.Generator().manual_seed(13)
    feats = torch.rand(coords.shape[0], 3, generator=g) - 0.3
    conv = ME.MinkowskiGenerativeConvolutionTranspose(3, 5, kernel_generator=generator(ME, FIVE, stride=2), dimension=3)
    with torch.no_grad():
        conv.kernel.copy_(torch.rand(conv.kernel.shape, generator=g) - 0.5)
    conv = conv.to(device)
    x = ME.SparseTensor(feats.to(device), coords.to(device), tensor_stride=2, requires_grad=True)
    y = conv(x)
    assert y.tensor_stride == [1, 1, 1]
    # c + offsets[k] * dilation * OUT tensor stride, rows by input row, then k; the first occurrence wins
    cand = np.repeat(in_c, len(FIVE), axis=0)
    cand[:, 1:] += np.tile(np.asarray(FIVE, np.int32), (in_c.shape[0], 1))
    want_c = cand[O.insert_and_map(cand)[0]]
    out_c = y.C.cpu().numpy()
    assert np.array_equal(out_c, want_c)
    assert in_c.shape[0] < out_c.shape[0] < cand.shape[0]          # (duplicates were there to remove)
    # the map is built coarse -> fine with the finer stride and swapped
    km = transposed(expected_kmap(out_c, in_c, FIVE))
    w = conv.kernel.detach().cpu().numpy()
    assert_close(y.F, O.conv_forward(feats.numpy(), w, km, out_c.shape[0]), what="forward")
    gy = torch.rand(y.F.shape, generator=g) - 0.5
    y.F.backward(gy.to(device))
    gi, gw = O.conv_backward(feats.numpy(), gy.numpy(), w, km)
    assert_close(x.F.grad, gi, what="grad_in")
    assert_close(conv.kernel.grad, gw, what="grad_kernel")


def test_expanding_convolution_keeps_the_aligned_candidates(device, host_layer):
    """expand_coordinates=True on a regular layer: c + offsets[k] * dilation * IN tensor stride, only the candidates on the
    output grid are kept (the existing alignment filter)"""
    import minkowskiengine_amd as ME
    coords = make_cloud(200, 8, 3, seed=14, negative=True)
    in_c = coords.numpy()
    feats = torch.rand(coords.shape[0], 3, generator=torch.Generator().manual_seed(15)) - 0.3
    conv = ME.MinkowskiConvolution(3, 5, kernel_generator=generator(ME, FIVE, stride=2), expand_coordinates=True,
                                   dimension=3).to(device)
    y = conv(ME.SparseTensor(feats.to(device), coords.to(device)))
    assert y.tensor_stride == [2, 2, 2]
    cand = np.repeat(in_c, len(FIVE), axis=0)
    cand[:, 1:] += np.tile(np.asarray(FIVE, np.int32), (in_c.shape[0], 1))
    cand = cand[(cand[:, 1:] % 2 == 0).all(1)]
    want_c = cand[O.insert_and_map(cand)[0]]
    out_c = y.C.cpu().numpy()
    assert np.array_equal(out_c, want_c)
    km = expected_kmap(in_c, out_c, FIVE)
    assert_close(y.F, O.conv_forward(feats.numpy(), conv.kernel.detach().cpu().numpy(), km, out_c.shape[0]))


# ---- 7. recipe replay ------------------------------------------------------------------------------------------------------
def test_prefetch_replays_custom_maps_with_their_offsets(device, host_layer):
    import minkowskiengine_amd as ME
    conv = _conv(ME, 3, 5, SEVEN, device)
    a = make_cloud(800, 10, 3, seed=20, batch=2, negative=True)
    xa = ME.SparseTensor(torch.rand(a.shape[0], 3, device=device), a.to(device))
    conv(xa)
    recipe = xa.coordinate_manager.recipe()
    assert n_kernel_maps(xa.coordinate_manager) == 1
    b = make_cloud(900, 10, 3, seed=21, batch=2, negative=True)
    feats = torch.rand(b.shape[0], 3, generator=torch.Generator().manual_seed(22))
    xb = ME.SparseTensor(feats.to(device), b.to(device))
    assert xb.coordinate_manager is not xa.coordinate_manager and n_kernel_maps(xb.coordinate_manager) == 0
    assert xb.coordinate_manager.prefetch(recipe) >= 1
    built, logged = n_kernel_maps(xb.coordinate_manager), len(xb.coordinate_manager.recipe())
    assert built == 1
    y = conv(xb)
    assert n_kernel_maps(xb.coordinate_manager) == built, "the forward pass built a kernel map the replay had not"
    assert len(xb.coordinate_manager.recipe()) == logged, "the forward pass asked for a map / plan the replay had not built"
    km = expected_kmap(b.numpy(), b.numpy(), SEVEN)
    assert_close(y.F, O.conv_forward(feats.numpy(), conv.kernel.detach().cpu().numpy(), km, b.shape[0]))


# ---- 8. geometry shortcuts -------------------------------------------------------------------------------------------------
def test_single_offset_layers(device, host_layer):
    """the origin alone is F @ W on the same map (use_mm, the row-with-itself shortcut); one non-zero offset is a shift and
    takes neither shortcut"""
    import minkowskiengine_amd as ME
    coords = cloud("3000")
    c = coords.numpy()
    feats = torch.rand(coords.shape[0], 4, generator=torch.Generator().manual_seed(30)) - 0.5
    x = ME.SparseTensor(feats.to(device), coords.to(device))
    origin = _conv(ME, 4, 6, [[0, 0, 0]], device)
    assert origin.use_mm
    y = origin(x)
    assert y.coordinate_map_key == x.coordinate_map_key
    f64 = feats.numpy().astype(np.float64)
    assert_close(y.F, f64 @ origin.kernel.detach().cpu().numpy().astype(np.float64), what="origin")
    shift = _conv(ME, 4, 6, [[1, 0, 0]], device, seed=1)
    assert not shift.use_mm
    y = shift(x)
    q = c.copy()
    q[:, 1] += 1
    rows = O.find(c, q)
    assert 0 < (rows >= 0).sum() < len(rows)
    want = np.where((rows >= 0)[:, None], f64[np.maximum(rows, 0)], 0.0) @ shift.kernel.detach().cpu().numpy()[0].astype(np.float64)
    assert_close(y.F, want, what="shift")
    # the maps themselves: identity for the origin, the shifted pairs for [[1, 0, 0]]
    cm, key = x.coordinate_manager, x.coordinate_map_key
    ident = cm.kernel_map(key, key, kernel_size=-1, region_type=ME.RegionType.CUSTOM, region_offset=torch.tensor([[0, 0, 0]]))
    O.assert_same_kernel_map(ident, {0: np.stack((np.arange(len(c)), np.arange(len(c))))})
    moved = cm.kernel_map(key, key, kernel_size=-1, region_type=ME.RegionType.CUSTOM, region_offset=torch.tensor([[1, 0, 0]]))
    O.assert_same_kernel_map(moved, expected_kmap(c, c, [[1, 0, 0]]))


def test_invalid_offsets_raise_before_any_launch(device, host_layer):
    import minkowskiengine_amd as ME
    coords = cloud("130")
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device=device), coords.to(device))
    cm, key = x.coordinate_manager, x.coordinate_map_key
    for bad in (torch.IntTensor(), torch.tensor([[1, 0]]), torch.tensor([[1, 0, 0], [1, 0, 0]])):
        with pytest.raises((ValueError, RuntimeError), match="region_offsets"):
            cm.kernel_map(key, key, kernel_size=-1, region_type=ME.RegionType.CUSTOM, region_offset=bad)
    assert n_kernel_maps(cm) == 0
