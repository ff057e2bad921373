"""Window attention on the GPU, through both host layers: the window lists of csrc/serial_attention.hip bit for bit against
the numpy yardstick of tests/test_window_attention_cpu.py, and the attention kernels on those lists and their block table
(the _tab entry points of csrc/attention.hip) against the yardsticks of tests/test_gpu_attention_kernels.py with the window
of every row as its segment.

The bound is the project's: E_kernel <= FACTOR * E_torch per tensor against float64 (FACTOR = 4).  Every figure is printed
before it is asserted (pytest -s).  Measured ratios: DESIGN 8.15."""
import gc
import math
import os
import sys
import weakref

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import host as _host
from test_gpu_attention_kernels import FACTOR, draw, within_bound
from test_gpu_serialized_attention_kernels import lists_from_row_patch
from test_window_attention_cpu import (EDGE_SIZES, WINDOW, box_rows, cube_scene, edges_scene, row_windows,
                                       three_boxes_scene)

pytestmark = pytest.mark.gpu
NAMES = ("out", "dq", "dk", "dv")
DTYPES = (torch.float32, torch.bfloat16)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def scene_of(coords, device, stride=1):
    """a sparse tensor on the given unique int rows [n, 1 + D], in their order"""
    coords = torch.as_tensor(np.asarray(coords)).int()
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1), coordinates=coords, tensor_stride=stride, device=device)
    assert x.F.shape[0] == coords.shape[0] and torch.equal(x.C.cpu(), coords)
    return x


def random_scene(sizes, batches, D, stride, seed, lo=-20, hi=45):
    """sizes[i] unique voxels in instance batches[i], coordinates in [lo, hi) on the grid of `stride`, rows shuffled"""
    rng = np.random.default_rng(seed)
    first, cells = -(-lo // stride), (hi - 1) // stride + 1
    rows = []
    for m, b in zip(sizes, batches):
        pts = np.unique(rng.integers(first, cells, size=(4 * m + 16, D)), axis=0)
        pts = pts[rng.permutation(pts.shape[0])[:m]] * stride
        assert pts.shape[0] == m and pts.min() >= lo and pts.max() < hi
        rows.append(np.concatenate([np.full((m, 1), b), pts], 1))
    rows = np.concatenate(rows)
    return rows[rng.permutation(rows.shape[0])]


def lists(x, window_size, shift=0):
    return x.coordinate_manager.window_rows(x.coordinate_map_key, window_size, shift)


def check_lists(x, window_size, shift, what=""):
    """all four outputs of window_rows against the yardstick on the rows of the map -> the window of every row (int64)"""
    seg_ptr, seg_rows, blk_tab, row_window = (t.cpu().numpy() for t in lists(x, window_size, shift))
    n = x.F.shape[0]
    want = row_windows(x.C.cpu().numpy(), [int(t) for t in x.tensor_stride], window_size, shift)
    assert row_window.dtype == np.int32 and np.array_equal(row_window, want), \
        f"{what}: {int((row_window != want).sum())} of {n} rows in another window"
    want_lists = lists_from_row_patch(want, int(want.max()) + 1 if n else 0)          # no surplus segment: W was read back
    for name, got in (("seg_ptr", seg_ptr), ("seg_rows", seg_rows), ("blk_tab", blk_tab)):
        assert got.dtype == np.int32 and np.array_equal(got, want_lists[name]), f"{what}: {name} differs"
    return torch.from_numpy(want).to(x.F.device)


def run(x, q, k, v, dout, heads, window_size, shift, need=(True, True, True)):
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d)
    key, mgr = x.coordinate_map_key, x._manager._manager
    fw = ME.get_minkowski_function("WindowAttentionForward", q, key)
    bw = ME.get_minkowski_function("WindowAttentionBackward", q, key)
    out, lse = fw(q, k, v, heads, scale, window_size, shift, key, mgr)
    res = dict(out=out, lse=lse)
    res["dq"], res["dk"], res["dv"] = bw(q, k, v, out, lse, dout, heads, scale, window_size, shift, key, mgr,
                                         need_grad_q=need[0], need_grad_k=need[1], need_grad_v=need[2])
    return res


def run_global(x, q, k, v, dout, heads):
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d)
    key, mgr = x.coordinate_map_key, x._manager._manager
    fw = ME.get_minkowski_function("AttentionForward", q, key)
    bw = ME.get_minkowski_function("AttentionBackward", q, key)
    glob = _host.key_like(key)
    out, lse = fw(q, k, v, heads, scale, key, key, glob, mgr)
    dq, dk, dv = bw(q, k, v, out, lse, dout, heads, scale, key, key, glob, mgr)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _equal(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---- lists, bit-exact against the yardstick ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,stride", [(2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2)],
                         ids=["D2", "D2s2", "D3", "D3s2", "D4", "D4s2"])
def test_lists_equal_the_yardstick(device, host_layer, D, stride):
    """about 300 voxels in [-20, 45) in three instances with the batch indices 0, 2 and 5; window 4, window (4, 2, 3, ..) and
    window 1 (every voxel alone), each with shift 0, shift w // 2 and a negative shift"""
    x = scene_of(random_scene((130, 70, 100), (0, 2, 5), D, stride, seed=10 * D + stride), device, stride)
    assert int(x.C[:, 1:].min()) < 0 and sorted(set(x.C[:, 0].tolist())) == [0, 2, 5]
    per_axis = (4, 2, 3, 5)[:D]
    for window in (4, per_axis, 1):
        half = window // 2 if isinstance(window, int) else tuple(w // 2 for w in window)
        negative = -1 if isinstance(window, int) else (-1, -3, -2, -7)[:D]
        for shift in (0, half, negative):
            seg = check_lists(x, window, shift, f"D={D} stride={stride} w={window} s={shift} {host_layer}")
            if window == 1:
                assert torch.equal(torch.sort(seg).values.cpu(), torch.arange(300))


def test_a_window_of_two_blocks_and_its_split_under_a_shift(device, host_layer):
    """a dense 5 x 5 x 5 block inside one 8^3 window: 125 rows, two blocks in the table; under shift 4 eight windows"""
    x = scene_of(cube_scene(), device)
    seg_ptr, seg_rows, blk_tab, row_window = lists(x, WINDOW, 0)
    assert seg_ptr.tolist() == [0, 125] and seg_rows.tolist() == list(range(125)) and not row_window.any()
    assert blk_tab.tolist() == [0, 0, 0, 64, -1, -1]
    check_lists(x, WINDOW, 0)
    seg = check_lists(x, WINDOW, 4)
    assert sorted(torch.bincount(seg).tolist()) == [8, 12, 12, 12, 18, 18, 18, 27]
    assert lists(x, WINDOW, 4)[2].reshape(-1, 2)[:, 0].tolist() == list(range(8)) + [-1, -1]


def test_derived_maps(device, host_layer):
    """a strided map and a pruned map that lost an instance carry no bounding box: one reduction gives it"""
    x = scene_of(random_scene((150, 90, 60), (0, 1, 2), 3, 1, seed=5), device)
    y = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    assert y.tensor_stride[0] == 2
    for window, shift in ((4, 0), (4, 2), ((2, 3, 4), (1, -1, 2))):
        check_lists(y, window, shift, f"strided {host_layer}")
    z = ME.MinkowskiPruning()(x, x.C[:, 0] != 1)
    assert z.F.shape[0] == 210 and sorted(set(z.C[:, 0].tolist())) == [0, 2]
    for window, shift in ((4, 0), (6, 3)):
        check_lists(z, window, shift, f"pruned {host_layer}")


def test_cached_lists(device, host_layer):
    """a second call returns the cached tensors, shift and shift + w share one entry, another shift makes a second one, an
    int and the same value per axis are one entry, and the entries go with the manager that owns the map"""
    x = scene_of(random_scene((150, 90), (0, 1), 3, 1, seed=6), device)
    got = lists(x, 4, 1)
    again = lists(x, 4, 1)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, again))
    for same in (lists(x, 4, 5), lists(x, 4, -3), lists(x, (4, 4, 4), (1, 5, -7))):
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, same))
    other = lists(x, 4, 2)
    assert other[3].data_ptr() != got[3].data_ptr() and not torch.equal(other[3], got[3])
    if host_layer == "python":
        mgr = x.coordinate_manager._manager
        assert all(any(t is h for h in mgr.device_tensors()) for t in got + other)
        assert len(mgr._window_rows_cache) == 2
        ref = weakref.ref(mgr)
        del mgr, x, got, again, other, same
        gc.collect()
        assert ref() is None


def test_a_wide_scene(device, host_layer):
    """600 voxels in two instances spread over [0, 2^17) in x and y and [0, 64) in z, and neighbours of theirs that share
    their windows: 15 + 15 + 4 cell bits under window 4; the lists against the yardstick and one bf16 step in the bound"""
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.integers(0, (1 << 17) - 4, size=(300, 2)), rng.integers(0, 60, size=(300, 1))], 1)
    pts[0] = (0, 0, 0)
    pts = np.unique(np.concatenate([pts, pts + rng.integers(1, 4, size=(300, 3)), [[(1 << 17) - 1, (1 << 17) - 1, 63]]]), axis=0)
    coords = np.concatenate([rng.integers(0, 2, size=(pts.shape[0], 1)), pts], 1)
    x = scene_of(coords[rng.permutation(coords.shape[0])], device)
    seg = check_lists(x, 4, 0, "wide")
    check_lists(x, 4, 2, "wide")
    assert int(seg.max()) + 1 < coords.shape[0]
    step_within_bound(x, seg, 4, 0, 64, torch.bfloat16, 170, f"window wide scene bf16 {host_layer}")


def test_a_key_beyond_63_bits_raises_before_a_launch(device, host_layer):
    coords = torch.tensor([[0, 0, 0, 0, 0], [0, 70000, 70000, 70000, 70000], [1, 5, 5, 5, 5]]).int()
    x = ME.SparseTensor(torch.zeros(3, 1), coordinates=coords, device=device)       # window 1, D = 4: 4 * 17 cell bits
    with pytest.raises(Exception, match="63"):
        lists(x, 1, 0)
    lists(x, 4, 0)                                                                   # 4 * 15 cell bits and one batch bit
    with pytest.raises(ValueError, match="window_size"):
        lists(x, 0)
    with pytest.raises(ValueError, match="per spatial axis"):
        lists(x, (4, 4, 4))
    torch.cuda.synchronize(device)


# ---- bound ---------------------------------------------------------------------------------------------------------------------
def step_within_bound(x, seg, window_size, shift, d, dtype, seed, what):
    heads = 2
    n, c = x.F.shape[0], heads * d
    q, k, v, dout = (draw(n, c, dtype, x.F.device, seed + s) for s in range(4))
    r = run(x, q, k, v, dout, heads, window_size, shift)
    within_bound(r, q, k, v, dout, seg, seg, heads, what=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shift", [0, WINDOW // 2])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("case", ["cube", "edges"])
def test_windows_stay_within_the_bound(device, host_layer, case, d, shift, dtype):
    """window 8 on dense boxes: windows of 1, 31, 32, 33, 65 and 150 rows, and the 125-row window; under shift 4 the boxes
    are cut into the populations the yardstick gives"""
    coords = edges_scene() if case == "edges" else cube_scene()
    x = scene_of(coords, device)
    seg = lists(x, WINDOW, shift)[3].long()
    counts = torch.bincount(seg).tolist()
    if shift == 0:
        assert sorted(counts) == (sorted(EDGE_SIZES) if case == "edges" else [125])
    assert counts == np.bincount(row_windows(coords, 1, WINDOW, shift)).tolist()
    step_within_bound(x, seg, WINDOW, shift, d, dtype, 10 * d, f"window {case} d={d} shift={shift} {dtype} {host_layer}")


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_one_window_per_instance_equals_global_attention(device, host_layer, dtype):
    """window 128 with shift 64 holds [-64, 64) on every axis: the windows are the instances, so out, lse, dq, dk, dv equal
    MinkowskiSelfAttention's operators bit for bit — the table path finds the blocks the walk finds"""
    heads, d = 2, 64
    x = scene_of(random_scene((130, 63, 5), (0, 1, 2), 3, 1, seed=12), device)
    assert torch.bincount(lists(x, 128, 64)[3].long()).tolist() == torch.bincount(x.C[:, 0].long()).tolist()
    n, c = x.F.shape[0], heads * d
    q, k, v, dout = (draw(n, c, dtype, device, 90 + s) for s in range(4))
    ours = run(x, q, k, v, dout, heads, 128, 64)
    want = run_global(x, q, k, v, dout, heads)
    for name in NAMES + ("lse",):
        assert _equal(ours[name], want[name]), name


# ---- isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_window_does_not_see_its_neighbours(device, host_layer, dtype):
    """three windows of 65 rows in a line; the middle one holds data, the others Inf and NaN.  The middle window must give
    bit for bit what its rows give as a scene of their own"""
    heads, d, P = 2, 64, 65
    c = heads * d
    coords = three_boxes_scene()
    x = scene_of(coords, device)
    seg = lists(x, WINDOW, 0)[3].long()
    assert torch.bincount(seg).tolist() == [P, P, P]
    mine = (seg == 1).nonzero().reshape(-1)
    qa, ka, va, da = (draw(P, c, dtype, device, 70 + s) for s in range(4))
    xa = scene_of(coords[mine.cpu().numpy()], device)
    alone = run(xa, qa, ka, va, da, heads, WINDOW, 0)
    bad = torch.full((3 * P, c), math.inf, dtype=dtype, device=device)
    bad[::2] = math.nan
    bad[1::4] = -math.inf
    q, k, v, dout = (bad.clone().index_put_((mine,), t) for t in (qa, ka, va, da))
    both = run(x, q, k, v, dout, heads, WINDOW, 0)
    for name in NAMES + ("lse",):
        assert torch.isfinite(alone[name].float()).all()
        assert _equal(both[name][mine], alone[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_the_halves_of_a_split_window_stop_seeing_each_other(device, host_layer, dtype):
    """the 65-row window under shift (0, 4, 0) falls into the halves y < 4 (33 rows) and y >= 4 (32 rows).  With an output
    gradient on the first half only, dk and dv of the second half are exactly zero; under shift 0 they are not"""
    heads, d = 2, 32
    c = heads * d
    coords = box_rows(65, (0, 0, 0))
    x = scene_of(coords, device)
    lower = torch.from_numpy(coords[:, 2] < 4).to(device)
    assert int(lower.sum()) == 33
    seg = lists(x, WINDOW, (0, 4, 0))[3].long()
    assert torch.equal(seg == 0, lower) and torch.bincount(seg).tolist() == [33, 32]
    q, k, v, dout = (draw(65, c, dtype, device, 40 + s) for s in range(4))
    dout[~lower] = 0
    whole = run(x, q, k, v, dout, heads, WINDOW, 0)
    split = run(x, q, k, v, dout, heads, WINDOW, (0, 4, 0))
    for name in ("dk", "dv"):
        assert torch.isfinite(split[name].float()).all()
        assert float(split[name][~lower].float().abs().max()) == 0.0, name
        assert float(split[name][lower].float().abs().max()) > 0.0, name
        assert float(whole[name][~lower].float().abs().max()) > 0.0, name
    assert float(split["dq"][~lower].float().abs().max()) == 0.0


# ---- reproducibility, hosts, subsets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_calls_and_two_hosts_are_bitwise_equal(device, dtype):
    heads, d = 2, 64
    c = heads * d
    coords = edges_scene()
    results, tables = [], []
    prev = ME.get_host()
    try:
        for layer in ("python", "native", "python"):
            ME.set_host(layer)
            x = scene_of(coords, device)
            q, k, v, dout = (draw(x.F.shape[0], c, dtype, device, 90 + s) for s in range(4))
            results.append(run(x, q, k, v, dout, heads, WINDOW, (4, 0, 4)))
            results.append(run(x, q, k, v, dout, heads, WINDOW, (4, 0, 4)))
            tables.append(lists(x, WINDOW, (4, 0, 4)))
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for name in NAMES + ("lse",):
            assert _equal(results[0][name], other[name]), name
    for other in tables[1:]:
        assert all(torch.equal(a, b) for a, b in zip(tables[0], other))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gradient_subsets(device, host_layer, dtype):
    heads, d = 2, 32
    c = heads * d
    x = scene_of(edges_scene(), device)
    q, k, v, dout = (draw(x.F.shape[0], c, dtype, device, 50 + s) for s in range(4))
    full = run(x, q, k, v, dout, heads, WINDOW, 4)
    for mask in range(1, 8):
        need = tuple(bool(mask >> i & 1) for i in range(3))
        r = run(x, q, k, v, dout, heads, WINDOW, 4, need=need)
        for name, wanted in zip(("dq", "dk", "dv"), need):
            if wanted:
                assert _equal(r[name], full[name]), (need, name)
            else:
                assert r[name] is None, (need, name)


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_the_function_in_float64(device, host_layer):
    """H = 2, d = 5, 12 rows in three windows of 5, 4 and 3 rows (window 3, shift 1, negative coordinates)"""
    from test_gpu_attention_kernels import reference
    coords = np.concatenate([box_rows(5, (-4, -1, 2), side=3), box_rows(4, (2, -1, 2), side=3), box_rows(3, (2, 2, -4), side=3)])
    x = scene_of(coords, device)
    seg = lists(x, 3, 1)[3].long()
    assert torch.bincount(seg).tolist() == [5, 4, 3]
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(12, 10, generator=g, dtype=torch.float64).to(device).requires_grad_() for _ in range(3))

    def f(q_, k_, v_):
        return ME.MinkowskiWindowAttentionFunction.apply(q_, k_, v_, 2, None, 3, 1, x.coordinate_map_key, x.coordinate_manager)
    assert torch.autograd.gradcheck(f, (q, k, v), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    ref = reference(q, k, v, torch.ones_like(q), seg, seg, 2)
    assert float((f(q, k, v).detach() - ref["out"]).abs().max()) <= 1e-12


# ---- module and functional ------------------------------------------------------------------------------------------------------
def _mha_per_segment(state, dtype, feats, dout, seg, embed_dim, heads, bias):
    """torch.nn.MultiheadAttention in `dtype` with the parameters `state` on the rows of every segment -> (out, grads)"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    mha = torch.nn.MultiheadAttention(embed_dim, heads, bias=bias, batch_first=True).to(feats.device).to(dtype)
    mha.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=True)
    x = feats.detach().to(dtype).requires_grad_()
    out = torch.zeros_like(x)
    with sdpa_kernel(SDPBackend.MATH):
        for s in torch.unique(seg).tolist():
            m = (seg == s).nonzero().reshape(-1)
            xb = x[m][None]
            out = out.index_copy(0, m, mha(xb, xb, xb, need_weights=False)[0][0])
        out.backward(dout.to(dtype))
    grads = {k: p.grad for k, p in mha.named_parameters()}
    grads["input"] = x.grad
    return out.detach(), grads


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_module_equals_multihead_attention_per_window(device, host_layer, dtype, bias):
    """the bound of the serialized module test: E_layer <= FACTOR * E_torch per tensor against float64, the parameter
    gradients included"""
    embed_dim, heads, shift = 64, 2, (4, 0, 4)
    x = scene_of(edges_scene(), device)
    n = x.F.shape[0]
    seg = lists(x, WINDOW, shift)[3].long()
    torch.manual_seed(11)
    layer = ME.MinkowskiWindowSelfAttention(embed_dim, heads, window_size=WINDOW, shift=shift, bias=bias).to(device).to(dtype)
    if bias:
        with torch.no_grad():
            layer.in_proj_bias.normal_(std=0.3)
            layer.out_proj.bias.normal_(std=0.3)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    feats, dout = draw(n, embed_dim, dtype, device, 1), draw(n, embed_dim, dtype, device, 2)
    f = feats.clone().requires_grad_()
    xin = ME.SparseTensor(f, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    out = layer(xin)
    assert out.coordinate_map_key == x.coordinate_map_key and out.F.dtype == dtype
    out.F.backward(dout)
    ours = {k: p.grad for k, p in layer.named_parameters()}
    ours["input"] = f.grad
    ref_out, ref = _mha_per_segment(state, torch.float64, feats, dout, seg, embed_dim, heads, bias)
    their_out, theirs = _mha_per_segment(state, dtype, feats, dout, seg, embed_dim, heads, bias)
    bad = []
    for name, a, b, r in [("out", out.F.detach(), their_out, ref_out)] + [(k, ours[k], theirs[k], ref[k]) for k in ref]:
        assert a is not None and torch.isfinite(a.float()).all(), name
        e, et = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"window module {dtype} bias={bias} {host_layer} {name}: E_layer {e:.3e}  E_torch {et:.3e}  "
              f"ratio {e / et if et else math.inf:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"beyond {FACTOR} x E_torch: {bad}"


def test_functional_and_its_errors(device, host_layer):
    from test_gpu_attention_kernels import reference, torch_attention
    heads, d = 2, 32
    x = scene_of(edges_scene(), device)
    n, c = x.F.shape[0], heads * d
    mk = lambda s: ME.SparseTensor(draw(n, c, torch.float32, device, s), coordinate_map_key=x.coordinate_map_key,  # noqa: E731
                                   coordinate_manager=x.coordinate_manager)
    xq, xk, xv = mk(1), mk(2), mk(3)
    y = ME.MinkowskiFunctional.window_attention(xq, xk, xv, heads, WINDOW, shift=(0, 4, 4))
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == x.coordinate_map_key
    seg = lists(x, WINDOW, (0, 4, 4))[3].long()
    dout = torch.zeros_like(xq.F)
    ref = reference(xq.F, xk.F, xv.F, dout, seg, seg, heads)
    theirs = torch_attention(xq.F, xk.F, xv.F, dout, seg, seg, heads)
    e = float((y.F.double() - ref["out"]).abs().max())
    et = float((theirs["out"].double() - ref["out"]).abs().max())
    print(f"window functional {host_layer}: E_layer {e:.3e}  E_torch {et:.3e}")
    assert e <= FACTOR * et
    coarse = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(xq)
    with pytest.raises(ValueError, match="one coordinate map"):
        ME.MinkowskiFunctional.window_attention(coarse, xk, xv, heads, WINDOW)
    with pytest.raises(ValueError, match="window_size"):
        ME.MinkowskiFunctional.window_attention(xq, xk, xv, heads, 0)
    with pytest.raises(ValueError, match="per spatial axis"):
        ME.MinkowskiFunctional.window_attention(xq, xk, xv, heads, (8, 8))
    with pytest.raises(ValueError, match="head dimension"):
        ME.MinkowskiFunctional.window_attention(xq, xk, xv, 4, WINDOW)
    with pytest.raises(TypeError, match="SparseTensor"):
        ME.MinkowskiFunctional.window_attention(xq.F, xk, xv, heads, WINDOW)
    field = ME.TensorField(torch.randn(3, 64), coordinates=torch.tensor([[0, 0.2, 0.1, 0.0], [0, 1.4, 0.3, 0.2],
                                                                         [1, 0.1, 2.2, 0.5]]), device=device)
    with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
        ME.MinkowskiWindowSelfAttention(64, 2).to(device)(field)
    torch.cuda.synchronize(device)


def test_the_examples_stage_runs(device, host_layer):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import window_attention_block as WB
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 24, (1500, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(device)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(device), coords)
    stage = WB.WindowStage(64, 2, depth=4, window_size=8).to(device)
    out = stage(x)
    assert tuple(out.F.shape) == tuple(x.F.shape) and out.coordinate_map_key == x.coordinate_map_key
    out.F.square().mean().backward()
    norm = float(stage.blocks[3].attn.in_proj_weight.grad.norm())
    assert math.isfinite(norm) and norm > 0
