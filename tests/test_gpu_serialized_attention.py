"""Serialized patch attention on the GPU, through both host layers: the keys and patch lists of csrc/serial_attention.hip
bit for bit against the numpy yardstick of tests/test_serialized_attention_cpu.py, and the attention kernels on those lists
and their block table (the _tab entry points of csrc/attention.hip) against the yardsticks of
tests/test_gpu_attention_kernels.py with the patch of every row as its segment.

Measured ratios E_kernel / E_torch (bound FACTOR = 4): see DESIGN 8.13.  Every figure is printed before it is asserted."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import host as _host
from test_gpu_attention_kernels import BK, FACTOR, draw, reference, torch_attention, within_bound  # noqa: F401
from test_gpu_serialized_attention_kernels import lists_from_row_patch
from test_serialized_attention_cpu import ORDERS, row_patches

pytestmark = pytest.mark.gpu
NAMES = ("out", "dq", "dk", "dv")
DTYPES = (torch.float32, torch.bfloat16)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def make_scene(sizes, device, D=3, stride=1, seed=0, lo=-20, hi=45):
    """sizes[b] unique voxels in instance b, coordinates in [lo, hi) on a map of tensor stride `stride`, rows shuffled"""
    g = torch.Generator().manual_seed(seed)
    cells = (hi - lo + stride - 1) // stride
    first = -(-lo // stride) * stride
    rows = []
    for b, n in enumerate(sizes):
        pts = torch.unique(torch.randint(0, cells, (4 * n + 16, D), generator=g), dim=0)
        pts = pts[torch.randperm(pts.shape[0], generator=g)[:n]] * stride + first
        assert pts.shape[0] == n and int(pts.min()) >= lo and int(pts.max()) < hi
        rows.append(torch.cat([torch.full((n, 1), b), pts], 1))
    coords = torch.cat(rows).int()
    coords = coords[torch.randperm(coords.shape[0], generator=g)]
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1), coordinates=coords, tensor_stride=stride, device=device)
    assert x.F.shape[0] == coords.shape[0]
    return x


def lists(x, patch_size, order):
    return x.coordinate_manager.patch_rows(x.coordinate_map_key, patch_size, order)


def run(x, q, k, v, dout, heads, patch_size, order, need=(True, True, True)):
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d)
    key, mgr = x.coordinate_map_key, x._manager._manager
    fw = ME.get_minkowski_function("SerializedAttentionForward", q, key)
    bw = ME.get_minkowski_function("SerializedAttentionBackward", q, key)
    out, lse = fw(q, k, v, heads, scale, patch_size, order, key, mgr)
    res = dict(out=out, lse=lse)
    res["dq"], res["dk"], res["dv"] = bw(q, k, v, out, lse, dout, heads, scale, patch_size, order, key, mgr,
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


# ---- keys and lists, bit-exact against the yardstick --------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D,stride", [(3, 1), (3, 2), (2, 1), (4, 1)], ids=["D3", "D3s2", "D2", "D4"])
def test_lists_equal_the_yardstick(device, host_layer, D, stride, order):
    P = 32
    x = make_scene([170, 131], device, D=D, stride=stride, seed=10 * D + stride)
    n = x.F.shape[0]
    seg_ptr, seg_rows, blk_tab, row_patch = (t.cpu().numpy() for t in lists(x, P, order))
    n_seg = -(-n // P) + 2
    assert seg_ptr.shape == (n_seg + 1,) and seg_rows.shape == (n,) and row_patch.shape == (n,)
    assert blk_tab.shape == (2 * (-(-n // 64) + n_seg),)
    want = row_patches(x.C.cpu().numpy(), [stride] * D, order, P)
    assert np.array_equal(row_patch, want), f"{int((row_patch != want).sum())} of {n} rows in another patch"
    assert np.array_equal(np.sort(seg_rows), np.arange(n))
    assert seg_ptr[0] == 0 and seg_ptr[-1] == n and (np.diff(seg_ptr) >= 0).all() and np.diff(seg_ptr).max() <= P
    entries = []
    for s in range(n_seg):
        rows = seg_rows[seg_ptr[s]:seg_ptr[s + 1]]
        assert (np.diff(rows) > 0).all() and (row_patch[rows] == s).all()
        entries += [(s, t0) for t0 in range(0, len(rows), 64)]
    entries += [(-1, None)] * (len(blk_tab) // 2 - len(entries))
    tab = blk_tab.reshape(-1, 2)
    for e, (s, t0) in enumerate(entries):
        assert tab[e, 0] == s and (s < 0 or tab[e, 1] == t0), (e, tab[e], s, t0)


def test_the_block_table_steps_through_long_patches(device, host_layer):
    x = make_scene([200, 70], device, seed=3)
    seg_ptr, seg_rows, blk_tab, row_patch = (t.cpu().numpy() for t in lists(x, 150, "hilbert"))
    assert np.diff(seg_ptr).tolist() == [100, 100, 70, 0]                       # S = ceil(270 / 150) + 2 = 4
    tab = blk_tab.reshape(-1, 2)
    assert tab.shape[0] == -(-270 // 64) + 4
    assert tab[:6].tolist() == [[0, 0], [0, 64], [1, 0], [1, 64], [2, 0], [2, 64]] and (tab[6:, 0] == -1).all()


def test_a_key_beyond_63_bits_raises_before_a_launch(device, host_layer):
    coords = torch.tensor([[0, 0, 0, 0, 0], [0, 40000, 40000, 40000, 40000], [1, 5, 5, 5, 5]]).int()
    x = ME.SparseTensor(torch.zeros(3, 1), coordinates=coords, device=device)       # depth 16, D = 4: 64 code bits
    with pytest.raises(Exception, match="63"):
        lists(x, 32, "z")
    torch.cuda.synchronize(device)


def test_a_derived_map_and_cached_lists(device, host_layer):
    """a strided (derived) map carries no bounding box: its lists equal the yardstick too; a second call returns the cached
    tensors, another order gets its own, and the manager that owns the map holds them"""
    x = make_scene([150, 90], device, seed=5)
    y = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    assert y.tensor_stride[0] == 2
    got = lists(y, 16, "hilbert_trans")
    want = row_patches(y.C.cpu().numpy(), [2, 2, 2], "hilbert_trans", 16)
    assert np.array_equal(got[3].cpu().numpy(), want)
    again = lists(y, 16, "hilbert_trans")
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, again))
    other = lists(y, 16, "hilbert")
    assert other[3].data_ptr() != got[3].data_ptr()
    if host_layer == "python":                       # the lists live in the manager's cache and go with the manager
        mgr = x.coordinate_manager._manager
        assert all(any(t is h for h in mgr.device_tensors()) for t in got + other)
        assert len(mgr._patch_rows_cache) == 2


# ---- bound ---------------------------------------------------------------------------------------------------------------------
CASES = {"edges": ([1, 31, 32, 33, 65, 150], 32), "second_block": ([200], 96)}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("order", ["hilbert", "z_trans"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_patches_stay_within_the_bound(device, host_layer, case, d, order, dtype):
    """P = 32 on instances around the patch size; P = 96 on 200 rows: patches of 66 or 67 rows, which end a few rows into
    their second 64-row block"""
    sizes, P = CASES[case]
    heads = 2
    x = make_scene(sizes, device, seed=7)
    n, c = x.F.shape[0], heads * d
    patch = lists(x, P, order)[3].long()
    counts = torch.bincount(patch).tolist()
    if case == "second_block":
        assert sorted(counts) == [66, 67, 67]
    else:
        assert sorted(counts) == sorted([1, 31, 32, 16, 17, 21, 22, 22, 30, 30, 30, 30, 30])
    q, k, v, dout = (draw(n, c, dtype, device, 10 * d + s) for s in range(4))
    r = run(x, q, k, v, dout, heads, P, order)
    within_bound(r, q, k, v, dout, patch, patch, heads, what=f"serial {case} d={d} {order} {dtype} {host_layer}")


# ---- scenes beyond one sort tile's regime: deep keys, sparse and missing batch indices, long patches ----------------------------
def scene_of(coords, device, stride=1):
    """a sparse tensor on the given unique int rows [n, 1 + D]"""
    coords = torch.as_tensor(np.asarray(coords)).int()
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1), coordinates=coords, tensor_stride=stride, device=device)
    assert x.F.shape[0] == coords.shape[0]
    return x


def check_lists(x, patch_size, order, n_batch):
    """all four outputs of patch_rows against the yardstick on the rows of the map -> the patch of every row (int64)"""
    seg_ptr, seg_rows, blk_tab, row_patch = (t.cpu().numpy() for t in lists(x, patch_size, order))
    n = x.F.shape[0]
    want = row_patches(x.C.cpu().numpy(), [int(t) for t in x.tensor_stride], order, patch_size)
    assert np.array_equal(row_patch, want), f"{int((row_patch != want).sum())} of {n} rows in another patch"
    want_lists = lists_from_row_patch(want, -(-n // patch_size) + n_batch)
    assert np.array_equal(seg_ptr, want_lists["seg_ptr"]) and np.array_equal(seg_rows, want_lists["seg_rows"])
    assert np.array_equal(blk_tab, want_lists["blk_tab"])
    return torch.from_numpy(want).to(x.F.device)


def step_within_bound(x, patch, patch_size, order, d, dtype, seed, what):
    heads = 2
    n, c = x.F.shape[0], heads * d
    q, k, v, dout = (draw(n, c, dtype, x.F.device, seed + s) for s in range(4))
    r = run(x, q, k, v, dout, heads, patch_size, order)
    within_bound(r, q, k, v, dout, patch, patch, heads, what=what)


def test_a_wide_scene(device, host_layer):
    """600 voxels in two instances spread over [0, 2^17) in x and y and [0, 64) in z: depth 17, 51 code bits, seven radix
    passes; the lists against the yardstick and one bf16 step within the bound"""
    rng = np.random.default_rng(17)
    rows = []
    for b, m in enumerate((330, 270)):
        pts = np.concatenate([rng.integers(0, 1 << 17, size=(2 * m, 2)), rng.integers(0, 64, size=(2 * m, 1))], 1)
        pts = np.unique(pts, axis=0)
        pts = pts[rng.permutation(pts.shape[0])[:m]]
        if b == 0:
            pts[0], pts[1] = (0, 0, 0), ((1 << 17) - 1, (1 << 17) - 1, 63)
        rows.append(np.concatenate([np.full((m, 1), b), pts], 1))
    coords = np.concatenate(rows)
    x = scene_of(coords[rng.permutation(600)], device)
    patch = check_lists(x, 48, "hilbert", 2)
    step_within_bound(x, patch, 48, "hilbert", 64, torch.bfloat16, 170, f"serial wide scene bf16 {host_layer}")


def test_batch_indices_with_a_gap(device, host_layer):
    """instances with the batch indices 0, 2 and 5: the instances of the lists are the ranks of the indices"""
    y = make_scene([70, 40, 90], device, seed=25)
    coords = y.C.cpu().clone()
    coords[:, 0] = torch.tensor([0, 2, 5])[coords[:, 0].long()]
    x = scene_of(coords, device)
    assert sorted(set(x.C[:, 0].tolist())) == [0, 2, 5]
    patch = check_lists(x, 32, "z_trans", 3)
    assert torch.bincount(patch).tolist() == [24, 23, 23, 20, 20, 30, 30, 30]
    step_within_bound(x, patch, 32, "z_trans", 32, torch.float32, 250, f"serial batch gap fp32 {host_layer}")


def test_an_instance_that_vanished(device, host_layer):
    """three instances, every row of instance 1 pruned away: the origin still has three instances, the map two, so n_batch
    exceeds the number of instances the sorted keys show and the last one is empty"""
    x = make_scene([80, 50, 60], device, seed=26)
    y = ME.MinkowskiPruning()(x, x.C[:, 0] != 1)
    assert y.F.shape[0] == 140 and sorted(set(y.C[:, 0].tolist())) == [0, 2]
    patch = check_lists(y, 32, "hilbert", 3)
    assert torch.bincount(patch).tolist() == [27, 27, 26, 30, 30]
    step_within_bound(y, patch, 32, "hilbert", 32, torch.float32, 260, f"serial vanished instance fp32 {host_layer}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_long_patches(device, host_layer, dtype):
    """instances of 700 and 301 rows, P = 300: patches of 233 / 234 and 150 / 151 rows, up to four 64-row blocks with the
    last one partial"""
    x = make_scene([700, 301], device, seed=27)
    patch = lists(x, 300, "hilbert")[3].long()
    assert sorted(torch.bincount(patch).tolist()) == [150, 151, 233, 233, 234]
    step_within_bound(x, patch, 300, "hilbert", 64, dtype, 270, f"serial long patches {dtype} {host_layer}")


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("order", ["z", "hilbert"])
def test_one_patch_per_instance_equals_global_attention(device, host_layer, order, dtype):
    """patch_size >= every instance: the patches are the instances, so out, lse, dq, dk, dv equal MinkowskiSelfAttention's
    operators bit for bit — the table path finds the blocks the walk finds"""
    heads, d = 2, 64
    x = make_scene([2 * BK + 2, BK - 1, 5], device, seed=12)
    n, c = x.F.shape[0], heads * d
    q, k, v, dout = (draw(n, c, dtype, device, 90 + s) for s in range(4))
    ours = run(x, q, k, v, dout, heads, 2 * BK + 2, order)
    want = run_global(x, q, k, v, dout, heads)
    for name in NAMES + ("lse",):
        assert _equal(ours[name], want[name]), name


# ---- independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_patch_does_not_see_its_neighbours(device, host_layer, dtype):
    """three patches of BK + 1 rows in one instance; the middle one holds data, the others Inf and NaN.  The middle patch
    must give bit for bit what its rows give as a scene of their own (one patch)"""
    heads, d, P = 2, 64, BK + 1
    c = heads * d
    x = make_scene([3 * P], device, seed=33)
    patch = lists(x, P, "hilbert")[3].long()
    assert torch.bincount(patch).tolist() == [P, P, P]
    mine = (patch == 1).nonzero().reshape(-1)
    qa, ka, va, da = (draw(P, c, dtype, device, 70 + s) for s in range(4))
    xa = ME.SparseTensor(torch.zeros(P, 1), coordinates=x.C[mine].cpu(), device=device)
    assert torch.equal(xa.C, x.C[mine])
    alone = run(xa, qa, ka, va, da, heads, P, "hilbert")
    bad = torch.full((3 * P, c), math.inf, dtype=dtype, device=device)
    bad[::2] = math.nan
    bad[1::4] = -math.inf
    q, k, v, dout = (bad.clone().index_put_((mine,), t) for t in (qa, ka, va, da))
    both = run(x, q, k, v, dout, heads, P, "hilbert")
    for name in NAMES + ("lse",):
        assert torch.isfinite(alone[name].float()).all()
        assert _equal(both[name][mine], alone[name]), name


# ---- reproducibility, hosts, subsets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_calls_and_two_hosts_are_bitwise_equal(device, dtype):
    heads, d, P = 2, 64, 48
    c = heads * d
    results, tables = [], []
    prev = ME.get_host()
    try:
        for layer in ("python", "native", "python"):
            ME.set_host(layer)
            x = make_scene([2 * BK + 2, BK - 1, 5], device, seed=12)
            q, k, v, dout = (draw(x.F.shape[0], c, dtype, device, 90 + s) for s in range(4))
            results.append(run(x, q, k, v, dout, heads, P, "hilbert_trans"))
            results.append(run(x, q, k, v, dout, heads, P, "hilbert_trans"))
            tables.append(lists(x, P, "hilbert_trans"))
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for name in NAMES + ("lse",):
            assert _equal(results[0][name], other[name]), name
    for other in tables[1:]:
        assert all(torch.equal(a, b) for a, b in zip(tables[0], other))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gradient_subsets(device, host_layer, dtype):
    heads, d, P = 2, 32, 40
    c = heads * d
    x = make_scene([BK + 2, 30], device, seed=8)
    q, k, v, dout = (draw(x.F.shape[0], c, dtype, device, 50 + s) for s in range(4))
    full = run(x, q, k, v, dout, heads, P, "z")
    for mask in range(1, 8):
        need = tuple(bool(mask >> i & 1) for i in range(3))
        r = run(x, q, k, v, dout, heads, P, "z", need=need)
        for name, wanted in zip(("dq", "dk", "dv"), need):
            if wanted:
                assert _equal(r[name], full[name]), (need, name)
            else:
                assert r[name] is None, (need, name)


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_the_function_in_float64(device, host_layer):
    """H = 2, d = 4, 13 rows in two instances of 7 and 6, P = 4: patches of 4, 3 and 3, 3 rows"""
    x = make_scene([7, 6], device, seed=2, lo=0, hi=6)
    patch = lists(x, 4, "hilbert")[3].long()
    assert sorted(torch.bincount(patch).tolist()) == [3, 3, 3, 4]
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(13, 8, generator=g, dtype=torch.float64).to(device).requires_grad_() for _ in range(3))

    def f(q_, k_, v_):
        return ME.MinkowskiSerializedAttentionFunction.apply(q_, k_, v_, 2, None, 4, "hilbert", x.coordinate_map_key,
                                                             x.coordinate_manager)
    assert torch.autograd.gradcheck(f, (q, k, v), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    ref = reference(q, k, v, torch.ones_like(q), patch, patch, 2)
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
def test_module_equals_multihead_attention_per_patch(device, host_layer, dtype, bias):
    embed_dim, heads, P, order = 64, 2, 48, "hilbert"
    x = make_scene([BK + 1, 37, 1, 2 * BK + 2], device, seed=4)
    n = x.F.shape[0]
    patch = lists(x, P, order)[3].long()
    torch.manual_seed(11)
    layer = ME.MinkowskiSerializedSelfAttention(embed_dim, heads, patch_size=P, order=order, bias=bias).to(device).to(dtype)
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
    ref_out, ref = _mha_per_segment(state, torch.float64, feats, dout, patch, embed_dim, heads, bias)
    their_out, theirs = _mha_per_segment(state, dtype, feats, dout, patch, embed_dim, heads, bias)
    bad = []
    for name, a, b, r in [("out", out.F.detach(), their_out, ref_out)] + [(k, ours[k], theirs[k], ref[k]) for k in ref]:
        assert a is not None and torch.isfinite(a.float()).all(), name
        e, et = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"serial module {dtype} bias={bias} {host_layer} {name}: E_layer {e:.3e}  E_torch {et:.3e}  "
              f"ratio {e / et if et else math.inf:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"beyond {FACTOR} x E_torch: {bad}"


def test_functional_and_its_errors(device, host_layer):
    heads, d = 2, 32
    x = make_scene([BK + 7, 40], device, seed=6)
    n, c = x.F.shape[0], heads * d
    mk = lambda s: ME.SparseTensor(draw(n, c, torch.float32, device, s), coordinate_map_key=x.coordinate_map_key,  # noqa: E731
                                   coordinate_manager=x.coordinate_manager)
    xq, xk, xv = mk(1), mk(2), mk(3)
    y = ME.MinkowskiFunctional.serialized_attention(xq, xk, xv, heads, 32, order="z_trans")
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == x.coordinate_map_key
    patch = lists(x, 32, "z_trans")[3].long()
    dout = torch.zeros_like(xq.F)
    ref = reference(xq.F, xk.F, xv.F, dout, patch, patch, heads)
    theirs = torch_attention(xq.F, xk.F, xv.F, dout, patch, patch, heads)
    e = float((y.F.double() - ref["out"]).abs().max())
    et = float((theirs["out"].double() - ref["out"]).abs().max())
    print(f"serial functional {host_layer}: E_layer {e:.3e}  E_torch {et:.3e}")
    assert e <= FACTOR * et
    coarse = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(xq)
    with pytest.raises(ValueError, match="one coordinate map"):
        ME.MinkowskiFunctional.serialized_attention(coarse, xk, xv, heads, 32)
    with pytest.raises(ValueError, match="order"):
        ME.MinkowskiFunctional.serialized_attention(xq, xk, xv, heads, 32, order="peano")
    with pytest.raises(ValueError, match="patch_size"):
        ME.MinkowskiFunctional.serialized_attention(xq, xk, xv, heads, 0)
    with pytest.raises(ValueError, match="head dimension"):
        ME.MinkowskiFunctional.serialized_attention(xq, xk, xv, 4, 32)
    field = ME.TensorField(torch.randn(3, 64), coordinates=torch.tensor([[0, 0.2, 0.1, 0.0], [0, 1.4, 0.3, 0.2],
                                                                         [1, 0.1, 2.2, 0.5]]), device=device)
    with pytest.raises(TypeError, match="SparseTensor.*TensorField"):
        ME.MinkowskiSerializedSelfAttention(64, 2).to(device)(field)
    torch.cuda.synchronize(device)


def test_the_examples_block_runs(device, host_layer):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import serialized_attention_block as SB
    g = torch.Generator().manual_seed(0)
    pts = torch.unique(torch.randint(0, 24, (1500, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(device)
    x = ME.SparseTensor(torch.randn(coords.shape[0], 64, generator=g).to(device), coords)
    stage = SB.SerializedStage(64, 2, depth=4, patch_size=64).to(device)
    out = stage(x)
    assert tuple(out.F.shape) == tuple(x.F.shape) and out.coordinate_map_key == x.coordinate_map_key
    out.F.square().mean().backward()
    norm = float(stage.blocks[3].attn.in_proj_weight.grad.norm())
    assert math.isfinite(norm) and norm > 0
