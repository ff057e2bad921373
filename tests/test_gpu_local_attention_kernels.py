"""Operator-level tests of the local attention kernels (csrc/local_attention.hip) through LocalAttentionForwardGPU /
LocalAttentionBackwardGPU of both host layers.

Yardstick (`yardstick`): the torch gather formulation in float64 — gather k[nbr], v[nbr] to [N, K, H, d], -inf at the
holes, softmax, einsum, autograd for dq, dk, dv and the gradient of the bias.  The neighbour table comes from the
coordinate manager's public kernel_map; no expected value comes from a kernel (tests/test_local_attention_cpu.py checks the
yardstick itself against a plain Python loop over a coordinate dictionary).  Exact cases (uniform weights, one-hot
attention, isolated voxels) are the lane-map checks: integer data and asymmetric operands, so a permuted lane group cannot
pass.  Bitwise cases (holes, strided operands, reproducibility, gradient subsets, host layers) compare two runs of the
kernels.

Error bound for fp32 and bf16 (`within_bound`), the rule of tests/test_gpu_attention_kernels.py: E_torch is the maximum
absolute error, against the float64 result, of the SAME torch formulation run in the dtype under test; the kernels must stay
within FACTOR * E_torch per tensor (out, dq, dk, dv, dbias).  Every figure is printed before it is asserted (pytest -s)."""
import itertools
import math

import pytest
import torch

import minkowskiengine_amd as ME

pytestmark = pytest.mark.gpu

# The kernels add the K terms of a row in ascending k with an online softmax, torch in one pass with its own reduction
# order, and on draws of a few hundred rows the error of either fluctuates by about a factor of two: 4 covers both (the
# reasoning and the constant of tests/test_gpu_attention_kernels.py).  The measured maxima are in DESIGN 8.12.
FACTOR = 4.0
DTYPES = (torch.float32, torch.bfloat16)
NAMES = ("out", "dq", "dk", "dv", "dbias")


# ---- scenes -----------------------------------------------------------------------------------------------------------
class Scene:
    """a key / value map, a query map of the same manager and the kernel generator between them"""

    def __init__(self, coords, device, gen=None, stride=1, dimension=3, **kw):
        coords = torch.as_tensor(coords).int()
        x = ME.SparseTensor(torch.zeros(coords.shape[0], 1), coordinates=coords, device=device)
        assert x.F.shape[0] == coords.shape[0], "the scene's coordinates must be unique"
        self.mgr = x.coordinate_manager
        self.kv_key = x.coordinate_map_key
        self.q_key = self.mgr.stride(self.kv_key, stride) if stride != 1 else self.kv_key
        self.gen = gen or ME.KernelGenerator(stride=stride, dimension=dimension, **kw)
        self.n_in, self.n_out = coords.shape[0], self.mgr.size(self.q_key)
        self.device = device

    def table(self):
        """int64 [K, n_out]: the in row of offset k of out row i or -1, from the manager's pair lists"""
        g = self.gen
        custom = g.region_type == ME.RegionType.CUSTOM
        km = self.mgr.kernel_map(self.kv_key, self.q_key, stride=g.kernel_stride, kernel_size=g.kernel_size,
                                 dilation=g.kernel_dilation, region_type=g.region_type,
                                 region_offset=g.region_offsets if custom else None, is_pool=True)
        nbr = torch.full((g.kernel_volume, self.n_out), -1, dtype=torch.int64, device=self.device)
        for k, pairs in km.items():
            nbr[int(k), pairs[1].long()] = pairs[0].long()
        return nbr


def batched(points, b=0):
    points = torch.as_tensor(points)
    return torch.cat([torch.full((points.shape[0], 1), b), points], 1)


def box(*sides):
    return torch.cartesian_prod(*[torch.arange(s) for s in sides]).reshape(-1, len(sides))


def scattered(n, side, seed, dims=3):
    g = torch.Generator().manual_seed(seed)
    pts = torch.unique(torch.randint(0, side, (4 * n, dims), generator=g), dim=0)
    return pts[torch.randperm(pts.shape[0], generator=g)][:n]


def draw(n, c, dtype, device, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    return (amp * torch.randn(n, c, generator=g)).to(dtype).to(device)


def operands(sc, heads, d, dtype, seed=0, amp=1.0, bias=True):
    c = heads * d
    q, dout = draw(sc.n_out, c, dtype, sc.device, seed, amp), draw(sc.n_out, c, dtype, sc.device, seed + 3)
    k, v = draw(sc.n_in, c, dtype, sc.device, seed + 1, amp), draw(sc.n_in, c, dtype, sc.device, seed + 2)
    b = draw(heads, sc.gen.kernel_volume, torch.float32, sc.device, seed + 4) if bias else None
    return q, k, v, dout, b


# ---- the operators ------------------------------------------------------------------------------------------------------
def run(sc, q, k, v, dout, heads, bias=None, scale=None, need=(True, True, True, True), backward=True):
    """forward (+ backward) through the operators of the current host -> dict of device tensors"""
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    g, mgr = sc.gen, sc.mgr._manager
    region = (g.kernel_size, g.kernel_stride, g.kernel_dilation, g.region_type, g.region_offsets)
    fw = ME.get_minkowski_function("LocalAttentionForward", q, sc.q_key)
    bw = ME.get_minkowski_function("LocalAttentionBackward", q, sc.q_key)
    out, lse = fw(q, k, v, bias, heads, scale, *region, sc.q_key, sc.kv_key, mgr)
    assert tuple(lse.shape) == (2, q.shape[0], heads)                      # the log-sum-exp and the residual of its rounding
    res = dict(out=out, lse=lse[0], lse_lo=lse[1])
    if backward:
        res["dq"], res["dk"], res["dv"], res["dbias"] = bw(
            q, k, v, bias, out, lse, dout, heads, scale, *region, sc.q_key, sc.kv_key, mgr, need_grad_q=need[0],
            need_grad_k=need[1], need_grad_v=need[2], need_grad_bias=need[3])
    return res


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def yardstick(q, k, v, dout, nbr, heads, bias=None, scale=None, dtype=torch.float64):
    """the torch gather formulation in `dtype`: k[nbr], v[nbr] as [N, K, H, d], -inf at the holes, softmax, einsum, and
    autograd for the gradients; a row without a neighbour gives zeros and lse = -inf"""
    n, c = q.shape
    d = c // heads
    vol = nbr.shape[0]
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    q_, k_, v_ = (t.detach().to(dtype).requires_grad_() for t in (q, k, v))
    b_ = bias.detach().to(dtype).requires_grad_() if bias is not None else None
    idx, hole = nbr.clamp(min=0).t(), (nbr < 0).t()                       # [N, K]
    kg, vg = k_[idx].view(n, vol, heads, d), v_[idx].view(n, vol, heads, d)
    s = torch.einsum("nhd,nkhd->nhk", q_.view(n, heads, d), kg) * scale
    if b_ is not None:
        s = s + b_[None]
    masked = s.masked_fill(hole[:, None, :], -math.inf)
    lse = torch.logsumexp(masked.detach().double(), -1)
    empty = hole.all(1)[:, None, None]
    p = torch.softmax(masked.masked_fill(empty, 0.0), -1).masked_fill(hole[:, None, :], 0.0)
    out = torch.einsum("nhk,nkhd->nhd", p, vg).reshape(n, c)
    res = dict(out=out.detach(), lse=lse)
    if dout is not None:
        out.backward(dout.to(dtype))
        z = torch.zeros_like
        res.update(dq=q_.grad if q_.grad is not None else z(q_), dk=k_.grad if k_.grad is not None else z(k_),
                   dv=v_.grad if v_.grad is not None else z(v_))
        if b_ is not None:
            res["dbias"] = b_.grad if b_.grad is not None else z(b_)
    return res


def within_bound(ours, sc, q, k, v, dout, heads, bias=None, scale=None, what=""):
    nbr = sc.table()
    ref = yardstick(q, k, v, dout, nbr, heads, bias, scale)
    theirs = yardstick(q, k, v, dout, nbr, heads, bias, scale, dtype=q.dtype)
    bad = []
    for name in NAMES:
        if name not in ref:
            continue
        assert torch.isfinite(ours[name].float()).all(), f"{what} {name}: not finite"
        e = float((ours[name].double() - ref[name]).abs().max())
        et = float((theirs[name].double() - ref[name]).abs().max())
        ratio = e / et if et > 0 else float("inf") if e > 0 else 0.0
        print(f"{what} {q.dtype} {name}: E_kernel {e:.3e}  E_torch {et:.3e}  ratio {ratio:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    finite = torch.isfinite(ref["lse"])
    assert torch.equal(torch.isfinite(ours["lse"]), finite), f"{what}: lse is -inf on other rows than the yardstick's"
    if finite.any():
        err = float((ours["lse"].double()[finite] - ref["lse"][finite]).abs().max())
        assert err <= 1e-5 * max(1.0, float(ref["lse"][finite].abs().max())), f"{what}: lse off by {err}"
    assert not bad, f"{what}: beyond {FACTOR} x E_torch: {bad}"
    return ref


# ---- 1. exact data: the lane-map checks -----------------------------------------------------------------------------------
def pow2_scene(device):
    """a 2x2x2 cube (8 neighbours a row), a 2x2 plate (4), a pair (2) and a single voxel (1), far from each other"""
    pts = torch.cat([box(2, 2, 2), box(2, 2, 1) + torch.tensor([10, 0, 0]), box(2, 1, 1) + torch.tensor([20, 0, 0]),
                     box(1, 1, 1) + torch.tensor([30, 0, 0])])
    return Scene(batched(pts), device, kernel_size=3)


def integers(n, c, dtype, device, a=7, b=3, m=17):
    rows, cols = torch.arange(n, device=device)[:, None], torch.arange(c, device=device)[None]
    return ((rows * a + cols * b) % m).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_uniform_weights_give_the_neighbour_mean_exactly(device, host_layer, d, heads, dtype):
    """q = k = 0 without bias: every weight is 1 / count.  v = small asymmetric integers and counts 8, 4, 2, 1: the mean is
    exact in fp32, so out must EQUAL it (rounded once to the row dtype)."""
    sc = pow2_scene(device)
    nbr = sc.table()
    count = (nbr >= 0).sum(0)
    assert sorted(set(count.tolist())) == [1, 2, 4, 8]
    c = heads * d
    v = integers(sc.n_in, c, dtype, device)
    q = torch.zeros(sc.n_out, c, dtype=dtype, device=device)
    r = run(sc, q, q.clone(), v, None, heads, backward=False)
    gathered = v.float()[nbr.clamp(min=0)] * (nbr >= 0)[:, :, None]       # [K, N, C]
    want = (gathered.sum(0) / count[:, None]).to(dtype)
    assert torch.equal(r["out"], want)
    assert float((r["lse"] - count.float().log()[:, None]).abs().max()) <= 1e-6       # log(count): every score is 0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_a_large_bias_gives_one_hot_attention_bitwise(device, host_layer, d, heads, dtype):
    """bias 1e4 on one offset of every head (another one per head): exp of every other term underflows to 0, so a row that
    has this neighbour returns its v BITWISE, whatever q and k hold"""
    sc = Scene(batched(torch.cat([box(3, 3, 2), scattered(20, 6, 1) + torch.tensor([8, 0, 0])])), device, kernel_size=3)
    nbr = sc.table()
    c = heads * d
    q, k = integers(sc.n_out, c, dtype, device, 5, 2, 7) - 3, integers(sc.n_in, c, dtype, device, 3, 5, 5) - 2
    v = integers(sc.n_in, c, dtype, device)
    some = ((nbr >= 0).sum(1) > 0).nonzero().reshape(-1)                    # offsets that some row has
    hot = [int(some[(2 * h + 1) % some.numel()]) for h in range(heads)]
    bias = torch.zeros(heads, nbr.shape[0], device=device)
    for h, kk in enumerate(hot):
        bias[h, kk] = 1e4
    r = run(sc, q, k, v, None, heads, bias=bias, backward=False)
    checked = 0
    for h, kk in enumerate(hot):
        rows = (nbr[kk] >= 0).nonzero().reshape(-1)
        checked += rows.numel()
        assert torch.equal(r["out"][rows, h * d:(h + 1) * d], v[nbr[kk, rows], h * d:(h + 1) * d]), (h, kk)
    assert checked > 0


# ---- 2. isolated voxels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d,heads", [(8, 3), (32, 2), (128, 1)])
def test_isolated_voxels_return_their_own_value(device, host_layer, d, heads, dtype):
    """only the centre offset has a row: p = 1, so out == v, dv == dout BITWISE and dq == dk == dbias == 0 EXACTLY (delta
    and dp are the same chain of operations on the same lanes)"""
    sc = Scene(batched(scattered(70, 12, 2) * 5), device, kernel_size=3)
    assert int((sc.table() >= 0).sum()) == sc.n_out
    q, k, v, dout, bias = operands(sc, heads, d, dtype, seed=d)
    r = run(sc, q, k, v, dout, heads, bias=bias)
    assert torch.equal(r["out"], v)
    assert torch.equal(r["dv"], dout)
    for name in ("dq", "dk", "dbias"):
        assert torch.count_nonzero(r[name]) == 0, name


# ---- 3. edge scenes -------------------------------------------------------------------------------------------------------
def two_instances(device):
    g = torch.Generator().manual_seed(5)
    c = torch.cat([batched(scattered(150, 6, 3), 0), batched(scattered(120, 6, 4), 1)])
    return Scene(c[torch.randperm(c.shape[0], generator=g)], device, kernel_size=3)


def custom_no_origin(device, stride=1):
    offsets = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1]]
    pts = torch.cat([torch.zeros(1, 3, dtype=torch.long), scattered(200, 9, 6)])
    pts = torch.unique(pts, dim=0)                                          # (0, 0, 0) stays row 0
    gen = ME.KernelGenerator(stride=stride, region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=3)
    return Scene(batched(pts), device, gen=gen, stride=stride)


EDGE_SCENES = {
    "block5": lambda dev: Scene(batched(torch.cat([box(5, 5, 5), scattered(40, 8, 7) + torch.tensor([9, 0, 0])])), dev,
                                kernel_size=3),
    "two_instances": two_instances,
    "n63": lambda dev: Scene(batched(box(4, 4, 4)[:63]), dev, kernel_size=3),
    "n65": lambda dev: Scene(batched(box(5, 4, 4)[:65]), dev, kernel_size=3),
    "n255": lambda dev: Scene(batched(box(8, 8, 4)[:255]), dev, kernel_size=3),
    "n257": lambda dev: Scene(batched(box(8, 8, 5)[:257]), dev, kernel_size=3),
    "volume1": lambda dev: Scene(batched(scattered(130, 6, 8)), dev, kernel_size=1),
    "k2s2": lambda dev: Scene(batched(scattered(300, 8, 9)), dev, stride=2, kernel_size=2),
    "k3s2": lambda dev: Scene(batched(scattered(300, 8, 10)), dev, stride=2, kernel_size=3),
    "dilation2": lambda dev: Scene(batched(scattered(250, 7, 11)), dev, kernel_size=3, dilation=2),
    "custom_no_origin": custom_no_origin,
    "4d_81": lambda dev: Scene(batched(scattered(150, 4, 12, dims=4)), dev, dimension=4, kernel_size=3),
}
# (heads, d): the rows n63 .. n257 with one head of 32 are one less / one more than a multiple of the items of a wave
# (8 fp32, 16 bf16) and of a workgroup (32 fp32, 64 bf16), and of the 256 threads themselves
EDGE_SHAPES = {"n63": (1, 32), "n65": (1, 32), "n255": (1, 8), "n257": (1, 8), "4d_81": (2, 16), "block5": (2, 64),
               "two_instances": (3, 32)}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", list(EDGE_SCENES))
def test_edge_scenes_stay_within_the_bound(device, host_layer, name, dtype):
    sc = EDGE_SCENES[name](device)
    heads, d = EDGE_SHAPES.get(name, (2, 32))
    nbr = sc.table()
    if name == "block5":
        assert int((nbr >= 0).sum(0).max()) == 27
    if name == "4d_81":
        assert nbr.shape[0] == 81
    q, k, v, dout, bias = operands(sc, heads, d, dtype, seed=len(name))
    r = run(sc, q, k, v, dout, heads, bias=bias)
    within_bound(r, sc, q, k, v, dout, heads, bias, what=name)
    empty = (nbr < 0).all(0)
    if name == "custom_no_origin":
        assert 0 < int(empty.sum()) < sc.n_out
    if empty.any():                                                         # zero row, lse = -inf, zero gradient
        assert torch.count_nonzero(r["out"][empty]) == 0 and torch.count_nonzero(r["dq"][empty]) == 0
        assert bool((r["lse"][empty] == -math.inf).all())


# ---- 4. large logits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_large_logits_stay_finite_and_within_the_bound(device, host_layer, dtype):
    sc = two_instances(device)
    heads, d = 2, 32
    q, k, v, dout, bias = operands(sc, heads, d, dtype, seed=21, amp=16.0)
    ref = yardstick(q, k, v, None, sc.table(), heads, bias)
    assert float(ref["lse"][torch.isfinite(ref["lse"])].abs().max()) > 200
    r = run(sc, q, k, v, dout, heads, bias=bias)
    within_bound(r, sc, q, k, v, dout, heads, bias, what="large logits")


# ---- 5. holes are never read as values --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("poison", [math.nan, math.inf])
def test_rows_that_no_query_sees_are_never_read_as_values(device, host_layer, poison, dtype):
    """stride 2 with a CUSTOM list without the origin: some in rows (row 0, which every hole is clamped to, among them) are
    seen by no query.  NaN / Inf in their k and v rows changes no bit of any output"""
    sc = custom_no_origin(device, stride=2)
    nbr = sc.table()
    seen = torch.zeros(sc.n_in, dtype=torch.bool, device=device)
    seen[nbr[nbr >= 0]] = True
    assert not bool(seen[0]) and 0 < int(seen.sum()) < sc.n_in
    heads, d = 2, 32
    q, k, v, dout, bias = operands(sc, heads, d, dtype, seed=31)
    k[~seen], v[~seen] = 0.0, 0.0
    clean = run(sc, q, k, v, dout, heads, bias=bias)
    k[~seen], v[~seen] = poison, poison
    dirty = run(sc, q, k, v, dout, heads, bias=bias)
    for name in ("out", "lse", "lse_lo") + NAMES[1:]:
        assert torch.equal(clean[name], dirty[name]), name
    assert torch.count_nonzero(dirty["dk"][~seen]) == 0 and torch.count_nonzero(dirty["dv"][~seen]) == 0


# ---- 6. strided operands --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_column_views_of_one_projection_equal_contiguous_copies(device, host_layer, dtype):
    sc = two_instances(device)
    heads, d = 2, 32
    c = heads * d
    qkv = draw(sc.n_in, 3 * c, dtype, device, 41)
    dout, bias = draw(sc.n_out, c, dtype, device, 42), draw(heads, 27, torch.float32, device, 43)
    views = (qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:])
    assert not views[1].is_contiguous()
    a = run(sc, *views, dout, heads, bias=bias)
    b = run(sc, *(t.contiguous() for t in views), dout, heads, bias=bias)
    for name in ("out", "lse", "lse_lo") + NAMES[1:]:
        assert torch.equal(a[name], b[name]), name


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_runs_and_every_gradient_subset_give_the_same_bits(device, host_layer, dtype):
    sc = EDGE_SCENES["k3s2"](device)
    heads, d = 3, 16
    q, k, v, dout, bias = operands(sc, heads, d, dtype, seed=51)
    first = run(sc, q, k, v, dout, heads, bias=bias)
    again = run(sc, q, k, v, dout, heads, bias=bias)
    for name in ("out", "lse", "lse_lo") + NAMES[1:]:
        assert torch.equal(first[name], again[name]), name
    for need in itertools.product((False, True), repeat=4):
        r = run(sc, q, k, v, dout, heads, bias=bias, need=need)
        for want, name in zip(need, NAMES[1:]):
            if want:
                assert torch.equal(r[name], first[name]), (need, name)
            else:
                assert r[name] is None, (need, name)


# ---- 8. host layers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + (torch.float64,), ids=str)
def test_python_and_native_host_layers_give_the_same_bits(device, dtype):
    from minkowskiengine_amd import host
    assert host.native_module() is not None, host.native_error()
    prev = ME.get_host()
    res = {}
    try:
        for layer in ("python", "native"):
            ME.set_host(layer)
            sc = EDGE_SCENES["k3s2"](device)
            q, k, v, dout, bias = operands(sc, 2, 32, dtype, seed=61)
            res[layer] = run(sc, q, k, v, dout, 2, bias=bias)
    finally:
        ME.set_host(prev)
    for name in ("out", "lse", "lse_lo") + NAMES[1:]:
        assert torch.equal(res["python"][name], res["native"][name]), name


def test_float64_twins_match_the_yardstick(device, host_layer):
    """the plain-double kernels behind gradcheck, any head dimension (5 here), bias included"""
    sc = custom_no_origin(device)
    heads, d = 2, 5
    q, k, v, dout, bias = operands(sc, heads, d, torch.float64, seed=71)
    r = run(sc, q, k, v, dout, heads, bias=bias.double())
    ref = yardstick(q, k, v, dout, sc.table(), heads, bias.double())
    for name in NAMES:
        assert float((r[name] - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max())), name
    finite = torch.isfinite(ref["lse"])
    assert torch.equal(torch.isfinite(r["lse"]), finite)
    assert float((r["lse"][finite] - ref["lse"][finite]).abs().max()) <= 1e-12
