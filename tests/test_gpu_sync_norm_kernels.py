"""The two-level batch-norm entry points behind MinkowskiSyncBatchNorm (csrc/norm.hip: me_bn_local_moments,
me_bn_stats_from_moments, me_bn_backward_sums, me_bn_backward_reduce, me_bn_backward_apply) in ONE process, through
backend.py's wrappers: the "ranks" are row blocks of one matrix and their records are stacked as an all-gather would
leave them.  Checked against torch.nn.BatchNorm1d in float64 on the whole matrix with the bounds tests/test_gpu_norm.py
uses for the one-level kernels (the same arithmetic with one more merge level), and bit for bit against the one-level
kernels when there is one block."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1


def close(a, b, tol=1e-5):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


def _inputs(n, c, offset=0.0, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed + n + c)
    x = (torch.randn(n, c, generator=g) * (1.0 + torch.arange(c) % 5) + offset).to(dtype)
    gy = torch.randn(n, c, generator=g).to(dtype)
    w, b = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    return x, gy, w, b


def _reference(x64, w, b, gy64):
    bn = torch.nn.BatchNorm1d(x64.shape[1], eps=EPS, momentum=MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(w.double())
        bn.bias.copy_(b.double())
    x = x64.clone().requires_grad_(True)
    y = bn(x)
    y.backward(gy64)
    mean = x64.mean(0)
    rstd = torch.rsqrt(x64.var(0, unbiased=False) + EPS)
    return dict(mean=mean, rstd=rstd, y=y.detach(), dx=x.grad, dw=bn.weight.grad, db=bn.bias.grad,
                rm=bn.running_mean, rv=bn.running_var)


def _two_level(device, x, gy, w, b, blocks, relu=False, skip=None):
    """every block is a rank: local record -> stacked records -> merge -> apply; local sums -> stacked sums -> sum in
    rank order -> apply with the global count (on the device, as the module passes it)"""
    from minkowskiengine_amd import backend as MEB
    assert sum(blocks) == x.shape[0]
    c = x.shape[1]
    w, b = w.to(device), b.to(device)
    edges = [0]
    for r in blocks:
        edges.append(edges[-1] + r)
    cut = lambda t: [t[lo:hi].to(device).clone() for lo, hi in zip(edges[:-1], edges[1:])]   # own allocations
    xs, gs = cut(x), cut(gy)
    ss = cut(skip) if skip is not None else [None] * len(blocks)
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    nbt = torch.zeros((), dtype=torch.int64, device=device)
    records = torch.stack([MEB.bn_local_moments(xb) for xb in xs])
    counts = records[:, :2].contiguous().view(torch.int64).flatten().tolist()
    assert counts == list(blocks), "the record carries the row count as an integer"
    for rec, r in zip(records, blocks):
        if r == 0:
            assert not bool(rec.any()), "an empty rank's record is count 0, mean 0, M2 0"
    mean, rstd, n_total = MEB.bn_stats_from_moments(records, EPS, MOMENTUM, rm, rv, nbt)
    assert int(n_total) == x.shape[0] and int(nbt) == 1
    ys = []
    for xb, sb in zip(xs, ss):
        if xb.shape[0] == 0:
            ys.append(torch.empty_like(xb))
        elif sb is None:
            ys.append(MEB.bn_apply(xb, mean, rstd, w, b, relu))
        else:
            ys.append(MEB.bn_apply_residual(xb, sb, mean, rstd, w, b, relu))
    youts = [yb if (skip is not None and relu) else None for yb in ys]
    local = [MEB.bn_backward_sums(xb, gb, mean, rstd, w, b, relu, yo) for xb, gb, yo in zip(xs, gs, youts)]
    for s, r in zip(local, blocks):
        if r == 0:
            assert not bool(s.any()), "an empty rank's sums are zeros"
    sums = MEB.bn_backward_reduce(torch.stack(local))
    outs = [MEB.bn_backward_apply(xb, gb, n_total, mean, rstd, w, b, sums, relu, yo, need_dskip=skip is not None)
            for xb, gb, yo in zip(xs, gs, youts)]
    res = dict(mean=mean, rstd=rstd, y=torch.cat(ys), dx=torch.cat([o[0] for o in outs]), rm=rm, rv=rv,
               dw=torch.stack([s[1] for s in local]).sum(0), db=torch.stack([s[0] for s in local]).sum(0), sums=sums)
    if skip is not None:
        res["dskip"] = torch.cat([o[1] for o in outs])
    return res


def _assert_matches_float64(got, ref, tol):
    for k in ("mean", "rstd", "y", "dx"):
        assert close(got[k], ref[k], tol), k
    assert close(got["dw"], ref["dw"], tol * 10) and close(got["db"], ref["db"], tol * 10)
    # the rank-ordered sum of the local sums IS the gradient of the whole matrix
    assert close(got["sums"][1], ref["dw"], tol * 10) and close(got["sums"][0], ref["db"], tol * 10)
    assert close(got["rm"], ref["rm"], 1e-5) and close(got["rv"], ref["rv"], 1e-4)


@pytest.mark.parametrize("blocks", [(0, 1, 17, 3000), (3000, 0, 2)])
@pytest.mark.parametrize("c", [3, 20, 64, 96])      # scalar, 4-channel and 16-byte pieces
def test_merged_blocks_match_torch_float64(device, c, blocks):
    x, gy, w, b = _inputs(sum(blocks), c)
    ref = _reference(x.double(), w, b, gy.double())
    _assert_matches_float64(_two_level(device, x, gy, w, b, blocks), ref, 1e-5)


def test_more_ranks_than_a_wave_has_lanes(device):
    blocks = (40,) * 65
    x, gy, w, b = _inputs(sum(blocks), 20)
    ref = _reference(x.double(), w, b, gy.double())
    _assert_matches_float64(_two_level(device, x, gy, w, b, blocks), ref, 1e-5)


def test_shift_comes_from_the_first_rank_that_has_rows(device):
    """rows offset by +300 (|mean| >> std) and an EMPTY first block: with a shift of 0 taken from the empty record
    B - A^2 / N cancels; 2e-4 is test_gpu_norm's bound for the offset case (1e-7 * 300 relative to std)"""
    blocks = (0, 2000, 1000)
    x, gy, w, b = _inputs(sum(blocks), 64, offset=300.0)
    ref = _reference(x.double(), w, b, gy.double())
    _assert_matches_float64(_two_level(device, x, gy, w, b, blocks), ref, 2e-4)


def test_merged_blocks_bf16(device):
    """bf16 rows: test_batch_norm_bf16_rows' bounds (one bf16 rounding of the output: 2^-8 relative + 1e-3 of the range)"""
    blocks = (0, 9, 4000)
    g = torch.Generator().manual_seed(1)
    n, c = sum(blocks), 64
    x = (torch.randn(n, c, generator=g) * 2 + 1).bfloat16()
    w, b = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    gy = torch.randn(n, c, generator=g).bfloat16()
    ref = _reference(x.double(), w, b, gy.double())
    got = _two_level(device, x, gy, w, b, blocks)
    assert got["y"].dtype == torch.bfloat16 and got["dx"].dtype == torch.bfloat16 and got["dw"].dtype == torch.float32
    for k in ("y", "dx"):
        err = (got[k].double().cpu() - ref[k]).abs()
        assert bool((err <= 2.0 ** -8 * ref[k].abs() + 1e-3 * ref[k].abs().max()).all()), k
    assert close(got["dw"], ref["dw"], 1e-4) and close(got["db"], ref["db"], 1e-4)
    assert close(got["mean"], ref["mean"], 1e-5) and close(got["rstd"], ref["rstd"], 1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["plain", "relu", "residual"])
@pytest.mark.parametrize("n,c", [(2500, 20), (3001, 96)])
def test_one_block_is_bit_identical_to_the_one_level_kernels(device, n, c, form, dtype):
    """one rank: merging one record, summing one row of sums and applying with n_total = n must give the bits of
    bn_stats + bn_apply + bn_backward (and of their ReLU-fused and residual forms)"""
    from minkowskiengine_amd import backend as MEB
    x, gy, w, b = _inputs(n, c, dtype=dtype, seed=7)
    skip = None
    if form == "residual":
        skip = torch.randn(n, c, generator=torch.Generator().manual_seed(n)).to(dtype)
    relu = form != "plain"
    got = _two_level(device, x, gy, w, b, (n,), relu=relu, skip=skip)
    xd, gd, wd, bd = x.to(device), gy.to(device), w.to(device), b.to(device)
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    mean, rstd = MEB.bn_stats(xd, EPS, MOMENTUM, rm, rv)
    if skip is None:
        y = MEB.bn_apply(xd, mean, rstd, wd, bd, relu)
        dx, gg, gb = MEB.bn_backward(xd, gd, mean, rstd, wd, bd, relu)
    else:
        y = MEB.bn_apply_residual(xd, skip.to(device), mean, rstd, wd, bd, relu)
        dx, dskip, gg, gb = MEB.bn_backward_residual(xd, gd, y, mean, rstd, wd, bd, relu)
        assert torch.equal(got["dskip"], dskip)
        assert float((y == 0).float().mean()) > 0.2          # the ReLU does mask something
    for k, want in (("mean", mean), ("rstd", rstd), ("rm", rm), ("rv", rv), ("y", y), ("dx", dx), ("dw", gg), ("db", gb)):
        assert torch.equal(got[k], want), k
    assert torch.equal(got["sums"][1], gg) and torch.equal(got["sums"][0], gb)


def test_global_count_by_value_and_on_the_device_agree(device):
    """me_bn_backward_apply takes 1 / n from n_total — a host integer or the int64 the merge left on the device — while
    its row bound stays the block's own row count"""
    from minkowskiengine_amd import backend as MEB
    blocks = (700, 1300)
    x, gy, w, b = _inputs(sum(blocks), 32)
    got = _two_level(device, x, gy, w, b, blocks)
    xb, gb = x[:700].to(device).clone(), gy[:700].to(device).clone()
    dx, _ = MEB.bn_backward_apply(xb, gb, sum(blocks), got["mean"], got["rstd"], w.to(device), b.to(device), got["sums"])
    assert torch.equal(dx, got["dx"][:700])


def test_a_step_without_any_row_is_not_a_tracked_batch(device):
    """every rank empty: the running statistics and num_batches_tracked stay as they were, the global count is 0"""
    from minkowskiengine_amd import backend as MEB
    c = 20
    records = torch.stack([MEB.bn_local_moments(torch.empty(0, c, device=device)) for _ in range(3)])
    rm, rv = torch.full((c,), 0.25, device=device), torch.full((c,), 2.0, device=device)
    nbt = torch.full((), 7, dtype=torch.int64, device=device)
    mean, rstd, n_total = MEB.bn_stats_from_moments(records, EPS, MOMENTUM, rm, rv, nbt)
    assert int(n_total) == 0 and int(nbt) == 7
    assert bool((rm == 0.25).all()) and bool((rv == 2.0).all())
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all())


def test_merged_blocks_are_reproducible(device):
    blocks = (0, 1, 17, 3000, 40, 40)
    x, gy, w, b = _inputs(sum(blocks), 64)
    a = _two_level(device, x, gy, w, b, blocks, relu=True)
    b2 = _two_level(device, x, gy, w, b, blocks, relu=True)
    assert all(torch.equal(a[k], b2[k]) for k in a)
