"""MinkowskiSyncBatchNorm on the package's batch-norm kernels, with a REAL exchange: two ranks (two processes) share
cuda:0 and talk over gloo, as tests/test_gpu_distributed.py does.  Rank 0 holds 2500 rows, rank 1 holds 700; the
layer is a MinkowskiBatchNorm with fuse_relu inside a module that also calls forward_residual, converted by
convert_sync_batchnorm.  Checked against torch in float64 on the concatenated rows (synchronised statistics are the
statistics of all rows) with the bounds of tests/test_gpu_norm.py.  One spawn serves every test of this file."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, C = (2500, 700), 32
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _coords(n, batch_index):
    """n distinct voxels of one batch index, in row order"""
    i = torch.arange(n, dtype=torch.int32)
    return torch.stack([torch.full_like(i, batch_index), i % 50, i // 50, torch.zeros_like(i)], 1).contiguous()


def _data(rank, dtype):
    """features, residual branch and the two output gradients of a rank"""
    g = torch.Generator().manual_seed(70 + rank)
    n = ROWS[rank]
    return [(torch.randn(n, C, generator=g) * s + o).to(dtype) for s, o in ((2.0, 1.0), (1.0, 0.0), (1.0, 0.0), (1.0, 0.0))]


def _parameters():
    g = torch.Generator().manual_seed(5)
    return torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5


def _block(ME):
    import torch.nn as nn

    class Block(nn.Module):
        """one batch norm used twice: followed by a ReLU (fused into it), and as the tail of a residual block"""

        def __init__(self):
            super().__init__()
            self.norm = ME.MinkowskiBatchNorm(C)
            self.norm.fuse_relu = True
            self.relu = ME.MinkowskiReLU()

        def forward(self, x, x2, skip):
            mid = self.norm(x)
            out = self.relu(mid)
            return out, out is mid and bool(getattr(mid, "_rectified", False)), self.norm.forward_residual(x2, skip)

    blk = Block()
    w, b = _parameters()
    with torch.no_grad():
        blk.norm.bn.weight.copy_(w)
        blk.norm.bn.bias.copy_(b)
    return blk


def _run(ME, blk, dev, coords, x, skip, ga, gr):
    x2 = x.to(dev).requires_grad_(True)                  # (the same rows feed both uses: two leaves, two gradients)
    x = x.to(dev).requires_grad_(True)
    skip = skip.to(dev).requires_grad_(True)
    if x.shape[0] > 0:
        sx = ME.SparseTensor(x, coords.to(dev))
    else:
        # (a rank without rows: the layer reads only the feature matrix; the coordinate map of a one-voxel tensor stands
        # in, since a coordinate map cannot be empty)
        one = ME.SparseTensor(torch.zeros(1, C, device=dev, dtype=x.dtype), _coords(1, 0).to(dev))
        sx = ME.SparseTensor(x, coordinate_map_key=one.coordinate_map_key, coordinate_manager=one.coordinate_manager)
    like = lambda f: ME.SparseTensor(f, coordinate_map_key=sx.coordinate_map_key, coordinate_manager=sx.coordinate_manager)
    a, rectified, r = blk(sx, like(x2), like(skip))
    ((a.F.float() * ga.to(dev).float()).sum() + (r.F.float() * gr.to(dev).float()).sum()).backward()
    torch.cuda.synchronize()
    bn = blk.norm.bn
    return dict(a=a.F.detach().cpu(), r=r.F.detach().cpu(), dx=x.grad.cpu(), dx2=x2.grad.cpu(), dskip=skip.grad.cpu(),
                dw=bn.weight.grad.cpu(), db=bn.bias.grad.cpu(), rm=bn.running_mean.cpu().clone(),
                rv=bn.running_var.cpu().clone(), nbt=int(bn.num_batches_tracked), rectified=rectified)


def _run_plain(ME, dev, coords, x, gy, sync):
    """a layer without parameters and without running statistics (weight / bias / buffers are None all the way down)"""
    bn = ME.MinkowskiBatchNorm(C, affine=False, track_running_stats=False)
    if sync:
        bn = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(bn)
        assert isinstance(bn, ME.MinkowskiSyncBatchNorm) and bn.bn.weight is None and bn.bn.running_mean is None
    f = x.to(dev).requires_grad_(True)
    y = bn.to(dev).train()(ME.SparseTensor(f, coords.to(dev)))
    y.F.backward(gy.to(dev))
    torch.cuda.synchronize()
    return dict(y=y.F.detach().cpu(), dx=f.grad.cpu())


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import minkowskiengine_amd as ME
    from minkowskiengine_amd import distributed as D
    _, _, lr = D.init_from_env()                       # 1 GPU, 2 ranks -> gloo
    assert D.backend_name() == "gloo"
    dev = D.local_device(lr)
    for name, dtype in DTYPES.items():
        blk = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_block(ME)).to(dev).train()
        assert isinstance(blk.norm, ME.MinkowskiSyncBatchNorm) and type(blk.norm.bn) is torch.nn.SyncBatchNorm
        res = _run(ME, blk, dev, _coords(ROWS[rank], rank), *_data(rank, dtype))
        res["fuse_relu"] = blk.norm.fuse_relu
        out[f"{name}{rank}"] = res
    x, _, ga, _ = _data(rank, torch.float32)
    out[f"plain{rank}"] = _run_plain(ME, dev, _coords(ROWS[rank], rank), x, ga, sync=True)
    # one rank without rows: rank 0 passes a [0, C] matrix, rank 1 its 700 rows; and what rank 1 computes alone
    x, skip, ga, gr = _data(rank, torch.float32)
    if rank == 0:
        x, skip, ga, gr = x[:0], skip[:0], ga[:0], gr[:0]
    blk = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_block(ME)).to(dev).train()
    out[f"empty{rank}"] = _run(ME, blk, dev, _coords(x.shape[0], rank), x, skip, ga, gr)
    if rank == 1:
        out["alone1"] = _run(ME, _block(ME).to(dev).train(), dev, _coords(x.shape[0], rank), x, skip, ga, gr)
    D.barrier()
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(device):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return dict(out)


@pytest.fixture(scope="module")
def single(device):
    """the unconverted module in ONE process on the concatenated rows (batch indices 0 and 1), per dtype"""
    import minkowskiengine_amd as ME
    coords = torch.cat([_coords(ROWS[rank], rank) for rank in range(2)])
    cat = lambda dtype: [torch.cat(t) for t in zip(*[_data(rank, dtype) for rank in range(2)])]
    res = {name: _run(ME, _block(ME).to(device).train(), device, coords, *cat(dtype)) for name, dtype in DTYPES.items()}
    x, _, ga, _ = cat(torch.float32)
    res["plain"] = _run_plain(ME, device, coords, x, ga, sync=False)
    return res


def _float64(dtype):
    """relu(bn(x)) and relu(bn(x) + skip) of the concatenated rows in float64: outputs, input gradients, parameter
    gradients (both uses) and the pre-addition value z of the residual form"""
    xs, ss, gas, grs = zip(*[_data(rank, dtype) for rank in range(2)])
    x, skip = torch.cat(xs).double(), torch.cat(ss).double()
    ga, gr = torch.cat(gas).double(), torch.cat(grs).double()
    w, b = _parameters()
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(w.double())
        bn.bias.copy_(b.double())
    x1, x2, sk = x.clone().requires_grad_(True), x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    a = torch.relu(bn(x1))
    z = bn(x2)
    r = torch.relu(z + sk)
    ((a * ga).sum() + (r * gr).sum()).backward()
    return dict(a=a.detach(), r=r.detach(), z=z.detach(), dx=x1.grad, dx2=x2.grad, dskip=sk.grad, dw=bn.weight.grad,
                db=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)


def close(a, b, tol=1e-5):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


def test_conversion_keeps_fuse_relu_and_the_output_is_marked_rectified(ranks):
    for key in ("f320", "f321", "bf160", "bf161"):
        assert ranks[key]["fuse_relu"] is True and ranks[key]["rectified"] is True, key
        assert float(ranks[key]["a"].float().min()) >= 0.0


def test_both_ranks_hold_the_same_running_statistics(ranks):
    for name in DTYPES:
        r0, r1 = ranks[f"{name}0"], ranks[f"{name}1"]
        assert torch.equal(r0["rm"], r1["rm"]) and torch.equal(r0["rv"], r1["rv"]), name
        assert r0["nbt"] == 2 and r1["nbt"] == 2          # two uses of the layer per step


def test_each_rank_matches_one_process_on_the_concatenated_rows(ranks, single):
    """outputs and input gradients of each rank == MinkowskiBatchNorm in one process on all rows, on that rank's rows:
    the same kernels, statistics that differ in the last bits of the merge.  fp32: close(1e-5); bf16:
    test_batch_norm_bf16_rows' bound on EVERY element (2^-8 relative + 1e-3 of the range), plain, ReLU-fused and
    residual forms alike"""
    n0 = ROWS[0]
    for rank, rows in ((0, slice(0, n0)), (1, slice(n0, None))):
        for k in ("a", "r", "dx", "dx2", "dskip"):
            assert close(ranks[f"f32{rank}"][k], single["f32"][k][rows], 1e-5), (rank, k)
        for k in ("y", "dx"):
            assert close(ranks[f"plain{rank}"][k], single["plain"][k][rows], 1e-5), (rank, k)
        for k in ("a", "r", "dx", "dx2", "dskip"):
            got, ref = ranks[f"bf16{rank}"][k], single["bf16"][k]
            assert got.dtype == torch.bfloat16
            want = ref[rows].double()
            err = (got.double() - want).abs()
            out = err > 2.0 ** -8 * want.abs() + 1e-3 * ref.double().abs().max()
            print(f"bf16 rank {rank} {k}: {int(out.sum())} of {out.numel()} elements outside the bound, "
                  f"{int((err > 0).sum())} differ at all")
            assert not bool(out.any()), (rank, k)


def test_weight_gradients_of_the_ranks_sum_to_the_one_process_gradient(ranks, single):
    """the ranks' parameter gradients are their LOCAL sums (DistributedDataParallel averages them): together they are
    the gradient MinkowskiBatchNorm computes on all rows in one process — 10x the element bound in fp32, the fused
    test's 2e-3 in bf16, as tests/test_gpu_norm.py has them"""
    for name, tol in (("f32", 1e-4), ("bf16", 2e-3)):
        r0, r1, one = ranks[f"{name}0"], ranks[f"{name}1"], single[name]
        assert close(r0["dw"] + r1["dw"], one["dw"], tol), name
        assert close(r0["db"] + r1["db"], one["db"], tol), name
        assert close(r0["rm"], one["rm"], 1e-5) and close(r0["rv"], one["rv"], 1e-4), name


def test_layer_without_parameters_and_running_statistics(ranks):
    """affine=False, track_running_stats=False on two ranks against float64 on all rows (test_gpu_norm's 1e-5)"""
    x, _, ga, _ = [torch.cat(t).double() for t in zip(*[_data(rank, torch.float32) for rank in range(2)])]
    f = x.clone().requires_grad_(True)
    y = torch.nn.functional.batch_norm(f, None, None, None, None, True, 0.1, 1e-5)
    y.backward(ga)
    n0 = ROWS[0]
    for rank, rows in ((0, slice(0, n0)), (1, slice(n0, None))):
        assert close(ranks[f"plain{rank}"]["y"], y.detach()[rows], 1e-5), rank
        assert close(ranks[f"plain{rank}"]["dx"], f.grad[rows], 1e-5), rank


def test_two_ranks_match_float64_on_the_concatenated_rows(ranks):
    ref = _float64(torch.float32)
    n0 = ROWS[0]
    for rank, rows in ((0, slice(0, n0)), (1, slice(n0, None))):
        got = ranks[f"f32{rank}"]
        for k in ("a", "r", "dx", "dx2", "dskip"):
            assert close(got[k], ref[k][rows], 1e-5), (rank, k)
    # the ranks' weight gradients are their LOCAL sums (DistributedDataParallel averages them): together, the gradient
    assert close(ranks["f320"]["dw"] + ranks["f321"]["dw"], ref["dw"], 1e-4)
    assert close(ranks["f320"]["db"] + ranks["f321"]["db"], ref["db"], 1e-4)
    # running statistics after the two uses of the layer: global count, unbiased variance
    assert close(ranks["f320"]["rm"], ref["rm"], 1e-5) and close(ranks["f320"]["rv"], ref["rv"], 1e-4)


def test_two_ranks_bf16(ranks):
    """An extra beside test_each_rank_matches_one_process_on_the_concatenated_rows: bf16 rows against float64.  Plain form (output and input gradient): test_fused_batch_norm_relu's bf16 bounds —
    2^-7 relative + 2e-3 of the range; an element within rounding of the ReLU threshold may flip its mask: a handful.
    The residual output is rounded twice by construction — T(T(z) + skip), as the three separate operators do — so
    its bound is two roundings, 2^-8 |z| + 2^-8 |z + skip| (bf16 keeps 8 significant bits: half an ulp is up to 2^-8
    relative, test_batch_norm_bf16_rows' figure), on top of that test's 1e-3 of the range.
    The residual form takes its ReLU mask from that stored output: where |z + skip| is inside the rounding of T(z)
    (2^-8 |z|, plus the 1e-3 of the range above) the mask may legitimately differ from float64's, so the gradients of
    the residual form are compared outside that band — there without exception."""
    ref = _float64(torch.bfloat16)
    n0 = ROWS[0]
    for rank, rows in ((0, slice(0, n0)), (1, slice(n0, None))):
        got = ranks[f"bf16{rank}"]
        assert got["a"].dtype == torch.bfloat16 and got["dx"].dtype == torch.bfloat16 and got["dw"].dtype == torch.float32
        for k in ("a", "dx"):
            want = ref[k][rows]
            err = (got[k].double() - want).abs()
            n_out = int((err > 2.0 ** -7 * want.abs() + 2e-3 * ref[k].abs().max()).sum())
            print(f"bf16 rank {rank} {k}: {n_out} elements outside the bound")
            assert n_out <= 5, (rank, k)
        want, z = ref["r"][rows], ref["z"][rows]
        err = (got["r"].double() - want).abs()
        bound = 2.0 ** -8 * z.abs() + 2.0 ** -8 * want.abs() + 1e-3 * ref["r"].abs().max()
        print(f"bf16 rank {rank} r: {int((err > bound).sum())} elements outside the bound")
        assert int((err > bound).sum()) <= 5, rank
        pre = z + torch.cat([_data(q, torch.bfloat16)[1] for q in range(2)]).double()[rows]      # z + skip
        decided = pre.abs() > 2.0 ** -8 * z.abs() + 1e-3 * ref["r"].abs().max()
        assert float(decided.double().mean()) > 0.98
        for k in ("dx2", "dskip"):
            want = ref[k][rows]
            err = (got[k].double() - want).abs()
            out = (err > 2.0 ** -7 * want.abs() + 2e-3 * ref[k].abs().max()) & decided
            print(f"bf16 rank {rank} {k}: {int(out.sum())} decided elements outside the bound")
            assert not bool(out.any()), (rank, k)
    # (the parameter gradients sum over the flipped masks too: they are compared with the one-process bf16 module,
    # test_weight_gradients_of_the_ranks_sum_to_the_one_process_gradient)


def test_a_rank_without_rows_enters_the_exchange(ranks):
    """rank 0 holds no rows: both ranks finish, rank 0 ends with rank 1's statistics and zero parameter gradients, and
    rank 1 computes exactly what it computes alone (merging an empty record and adding zero sums changes no bit)"""
    e0, e1, alone = ranks["empty0"], ranks["empty1"], ranks["alone1"]
    assert e0["a"].shape == (0, C) and e0["dx"].shape == (0, C) and e0["dx2"].shape == (0, C)
    assert e0["r"].shape == (0, C) and e0["dskip"].shape == (0, C)
    assert not bool(e0["dw"].any()) and not bool(e0["db"].any())
    assert torch.equal(e0["rm"], e1["rm"]) and torch.equal(e0["rv"], e1["rv"]) and e0["nbt"] == e1["nbt"] == 2
    for k in ("a", "r", "dx", "dx2", "dskip", "dw", "db", "rm", "rv"):
        assert torch.equal(e1[k], alone[k]), k
