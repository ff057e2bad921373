"""Forward + backward time of ONE synchronised batch-norm layer: MinkowskiSyncBatchNorm on the package's kernels
(csrc/norm.hip around one all-gather per direction) against torch.nn.SyncBatchNorm on the same rows, and the time of
the exchange alone.  Two ranks share cuda:0 and talk over gloo (RCCL refuses two ranks on one device), so the exchange
is staged through the host: the figure says what the kernels save, not what RCCL costs — that needs more than one GPU.

    python scripts/sync_bn_bench.py [--rows 200000] [--steps 50] [--warmup 10] [--log profiles/sync_bn_bench.log]

Every case (channels x dtype) is its own process group in its own child process under its own `timeout`; the cases
are chained with `&&`, so a case that fails or hangs ends the run.  One JSON line per case."""
import argparse
import json
import os
import shlex
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(32, "f32"), (96, "f32"), (32, "bf16"), (96, "bf16")]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _timed(fn, steps, warmup, barrier, sync):
    """median wall time of fn() in microseconds; every step starts from a barrier and ends with a device sync (the
    gloo exchange runs on the host: device events would miss it)"""
    out = []
    for i in range(warmup + steps):
        sync()
        barrier()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def _worker(rank, world, port, args, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import minkowskiengine_amd as ME
    from minkowskiengine_amd import distributed as D
    from minkowskiengine_amd import layers as L
    _, _, lr = D.init_from_env()
    dev = D.local_device(lr)
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    n, c = args.rows, args.channels
    g = torch.Generator().manual_seed(rank)
    i = torch.arange(n, dtype=torch.int32)
    coords = torch.stack([torch.zeros_like(i), i % 512, i // 512, torch.zeros_like(i)], 1).contiguous().to(dev)
    f = torch.randn(n, c, generator=g).to(dtype).to(dev).requires_grad_(True)
    gy = torch.randn(n, c, generator=g).to(dtype).to(dev)
    x = ME.SparseTensor(f, coords)
    ours = ME.MinkowskiSyncBatchNorm(c).to(dev).train()
    theirs = torch.nn.SyncBatchNorm(c).to(dev).train()
    sync = torch.cuda.synchronize

    def step_ours():
        f.grad = None
        ours(x).F.backward(gy)

    def step_torch():
        f.grad = None
        theirs(f).backward(gy)

    rec = torch.zeros(2 + 2 * c, device=dev)
    sums = torch.zeros(2, c, device=dev)

    def step_exchange():
        L._all_gather_rows(rec, dist.group.WORLD)
        L._all_gather_rows(sums, dist.group.WORLD)

    res = {"rows_per_rank": n, "channels": c, "dtype": args.dtype, "ranks": world, "backend": D.backend_name(),
           "ours_us": _timed(step_ours, args.steps, args.warmup, dist.barrier, sync),
           "torch_us": _timed(step_torch, args.steps, args.warmup, dist.barrier, sync),
           "exchange_us": _timed(step_exchange, args.steps, args.warmup, dist.barrier, sync)}
    if rank == 0:
        out.update(res)
    D.barrier()
    dist.destroy_process_group()


def _case(args):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), args, out), nprocs=2, join=True)
    print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v) for k, v in dict(out).items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000, help="rows per rank")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--case-timeout", type=int, default=150, help="seconds per case")
    ap.add_argument("--log", default=None, help="also append the output to this file")
    ap.add_argument("--channels", type=int, default=None, help="(child) run this one case")
    ap.add_argument("--dtype", default=None)
    args = ap.parse_args()
    if args.channels is not None:
        return _case(args)
    me = shlex.quote(os.path.abspath(__file__))
    steps = [f"timeout -k 10 {args.case_timeout} {shlex.quote(sys.executable)} {me} --rows {args.rows} "
             f"--steps {args.steps} --warmup {args.warmup} --channels {c} --dtype {d}" for c, d in CASES]
    chain = " && ".join(steps)
    if args.log:
        chain = f"set -o pipefail; ( {chain} ) 2>&1 | tee -a {shlex.quote(args.log)}"
    sys.exit(subprocess.call(["bash", "-c", chain]))


if __name__ == "__main__":
    main()
