"""Group normalisation (csrc/group_norm.hip): time per call of MinkowskiGroupNorm next to MinkowskiInstanceNorm at the
same shape and next to the only alternative without it, a Python loop of torch.nn.functional.group_norm over
`decomposed_features` with its `cat` — forward, and forward + backward through autograd, in one process on one GPU.
The kernels alone (statistics + apply, backward) are also timed through the C ABI on the prepared batch_row table, for the
achieved bytes/s against the compulsory traffic.

    python scripts/group_norm_bench.py [--iters 100] [--json out.jsonl]

Shapes: 2 instances of 100k rows, C in {32, 64, 256}, 8 groups, fp32 and bf16.  Byte model (compulsory traffic, as
scripts/instance_norm_bench.py): forward e*n*C*3 + 8n (x read by the statistics and by the apply pass, y written, batch_row
read twice), backward e*n*C*5 + 12n; e = 4 (fp32) or 2 (bf16).  Fraction of 6.3 TB/s (achievable HBM rate of the MI355X)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib
from bench import make_scene

HBM = 6.3e12
EPS = 1e-5
GROUPS = 8


def timed(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def case(coords, C, dtype, iters, dev):
    n, n_batch = coords.shape[0], int(coords[:, 0].max()) + 1
    feats = (torch.randn(n, C, device=dev) * 0.5 + 1.0).to(dtype).requires_grad_(True)
    x = ME.SparseTensor(feats, coords.to(dev))
    dy = (torch.rand(n, C, device=dev) - 0.5).to(dtype)
    gn = ME.MinkowskiGroupNorm(GROUPS, C, eps=EPS).to(dev)
    inorm = ME.MinkowskiInstanceNorm(C).to(dev)
    w, b = gn.weight, gn.bias
    wd, bd = w.detach().to(dtype), b.detach().to(dtype)

    def loop(t):
        parts = [torch.nn.functional.group_norm(f.t()[None], GROUPS, wd, bd, EPS)[0].t() for f in t.decomposed_features]
        return torch.cat(parts, 0)

    def step(fwd):
        def run():
            feats.grad = None
            fwd().backward(dy)
        return run
    fns = dict(gn=lambda: gn(x).F, inorm=lambda: inorm(x).F, loop=lambda: loop(x))
    # parity of the module and the loop on this input (rows of a batched scene are in instance order)
    with torch.no_grad():
        d_out = float((fns["gn"]().float() - fns["loop"]().float()).abs().max())
    r = dict(dtype="bf16" if dtype == torch.bfloat16 else "f32", n=n, n_batch=n_batch, C=C, groups=GROUPS,
             max_abs_diff_out_vs_loop=d_out)
    for name, fn in fns.items():
        with torch.no_grad():
            r[f"{name}_fwd_us"] = round(timed(fn, iters) * 1e6, 1)
        r[f"{name}_step_us"] = round(timed(step(fn), iters) * 1e6, 1)
    # the kernels alone, through the C ABI
    lib = _lib.load()
    rows = coords[:, 0].contiguous().to(dev)          # the batch index of every row (int32)
    bf = 1 if dtype == torch.bfloat16 else 0
    f = feats.detach()
    ws = torch.empty(max(256, lib.me_gnorm_workspace_bytes(n, n_batch, C, GROUPS)), dtype=torch.uint8, device=dev)
    mean, rstd = torch.empty(n_batch * GROUPS, device=dev), torch.empty(n_batch * GROUPS, device=dev)
    y, dx = torch.empty_like(f), torch.empty_like(f)
    gw, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def abi_fwd():
        _lib.check(lib.me_gnorm_stats(f.data_ptr(), bf, rows.data_ptr(), n, n_batch, C, GROUPS, EPS, mean.data_ptr(),
                                      rstd.data_ptr(), ws.data_ptr(), ws.numel(), st))
        _lib.check(lib.me_gnorm_apply(f.data_ptr(), bf, rows.data_ptr(), n, n_batch, C, GROUPS, mean.data_ptr(),
                                      rstd.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), st))

    def abi_bwd():
        _lib.check(lib.me_gnorm_backward(f.data_ptr(), dy.data_ptr(), bf, rows.data_ptr(), n, n_batch, C, GROUPS,
                                         mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dx.data_ptr(), gw.data_ptr(),
                                         gb.data_ptr(), ws.data_ptr(), ws.numel(), st))
    abi_fwd()
    t_f, t_b = timed(abi_fwd, iters), timed(abi_bwd, iters)
    e = 2 if bf else 4
    by_f, by_b = e * n * C * 3 + 8 * n, e * n * C * 5 + 12 * n
    r.update(kernels_fwd_us=round(t_f * 1e6, 1), kernels_bwd_us=round(t_b * 1e6, 1),
             fwd_model_MB=round(by_f / 1e6, 1), bwd_model_MB=round(by_b / 1e6, 1),
             fwd_TBps=round(by_f / t_f / 1e12, 2), bwd_TBps=round(by_b / t_b / 1e12, 2),
             fwd_hbm_frac=round(by_f / t_f / HBM, 3), bwd_hbm_frac=round(by_b / t_b / HBM, 3),
             gn_over_inorm_fwd=round(r["gn_fwd_us"] / r["inorm_fwd_us"], 2),
             gn_over_inorm_step=round(r["gn_step_us"] / r["inorm_step_us"], 2),
             loop_over_gn_fwd=round(r["loop_fwd_us"] / r["gn_fwd_us"], 2),
             loop_over_gn_step=round(r["loop_step_us"] / r["gn_step_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    dev = torch.device("cuda:0")
    parts = []
    for b in range(2):
        pts = make_scene(100000, 70, b)
        pts[:, 0] = b
        parts.append(pts)
    coords = torch.cat(parts, 0)
    results = []
    for C in (32, 64, 256):
        for dt in (torch.float32, torch.bfloat16):
            r = case(coords, C, dt, args.iters, dev)
            results.append(r)
            print(json.dumps(r), flush=True)
    print(f"{'dtype':5s} {'C':>4s} | fwd us: {'gn':>7s} {'inorm':>7s} {'loop':>8s} | fwd+bwd us: {'gn':>7s} {'inorm':>7s} "
          f"{'loop':>8s} | kernels: {'fwd us':>7s} {'TB/s':>5s} {'bwd us':>7s} {'TB/s':>5s}")
    for r in results:
        print(f"{r['dtype']:5s} {r['C']:4d} |         {r['gn_fwd_us']:7.1f} {r['inorm_fwd_us']:7.1f} {r['loop_fwd_us']:8.1f} |"
              f"             {r['gn_step_us']:7.1f} {r['inorm_step_us']:7.1f} {r['loop_step_us']:8.1f} |          "
              f"{r['kernels_fwd_us']:7.1f} {r['fwd_TBps']:5.2f} {r['kernels_bwd_us']:7.1f} {r['bwd_TBps']:5.2f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
