"""Local attention over a kernel map (csrc/local_attention.hip): time per call of MinkowskiLocalAttentionFunction next to
the torch gather formulation a user writes without it, forward and forward + backward with all gradients (q, k, v and the
bias table) through autograd, in one process on one GPU.

    python scripts/local_attention_bench.py [--shape 100k] [--dtype bf16] [--iters 50] [--json out.jsonl]

Protocol of scripts/attention_bench.py: 10 warm-up calls, then `iters` calls between two device events.  One exception:
a torch call that takes longer than 50 ms (the bf16 autograd backward of the gather takes seconds) is timed with 2 warm-up
and 5 timed calls, and the row says so (`gather_step_calls`).
  ours    MinkowskiLocalAttentionFunction on q, k, v [N, C] and rel_pos_bias [H, 27] (the kernel map and its two dense
          tables are cached in the manager after the first call)
  gather  the torch formulation on the SAME table in the same run: k[nbr], v[nbr] as [N, 27, H, d], -inf at the holes,
          softmax, two einsums; autograd backward (index_add_ atomics).  The table is built outside the timed region.
Layouts: rows in coordinate order and rows shuffled.  Dtypes: bf16 and fp32.  Shapes (kernel 3x3x3 on one map, a scene of
30 % occupancy): 100k voxels x 128 channels x 4 heads; 200k x 64 x 2; 20k x 256 x 8.  The results of the two are compared
(max |difference| of out and of dq).
Derived: bytes/s of the layer against a byte model of one forward + backward step that counts q, out and their gradients
once, k and v once and the table once."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME

SHAPES = {"100k": (100000, 128, 4), "200k": (200000, 64, 2), "20k": (20000, 256, 8)}
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


SLOW_CALL_S = 0.05


def probe(fn):
    """seconds of one call after one warm-up call"""
    fn()
    return timed(fn, 1, warm=0)


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


def make_coords(n, shuffle, seed=0, occupancy=0.3):
    """n distinct voxels of one scene in a cube of the given occupancy, in coordinate order or shuffled"""
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil((n / occupancy) ** (1 / 3)))
    cells = torch.randperm(side ** 3, generator=g)[:n]
    cells = cells[torch.randperm(n, generator=g)] if shuffle else torch.sort(cells).values
    return torch.stack([torch.zeros_like(cells), cells // (side * side), cells // side % side, cells % side], 1).int()


def case(name, n, C, heads, dt, shuffle, iters, dev):
    dtype = DTYPES[dt]
    x = ME.SparseTensor(torch.zeros(n, 1), coordinates=make_coords(n, shuffle), device=dev)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    gen = ME.KernelGenerator(kernel_size=3, dimension=3)
    vol, d = gen.kernel_volume, C // heads
    q, k, v = (torch.randn(n, C, device=dev).to(dtype).requires_grad_(True) for _ in range(3))
    bias = (0.5 * torch.randn(heads, vol, device=dev)).requires_grad_(True)
    dout = torch.randn(n, C, device=dev).to(dtype)
    nbr = torch.full((vol, n), -1, dtype=torch.int64, device=dev)                 # outside the timed region
    for kk, pairs in mgr.kernel_map(key, key, kernel_size=3, is_pool=True).items():
        nbr[int(kk), pairs[1].long()] = pairs[0].long()
    idx, hole = nbr.clamp(min=0).t().contiguous(), (nbr < 0).t()[:, None, :].contiguous()
    pairs = int((nbr >= 0).sum())

    def ours():
        return ME.MinkowskiLocalAttentionFunction.apply(q, k, v, bias, heads, None, gen, key, key, mgr)

    def gather():
        s = torch.einsum("nhd,nkhd->nhk", q.view(n, heads, d), k[idx].view(n, vol, heads, d)) / math.sqrt(d)
        s = (s + bias[None].to(dtype)).masked_fill(hole, -math.inf)
        return torch.einsum("nhk,nkhd->nhd", torch.softmax(s, -1), v[idx].view(n, vol, heads, d)).reshape(n, C)

    def step(fwd):
        def run():
            q.grad = k.grad = v.grad = bias.grad = None
            fwd().backward(dout)
        return run
    fns = dict(ours=ours, gather=gather)
    res, grads = {}, {}
    for nm, fn in fns.items():
        step(fn)()
        res[nm], grads[nm] = fn().detach().float(), q.grad.float().clone()
    esz = 2 if dtype == torch.bfloat16 else 4
    model = 4 * n * C * esz + 2 * n * C * esz + vol * n * 4
    r = dict(shape=name, dtype=dt, layout="shuffled" if shuffle else "ordered", n=n, C=C, heads=heads, pairs=pairs,
             neighbours_per_row=round(pairs / n, 2), out_diff=float((res["ours"] - res["gather"]).abs().max()),
             dq_diff=float((grads["ours"] - grads["gather"]).abs().max()))
    for nm, fn in fns.items():
        with torch.no_grad():
            r[f"{nm}_fwd_us"] = round(timed(fn, iters) * 1e6, 1)
        slow = nm != "ours" and probe(step(fn)) > SLOW_CALL_S
        r[f"{nm}_step_calls"] = 5 if slow else iters
        r[f"{nm}_step_us"] = round((timed(step(fn), 5, warm=2) if slow else timed(step(fn), iters)) * 1e6, 1)
    r.update(step_model_bytes=model, step_model_gbs=round(model / r["ours_step_us"] * 1e-3, 1),
             gathered_bytes=2 * pairs * C * esz,
             gather_over_ours_fwd=round(r["gather_fwd_us"] / r["ours_fwd_us"], 2),
             gather_over_ours_step=round(r["gather_step_us"] / r["ours_step_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    ap.add_argument("--dtype", choices=list(DTYPES), default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 20
    dev = torch.device("cuda:0")
    results = []
    for name, (n, C, heads) in SHAPES.items():
        for dt in DTYPES:
            if (args.shape and name != args.shape) or (args.dtype and dt != args.dtype):
                continue
            for shuffle in (False, True):
                r = case(name, n, C, heads, dt, shuffle, args.iters, dev)
                results.append(r)
                print(json.dumps(r), flush=True)
    print(f"{'shape':6s} {'dtype':5s} {'layout':8s} | fwd us: {'ours':>8s} {'gather':>8s} | fwd+bwd us: {'ours':>8s} "
          f"{'gather':>8s} | gather/ours: {'fwd':>5s} {'step':>5s} | model GB/s (step)")
    for r in results:
        print(f"{r['shape']:6s} {r['dtype']:5s} {r['layout']:8s} |         {r['ours_fwd_us']:8.1f} {r['gather_fwd_us']:8.1f} |"
              f"             {r['ours_step_us']:8.1f} {r['gather_step_us']:8.1f} |              "
              f"{r['gather_over_ours_fwd']:5.2f} {r['gather_over_ours_step']:5.2f} | {r['step_model_gbs']:8.1f}")
    if args.json:
        with open(args.json, "a") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
