"""Arithmetic between sparse tensors on different coordinate maps (csrc/union_arith.hip): time per call of `a (op) b`
on 200k rows x 96 channels, fp32 and bf16, against a byte model and against the reference's formulation computed with
torch on the same row tables in the same run.

    python scripts/arith_bench.py [--iters 30] [--json out.jsonl]

Two pairs: "sparse" (a and b of 200k rows each, about half of them shared: 300k union rows) and "nested" (b = 100k of
a's 200k rows).  Per pair, dtype and operator: the cached call (union map and row tables already in the manager: what
every call after the first costs), forward and forward + backward.  torch: the reference's five steps
(MinkowskiTensor.py:531-537: zero fill, indexed write of a, gather of the union rows of b, the operator, indexed write)
on the union maps of the same manager, under autograd for the backward.
Byte model of the forward: (Na + Nb + Nu) * C * sizeof + 8 * Nu; fraction of 6.3 TB/s.
The first call on a pair (coordinate insert of Na + Nb rows, the four row tables, then the kernel) is reported apart,
as the median wall time of three fresh managers."""
import argparse
import json
import operator
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from field_bench import HBM, timed

OPS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul, "div": operator.truediv}


def clouds(kind, n, g):
    """two coordinate sets of one batch on a 120^3 grid"""
    pool = torch.unique(torch.randint(0, 120, (int(2.2 * n), 3), generator=g), dim=0)
    pool = pool[torch.randperm(pool.shape[0], generator=g)]
    assert pool.shape[0] >= n + n // 2
    if kind == "sparse":
        a, b = pool[:n], pool[n // 2:n + n // 2]
    else:
        a, b = pool[:n], pool[torch.randperm(n, generator=g)[:n // 2]]
    b = b[torch.randperm(b.shape[0], generator=g)]
    bat = lambda p: torch.cat([torch.zeros(p.shape[0], 1, dtype=torch.long), p], 1).int().contiguous()
    return bat(a), bat(b)


def torch_formulation(fa, fb, ma, mb, n_out, fn):
    out = torch.zeros((n_out, fa.shape[1]), dtype=fa.dtype, device=fa.device)
    out[ma[1]] = fa[ma[0]]
    out[mb[1]] = fn(out[mb[1]], fb[mb[0]])
    return out


def case(kind, n, C, dtype, iters, dev, rows, g):
    e = 2 if dtype == torch.bfloat16 else 4
    ca, cb = clouds(kind, n, g)
    fa = torch.randn(ca.shape[0], C, generator=g).to(dtype).to(dev).requires_grad_(True)
    fb = (torch.rand(cb.shape[0], C, generator=g) + 0.5).to(dtype).to(dev).requires_grad_(True)
    ca, cb = ca.to(dev), cb.to(dev)

    def fresh():
        a = ME.SparseTensor(fa, ca)
        return a, ME.SparseTensor(fb, cb, coordinate_manager=a.coordinate_manager)

    first = []
    for _ in range(3):                      # the one-off cost: union map + row tables + the kernel
        a, b = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = a + b
        torch.cuda.synchronize()
        first.append(time.perf_counter() - t0)
    n_out = len(s)
    mgr = a.coordinate_manager
    ma, mb = mgr.union_map([a.coordinate_map_key, b.coordinate_map_key], ME.CoordinateMapKey(4))
    go = torch.rand(n_out, C, device=dev).to(dtype)
    nbytes = (ca.shape[0] + cb.shape[0] + n_out) * C * e + 8 * n_out
    head = dict(pair=kind, Na=ca.shape[0], Nb=cb.shape[0], Nu=n_out, C=C, dtype=str(dtype).split(".")[-1])
    r = dict(head, op="first call (map build + tables + add)", us=round(statistics.median(first) * 1e6, 1))
    rows.append(r)
    print(json.dumps(r), flush=True)
    for name, fn in OPS.items():
        got, want = fn(a, b), torch_formulation(fa, fb, ma, mb, n_out, fn)
        assert torch.equal(got.C, mgr.get_coordinates(got.coordinate_map_key))
        assert torch.allclose(got.F.float(), want.float(), rtol=1e-2 if e == 2 else 1e-6, atol=1e-6), name

        def fused_fb():
            fa.grad = fb.grad = None
            fn(a, b).F.backward(go)

        def torch_fb():
            fa.grad = fb.grad = None
            torch_formulation(fa, fb, ma, mb, n_out, fn).backward(go)

        with torch.no_grad():
            t_f = timed(lambda: fn(a, b), iters)
            t_t = timed(lambda: torch_formulation(fa, fb, ma, mb, n_out, fn), iters)
        t_fb, t_tb = timed(fused_fb, max(3, iters // 3)), timed(torch_fb, max(3, iters // 3))
        r = dict(head, op=name, fwd_us=round(t_f * 1e6, 1), fwd_hbm_frac=round(nbytes / t_f / HBM, 3),
                 torch_fwd_us=round(t_t * 1e6, 1), fwd_bwd_us=round(t_fb * 1e6, 1), torch_fwd_bwd_us=round(t_tb * 1e6, 1))
        rows.append(r)
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps(dict(host=ME.get_host(), device=torch.cuda.get_device_name(0), rows=a.rows, C=96)), flush=True)
    g = torch.Generator().manual_seed(0)
    rows = []
    for kind in ("sparse", "nested"):
        for dt in (torch.float32, torch.bfloat16):
            case(kind, a.rows, 96, dt, a.iters, dev, rows, g)
    if a.json:
        with open(a.json, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
