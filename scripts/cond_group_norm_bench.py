"""Conditional group normalisation (the k_gnc_* kernels of csrc/group_norm.hip): time per call of
MinkowskiConditionalGroupNorm with a SiLU and a per-instance scale / shift next to MinkowskiGroupNorm alone at the same
shape and next to the chain a user writes without it — MinkowskiGroupNorm, then `F * (1 + scale[b]) + shift[b]` in torch,
then MinkowskiSiLU — forward, and forward + backward through autograd, in one process on one GPU.

    python scripts/cond_group_norm_bench.py [--iters 100] [--json out.jsonl]

Protocol of scripts/group_norm_bench.py: 10 warm-up calls, then `iters` calls between two device events.  Shapes: 2
instances of 100k rows, C in {32, 64, 256}, 8 groups, fp32 and bf16.  (a) cgn: the fused module; (b) gn: MinkowskiGroupNorm
alone (no modulation, no activation: the floor of the pass counts); (c) chain: the unfused formulation.  In the steps the
features, scale and shift require gradients."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from bench import make_scene

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
    scale = (0.5 * torch.randn(n_batch, C, device=dev)).requires_grad_(True)
    shift = torch.randn(n_batch, C, device=dev).requires_grad_(True)
    b = coords[:, 0].long().to(dev)
    cgn = ME.MinkowskiConditionalGroupNorm(GROUPS, C, eps=EPS, activation="silu").to(dev)
    gn = ME.MinkowskiGroupNorm(GROUPS, C, eps=EPS).to(dev)
    silu = ME.MinkowskiSiLU()

    def chain():
        h = gn(x)
        f = h.F * (1 + scale[b]).to(dtype) + shift[b].to(dtype)
        return silu(ME.SparseTensor(f, coordinate_map_key=h.coordinate_map_key, coordinate_manager=h.coordinate_manager)).F

    def step(fwd):
        def run():
            feats.grad = scale.grad = shift.grad = None
            fwd().backward(dy)
        return run
    fns = dict(cgn=lambda: cgn(x, scale, shift).F, gn=lambda: gn(x).F, chain=chain)
    with torch.no_grad():
        d_out = float((fns["cgn"]().float() - fns["chain"]().float()).abs().max())
    r = dict(dtype="bf16" if dtype == torch.bfloat16 else "f32", n=n, n_batch=n_batch, C=C, groups=GROUPS,
             max_abs_diff_out_vs_chain=d_out)
    for name, fn in fns.items():
        with torch.no_grad():
            r[f"{name}_fwd_us"] = round(timed(fn, iters) * 1e6, 1)
        r[f"{name}_step_us"] = round(timed(step(fn), iters) * 1e6, 1)
    r.update(cgn_over_gn_fwd=round(r["cgn_fwd_us"] / r["gn_fwd_us"], 2),
             cgn_over_gn_step=round(r["cgn_step_us"] / r["gn_step_us"], 2),
             chain_over_cgn_fwd=round(r["chain_fwd_us"] / r["cgn_fwd_us"], 2),
             chain_over_cgn_step=round(r["chain_step_us"] / r["cgn_step_us"], 2))
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
    print(f"{'dtype':5s} {'C':>4s} | fwd us: {'cgn':>7s} {'gn':>7s} {'chain':>8s} | fwd+bwd us: {'cgn':>7s} {'gn':>7s} "
          f"{'chain':>8s} | cgn/gn: {'fwd':>5s} {'step':>5s} | chain/cgn: {'fwd':>5s} {'step':>5s}")
    for r in results:
        print(f"{r['dtype']:5s} {r['C']:4d} |         {r['cgn_fwd_us']:7.1f} {r['gn_fwd_us']:7.1f} {r['chain_fwd_us']:8.1f} |"
              f"             {r['cgn_step_us']:7.1f} {r['gn_step_us']:7.1f} {r['chain_step_us']:8.1f} |         "
              f"{r['cgn_over_gn_fwd']:5.2f} {r['cgn_over_gn_step']:5.2f} |            {r['chain_over_cgn_fwd']:5.2f} "
              f"{r['chain_over_cgn_step']:5.2f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
