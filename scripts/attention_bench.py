"""Per-instance multi-head attention (csrc/attention.hip): time per call of MinkowskiAttentionFunction next to the two torch
formulations a user writes without it, forward and forward + backward through autograd, in one process on one GPU.

    python scripts/attention_bench.py [--iters 50] [--json out.jsonl]

Protocol of scripts/cond_group_norm_bench.py: 10 warm-up calls, then `iters` calls between two device events.
  ours    MinkowskiAttentionFunction on q, k, v [N, C] (the row lists are cached in the manager after the first call)
  loop    (a) a Python loop over the instances: gather the rows, torch scaled_dot_product_attention, `cat`, scatter back.
          The index lists are built outside the timed region (the read-back of the sizes is not charged to torch).
  padded  (b) every instance padded to the longest one, one scaled_dot_product_attention with a key-padding mask
Layouts: rows grouped by instance and rows shuffled.  Dtypes: bf16 and fp32.  Shapes: 2 x 2,500 rows x 256 channels x 4
heads (a tensor-stride-16 level); 4 x 1,250 x 256 x 8; 8 instances of unequal sizes summing to 20,000 x 128 x 4 (a
tensor-stride-8 level).  The results of the three are compared (max |difference| of out and of dq).
Derived: FLOPs = 4 sum_b n_b^2 C forward (S = Q K^T and O = P V) and 14 sum_b n_b^2 C more backward (S and dP in both
kernels, dV, dK, dQ: seven products with the recomputation); TFLOP/s against the MFMA peaks of MI355X (bf16 2500, fp32
157.3 TFLOP/s); byte model: q, k, v read and out written once forward."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME

PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}
SHAPES = (("2x2500", [2500, 2500], 256, 4), ("4x1250", [1250] * 4, 256, 8),
          ("8 unequal", [5200, 4100, 3300, 2600, 2000, 1400, 900, 500], 128, 4))


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


def make_coords(sizes, shuffle, seed=0):
    """sizes[b] distinct voxels of instance b on a 3-D grid"""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for b, n in enumerate(sizes):
        side = int(math.ceil(n ** (1 / 3))) + 1
        cells = torch.randperm(side ** 3, generator=g)[:n]
        parts.append(torch.stack([torch.full((n,), b), cells // (side * side), cells // side % side, cells % side], 1))
    coords = torch.cat(parts).int()
    if shuffle:
        coords = coords[torch.randperm(coords.shape[0], generator=g)]
    return coords


def case(name, sizes, C, heads, dtype, shuffle, iters, dev):
    x = ME.SparseTensor(torch.zeros(sum(sizes), 1), coordinates=make_coords(sizes, shuffle), device=dev)
    batch = x.C[:, 0].long()
    n, d = batch.numel(), C // heads
    q, k, v = (torch.randn(n, C, device=dev).to(dtype).requires_grad_(True) for _ in range(3))
    dout = torch.randn(n, C, device=dev).to(dtype)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    rows = [(batch == b).nonzero().reshape(-1) for b in range(len(sizes))]        # outside the timed region
    longest = max(sizes)
    pad_index = torch.zeros(len(sizes), longest, dtype=torch.long, device=dev)
    pad_mask = torch.zeros(len(sizes), longest, dtype=torch.bool, device=dev)
    for b, r in enumerate(rows):
        pad_index[b, :r.numel()] = r
        pad_mask[b, :r.numel()] = True
    flat_valid = pad_mask.reshape(-1).nonzero().reshape(-1)
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def ours():
        return ME.MinkowskiAttentionFunction.apply(q, k, v, heads, None, key, key, None, mgr)

    def loop():
        outs = []
        for r in rows:
            qb, kb, vb = (t[r].view(1, r.numel(), heads, d).transpose(1, 2) for t in (q, k, v))
            outs.append(sdpa(qb, kb, vb)[0].transpose(0, 1).reshape(r.numel(), C))
        out = torch.empty_like(q)
        return out.index_copy(0, torch.cat(rows), torch.cat(outs))

    def padded():
        qb, kb, vb = (t[pad_index.reshape(-1)].view(len(sizes), longest, heads, d).transpose(1, 2) for t in (q, k, v))
        o = sdpa(qb, kb, vb, attn_mask=pad_mask[:, None, None, :]).transpose(1, 2).reshape(-1, C)
        out = torch.empty_like(q)
        return out.index_copy(0, pad_index.reshape(-1)[flat_valid], o[flat_valid])

    def step(fwd):
        def run():
            q.grad = k.grad = v.grad = None
            fwd().backward(dout)
        return run
    fns = dict(ours=ours, loop=loop, padded=padded)
    res, grads = {}, {}
    for nm, fn in fns.items():
        step(fn)()
        res[nm], grads[nm] = fn().detach().float(), q.grad.float().clone()
    pairs = float(sum(s * s for s in sizes))
    fwd_flops = 4.0 * pairs * C                         # S = Q K^T and O = P V
    step_flops = fwd_flops + 14.0 * pairs * C           # backward: S and dP twice (two kernels), dV, dK, dQ
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    r = dict(shape=name, dtype=dt, layout="shuffled" if shuffle else "grouped", n=n, C=C, heads=heads,
             out_diff_loop=float((res["ours"] - res["loop"]).abs().max()),
             out_diff_padded=float((res["ours"] - res["padded"]).abs().max()),
             dq_diff_loop=float((grads["ours"] - grads["loop"]).abs().max()),
             dq_diff_padded=float((grads["ours"] - grads["padded"]).abs().max()))
    for nm, fn in fns.items():
        with torch.no_grad():
            r[f"{nm}_fwd_us"] = round(timed(fn, iters) * 1e6, 1)
        r[f"{nm}_step_us"] = round(timed(step(fn), iters) * 1e6, 1)
    esz = 2 if dtype == torch.bfloat16 else 4
    r.update(fwd_tflops=round(fwd_flops / r["ours_fwd_us"] * 1e-6, 2),
             step_tflops=round(step_flops / r["ours_step_us"] * 1e-6, 2),
             fwd_peak_fraction=round(fwd_flops / r["ours_fwd_us"] * 1e-6 / PEAK_TFLOPS[dt], 4),
             fwd_model_bytes=4 * n * C * esz,
             fwd_model_gbs=round(4 * n * C * esz / r["ours_fwd_us"] * 1e-3, 1),
             loop_over_ours_fwd=round(r["loop_fwd_us"] / r["ours_fwd_us"], 2),
             loop_over_ours_step=round(r["loop_step_us"] / r["ours_step_us"], 2),
             padded_over_ours_fwd=round(r["padded_fwd_us"] / r["ours_fwd_us"], 2),
             padded_over_ours_step=round(r["padded_step_us"] / r["ours_step_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 20
    dev = torch.device("cuda:0")
    results = []
    for name, sizes, C, heads in SHAPES:
        for dt in (torch.bfloat16, torch.float32):
            for shuffle in (False, True):
                r = case(name, sizes, C, heads, dt, shuffle, args.iters, dev)
                results.append(r)
                print(json.dumps(r), flush=True)
    print(f"{'shape':10s} {'dtype':5s} {'layout':8s} | fwd us: {'ours':>8s} {'loop':>8s} {'padded':>8s} | fwd+bwd us: "
          f"{'ours':>8s} {'loop':>8s} {'padded':>8s} | loop/ours: {'fwd':>5s} {'step':>5s} | TF/s fwd {'step':>6s} | of peak")
    for r in results:
        print(f"{r['shape']:10s} {r['dtype']:5s} {r['layout']:8s} |         {r['ours_fwd_us']:8.1f} {r['loop_fwd_us']:8.1f} "
              f"{r['padded_fwd_us']:8.1f} |             {r['ours_step_us']:8.1f} {r['loop_step_us']:8.1f} "
              f"{r['padded_step_us']:8.1f} |            {r['loop_over_ours_fwd']:5.2f} {r['loop_over_ours_step']:5.2f} | "
              f"{r['fwd_tflops']:8.2f} {r['step_tflops']:6.2f} | {r['fwd_peak_fraction']:.4f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
