"""Rotary position embedding from voxel coordinates (csrc/rope.hip): time per call in one process on one GPU of

  table    the table build (me_rope_table), which the manager does once per (map, d, base, unit, dtype)
  fwd      MinkowskiRotaryEmbeddingFunction forward on contiguous [n, C] rows
  qk       forward + backward on the fused [n, 2C] view of a projected [n, 3C] matrix with 2H heads, as the self-attention
           modules call it with rope=True
  torch    the torch formulation ON THE SAME TABLE: the pairs sliced out of a [n, H, d / 2, 2] view, four element-wise
           products, a sum, a difference and a stack (forward, and forward + backward through autograd)
  layer    MinkowskiWindowSelfAttention (windows of 8^3) forward + backward with rope off and on

    python scripts/rope_bench.py [--iters 30] [--json out.jsonl]

Protocol of scripts/window_attention_bench.py: 10 warm-up calls, then `iters` calls between two device events.  Shapes: one
scene of 100k and of 200k voxels (a quarter of the cells occupied) x 128 channels x 4 heads, bf16 and fp32.  Byte model
of an apply call: n C elem read + n C elem written + n d 4 of table; the fraction is against an HBM rate of 6.3 TB/s, the
figure the sibling scripts use (the working sets here fit the 256 MiB last-level cache, so fractions above 1 are possible)."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib

HBM = 6.3e12
C, HEADS, WINDOW = 128, 4, 8


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


def make_scene(n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil((4 * n) ** (1 / 3)))              # a quarter of the cells are occupied
    cells = torch.randperm(side ** 3, generator=g)[:n]
    coords = torch.stack([torch.zeros(n, dtype=torch.long), cells // (side * side), cells // side % side, cells % side], 1)
    return ME.SparseTensor(torch.zeros(n, 1), coordinates=coords.int(), device=dev)


def torch_rope(x, table, heads):
    """the same rotation in torch on the same (cos, sin) table [n, d / 2, 2] (fp32 arithmetic, one rounding for bf16)"""
    n, c = x.shape
    xh = x.reshape(n, heads, c // heads // 2, 2).float()
    x0, x1 = xh[..., 0], xh[..., 1]
    cs, sn = table[:, None, :, 0], table[:, None, :, 1]
    return torch.stack((x0 * cs - x1 * sn, x0 * sn + x1 * cs), -1).reshape(n, c).to(x.dtype)


def case(n, dtype, iters, dev):
    lib = _lib.load()
    x = make_scene(n, dev)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    d = C // HEADS
    elem = 2 if dtype == torch.bfloat16 else 4
    table = mgr.rope_table(key, d)
    coords = x.C.contiguous()
    scratch = torch.empty_like(table)
    unit = (ctypes.c_int32 * 3)(1, 1, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def build():
        _lib.check(lib.me_rope_table(coords.data_ptr(), n, 4, unit, d, 10000.0, 0, scratch.data_ptr(), stream))
    build()
    assert torch.equal(scratch, table)

    feats = torch.randn(n, C, device=dev).to(dtype)
    qkv = torch.randn(n, 3 * C, device=dev).to(dtype).requires_grad_(True)
    dout = torch.randn(n, 2 * C, device=dev).to(dtype)
    fn = ME.MinkowskiRotaryEmbeddingFunction

    def fwd():
        return fn.apply(feats, HEADS, 10000.0, None, key, mgr)

    def fwd_torch():
        return torch_rope(feats, table, HEADS)

    def qk_step():
        qkv.grad = None
        fn.apply(qkv[:, :2 * C], 2 * HEADS, 10000.0, None, key, mgr).backward(dout)

    def qk_step_torch():
        qkv.grad = None
        torch_rope(qkv[:, :2 * C], table, 2 * HEADS).backward(dout)

    diff = float((fwd().float() - fwd_torch().float()).abs().max())
    layers = {}
    for rope in (False, True):
        torch.manual_seed(0)
        layers[rope] = ME.MinkowskiWindowSelfAttention(C, HEADS, window_size=WINDOW, rope=rope).to(dev).to(dtype)
    lin = torch.randn(n, C, device=dev).to(dtype).requires_grad_(True)
    lout = torch.randn(n, C, device=dev).to(dtype)

    def layer_step(rope):
        def run():
            lin.grad = None
            layers[rope].zero_grad(set_to_none=True)
            out = layers[rope](ME.SparseTensor(lin, coordinate_map_key=key, coordinate_manager=mgr))
            out.F.backward(lout)
        return run

    r = dict(n=n, dtype="bf16" if dtype == torch.bfloat16 else "f32", C=C, heads=HEADS, d=d, fwd_diff_torch=diff,
             table_us=round(timed(build, iters) * 1e6, 1),
             fwd_us=round(timed(fwd, iters) * 1e6, 1), torch_fwd_us=round(timed(fwd_torch, iters) * 1e6, 1),
             qk_step_us=round(timed(qk_step, iters) * 1e6, 1), torch_qk_step_us=round(timed(qk_step_torch, iters) * 1e6, 1),
             layer_step_us=round(timed(layer_step(False), iters) * 1e6, 1),
             layer_rope_step_us=round(timed(layer_step(True), iters) * 1e6, 1))
    fwd_bytes = 2 * n * C * elem + n * d * 4
    r.update(fwd_hbm_frac=round(fwd_bytes / (r["fwd_us"] * 1e-6) / HBM, 3),
             table_bytes=n * d * 4,
             torch_over_ours_fwd=round(r["torch_fwd_us"] / r["fwd_us"], 2),
             torch_over_ours_qk_step=round(r["torch_qk_step_us"] / r["qk_step_us"], 2),
             layer_rope_overhead_us=round(r["layer_rope_step_us"] - r["layer_step_us"], 1),
             layer_rope_over_plain=round(r["layer_rope_step_us"] / r["layer_step_us"], 3))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 200000])
    args = ap.parse_args()
    assert args.iters >= 20
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no GPU, no number"
    dev = torch.device("cuda:0")
    results = []
    for n in args.sizes:
        for dt in (torch.bfloat16, torch.float32):
            r = case(n, dt, args.iters, dev)
            results.append(r)
            print(json.dumps(r), flush=True)
    print(f"{'n':>7s} {'dtype':5s} | {'table us':>8s} | fwd us: {'ours':>7s} {'torch':>7s} {'HBM frac':>8s} | qk fwd+bwd us: "
          f"{'ours':>7s} {'torch':>7s} | window layer fwd+bwd us: {'plain':>8s} {'rope':>8s} {'ratio':>6s}")
    for r in results:
        print(f"{r['n']:7d} {r['dtype']:5s} | {r['table_us']:8.1f} |         {r['fwd_us']:7.1f} {r['torch_fwd_us']:7.1f} "
              f"{r['fwd_hbm_frac']:8.3f} |                {r['qk_step_us']:7.1f} {r['torch_qk_step_us']:7.1f} | "
              f"                         {r['layer_step_us']:8.1f} {r['layer_rope_step_us']:8.1f} "
              f"{r['layer_rope_over_plain']:6.3f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
