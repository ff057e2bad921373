"""Serialized patch attention (csrc/serial_attention.hip + the block-table path of csrc/attention.hip): time per call of
MinkowskiSerializedAttentionFunction, forward + backward with all three gradients, in one process on one GPU, next to

  torch   (a) the torch formulation on the same lists: a padded gather to [patches, P, H, d], scaled_dot_product_attention
          (with a key mask when the patches are not all full) and a scatter back, through autograd.  The index tensors are
          built outside the timed region.
  walk    (b) our kernels through the C ABI with NULL block tables: every workgroup walks seg_ptr to find its block
  table   the same C-ABI calls with the block table: (b) against this is what the table buys
  build   the list build (keys, radix sort, patch ids, me_csr_from_coo, block table: me_attn_patch_lists), which the
          manager does once per (map, patch size, order) — timed apart from the cached call

    python scripts/serial_attention_bench.py [--iters 50] [--json out.jsonl]

Protocol of scripts/attention_bench.py: 10 warm-up calls, then `iters` calls between two device events.  Shapes: one scene
of 100k and of 200k voxels x 128 channels x 4 heads, patch sizes 128 and 1024, order hilbert, bf16 and fp32.
FLOPs = 4 sum_p n_p^2 C forward + 14 sum_p n_p^2 C backward; TFLOP/s against the MFMA peaks (bf16 2500, fp32 157.3)."""
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

PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}
ORDER = "hilbert"
C, HEADS = 128, 4


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


def c_abi_step(lib, q, k, v, dout, seg_ptr, seg_rows, tab, scale, stream):
    """forward + backward through me_attn_forward_tab / me_attn_backward_tab; tab None: the linear walk"""
    n, c = q.shape
    n_seg = seg_ptr.numel() - 1
    bf = 1 if q.dtype == torch.bfloat16 else 0
    out, lse = torch.empty_like(q), torch.empty(n, HEADS, dtype=torch.float32, device=q.device)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    ws = torch.empty(int(lib.me_attn_workspace_bytes(n, n, n_seg, HEADS)), dtype=torch.uint8, device=q.device)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def run():
        _lib.check(lib.me_attn_forward_tab(p(q), p(k), p(v), bf, c, c, c, p(seg_ptr), p(seg_rows), p(seg_ptr), p(seg_rows),
                                           p(tab), p(tab), n, n, n_seg, c, HEADS, scale, p(out), c, p(lse), stream))
        _lib.check(lib.me_attn_backward_tab(p(q), p(k), p(v), p(out), p(lse), p(dout), bf, c, c, c, c, c, p(seg_ptr),
                                            p(seg_rows), p(seg_ptr), p(seg_rows), p(tab), p(tab), n, n, n_seg, c, HEADS,
                                            scale, p(dq), c, p(dk), c, p(dv), c, p(ws), ws.numel(), stream))
        return out, dq, dk, dv
    return run


def build_fn(lib, x, patch, stream):
    """me_attn_patch_lists on the coordinates of x, geometry from one read-back outside the timed region"""
    coords = x.C.contiguous()
    n, ncol = coords.shape
    lo, hi = coords.amin(0).tolist(), coords.amax(0).tolist()
    depth = max((hi[1 + a] - lo[1 + a]).bit_length() for a in range(ncol - 1))
    ts, c_lo = (ctypes.c_int32 * (ncol - 1))(*([1] * (ncol - 1))), (ctypes.c_int32 * (ncol - 1))(*lo[1:])
    n_seg = -(-n // patch) + 1
    i32 = dict(dtype=torch.int32, device=coords.device)
    seg_ptr, seg_rows = torch.empty(n_seg + 1, **i32), torch.empty(n, **i32)
    tab, row_patch = torch.empty(2 * (-(-n // 64) + n_seg), **i32), torch.empty(n, **i32)
    ws = torch.empty(int(lib.me_attn_patch_lists_workspace_bytes(n, 1, patch)), dtype=torch.uint8, device=coords.device)
    code = ("z", "z_trans", "hilbert", "hilbert_trans").index(ORDER)

    def run():
        _lib.check(lib.me_attn_patch_lists(coords.data_ptr(), n, ncol, ts, c_lo, depth, hi[0], code, 1, patch,
                                           seg_ptr.data_ptr(), seg_rows.data_ptr(), tab.data_ptr(), row_patch.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream))
        return row_patch
    return run


def case(n, patch, dtype, iters, dev):
    lib = _lib.load()
    x = make_scene(n, dev)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    seg_ptr, seg_rows, tab, row_patch = mgr.patch_rows(key, patch, ORDER)
    sizes = (seg_ptr[1:] - seg_ptr[:-1]).long()
    sizes = sizes[sizes > 0]
    n_patches, longest = int(sizes.numel()), int(sizes.max())
    d = C // HEADS
    scale = 1.0 / math.sqrt(d)
    q, k, v = (torch.randn(n, C, device=dev).to(dtype).requires_grad_(True) for _ in range(3))
    dout = torch.randn(n, C, device=dev).to(dtype)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # (a): the padded index [patches, longest] of the same lists, outside the timed region
    slot = torch.arange(longest, device=dev)[None]
    pad_mask = slot < sizes[:, None]
    pad_index = torch.zeros(n_patches, longest, dtype=torch.long, device=dev)
    pad_index[pad_mask] = seg_rows.long()
    flat_valid = pad_mask.reshape(-1).nonzero().reshape(-1)
    full = bool(pad_mask.all())
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def ours():
        return ME.MinkowskiSerializedAttentionFunction.apply(q, k, v, HEADS, None, patch, ORDER, key, mgr)

    def torch_padded():
        qb, kb, vb = (t[pad_index.reshape(-1)].view(n_patches, longest, HEADS, d).transpose(1, 2) for t in (q, k, v))
        o = sdpa(qb, kb, vb, attn_mask=None if full else pad_mask[:, None, None, :]).transpose(1, 2).reshape(-1, C)
        out = torch.empty_like(q)
        return out.index_copy(0, pad_index.reshape(-1)[flat_valid], o[flat_valid])

    def step(fwd):
        def run():
            q.grad = k.grad = v.grad = None
            fwd().backward(dout)
        return run
    res = {}
    for nm, fn in (("ours", ours), ("torch", torch_padded)):
        step(fn)()
        res[nm] = (fn().detach().float(), q.grad.float().clone())
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    walk = c_abi_step(lib, qd, kd, vd, dout, seg_ptr, seg_rows, None, scale, stream)
    table = c_abi_step(lib, qd, kd, vd, dout, seg_ptr, seg_rows, tab, scale, stream)
    w, t = [a.clone() for a in walk()], [a.clone() for a in table()]
    build = build_fn(lib, x, patch, stream)
    assert torch.equal(build(), row_patch)
    pairs = float((sizes * sizes).sum())
    step_flops = 18.0 * pairs * C
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    r = dict(n=n, patch_size=patch, dtype=dt, C=C, heads=HEADS, order=ORDER, patches=n_patches, longest=longest,
             segments=int(seg_ptr.numel()) - 1,
             out_diff_torch=float((res["ours"][0] - res["torch"][0]).abs().max()),
             dq_diff_torch=float((res["ours"][1] - res["torch"][1]).abs().max()),
             walk_equals_table=all(torch.equal(a, b) for a, b in zip(w, t)),
             ours_step_us=round(timed(step(ours), iters) * 1e6, 1),
             torch_step_us=round(timed(step(torch_padded), iters) * 1e6, 1),
             walk_step_us=round(timed(walk, iters) * 1e6, 1),
             table_step_us=round(timed(table, iters) * 1e6, 1),
             build_us=round(timed(build, iters) * 1e6, 1))
    r.update(step_tflops=round(step_flops / r["ours_step_us"] * 1e-6, 2),
             step_peak_fraction=round(step_flops / r["ours_step_us"] * 1e-6 / PEAK_TFLOPS[dt], 4),
             torch_over_ours=round(r["torch_step_us"] / r["ours_step_us"], 2),
             walk_over_table=round(r["walk_step_us"] / r["table_step_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 20
    dev = torch.device("cuda:0")
    results = []
    for n in (100000, 200000):
        for patch in (128, 1024):
            for dt in (torch.bfloat16, torch.float32):
                r = case(n, patch, dt, args.iters, dev)
                results.append(r)
                print(json.dumps(r), flush=True)
    print(f"{'n':>7s} {'P':>5s} {'dtype':5s} | fwd+bwd us: {'ours':>9s} {'torch':>9s} {'walk':>9s} {'table':>9s} | "
          f"{'build us':>9s} | torch/ours walk/table | TF/s  of peak")
    for r in results:
        print(f"{r['n']:7d} {r['patch_size']:5d} {r['dtype']:5s} |             {r['ours_step_us']:9.1f} {r['torch_step_us']:9.1f} "
              f"{r['walk_step_us']:9.1f} {r['table_step_us']:9.1f} | {r['build_us']:9.1f} | {r['torch_over_ours']:10.2f} "
              f"{r['walk_over_table']:10.2f} | {r['step_tflops']:5.2f} {r['step_peak_fraction']:.4f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
