"""Shifted-window attention (the window lists of csrc/serial_attention.hip + the block-table path of csrc/attention.hip):
time per call of MinkowskiWindowAttentionFunction, forward + backward with all three gradients, in one process on one GPU,
next to

  torch   the padded torch formulation on the same lists: a gather to [W, max rows, H, d], scaled_dot_product_attention with
          a key mask and a scatter back, through autograd.  The index tensors are built outside the timed region.
  serial  MinkowskiSerializedAttentionFunction (order hilbert) at a patch size equal to the mean window population: the same
          work per row in patches that are all full
  build   the list build (me_attn_window_ids, the 4-byte read-back of the window count, me_attn_segment_lists), which the
          manager does once per (map, window sizes, shifts) — timed apart from the cached call

    python scripts/window_attention_bench.py [--iters 30] [--json out.jsonl]

Protocol of scripts/serial_attention_bench.py: 10 warm-up calls, then `iters` calls between two device events.  Shapes: one
scene of 100k and of 200k voxels (a quarter of the cells occupied) x 128 channels x 4 heads, windows of 4^3, 8^3 and 16^3
voxels (16, 128 and 1024 rows per full window at that density), shift 0 and shift w / 2, bf16 and fp32.  The distribution
of rows per window is printed with every case.  FLOPs = 18 sum_w n_w^2 C (4 forward + 14 backward); TFLOP/s is the
whole-call rate against the MFMA peaks (bf16 2500, fp32 157.3), not a kernel's share of peak."""
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


def build_fn(lib, x, window, shift, stream):
    """the two C-ABI calls of CoordinateManager.window_rows with the read-back between them; the bounding box comes from
    one reduction outside the timed region"""
    coords = x.C.contiguous()
    n, ncol = coords.shape
    D = ncol - 1
    lo, hi = coords.amin(0).tolist(), coords.amax(0).tolist()
    i32s = lambda v: (ctypes.c_int32 * D)(*v)   # noqa: E731
    ts, w, s, c_lo, c_hi = i32s([1] * D), i32s([window] * D), i32s([shift] * D), i32s(lo[1:]), i32s(hi[1:])
    i32 = dict(dtype=torch.int32, device=coords.device)
    row_window, count = torch.empty(n, **i32), torch.zeros(1, **i32)
    ws = torch.empty(int(lib.me_attn_window_ids_workspace_bytes(n)), dtype=torch.uint8, device=coords.device)
    seg_ptr, seg_rows = torch.empty(n + 1, **i32), torch.empty(n, **i32)
    tab = torch.empty(2 * (-(-n // 64) + n), **i32)
    ws2 = torch.empty(int(lib.me_attn_segment_lists_workspace_bytes(n, n)), dtype=torch.uint8, device=coords.device)

    def run():
        _lib.check(lib.me_attn_window_ids(coords.data_ptr(), n, ncol, ts, w, s, D, c_lo, c_hi, lo[0], hi[0],
                                          row_window.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        n_seg = int(count.item())
        _lib.check(lib.me_attn_segment_lists(row_window.data_ptr(), n, n_seg, seg_ptr.data_ptr(), seg_rows.data_ptr(),
                                             tab.data_ptr(), ws2.data_ptr(), ws2.numel(), stream))
        return row_window
    return run


def quantiles(sizes):
    s = torch.sort(sizes).values
    pick = lambda f: int(s[min(int(f * s.numel()), s.numel() - 1)])   # noqa: E731
    return dict(min=int(s[0]), p10=pick(0.1), median=pick(0.5), p90=pick(0.9), max=int(s[-1]),
                mean=round(float(sizes.float().mean()), 1))


def case(n, window, shift, dtype, iters, dev):
    lib = _lib.load()
    x = make_scene(n, dev)
    key, mgr = x.coordinate_map_key, x.coordinate_manager
    seg_ptr, seg_rows, tab, row_window = mgr.window_rows(key, window, shift)
    sizes = (seg_ptr[1:] - seg_ptr[:-1]).long()
    assert int(sizes.min()) > 0                            # the window count was read back: no empty segment
    n_windows, longest = int(sizes.numel()), int(sizes.max())
    patch = max(1, round(n / n_windows))
    d = C // HEADS
    q, k, v = (torch.randn(n, C, device=dev).to(dtype).requires_grad_(True) for _ in range(3))
    dout = torch.randn(n, C, device=dev).to(dtype)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # the padded slots [windows, longest] of the same lists, outside the timed region
    slot = torch.arange(longest, device=dev)[None]
    pad_mask = slot < sizes[:, None]
    flat_valid = pad_mask.reshape(-1).nonzero().reshape(-1)      # slot of the i-th row of seg_rows (segment-major)
    rows = seg_rows.long()
    full = bool(pad_mask.all())
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def ours():
        return ME.MinkowskiWindowAttentionFunction.apply(q, k, v, HEADS, None, window, shift, key, mgr)

    def serial():
        return ME.MinkowskiSerializedAttentionFunction.apply(q, k, v, HEADS, None, patch, "hilbert", key, mgr)

    def padded(t):
        # the rows in list order (a permutation: its gradient is a gather, no atomics) copied into the occupied slots of a
        # zeroed [W * longest, C] buffer; gathering with a dummy index for the empty slots instead makes the backward pass
        # accumulate every empty slot into one row, which costs 100 ms and more where half the slots are empty
        buf = torch.zeros(n_windows * longest, C, dtype=t.dtype, device=dev).index_copy(0, flat_valid, t[rows])
        return buf.view(n_windows, longest, HEADS, d).transpose(1, 2)

    def torch_padded():
        o = sdpa(padded(q), padded(k), padded(v), attn_mask=None if full else pad_mask[:, None, None, :])
        o = o.transpose(1, 2).reshape(-1, C)
        return torch.empty_like(q).index_copy(0, rows, o[flat_valid])

    def step(fwd):
        def run():
            q.grad = k.grad = v.grad = None
            fwd().backward(dout)
        return run
    res = {}
    for nm, fn in (("ours", ours), ("torch", torch_padded)):
        step(fn)()
        res[nm] = (fn().detach().float(), q.grad.float().clone())
    build = build_fn(lib, x, window, shift, stream)
    assert torch.equal(build(), row_window)
    pairs = float((sizes * sizes).sum())
    step_flops = 18.0 * pairs * C
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    r = dict(n=n, window=window, shift=shift, dtype=dt, C=C, heads=HEADS, windows=n_windows, rows_per_window=quantiles(sizes),
             blocks=int((tab[0::2] >= 0).sum()), serial_patch_size=patch,
             out_diff_torch=float((res["ours"][0] - res["torch"][0]).abs().max()),
             dq_diff_torch=float((res["ours"][1] - res["torch"][1]).abs().max()),
             ours_step_us=round(timed(step(ours), iters) * 1e6, 1),
             torch_step_us=round(timed(step(torch_padded), iters) * 1e6, 1),
             serial_step_us=round(timed(step(serial), iters) * 1e6, 1),
             build_us=round(timed(build, iters) * 1e6, 1))
    r.update(step_tflops=round(step_flops / r["ours_step_us"] * 1e-6, 2),
             step_peak_fraction=round(step_flops / r["ours_step_us"] * 1e-6 / PEAK_TFLOPS[dt], 4),
             torch_over_ours=round(r["torch_step_us"] / r["ours_step_us"], 2),
             serial_over_ours=round(r["serial_step_us"] / r["ours_step_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 200000])
    ap.add_argument("--windows", type=int, nargs="+", default=[4, 8, 16])
    args = ap.parse_args()
    assert args.iters >= 20
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no GPU, no number"
    dev = torch.device("cuda:0")
    results = []
    for n in args.sizes:
        for window in args.windows:
            for shift in (0, window // 2):
                for dt in (torch.bfloat16, torch.float32):
                    r = case(n, window, shift, dt, args.iters, dev)
                    results.append(r)
                    print(json.dumps(r), flush=True)
    print(f"{'n':>7s} {'w':>3s} {'s':>2s} {'dtype':5s} {'windows':>7s} {'mean':>7s} {'max':>5s} | fwd+bwd us: {'ours':>9s} "
          f"{'torch':>9s} {'serial':>9s} | {'build us':>9s} | torch/ours serial/ours | TF/s  of peak")
    for r in results:
        rw = r["rows_per_window"]
        print(f"{r['n']:7d} {r['window']:3d} {r['shift']:2d} {r['dtype']:5s} {r['windows']:7d} {rw['mean']:7.1f} {rw['max']:5d} |"
              f"             {r['ours_step_us']:9.1f} {r['torch_step_us']:9.1f} {r['serial_step_us']:9.1f} | {r['build_us']:9.1f} | "
              f"{r['torch_over_ours']:10.2f} {r['serial_over_ours']:11.2f} | {r['step_tflops']:5.2f} {r['step_peak_fraction']:.4f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
