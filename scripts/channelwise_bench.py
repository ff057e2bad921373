"""Channelwise convolution (csrc/conv_channelwise.hip): time per call of the forward and the backward (dx + dW + db)
through the C ABI on cached kernel maps, against a byte model and against the reference's formulation on the same GPU
(MinkowskiChannelwiseConvolution.py:184-189: per offset index_select, multiply and index_add_; autograd backward).

    python scripts/channelwise_bench.py [--iters 50] [--json out.jsonl]

Byte model (compulsory traffic): forward e*C*(n_in + n_out) + 4*volume*n_out (features read once, output written once,
the neighbour table); backward e*C*(n_in + n_out) + 4*volume*n_in + e*C*n_in (x and dy read once, the transposed table,
dx written).  e = 4 (fp32) or 2 (bf16).  Fraction of 6.3 TB/s (achievable HBM rate of the MI355X)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib
from bench import make_scene

HBM = 6.3e12


def timed(fn, iters, warm=5):
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


def case(name, coords, C, dtype, iters, dev):
    x = ME.SparseTensor(torch.rand(coords.shape[0], C, device=dev).to(dtype), coords)
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=3, bias=True, dimension=3).to(dev)
    y = layer(x)
    mgr = x.coordinate_manager._manager
    kg = layer.kernel_generator
    km = mgr._kernel_map(x.coordinate_map_key, y.coordinate_map_key, kg.kernel_size, kg.kernel_stride,
                         kg.kernel_dilation, kg.region_type, None, False, False) if hasattr(mgr, "_kernel_map") else None
    if km is None:
        raise SystemExit("run with ME_AMD_HOST=python: the benchmark reads the Python host's kernel-map tables")
    n_in, n_out, vol = km.n_in, km.n_out, km.volume
    tbl, tbl_t = km.table("out"), km.table("in")
    lib = _lib.load()
    sfx = "bf16" if dtype == torch.bfloat16 else "f32"
    fwd, bwd = getattr(lib, "me_cwconv_forward_" + sfx), getattr(lib, "me_cwconv_backward_" + sfx)
    feats, w, b = x.F, layer.kernel.detach(), layer.bias.detach()
    out = torch.empty((n_out, C), dtype=dtype, device=dev)
    dy = (torch.rand((n_out, C), device=dev) - 0.5).to(dtype)
    dx = torch.empty_like(feats)
    dw = torch.empty_like(w)
    db = torch.empty((C,), device=dev)
    ws = torch.empty(max(256, lib.me_cwconv_backward_workspace_bytes(n_in, vol, C)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    f_call = lambda: _lib.check(fwd(feats.data_ptr(), C, w.data_ptr(), b.data_ptr(), tbl.data_ptr(), n_in, n_out, vol,
                                    out.data_ptr(), st))
    b_call = lambda: _lib.check(bwd(feats.data_ptr(), dy.data_ptr(), C, w.data_ptr(), tbl_t.data_ptr(), n_in, n_out, vol,
                                    1, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st))
    t_f, t_b = timed(f_call, iters), timed(b_call, iters)
    # the reference's formulation on the same kernel map (pairs as int64 on the device, built once)
    pairs = [(int(k), v[0].long().to(dev), v[1].long().to(dev))
             for k, v in x.coordinate_manager.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 1, 3, 1).items()]
    xr = feats.detach().clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)

    def ref_fwd():
        o = torch.zeros((n_out, C), dtype=dtype, device=dev)
        for k, i, j in pairs:
            o.index_add_(0, j, xr.index_select(0, i) * wr[k].to(dtype))
        return o + br.to(dtype)

    def ref_fwd_nograd():
        with torch.no_grad():
            ref_fwd()

    def ref_step():
        ref_fwd().backward(dy)

    t_rf = timed(ref_fwd_nograd, max(5, iters // 5))
    t_rs = timed(ref_step, max(5, iters // 5))
    t_rb = max(t_rs - t_rf, 0.0)
    e = 2 if dtype == torch.bfloat16 else 4
    by_f = e * C * (n_in + n_out) + 4 * vol * n_out
    by_b = e * C * (n_in + n_out) + 4 * vol * n_in + e * C * n_in
    r = dict(case=name, dtype=sfx, C=C, n_in=n_in, n_out=n_out, volume=vol, pairs=int(km.n_pairs),
             fwd_us=round(t_f * 1e6, 2), bwd_us=round(t_b * 1e6, 2),
             fwd_model_MB=round(by_f / 1e6, 2), bwd_model_MB=round(by_b / 1e6, 2),
             fwd_hbm_frac=round(by_f / t_f / HBM, 3), bwd_hbm_frac=round(by_b / t_b / HBM, 3),
             ref_fwd_us=round(t_rf * 1e6, 1), ref_bwd_us=round(t_rb * 1e6, 1),
             speedup_fwd=round(t_rf / t_f, 1), speedup_bwd=round(t_rb / t_b, 1) if t_rb > 0 else None)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ME.set_host("python")
    dev = torch.device("cuda:0")
    import minkunet as MU
    scene2 = make_scene(100000, 70, 0).to(dev)                 # bench.py conv3d (config 2): 100k voxels in 70^3
    ts1 = MU.synthetic_scene(200000, seed=0).to(dev)           # MinkUNet34C's input scene (ts1), 200k voxels
    rows = []
    for name, coords, C, dt in (("config2", scene2, 64, torch.float32), ("config2", scene2, 64, torch.bfloat16),
                                ("config2", scene2, 128, torch.float32), ("config2", scene2, 128, torch.bfloat16),
                                ("minkunet_ts1", ts1, 96, torch.float32), ("minkunet_ts1", ts1, 96, torch.bfloat16)):
        r = case(name, coords, C, dt, args.iters, dev)
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(f"{'case':14s} {'dtype':5s} {'C':>4s} {'fwd us':>8s} {'HBM':>6s} {'ref fwd':>9s} {'x':>6s} "
          f"{'bwd us':>8s} {'HBM':>6s} {'ref bwd':>9s} {'x':>6s}")
    for r in rows:
        print(f"{r['case']:14s} {r['dtype']:5s} {r['C']:4d} {r['fwd_us']:8.1f} {r['fwd_hbm_frac']:6.2f} "
              f"{r['ref_fwd_us']:9.1f} {r['speedup_fwd']:6.1f} {r['bwd_us']:8.1f} {r['bwd_hbm_frac']:6.2f} "
              f"{r['ref_bwd_us']:9.1f} {str(r['speedup_bwd']):>6s}")
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
