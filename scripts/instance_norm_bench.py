"""Instance normalisation (csrc/instance_norm.hip): time per call of the forward (statistics + apply) and of
forward + backward through the C ABI on a prepared batch_row table, next to the COMPOSED formulation on the same GPU in
the same process: the reference's operator chain (MinkowskiNormalization.py:204-310 plus the module's `* weight + bias`
and its autograd) on this package's existing global-pooling / broadcast kernels and torch element-wise ops.

    python scripts/instance_norm_bench.py [--iters 200] [--json out.jsonl]

Shapes: (a) config 2's scene split into 4 instances, 100k rows x C 64; (b) a MinkUNet level, 200k rows x C 96, batch 2;
(c) a launch-bound case, 3k rows x C 256, batch 8.  Byte model (compulsory traffic): forward e*n*C*3 + 8n (x read by the
statistics and by the apply pass, y written, batch_row read twice), backward e*n*C*5 + 12n (x and dy read twice, dx
written, batch_row three times); e = 4 (fp32) or 2 (bf16).  Fraction of 6.3 TB/s (achievable HBM rate of the MI355X)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from bench import make_scene

HBM = 6.3e12
EPS = 1e-8


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


def split(coords, n_batch):
    """rows of a one-instance scene cut into n_batch runs of consecutive rows"""
    c = coords.clone()
    c[:, 0] = (torch.arange(c.shape[0]) * n_batch // c.shape[0]).int()
    return c


def case(name, coords, n_batch, C, dtype, iters, dev):
    coords = split(coords, n_batch).to(dev)
    n = coords.shape[0]
    x = ME.SparseTensor((torch.randn(n, C, device=dev) * 0.5 + 1.0).to(dtype), coords)
    key, mgr = x.coordinate_map_key, x.coordinate_manager._manager
    gkey = backend.CoordinateMapKey(key.get_coordinate_size())
    feats = x.F
    w = torch.rand(C, device=dev) + 0.5
    b = torch.rand(C, device=dev) - 0.5
    dy = (torch.rand(n, C, device=dev) - 0.5).to(dtype)
    # operators once (also builds the origin map and the row table), results kept for the parity line
    out, mean, rstd = backend.InstanceNormForwardGPU(feats, w, b, EPS, key, gkey, mgr)
    rows = mgr._origin_rows(key)
    assert int(rows.max()) + 1 == n_batch
    lib = _lib.load()
    bf = 1 if dtype == torch.bfloat16 else 0
    ws = torch.empty(max(256, lib.me_inorm_workspace_bytes(n, n_batch, C)), dtype=torch.uint8, device=dev)
    y, dx = torch.empty_like(feats), torch.empty_like(feats)
    gw, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def fused_fwd():
        _lib.check(lib.me_inorm_stats(feats.data_ptr(), bf, rows.data_ptr(), n, n_batch, C, EPS, mean.data_ptr(),
                                      rstd.data_ptr(), ws.data_ptr(), ws.numel(), st))
        _lib.check(lib.me_inorm_apply(feats.data_ptr(), bf, rows.data_ptr(), n, n_batch, C, mean.data_ptr(),
                                      rstd.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), st))

    def fused_step():
        fused_fwd()
        _lib.check(lib.me_inorm_backward(feats.data_ptr(), dy.data_ptr(), bf, rows.data_ptr(), n, n_batch, C,
                                         mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dx.data_ptr(), gw.data_ptr(),
                                         gb.data_ptr(), ws.data_ptr(), ws.numel(), st))

    avg, add, mul = ME.PoolingMode.GLOBAL_AVG_POOLING_KERNEL, ME.BroadcastMode.ELEMENTWISE_ADDITON, \
        ME.BroadcastMode.ELEMENTWISE_MULTIPLICATION
    gpool = lambda f: backend.GlobalPoolingForwardGPU(f, avg, key, gkey, mgr)[0]
    bcast = lambda f, g, op: backend.BroadcastForwardGPU(f, g, op, key, gkey, mgr)
    wd, bd = w.to(dtype), b.to(dtype)

    def composed_fwd():
        m = gpool(feats)
        centered = bcast(feats, -m, add)
        var = gpool(centered ** 2)
        inv_std = 1 / (var + EPS).sqrt()
        norm = bcast(centered, inv_std, mul)
        return norm * wd + bd, inv_std, norm

    def composed_step():
        o, inv_std, norm = composed_fwd()
        g_w, g_b = (dy * norm).sum(0), dy.sum(0)          # autograd of `output * weight + bias`
        g = dy * wd
        mean_dout = gpool(g)
        mean_dout_feat = gpool(g * norm)
        t = bcast(norm, mean_dout_feat, mul)
        unnorm = bcast(g - t, -mean_dout, add)
        return o, bcast(unnorm, inv_std, mul), g_w, g_b

    # parity of the two paths on this input (max abs difference; bf16 rounds every composed intermediate)
    fused_step()
    co, cdx, _, _ = composed_step()
    torch.cuda.synchronize()
    d_out = float((y.float() - co.float()).abs().max())
    d_dx = float((dx.float() - cdx.float()).abs().max())
    t_f, t_s = timed(fused_fwd, iters), timed(fused_step, iters)
    t_cf, t_cs = timed(lambda: composed_fwd(), max(10, iters // 4)), timed(lambda: composed_step(), max(10, iters // 4))
    t_f2, t_s2 = timed(fused_fwd, iters), timed(fused_step, iters)          # alternated: the spread of the same call
    e = 2 if dtype == torch.bfloat16 else 4
    by_f, by_b = e * n * C * 3 + 8 * n, e * n * C * 5 + 12 * n
    t_f, t_s = min(t_f, t_f2), min(t_s, t_s2)
    return dict(case=name, dtype="bf16" if bf else "f32", n=n, n_batch=n_batch, C=C,
                fused_fwd_us=round(t_f * 1e6, 2), fused_step_us=round(t_s * 1e6, 2),
                fused_fwd_us_second=round(t_f2 * 1e6, 2), fused_step_us_second=round(t_s2 * 1e6, 2),
                composed_fwd_us=round(t_cf * 1e6, 2), composed_step_us=round(t_cs * 1e6, 2),
                fwd_model_MB=round(by_f / 1e6, 2), step_model_MB=round((by_f + by_b) / 1e6, 2),
                fwd_hbm_frac=round(by_f / t_f / HBM, 3), bwd_hbm_frac=round(by_b / max(t_s - t_f, 1e-9) / HBM, 3),
                speedup_fwd=round(t_cf / t_f, 2), speedup_step=round(t_cs / t_s, 2),
                max_abs_diff_out=d_out, max_abs_diff_dx=d_dx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ME.set_host("python")
    dev = torch.device("cuda:0")
    import minkunet as MU
    scene2 = make_scene(100000, 70, 0)                 # bench.py conv3d (config 2): 100k voxels in 70^3
    ts1 = MU.synthetic_scene(200000, seed=0).cpu()     # MinkUNet34C's input scene, 200k voxels
    small = make_scene(3000, 30, 1)
    rows = []
    for name, coords, nb, C in (("a_config2_b4", scene2, 4, 64), ("b_minkunet_b2", ts1, 2, 96),
                                ("c_small_b8", small, 8, 256)):
        for dt in (torch.float32, torch.bfloat16):
            r = case(name, coords, nb, C, dt, args.iters, dev)
            rows.append(r)
            print(json.dumps(r), flush=True)
    print(f"{'case':14s} {'dtype':5s} {'n':>7s} {'C':>4s} {'fwd us':>8s} {'HBM':>6s} {'composed':>9s} {'x':>6s} "
          f"{'fwd+bwd us':>10s} {'bwd HBM':>7s} {'composed':>9s} {'x':>6s}")
    for r in rows:
        print(f"{r['case']:14s} {r['dtype']:5s} {r['n']:7d} {r['C']:4d} {r['fused_fwd_us']:8.1f} {r['fwd_hbm_frac']:6.2f} "
              f"{r['composed_fwd_us']:9.1f} {r['speedup_fwd']:6.2f} {r['fused_step_us']:10.1f} {r['bwd_hbm_frac']:7.2f} "
              f"{r['composed_step_us']:9.1f} {r['speedup_step']:6.2f}")
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
