"""The causal conv1d (csrc/causal_conv1d.hip) on one MI355X against its torch formulation in the same process.

    python scripts/causal_conv1d_bench.py [--out profiles/r28_causal_conv1d_bench.log] [--reps 40] [--rows 184000]

Per channel count (256, 512) and dtype, K = 4 with bias and SiLU, order "z", two instances: µs per call forward and
forward + backward of the kernels (fused=True) and of the torch index formulation (fused=False, the path before the
kernels), alternating in blocks (device events around `reps` calls after a warm-up, as scripts/layer_norm_bench.py), and
the byte model over the kernels' time as a fraction of --peak TB/s.  The byte model moves every row once: forward
2 n d e bytes (x, y), backward 3 n d e (x, dy, dx); halos, row lists and the records of the parameter gradients are not in
it.  Then one MinkowskiMamba(128) training step (d_inner 256, d_state 16) with the conv on the kernels against the conv
on the torch formulation; the scan runs on its kernels in both (the layer's own fused=False would also send the scan to its
torch formulation, a Python loop over the rows that takes minutes at this size and would hide the conv).  The row lists
are built before the clock starts (they are cached per map and order)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402
from layer_norm_bench import timed  # noqa: E402

cc = sys.modules["minkowskiengine_amd.causal_conv1d"]     # the module: the package attribute of that name is the function


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rows", type=int, default=184_000)
    ap.add_argument("--peak", type=float, default=8.0, help="HBM bandwidth in TB/s that the fractions refer to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, k, scenes = args.rows, 4, 2
    side = int(round((n / scenes) ** (1 / 3))) + 2
    pts = [torch.unique(torch.randint(0, side, (2 * n // scenes, 3)), dim=0)[:n // scenes] for _ in range(scenes)]
    coords = torch.cat([torch.cat([torch.full((p.shape[0], 1), b), p], 1) for b, p in enumerate(pts)]).int().to(dev)
    rows_n = coords.shape[0]
    s = ME.SparseTensor(torch.zeros(rows_n, 1, device=dev), coords)
    key, mgr = s.coordinate_map_key, s.coordinate_manager
    say(f"n d k dtype | fwd us kernels / torch | fwd+bwd us kernels / torch | fwd, bwd fraction of {args.peak} TB/s "
        f"(byte model, kernels) | reps {args.reps}")
    for d in (256, 512):
        for dtype in (torch.bfloat16, torch.float32):
            e = torch.finfo(dtype).bits // 8
            x, dout = (torch.randn(rows_n, d, device=dev, dtype=dtype) for _ in range(2))
            w, b = torch.randn(d, k, device=dev) / 2, 0.5 * torch.randn(d, device=dev)
            leaves = (x, w, b)

            def fwd(fused):
                return cc.causal_conv1d(x, w, b, "silu", "z", False, key, mgr, fused=fused)

            def train(fused):
                for t in leaves:
                    t.grad = None
                fwd(fused).backward(dout)
            with torch.no_grad():
                f_ours, f_torch = timed([lambda: fwd(True), lambda: fwd(False)], args.reps)
            for t in leaves:
                t.requires_grad_(True)
            t_ours, t_torch = timed([lambda: train(True), lambda: train(False)], args.reps)
            fwd_bytes, bwd_bytes = 2 * d * rows_n * e, 3 * d * rows_n * e
            say(f"{rows_n} {d} {k} {str(dtype)[6:]} | {f_ours:.1f} / {f_torch:.1f} | {t_ours:.1f} / {t_torch:.1f} | "
                f"{fwd_bytes / f_ours / 1e6 / args.peak:.3f}, {bwd_bytes / max(t_ours - f_ours, 1e-9) / 1e6 / args.peak:.3f}")
    say("MinkowskiMamba(128) fwd+bwd us: dtype | conv on the kernels | conv on the torch formulation (scan on its kernels "
        "in both) | reps 8")
    for dtype in (torch.bfloat16, torch.float32):
        layer = ME.MinkowskiMamba(128, d_state=16).to(device=dev, dtype=dtype)
        feats = torch.randn(rows_n, 128, device=dev, dtype=dtype)
        dout = torch.randn(rows_n, 128, device=dev, dtype=dtype)
        fused_conv = cc.causal_conv1d

        def torch_conv(x, weight, bias, activation, order, reverse, key, manager, fused=None):
            return fused_conv(x, weight, bias, activation, order, reverse, key, manager, fused=False)

        def step(conv):
            cc.causal_conv1d = conv                # MinkowskiMamba.forward looks the function up at every call
            try:
                layer.zero_grad(set_to_none=True)
                layer(ME.SparseTensor(feats, coordinate_map_key=key, coordinate_manager=mgr)).F.backward(dout)
            finally:
                cc.causal_conv1d = fused_conv
        t_fused, t_conv_torch = timed([lambda: step(fused_conv), lambda: step(torch_conv)], 8)
        say(f"{str(dtype)[6:]} | {t_fused:.1f} | {t_conv_torch:.1f}")


if __name__ == "__main__":
    main()
