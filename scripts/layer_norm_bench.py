"""MinkowskiLayerNorm against torch.nn.functional.layer_norm (plus a torch add for the residual form) and against
MinkowskiGroupNorm, in one process, alternating, on one MI355X.

    python scripts/layer_norm_bench.py [--out profiles/r23_layer_norm_bench.log] [--reps 200]

Per shape, dtype and form (plain / residual): µs per call forward and forward + backward (device events around `reps`
calls after a warm-up of the same length, the candidates alternating in blocks of reps / 4), and the byte model over our
time: forward 2 n c e (4 n c e with the residual), backward 3 n c e.  Shapes up to 200k x 512 fit the 256 MiB last-level
cache, so their rates are cache-resident rates; 1M x 256 does not fit."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402

SHAPES = [(n, c) for n in (100_000, 200_000) for c in (64, 128, 256, 512)] + [(1_000_000, 256)]


def timed(fns, reps):
    """µs per call of every fn in `fns`, alternating in blocks"""
    total = [0.0] * len(fns)
    block = max(reps // 4, 1)
    for fn in fns:
        for _ in range(block):
            fn()
    for _ in range(reps // block):
        for i, fn in enumerate(fns):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(block):
                fn()
            end.record()
            end.synchronize()
            total[i] += start.elapsed_time(end) * 1e3
    return [t / (reps // block * block) for t in total]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["n c dtype form | fwd us ours / torch / groupnorm | fwd+bwd us ours / torch / groupnorm | TB/s fwd, bwd (ours)"]
    for n, c in SHAPES:
        side = int(round(n ** (1 / 3))) + 2
        pts = torch.unique(torch.randint(0, side, (2 * n, 3)), dim=0)[:n]
        n = pts.shape[0]
        coords = torch.cat([torch.zeros(n, 1, dtype=torch.long), pts], 1).int().to(dev)
        for dtype in (torch.bfloat16, torch.float32):
            e = torch.finfo(dtype).bits // 8
            x = ME.SparseTensor(torch.randn(n, c, device=dev, dtype=dtype), coords)
            r = ME.SparseTensor(torch.randn(n, c, device=dev, dtype=dtype), coordinate_map_key=x.coordinate_map_key,
                                coordinate_manager=x.coordinate_manager)
            ln, gn = ME.MinkowskiLayerNorm(c).to(dev), ME.MinkowskiGroupNorm(8, c).to(dev)
            w, b = ln.weight.detach().to(dtype), ln.bias.detach().to(dtype)
            dy = torch.randn(n, c, device=dev, dtype=dtype)
            for residual in (False, True):
                def ours():
                    return ln.forward_residual(x, r)[0].F if residual else ln(x).F

                def torch_():
                    return F.layer_norm(r.F + x.F if residual else x.F, (c,), w, b, 1e-5)

                def group():
                    return gn(r + x if residual else x).F

                def train(fn):
                    def step():
                        x.F.grad = r.F.grad = None
                        fn().backward(dy)
                    return step
                with torch.no_grad():
                    fwd = timed([ours, torch_, group], args.reps)
                x.F.requires_grad_(True)
                r.F.requires_grad_(True)
                both = timed([train(ours), train(torch_), train(group)], args.reps)
                x.F.requires_grad_(False)
                r.F.requires_grad_(False)
                fwd_bytes, bwd_bytes = (4 if residual else 2) * n * c * e, 3 * n * c * e
                lines.append(f"{n} {c} {str(dtype)[6:]} {'residual' if residual else 'plain'} | "
                             f"{fwd[0]:.1f} / {fwd[1]:.1f} / {fwd[2]:.1f} | {both[0]:.1f} / {both[1]:.1f} / {both[2]:.1f} | "
                             f"{fwd_bytes / fwd[0] / 1e6:.2f}, {bwd_bytes / max(both[0] - fwd[0], 1e-9) / 1e6:.2f}")
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
