"""MinkowskiAdaLayerNorm.forward_residual (gate, scale, shift) against MinkowskiLayerNorm.forward_residual plus the torch
gather / modulation chain, and against the all-torch chain, in one process, alternating, on one MI355X.

    python scripts/ada_layer_norm_bench.py [--out profiles/r26_ada_layer_norm_bench.log] [--reps 200] [--max-rows N]

Per shape, dtype and scene count (2, 8): µs per call forward and forward + backward (device events around `reps` calls
after a warm-up, the candidates alternating in blocks of reps / 4, as scripts/layer_norm_bench.py), and the byte model
over our time: forward 4 n c e, backward 6 n c e (stream, dy, dstream, input in; two gradients out).  The conditioning
tensors require gradients, so the torch chains pay their index_add_ reductions.  Shapes up to 200k x 512 fit the 256 MiB
last-level cache, so their rates are cache-resident rates; 1M x 256 does not fit.  The backward pass of the torch chains
costs tens to hundreds of milliseconds per call (index_add_ onto 2 or 8 rows), so a full run at --reps 200 takes long:
--reps 20 and --max-rows bound it.  The log is written line by line."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402
from layer_norm_bench import SHAPES, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--max-rows", type=int, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["n c dtype scenes | fwd us ours / layernorm+torch / torch | fwd+bwd us ours / layernorm+torch / torch | "
             "TB/s fwd, bwd (ours)"]
    out = open(args.out, "w") if args.out else None
    if out:
        out.write(lines[0] + "\n")
    for n, c in SHAPES:
        if args.max_rows is not None and n > args.max_rows:
            continue
        for scenes in (2, 8):
            side = int(round((n / scenes) ** (1 / 3))) + 2
            pts = [torch.unique(torch.randint(0, side, (2 * n // scenes, 3)), dim=0)[:n // scenes] for _ in range(scenes)]
            coords = torch.cat([torch.cat([torch.full((p.shape[0], 1), b), p], 1) for b, p in enumerate(pts)]).int().to(dev)
            rows_n = coords.shape[0]
            for dtype in (torch.bfloat16, torch.float32):
                e = torch.finfo(dtype).bits // 8
                x = ME.SparseTensor(torch.randn(rows_n, c, device=dev, dtype=dtype), coords)
                r = ME.SparseTensor(torch.randn(rows_n, c, device=dev, dtype=dtype), coordinate_map_key=x.coordinate_map_key,
                                    coordinate_manager=x.coordinate_manager)
                rows = x.coordinate_manager._manager._origin_rows(x.coordinate_map_key).long()
                ada, ln = ME.MinkowskiAdaLayerNorm(c).to(dev), ME.MinkowskiLayerNorm(c, eps=1e-6,
                                                                                    elementwise_affine=False).to(dev)
                scale, shift, gate = (torch.randn(scenes, c, device=dev) for _ in range(3))
                dy, ds = (torch.randn(rows_n, c, device=dev, dtype=dtype) for _ in range(2))

                def ours():
                    y, s = ada.forward_residual(x, r, scale, shift, gate)
                    return y.F, s.F

                def mixed():
                    gx = ME.SparseTensor(gate.to(dtype)[rows] * x.F, coordinate_map_key=x.coordinate_map_key,
                                         coordinate_manager=x.coordinate_manager)
                    y, s = ln.forward_residual(gx, r)
                    return y.F * (1 + scale.to(dtype)[rows]) + shift.to(dtype)[rows], s.F

                def torch_():
                    s = r.F + gate.to(dtype)[rows] * x.F
                    return F.layer_norm(s, (c,), None, None, 1e-6) * (1 + scale.to(dtype)[rows]) + shift.to(dtype)[rows], s

                leaves = (x.F, r.F, scale, shift, gate)

                def train(fn):
                    def step():
                        for t in leaves:
                            t.grad = None
                        torch.autograd.backward(fn(), [dy, ds])
                    return step
                with torch.no_grad():
                    fwd = timed([ours, mixed, torch_], args.reps)
                for t in leaves:
                    t.requires_grad_(True)
                both = timed([train(ours), train(mixed), train(torch_)], args.reps)
                for t in leaves:
                    t.requires_grad_(False)
                fwd_bytes, bwd_bytes = 4 * rows_n * c * e, 6 * rows_n * c * e
                lines.append(f"{rows_n} {c} {str(dtype)[6:]} {scenes} | {fwd[0]:.1f} / {fwd[1]:.1f} / {fwd[2]:.1f} | "
                             f"{both[0]:.1f} / {both[1]:.1f} / {both[2]:.1f} | "
                             f"{fwd_bytes / fwd[0] / 1e6:.2f}, {bwd_bytes / max(both[0] - fwd[0], 1e-9) / 1e6:.2f}")
                print(lines[-1], flush=True)
                if out:
                    out.write(lines[-1] + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
