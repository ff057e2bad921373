"""The selective scan (csrc/selective_scan.hip) on one MI355X: µs per call and the fraction of HBM bandwidth it reaches.

    python scripts/selective_scan_bench.py [--out profiles/r27_selective_scan_bench.log] [--reps 40] [--rows 200000]

Per channel count (128, 256), dtype and instance count (2, 8), S = 16, z, Dskip and delta_bias given, softplus on, order
"z": µs per call forward and forward + backward (device events around `reps` calls after a warm-up, in blocks of reps / 4,
as scripts/layer_norm_bench.py) and the byte model over the time, as a fraction of --peak TB/s.  The byte model reads and
writes every operand once: forward (4 d + 2 s) n e bytes (u, delta, z, out; B, C), backward (7 d + 4 s) n e (u, delta, z,
dout, du, ddelta, dz; B, C, dB, dC).  There is no earlier path to compare with: the torch formulation walks the rows one
by one.  The row lists are built before the clock starts (they are cached per map and order)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402
from layer_norm_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--peak", type=float, default=8.0, help="HBM bandwidth in TB/s that the fractions refer to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    s, n = 16, args.rows
    lines = [f"n d s dtype instances | fwd us | fwd+bwd us | fwd, bwd fraction of {args.peak} TB/s (byte model) | reps {args.reps}"]
    out = open(args.out, "w") if args.out else None
    if out:
        out.write(lines[0] + "\n")
    for scenes in (2, 8):
        side = int(round((n / scenes) ** (1 / 3))) + 2
        pts = [torch.unique(torch.randint(0, side, (2 * n // scenes, 3)), dim=0)[:n // scenes] for _ in range(scenes)]
        coords = torch.cat([torch.cat([torch.full((p.shape[0], 1), b), p], 1) for b, p in enumerate(pts)]).int().to(dev)
        rows_n = coords.shape[0]
        x = ME.SparseTensor(torch.zeros(rows_n, 1, device=dev), coords)
        key, mgr = x.coordinate_map_key, x.coordinate_manager
        for d in (128, 256):
            for dtype in (torch.bfloat16, torch.float32):
                e = torch.finfo(dtype).bits // 8
                u, z, dout = (torch.randn(rows_n, d, device=dev, dtype=dtype) for _ in range(3))
                delta = (0.5 * torch.randn(rows_n, d, device=dev)).to(dtype)
                B, C = (torch.randn(rows_n, s, device=dev, dtype=dtype) for _ in range(2))
                A = -(0.5 + torch.rand(d, s, device=dev))
                Dskip, bias = torch.randn(d, device=dev), 0.5 * torch.randn(d, device=dev)
                leaves = (u, delta, A, B, C, Dskip, z, bias)

                def fwd():
                    return ME.selective_scan(u, delta, A, B, C, Dskip, z, bias, True, "z", False, key, mgr, fused=True)

                def train():
                    for t in leaves:
                        t.grad = None
                    fwd().backward(dout)
                with torch.no_grad():
                    t_fwd = timed([fwd], args.reps)[0]
                for t in leaves:
                    t.requires_grad_(True)
                t_both = timed([train], args.reps)[0]
                fwd_bytes, bwd_bytes = (4 * d + 2 * s) * rows_n * e, (7 * d + 4 * s) * rows_n * e
                lines.append(f"{rows_n} {d} {s} {str(dtype)[6:]} {scenes} | {t_fwd:.1f} | {t_both:.1f} | "
                             f"{fwd_bytes / t_fwd / 1e6 / args.peak:.3f}, "
                             f"{bwd_bytes / max(t_both - t_fwd, 1e-9) / 1e6 / args.peak:.3f}")
                print(lines[-1], flush=True)
                if out:
                    out.write(lines[-1] + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
