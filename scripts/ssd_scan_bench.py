"""The SSD scan (csrc/ssd_scan.hip) on one MI355X: µs per call against the same chunked computation in torch operations and
against a byte / flop model.

    python scripts/ssd_scan_bench.py [--out profiles/r29_ssd_scan_bench.log] [--reps 40] [--rows 200000]

Per width H P (256, 512; P = 64), dtype and instance count (2, 8), S = 128, one group, D and dt_bias given, softplus on,
order "z": µs per call forward and forward + backward (device events around `reps` calls after a warm-up, in blocks of
reps / 4, as scripts/layer_norm_bench.py).  `torch` is the chunked formulation below (chunks of me_ssd_chunk positions, the
chunk carry a Python loop), forward and forward + backward through autograd, timed over --torch-reps calls.  The byte model
reads and writes every operand once and the entry states once each way: forward (2 H P + H + 2 S) n e + 8 n H S P / T bytes.
The flop model counts the products of one chunk and head: forward 2 T (T S + T P + 2 S P) flops.  Both are printed as the
time they take at --peak TB/s and --flops TFLOP/s (dense bf16 MFMA); the larger is the model.  The row lists are built
before the clock starts."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402
from layer_norm_bench import timed  # noqa: E402
from minkowskiengine_amd import _lib  # noqa: E402
from minkowskiengine_amd.selective_scan import scan_sequence  # noqa: E402


def chunked_torch(x, dt, A, B, C, D, bias, p, seq, starts, T):
    """the kernels' computation (csrc/ssd_scan.hip's header) with torch operations in float32, one group"""
    n, h = x.shape[0], x.shape[1] // p
    pad = -n % T
    take = lambda v: torch.nn.functional.pad(v[seq].float(), (0, 0, 0, pad)).view(-1, T, v.shape[1])
    X, Bc, Cc = take(x).unflatten(2, (h, p)), take(B), take(C)
    step = torch.nn.functional.pad(torch.nn.functional.softplus(dt[seq].float() + bias), (0, 0, 0, pad)).view(-1, T, h)
    cum = torch.cumsum(step * A, 1)                                             # [c, T, h]
    seg = torch.cumsum(torch.nn.functional.pad(starts.long(), (0, pad)).view(-1, T), 1)
    same = (seg[:, :, None] == seg[:, None, :]) & torch.tril(torch.ones(T, T, dtype=torch.bool, device=x.device))
    L = torch.exp((cum[:, :, None] - cum[:, None, :]).masked_fill(~same[..., None], -float("inf")))
    M = torch.einsum("cis,cjs->cij", Cc, Bc)[..., None] * L * step[:, None]
    y = torch.einsum("cijh,cjhp->cihp", M, X)
    f = torch.exp(cum[:, -1:] - cum) * (seg == seg[:, -1:])[..., None]
    end = torch.einsum("cjs,cjh,cjhp->chsp", Bc, f * step, X)
    decay = torch.exp(cum[:, -1]) * (seg[:, -1:] == 0)
    entry = [torch.zeros_like(end[0])]
    for c in range(end.shape[0] - 1):
        entry.append(decay[c, :, None, None] * entry[-1] + end[c])
    e = torch.exp(cum) * (seg == 0)[..., None]
    y = y + torch.einsum("cis,cih,chsp->cihp", Cc, e, torch.stack(entry)) + D[:, None] * X
    out = torch.empty(n, h * p, device=x.device)
    out[seq] = y.reshape(-1, h * p)[:n]
    return out.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--torch-reps", type=int, default=4)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--peak", type=float, default=8.0, help="HBM bandwidth in TB/s of the byte model")
    ap.add_argument("--flops", type=float, default=2500.0, help="dense bf16 MFMA TFLOP/s of the flop model")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    s, p, n, T = 128, 64, args.rows, int(_lib.load().me_ssd_chunk())
    lines = ["n HP s dtype instances | kernels fwd, fwd+bwd us | torch fwd, fwd+bwd us | model fwd us: bytes, flops | "
             f"reps {args.reps} / {args.torch_reps}"]
    out = open(args.out, "w") if args.out else None
    if out:
        out.write(lines[0] + "\n")
    for scenes in (2, 8):
        side = int(round((n / scenes) ** (1 / 3))) + 2
        pts = [torch.unique(torch.randint(0, side, (2 * n // scenes, 3)), dim=0)[:n // scenes] for _ in range(scenes)]
        coords = torch.cat([torch.cat([torch.full((q.shape[0], 1), b), q], 1) for b, q in enumerate(pts)]).int().to(dev)
        rows_n = coords.shape[0]
        sp = ME.SparseTensor(torch.zeros(rows_n, 1, device=dev), coords)
        key, mgr = sp.coordinate_map_key, sp.coordinate_manager
        seq, starts = (v.to(dev) for v in scan_sequence(key, mgr, "z", False))
        for hp in (256, 512):
            h = hp // p
            for dtype in (torch.bfloat16, torch.float32):
                e = torch.finfo(dtype).bits // 8
                x, dout = (torch.randn(rows_n, hp, device=dev, dtype=dtype) for _ in range(2))
                dt = (0.5 * torch.randn(rows_n, h, device=dev)).to(dtype)
                B, C = (torch.randn(rows_n, s, device=dev, dtype=dtype) for _ in range(2))
                A, D, bias = -(0.5 + torch.rand(h, device=dev)), torch.randn(h, device=dev), 0.5 * torch.randn(h, device=dev)
                leaves = (x, dt, A, B, C, D, bias)
                runs = {"kernels": lambda: ME.ssd_scan(x, dt, A, B, C, D, bias, True, p, 1, "z", False, key, mgr, fused=True),
                        "torch": lambda: chunked_torch(x, dt, A, B, C, D, bias, p, seq, starts, T)}
                times = {}
                for name, fwd in runs.items():
                    reps = args.reps if name == "kernels" else args.torch_reps

                    def train():
                        for t in leaves:
                            t.grad = None
                        fwd().backward(dout)
                    for t in leaves:
                        t.requires_grad_(False)
                    with torch.no_grad():
                        t_fwd = timed([fwd], reps)[0]
                    for t in leaves:
                        t.requires_grad_(True)
                    times[name] = (t_fwd, timed([train], reps)[0])
                    for t in leaves:
                        t.requires_grad_(False)
                nbytes = (2 * hp + h + 2 * s) * rows_n * e + 8 * rows_n * h * s * p // T
                flops = 2 * T * (T * s + T * p + 2 * s * p) * h * (-(-rows_n // T))
                lines.append(f"{rows_n} {hp} {s} {str(dtype)[6:]} {scenes} | {times['kernels'][0]:.1f}, {times['kernels'][1]:.1f} | "
                             f"{times['torch'][0]:.1f}, {times['torch'][1]:.1f} | "
                             f"{nbytes / args.peak / 1e6:.1f}, {flops / args.flops / 1e6:.1f}")
                print(lines[-1], flush=True)
                if out:
                    out.write(lines[-1] + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
