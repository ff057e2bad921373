"""MinkowskiFeedForward's fused kernels against the torch formulation linear -> gelu -> linear on the same tensors, in one
process, alternating, on one MI355X.

    python scripts/feed_forward_bench.py [--out profiles/r24_feed_forward_bench.log] [--reps 100]

Per row count, width, dtype: µs per call forward and forward + backward (all five gradients; device events around
`reps` calls after a warm-up, the two candidates alternating in blocks of reps / 4), and the multiply-add rate of our
forward, 4 n c hidden flop over its time.  hidden = 4 c.  Widths outside the width rule are listed as not served.

    python scripts/feed_forward_bench.py --gated [--out profiles/r25_gated_feed_forward_bench.log] [--repeat 2]

--gated: MinkowskiGatedFeedForward's kernels against torch's three-linear formulation fc2(silu(fc1_g(x)) * fc1_x(x)), all
seven gradients, widths 64 and 128, hidden = 4 c and 8 c / 3 rounded up to 32 (6 n c hidden flop forward).  --repeat R runs
the whole table R times in the process; the spread of a figure is the difference between its runs."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402
from minkowskiengine_amd import backend  # noqa: E402

SHAPES = [(n, c) for n in (20_000, 120_000) for c in (64, 128, 256)]
RATIO = 4
GATED_SHAPES = [(n, c) for n in (20_000, 120_000) for c in (64, 128)]


def gated_hiddens(c):
    return (4 * c, (8 * c // 3 + 31) // 32 * 32)


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


def table(args, dev, gated):
    """the timing table of the plain (gated: the gated) module against its torch formulation"""
    served = backend.gated_feed_forward_supported if gated else backend.feed_forward_supported
    cases = [(n, c, hd) for n, c in GATED_SHAPES for hd in gated_hiddens(c)] if gated else [(n, c, RATIO * c) for n, c in SHAPES]
    lines = ["n c hidden dtype | fwd us ours / torch | fwd+bwd us ours / torch | TFLOP/s fwd (ours)"]
    for n, c, hd in cases:
        for dtype in (torch.bfloat16, torch.float32):
            if not served(c, hd, c, dtype):
                lines.append(f"{n} {c} {hd} {str(dtype)[6:]} | not served (torch formulation)")
                print(lines[-1], flush=True)
                continue
            g = torch.Generator().manual_seed(0)
            rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).to(dev)
            x, dy = rnd(n, c), rnd(n, c)
            first = [rnd(hd, c) * c ** -0.5, rnd(hd)]
            if gated:
                first += [rnd(hd, c) * c ** -0.5, rnd(hd)]
            leaves = (x, *first, rnd(c, hd) * hd ** -0.5, rnd(c))

            def ours():
                if gated:
                    return ME.MinkowskiGatedFeedForwardFunction.apply(*leaves, "silu")
                return ME.MinkowskiFeedForwardFunction.apply(*leaves, "gelu")

            def torch_():
                if gated:
                    x, wg, bg, wu, bu, w2, b2 = leaves
                    return F.linear(F.silu(F.linear(x, wg, bg)) * F.linear(x, wu, bu), w2, b2)
                x, w1, b1, w2, b2 = leaves
                return F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)

            def train(fn):
                def step():
                    for t in leaves:
                        t.grad = None
                    fn().backward(dy)
                return step
            with torch.no_grad():
                fwd = timed([ours, torch_], args.reps)
            for t in leaves:
                t.requires_grad_(True)
            both = timed([train(ours), train(torch_)], args.reps)
            lines.append(f"{n} {c} {hd} {str(dtype)[6:]} | {fwd[0]:.1f} / {fwd[1]:.1f} | {both[0]:.1f} / {both[1]:.1f} | "
                         f"{(6.0 if gated else 4.0) * n * c * hd / fwd[0] / 1e6:.1f}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--gated", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    if args.gated:
        lines = []
        for run in range(args.repeat):
            lines += [f"# run {run + 1} of {args.repeat}"] + table(args, dev, True)
    else:
        lines = table(args, dev, False)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
