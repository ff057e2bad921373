"""Two-launch against three-launch backward pass of one fp32 convolution layer (me_debug_set_dgrad_reduce_tail 2 / 1)
per channel shape, on the headline scene (100k voxels in 70^3, k = 3): ms per forward + backward step, modes
alternating.  Backs the tail-length bound of me_conv_dgrad_reduce_tail_supported (kTailMaxRounds, conv_f32x3.hip).
usage: python scripts/dgrad_tail_sweep.py [steps] [rounds]"""
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minkowskiengine_amd as ME  # noqa: E402
from minkowskiengine_amd import _lib  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
lib = _lib.load()
g = torch.Generator().manual_seed(0)
n, extent = 100000, 70
pts = torch.unique(torch.randint(0, extent, (2 * n, 3), generator=g), dim=0)
pts = pts[torch.randperm(pts.shape[0], generator=g)][:n]
coords = torch.cat([torch.zeros(pts.shape[0], 1, dtype=torch.long), pts], 1).int().to(dev)

for cin, cout in ((64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 256)):
    ME.clear_global_coordinate_manager()
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=3, dimension=3).to(dev)
    x = ME.SparseTensor(torch.rand(coords.shape[0], cin, generator=g).to(dev), coords, requires_grad=True)
    gy = torch.ones(coords.shape[0], cout, device=dev)

    def step():
        x.F.grad = None
        conv.kernel.grad = None
        conv(x).F.backward(gy)

    def timed(mode):
        lib.me_debug_set_dgrad_reduce_tail(mode)
        for _ in range(10):
            step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    res = {1: [], 2: []}
    for _ in range(rounds):
        for mode in (1, 2):
            res[mode].append(timed(mode))
    lib.me_debug_set_dgrad_reduce_tail(0)
    policy = lib.me_conv_dgrad_reduce_tail_supported(cin, cout, 27, 834914)
    print(f"{cin:4d} -> {cout:4d}  three launches {st.median(res[1]):.4f} ms ({min(res[1]):.4f}-{max(res[1]):.4f})  "
          f"two launches {st.median(res[2]):.4f} ms ({min(res[2]):.4f}-{max(res[2]):.4f})  "
          f"delta {1e3 * (st.median(res[2]) - st.median(res[1])):+.1f} us  policy {'two' if policy else 'three'}", flush=True)
