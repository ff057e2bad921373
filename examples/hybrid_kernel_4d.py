"""A spatio-temporal network on a HYBRID kernel: a cube in space, a cross in time.

A 4-D hyper-cube of size 3 has 81 taps.  The hybrid kernel keeps the 27 spatial taps of the current frame and adds one
tap into the previous and one into the next frame: 29 taps, built by `ME.hybrid_region_offsets` and handed to the layers
as a `RegionType.CUSTOM` kernel generator.  The offsets are in units of the tensor stride, so ONE generator definition
serves every level of a network — the second layer below runs at tensor stride 2 with the same list.

    python examples/hybrid_kernel_4d.py --points 20000 --frames 4
"""
import argparse

import torch


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=20000, help="voxels of the synthetic scene")
    ap.add_argument("--extent", type=int, default=40, help="spatial extent of the scene: [0, extent)^3")
    ap.add_argument("--frames", type=int, default=4, help="temporal extent: [0, frames)")
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    return ap


def hybrid_generator(ME, stride=1):
    """KernelGenerator of the 29-tap kernel: axes 0-2 (space) a cube, axis 3 (time) a cross, all sizes 3"""
    cube, cross = ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS
    offsets = ME.hybrid_region_offsets([cube, cube, cube, cross], 3, 4)
    return ME.KernelGenerator(stride=stride, region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=4)


def synthetic_scene(n, extent, frames, seed=0):
    """unique int32 coordinates [n', 5] = (batch, x, y, z, t)"""
    g = torch.Generator().manual_seed(seed)
    c = torch.cat([torch.randint(0, extent, (n, 3), generator=g), torch.randint(0, frames, (n, 1), generator=g)], 1)
    c = torch.unique(c, dim=0)
    return torch.cat([torch.zeros(c.shape[0], 1, dtype=torch.long), c], 1).int()


class HybridNet(torch.nn.Module):
    """two layers on the hybrid kernel: stride 1, then a strided one on the same offsets"""

    def __init__(self, ME, cin, channels):
        super().__init__()
        self.conv1 = ME.MinkowskiConvolution(cin, channels, kernel_generator=hybrid_generator(ME), dimension=4)
        self.relu = ME.MinkowskiReLU()
        self.conv2 = ME.MinkowskiConvolution(channels, channels, stride=2, kernel_generator=hybrid_generator(ME, 2),
                                             dimension=4)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


def main(argv=None):
    args = build_parser().parse_args(argv)
    import minkowskiengine_amd as ME
    dev = torch.device("cuda")
    coords = synthetic_scene(args.points, args.extent, args.frames, args.seed)
    feats = torch.rand(coords.shape[0], 3, generator=torch.Generator().manual_seed(args.seed))
    net = HybridNet(ME, 3, args.channels).to(dev)
    print(net)
    x = ME.SparseTensor(feats.to(dev), coords.to(dev))
    y = net(x)
    y.F.square().mean().backward()
    print(f"{coords.shape[0]} voxels -> {y.F.shape[0]} voxels at tensor stride {y.tensor_stride}, "
          f"{net.conv1.kernel.shape[0]} taps per layer (a 4-D cube has 81)")


if __name__ == "__main__":
    main()
