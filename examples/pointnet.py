"""PointNet on a TensorField: per-point MinkowskiLinear / MinkowskiBatchNorm / MinkowskiReLU blocks, one
MinkowskiGlobalMaxPooling over each point cloud, and a dense classification head.  Runs one training step on a
synthetic batch and prints the loss.

    python examples/pointnet.py [--points 1024] [--batch 4] [--classes 10]
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import minkowskiengine_amd as ME  # noqa: E402


class PointNet(nn.Module):
    def __init__(self, in_channels=3, classes=10, widths=(64, 128, 256)):
        super().__init__()
        blocks, c = [], in_channels
        for w in widths:
            blocks += [ME.MinkowskiLinear(c, w, bias=False), ME.MinkowskiBatchNorm(w), ME.MinkowskiReLU()]
            c = w
        self.point_mlp = nn.Sequential(*blocks)
        self.pool = ME.MinkowskiGlobalMaxPooling()
        self.head = nn.Sequential(nn.Linear(c, 128), nn.ReLU(), nn.Linear(128, classes))

    def forward(self, field):
        per_cloud = self.pool(self.point_mlp(field))        # SparseTensor: one row per cloud, ascending batch index
        return self.head(per_cloud.F)


def synthetic_batch(points, batch, classes, device, seed=0):
    """`batch` clouds of unequal size: points on a sphere whose radius depends on the label"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, classes, (batch,), generator=g)
    coords = []
    for b in range(batch):
        n = points - 17 * b
        x = torch.randn(n, 3, generator=g)
        x = x / x.norm(dim=1, keepdim=True) * (1.0 + 0.3 * labels[b])
        coords.append(torch.cat([torch.full((n, 1), float(b)), x], 1))
    coords = torch.cat(coords)
    coords = coords[torch.randperm(len(coords), generator=g)]      # clouds interleaved
    return coords.to(device), labels.to(device)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--classes", type=int, default=10)
    args = ap.parse_args(argv)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    net = PointNet(classes=args.classes).to(device)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    coords, labels = synthetic_batch(args.points, args.batch, args.classes, device)
    field = ME.TensorField(coords[:, 1:].contiguous(), coordinates=coords)
    loss = nn.functional.cross_entropy(net(field), labels)
    opt.zero_grad()
    loss.backward()
    opt.step()
    print(f"pointnet: {len(coords)} points in {args.batch} clouds, loss {loss.item():.6f}")
    return loss.item()


if __name__ == "__main__":
    main()
