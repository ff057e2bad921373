"""A dense-in / dense-out network around sparse layers: a regular torch tensor goes in, ReLU runs on it as on any tensor,
`MinkowskiToSparseTensor` turns every cell into a row of a SparseTensor (the coordinates are generated once and reused,
since the shape is fixed), a strided convolution, batch norm, ReLU and a transposed convolution run sparse, and
`MinkowskiToDenseTensor` hands a regular tensor of the input's spatial shape back.  Gradients flow to the dense input.

    python examples/dense_network.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import minkowskiengine_amd as ME


def build(shape, in_channels=4, mid_channels=5, out_channels=6):
    dimension = len(shape) - 2
    coordinates = ME.dense_coordinates(shape)          # cached: the module uploads nothing it was not given
    return nn.Sequential(
        nn.ReLU(),
        ME.MinkowskiToSparseTensor(remove_zeros=False, coordinates=coordinates),
        ME.MinkowskiConvolution(in_channels, mid_channels, stride=2, kernel_size=3, dimension=dimension),
        ME.MinkowskiBatchNorm(mid_channels),
        ME.MinkowskiReLU(),
        ME.MinkowskiConvolutionTranspose(mid_channels, out_channels, stride=2, kernel_size=3, dimension=dimension),
        ME.MinkowskiToDenseTensor(shape),               # the channel count of `shape` is corrected to the layer's
    )


def main():
    device = torch.device("cuda:0")
    dense_tensor = torch.rand(3, 4, 11, 11, 11, 11, device=device, requires_grad=True)     # B x C x X1 x X2 x X3 x X4
    network = build(dense_tensor.shape).to(device)
    for i in range(5):
        dense_tensor.grad = None
        output = network(dense_tensor)                  # a regular torch tensor again
        output.sum().backward()
        print(f"iteration {i}: output {tuple(output.shape)}, |grad| {float(dense_tensor.grad.abs().sum()):.4f}")
    assert output.shape[2:] == dense_tensor.shape[2:] and dense_tensor.grad is not None


if __name__ == "__main__":
    main()
