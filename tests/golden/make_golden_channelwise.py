"""Generate the channelwise-convolution fixtures (channelwise_*.npz) from the reference's own kernel maps.

The reference's MinkowskiChannelwiseConvolution (MinkowskiEngine/MinkowskiChannelwiseConvolution.py:164-194) has no
native operator: its forward is `cm.kernel_map(in_key, stride(in_key), ...)` followed, per kernel offset k, by
`out_F[out_rows] += input.F[in_rows] * kernel[k]` and `out_F += bias`.  Here that kernel map comes from the reference's
CPU CoordinateMapManager (compiled unmodified into oracle/_ref/_C.so by oracle/build_ref.py, through oracle.ref), and
the formula is evaluated in float64 over it, with the analytic gradients
    dx[i] = sum_k W[k] * dy[o],   dW[k] = sum over the pairs (i, o) of k of x[i] * dy[o],   db = sum_o dy[o].
The fp32 inputs are stored as they are fed to the GPU; the results are float64.

Run where the reference's source tree is available (oracle/build_ref.py builds oracle/_ref from it):
    python tests/golden/make_golden_channelwise.py
The .npz files are committed; tests never need the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref  # noqa: E402

from make_golden import cloud, kmap_to_arrays  # noqa: E402


def channelwise_case(name, coords, c, kernel_size, stride=1, dilation=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    rc = ref.RefConv(coords, kernel_size, stride, dilation)
    km = rc.kernel_map()          # the conv map cm.kernel_map asks for (is_transpose=False, is_pool=False)
    n_in, n_out = rc.in_coordinates().shape[0], rc.out_coordinates().shape[0]
    volume = int(np.prod(rc.kernel_size))
    feats = torch.rand(n_in, c, generator=g) - 0.5
    kernel = torch.rand(volume, c, generator=g) - 0.5
    bias = torch.rand(1, c, generator=g) - 0.5
    grad_out = torch.rand(n_out, c, generator=g) - 0.5
    x, w, b, dy = (t.double().numpy() for t in (feats, kernel, bias, grad_out))
    out = np.zeros((n_out, c)) + b
    grad_in = np.zeros((n_in, c))
    grad_kernel = np.zeros((volume, c))
    for k, pairs in km.items():
        i, o = pairs[0].long().numpy(), pairs[1].long().numpy()
        np.add.at(out, o, x[i] * w[k])
        np.add.at(grad_in, i, dy[o] * w[k])
        grad_kernel[k] = (x[i] * dy[o]).sum(0)
    kk, kn, kp = kmap_to_arrays(km)
    data = dict(coords=coords.numpy().astype(np.int32), in_coords=rc.in_coordinates().numpy(),
                out_coords=rc.out_coordinates().numpy(), kernel_size=np.array(rc.kernel_size, np.int32),
                stride=np.array(rc.stride, np.int32), dilation=np.array(rc.dilation, np.int32),
                feats=feats.numpy(), kernel=kernel.numpy(), bias=bias.numpy(), grad_out=grad_out.numpy(),
                out=out, grad_in=grad_in, grad_kernel=grad_kernel, grad_bias=dy.sum(0, keepdims=True),
                kmap_k=kk, kmap_n=kn, kmap_pairs=kp)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **data)
    print(name, "n_in", n_in, "n_out", n_out, "pairs", int(kn.sum()))


def make_channelwise_cases():
    channelwise_case("channelwise_3d_k3s1_c8", cloud(400, 10, 3, 21, batch=2), 8, 3, 1, seed=1)
    channelwise_case("channelwise_3d_k2s2_c16", cloud(400, 12, 3, 22, batch=2), 16, 2, 2, seed=2)
    channelwise_case("channelwise_3d_k3d2_c5", cloud(400, 10, 3, 23, batch=2), 5, 3, 1, dilation=2, seed=3)
    channelwise_case("channelwise_2d_k5s1_c3", cloud(150, 20, 2, 24, batch=3), 3, 5, 1, seed=4)
    channelwise_case("channelwise_4d_k3s1_c17", cloud(250, 6, 4, 25, batch=2), 17, 3, 1, seed=5)


if __name__ == "__main__":
    make_channelwise_cases()
