"""CPU checks of the channelwise convolution's public surface: exports, reference-shaped parameters and state dicts,
repr, the C ABI declarations and the committed fixtures (no GPU needed)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW_CASES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "channelwise_*.npz")))
CW_SYMBOLS = ["me_cwconv_forward_f32", "me_cwconv_forward_bf16", "me_cwconv_forward_f64",
              "me_cwconv_backward_workspace_bytes", "me_cwconv_backward_f32", "me_cwconv_backward_bf16",
              "me_cwconv_backward_f64"]


def test_exported():
    import minkowskiengine_amd as ME
    assert issubclass(ME.MinkowskiChannelwiseConvolution, torch.nn.Module)
    assert issubclass(ME.MinkowskiChannelwiseConvolutionFunction, torch.autograd.Function)


@pytest.mark.parametrize("D,ks,bias", [(3, 3, True), (3, 2, False), (2, 5, True), (4, 3, True)])
def test_parameters_match_the_reference(D, ks, bias):
    import minkowskiengine_amd as ME
    C = 17
    layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, bias=bias, dimension=D)
    volume = ks ** D
    shapes = {n: tuple(p.shape) for n, p in layer.named_parameters()}
    want = {"kernel": (volume, C)}
    if bias:
        want["bias"] = (1, C)
    assert shapes == want
    assert all(p.dtype == torch.float32 for p in layer.parameters())
    # reset_parameters: U(-1 / sqrt(C * volume), +)
    bound = 1.0 / np.sqrt(C * volume)
    assert float(layer.kernel.detach().abs().max()) <= bound
    # a reference-shaped state dict loads strictly
    sd = {"kernel": torch.rand(volume, C)}
    if bias:
        sd["bias"] = torch.rand(1, C)
    layer.load_state_dict(sd, strict=True)
    assert torch.equal(layer.kernel.detach(), sd["kernel"])


def test_repr_is_the_reference_one():
    import minkowskiengine_amd as ME
    layer = ME.MinkowskiChannelwiseConvolution(8, kernel_size=3, stride=2, dimension=3)
    assert repr(layer) == ("MinkowskiChannelwiseConvolution(in=8, region_type=RegionType.HYPER_CUBE, "
                           "kernel_size=[3, 3, 3], stride=[2, 2, 2], dilation=[1, 1, 1])")


def test_abi_symbols_declared():
    from minkowskiengine_amd import _lib
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    declared = set(re.findall(r"\b(me_cwconv_\w+)\s*\(", header))
    assert declared == set(CW_SYMBOLS)
    assert set(CW_SYMBOLS) <= set(_lib.SIGNATURES)


def test_backend_operators_exist():
    from minkowskiengine_amd import backend
    assert callable(backend.ChannelwiseConvolutionForwardGPU)
    assert callable(backend.ChannelwiseConvolutionBackwardGPU)


def test_fixtures_load():
    assert len(CW_CASES) == 5
    keys = {"in_coords", "out_coords", "kernel_size", "stride", "dilation", "feats", "kernel", "bias", "grad_out", "out",
            "grad_in", "grad_kernel", "grad_bias", "kmap_k", "kmap_n", "kmap_pairs"}
    for path in CW_CASES:
        z = np.load(path)
        assert keys <= set(z.files), path
        n_in, c = z["feats"].shape
        n_out = z["out_coords"].shape[0]
        volume = int(np.prod(z["kernel_size"]))
        assert z["kernel"].shape == (volume, c) and z["bias"].shape == (1, c)
        assert z["out"].shape == (n_out, c) and z["grad_in"].shape == (n_in, c)
        assert z["grad_kernel"].shape == (volume, c) and z["grad_bias"].shape == (1, c)
        assert int(z["kmap_n"].sum()) == z["kmap_pairs"].shape[1]
        assert np.isclose(z["grad_bias"], z["grad_out"].astype(np.float64).sum(0)).all()
