"""Generate the instance-norm fixtures (instance_norm_*.npz) from the reference's own MinkowskiInstanceNorm.

oracle.ref.import_reference_package() imports the reference's unmodified Python package over its compiled CPU extension
(oracle/_ref/_C.so, built by oracle/build_ref.py); this script runs the reference's real
`MinkowskiInstanceNorm(C).double()` forward and `backward(grad_out)` in float64 — its chain of global average poolings
and broadcasts (MinkowskiEngine/MinkowskiNormalization.py:194-310, 361-399) — and stores, per case,

    coords, feats, weight, bias, grad_out     the fp32 / int32 inputs exactly as the tests feed them to the GPU
    out, grad_in, grad_weight, grad_bias      the reference's float64 results

It also asserts, in float64, that the recorded `out` equals the plain formula (x - mean_b) / sqrt(var_b + 1e-8) * w + b
(var: biased, per instance and channel) to 1e-12, so the fixture documents the formula and not an accident of the
reference's operator chain.  The work runs in a subprocess: importing the reference package rewires sys.modules.

Every committed file must stay below 1 MiB, and a row costs 24 bytes per channel here (two fp32 inputs, two float64
results), so the 64-channel case holds 2 x 330 rows — 6 forward and 11 backward chunks of the kernels, straddling
chunks included — instead of thousands; tests/test_gpu_instance_norm.py repeats that case at 2 x 3000 rows against the
formula asserted here.

Run where the reference's source tree is available:
    python tests/golden/make_golden_instance_norm.py
The .npz files are committed; tests never need the reference.  A rerun reproduces the inputs bit for bit and the float64
results to about 1e-14: the reference's CPU pooling does not add the rows of an instance in the same order every run.
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))


def formula(x, batch, w, b, eps):
    """float64 restatement: per instance and channel, biased variance"""
    out = np.empty_like(x)
    for i in np.unique(batch):
        m = batch == i
        mu = x[m].mean(0)
        var = ((x[m] - mu) ** 2).mean(0)
        out[m] = (x[m] - mu) / np.sqrt(var + eps) * w + b
    return out


def sized_cloud(sizes, extent, D, seed):
    """one cloud per entry of `sizes`, batch index = position"""
    from make_golden import cloud
    parts = []
    for b, n in enumerate(sizes):
        c = cloud(n, extent, D, seed + 17 * b)
        c[:, 0] = b
        parts.append(c)
    return torch.cat(parts, 0)


def instance_norm_case(RME, name, coords, c, seed, shuffle=False, offsets=False):
    g = torch.Generator().manual_seed(seed)
    if shuffle:
        coords = coords[torch.randperm(coords.shape[0], generator=g)]
    n = coords.shape[0]
    if offsets:   # channel means several times the spread: E[x^2] - E[x]^2 loses half its digits here
        feats = (torch.rand(1, c, generator=g) * 8 - 4) + 0.3 * torch.randn(n, c, generator=g)
    else:
        feats = torch.rand(n, c, generator=g) - 0.5
    weight = torch.rand(1, c, generator=g) + 0.5
    bias = torch.rand(1, c, generator=g) - 0.5
    grad_out = torch.rand(n, c, generator=g) - 0.5
    layer = RME.MinkowskiInstanceNorm(c).double()
    with torch.no_grad():
        layer.weight.copy_(weight.double())
        layer.bias.copy_(bias.double())
    feat_leaf = feats.double().requires_grad_(True)
    x = RME.SparseTensor(feat_leaf, coords)
    assert torch.equal(x.C.int(), coords.int()), "the reference kept the row order"
    y = layer(x)
    y.F.backward(grad_out.double())
    out = y.F.detach().numpy()
    want = formula(feats.double().numpy(), coords[:, 0].numpy(), weight.double().numpy(), bias.double().numpy(), 1e-8)
    err = float(np.abs(out - want).max())
    assert err <= 1e-12, (name, err)
    data = dict(coords=coords.numpy().astype(np.int32), feats=feats.numpy(), weight=weight.numpy(), bias=bias.numpy(),
                grad_out=grad_out.numpy(), out=out, grad_in=feat_leaf.grad.numpy(), grad_weight=layer.weight.grad.numpy(),
                grad_bias=layer.bias.grad.numpy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    print(name, "rows", n, "per instance", np.bincount(coords[:, 0].numpy()).tolist(), "formula err", err,
          "bytes", os.path.getsize(path))


def make_instance_norm_cases():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import ref
    RME = ref.import_reference_package()
    from make_golden import cloud
    instance_norm_case(RME, "instance_norm_3d_b2_c8", cloud(400, 12, 3, 31, batch=2), 8, seed=1)
    instance_norm_case(RME, "instance_norm_3d_b3_sizes_c16", sized_cloud([700, 40, 1], 14, 3, 32), 16, seed=2)
    instance_norm_case(RME, "instance_norm_3d_b2_interleaved_c5", cloud(400, 12, 3, 33, batch=2), 5, seed=3, shuffle=True)
    instance_norm_case(RME, "instance_norm_2d_b4_c3", cloud(150, 20, 2, 34, batch=4), 3, seed=4)
    instance_norm_case(RME, "instance_norm_4d_b2_c17", cloud(250, 6, 4, 35, batch=2), 17, seed=5)
    instance_norm_case(RME, "instance_norm_3d_b2_c64_offsets", cloud(330, 12, 3, 36, batch=2), 64, seed=6, offsets=True)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        make_instance_norm_cases()
    else:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker"])
