"""Golden fixture for arithmetic between sparse tensors on different coordinate maps, FROM THE REFERENCE's own Python
package on its CPU operators (oracle/_ref/_C.so): `a + b`, `a - b`, `a * b`, `a / b` through
MinkowskiTensor._binary_functor (union_map + torch indexing) and the gradients autograd gives for them.

Two pairs of clouds, two batches each, C = 3 and 32: one partially overlapping (about half of b's rows shared) and one
nested (b inside a).  Coordinates are unique per cloud; b's features have magnitude in [0.5, 2], so `/` is finite on
every row b holds (the 0 / 0 of a b-only row with a zero feature is pinned by a GPU test of its own).  Per pair, channel
count and operator: the union coordinates, the output features and the gradients of sum(out * w) for a recorded w.

    python tests/golden/make_golden_arith.py      (authoring container, needs /root/reference)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "arith_3d.npz")
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref  # noqa: E402

OPS = {"add": lambda x, y: x + y, "sub": lambda x, y: x - y, "mul": lambda x, y: x * y, "div": lambda x, y: x / y}


def pool(n, extent, g):
    """n unique rows (batch, x, y, z), batch in {0, 1}, in random order"""
    pts = torch.unique(torch.cat([torch.randint(0, 2, (4 * n, 1), generator=g),
                                  torch.randint(-extent // 2, extent // 2, (4 * n, 3), generator=g)], 1), dim=0)
    assert pts.shape[0] >= n
    return pts[torch.randperm(pts.shape[0], generator=g)][:n].int().contiguous()


def pairs(g):
    p = pool(170, 8, g)
    a, b = p[:120], p[70:170]                      # rows 70..119 are shared
    yield "overlap", a, b[torch.randperm(b.shape[0], generator=g)]
    p = pool(120, 8, g)
    yield "nested", p, p[torch.randperm(120, generator=g)[:60]]


if __name__ == "__main__":
    RME = ref.import_reference_package()          # (moves the working directory: PATH is absolute)
    g = torch.Generator().manual_seed(23)
    data = {}
    for pair, ca, cb in pairs(g):
        data[f"{pair}/a"], data[f"{pair}/b"] = ca.numpy(), cb.numpy()
        for c in (3, 32):
            fa = torch.randn(ca.shape[0], c, generator=g)
            sign = torch.where(torch.rand(cb.shape[0], c, generator=g) < 0.5, -1.0, 1.0)
            fb = (0.5 + 1.5 * torch.rand(cb.shape[0], c, generator=g)) * sign
            w = None
            data[f"{pair}/c{c}/fa"], data[f"{pair}/c{c}/fb"] = fa.numpy(), fb.numpy()
            for op, fn in OPS.items():
                xa, xb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
                A = RME.SparseTensor(xa, ca)
                B = RME.SparseTensor(xb, cb, coordinate_manager=A.coordinate_manager)
                assert torch.equal(A.C, ca) and torch.equal(B.C, cb), "the reference reordered unique coordinates"
                out = fn(A, B)
                if w is None:                      # one w per (pair, c): every operator has the same union size
                    w = torch.rand(out.F.shape, generator=g) + 0.5
                    data[f"{pair}/c{c}/w_coords"] = out.C.numpy().copy()
                    data[f"{pair}/c{c}/w"] = w.numpy()
                assert torch.equal(out.C, torch.from_numpy(data[f"{pair}/c{c}/w_coords"]))
                (out.F * w).sum().backward()
                assert torch.isfinite(out.F).all() and torch.isfinite(xb.grad).all()
                data[f"{pair}/c{c}/{op}/out"] = out.F.detach().numpy().copy()
                data[f"{pair}/c{c}/{op}/grad_a"] = xa.grad.numpy().copy()
                data[f"{pair}/c{c}/{op}/grad_b"] = xb.grad.numpy().copy()
        data[f"{pair}/out_coords"] = data[f"{pair}/c3/w_coords"]
        assert np.array_equal(data.pop(f"{pair}/c3/w_coords"), data.pop(f"{pair}/c32/w_coords"))
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), {k: v.shape for k, v in data.items() if k.endswith("out_coords")})
