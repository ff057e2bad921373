"""Direct max pooling and global pooling over fields, the parts that need no GPU: exported names, the C symbols, the
reference fixtures' own consistency (numpy over the .npz alone) and the CPU-tensor errors."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "direct_pool_*.npz")))
SYMBOLS = ["me_field_origin_rows_f32", "me_direct_max_pool_workspace_bytes", "me_direct_max_pool_f32",
           "me_direct_max_pool_bf16", "me_direct_max_pool_f64", "me_direct_max_pool_backward_workspace_bytes",
           "me_direct_max_pool_backward_f32", "me_direct_max_pool_backward_bf16", "me_direct_max_pool_backward_f64"]


def test_public_names():
    assert hasattr(ME, "MinkowskiDirectMaxPoolingFunction")
    import MinkowskiEngineBackend._C as C
    mods = [C, ME.MinkowskiEngineBackend]
    from minkowskiengine_amd import host
    if host.native_module() is not None:
        mods.append(host.native_module())
    for mod in mods:
        for name in ("direct_max_pool_fw", "direct_max_pool_bw"):
            assert hasattr(mod, name), (mod, name)
        for name in ("origin_field", "origin_field_map"):
            assert hasattr(mod.CoordinateMapManagerGPU_c10, name), (mod, name)
    for name in ("origin_field", "origin_field_map"):
        assert hasattr(ME.CoordinateManager, name), name


def test_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.SIGNATURES, s
    so = os.path.join(ROOT, "minkowskiengine_amd", "libme_amd.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.me_version() >= 210


def test_fixture_set_covers_the_cases():
    assert len(FIXTURES) >= 6
    seen = set()
    for path in FIXTURES:
        z = np.load(path)
        seen.add((str(z["in_map"].dtype), str(z["in_feat"].dtype), int(z["in_feat"].shape[1]), int(z["is_sorted"])))
    assert {d[0] for d in seen} == {"int32", "int64"}
    assert {d[1] for d in seen} == {"float32", "float64"}
    assert {1, 3, 16, 17} <= {d[2] for d in seen}
    assert {d[3] for d in seen} == {0, 1}
    assert any("field_coords" in np.load(p).files for p in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_conditions_and_masks(path):
    """the three conditions under which the reference's CPU kernel equals its GPU rule, and the masks point at the
    per-row maxima"""
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    im, om, f = z["in_map"].astype(np.int64), z["out_map"].astype(np.int64), z["in_feat"]
    n_out, c = int(z["out_nrows"]), f.shape[1]
    assert z["max_index"].dtype == z["in_map"].dtype and z["out_feat"].dtype == f.dtype
    assert set(om.tolist()) == set(range(n_out))                                  # 1. no empty output row
    assert (f >= 0.05).all() and (f < 1).all()                                    # 2. strictly positive
    if int(z["is_sorted"]):
        assert (np.diff(om) >= 0).all()
    grad_in = np.zeros_like(z["grad_in"])
    for o in range(n_out):
        rows = im[om == o]
        v = f[rows]
        for ch in range(c):
            assert len(np.unique(v[:, ch])) == len(rows)                          # 3. no ties
        assert np.array_equal(z["out_feat"][o], v.max(0))
        assert np.array_equal(z["max_index"][o], rows[v.argmax(0)] * c + np.arange(c))
        np.add.at(grad_in.reshape(-1), z["max_index"][o].astype(np.int64), z["grad_out"][o])
    assert np.array_equal(grad_in, z["grad_in"])


def test_cpu_tensors_raise():
    im, om = torch.arange(4), torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError):
        ME.MinkowskiEngineBackend.direct_max_pool_fw(im, om, torch.rand(4, 3), 1, False)
    with pytest.raises(RuntimeError):
        ME.MinkowskiEngineBackend.direct_max_pool_bw(torch.rand(1, 3), torch.zeros(1, 3, dtype=torch.long), 4)
    with pytest.raises(RuntimeError):
        ME.MinkowskiDirectMaxPoolingFunction.apply(im, om, torch.rand(4, 3), 1)
