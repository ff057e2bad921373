"""Tensor fields without a GPU: the public surface, create_splat_coordinates and the C ABI of csrc/field.hip."""
import glob
import os
import re

import numpy as np

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_SYMBOLS = ["me_field_quantize_f32", "me_field_quantize_f64", "me_field_lookup_workspace_bytes",
                 "me_field_lookup_f32", "me_field_lookup_f64", "me_field_interp_workspace_bytes",
                 "me_field_interp_map_f32", "me_field_interp_map_f64", "me_csr_from_coo_workspace_bytes",
                 "me_csr_from_coo", "me_csr_gather_f32", "me_csr_gather_bf16", "me_csr_gather_f64"]


def test_public_names():
    for name in ("TensorField", "MinkowskiInterpolation", "MinkowskiInterpolationFunction", "spmm",
                 "MinkowskiSPMMFunction", "MinkowskiSPMMAverageFunction", "create_splat_coordinates"):
        assert hasattr(ME, name), name
    for name in ("slice", "cat_slice", "interpolate", "features_at_coordinates"):
        assert hasattr(ME.SparseTensor, name), name
    for name in ("InterpolationForwardGPU", "InterpolationBackwardGPU", "coo_spmm_int32", "coo_spmm_average_int32"):
        assert hasattr(ME.MinkowskiEngineBackend, name), name
    for name in ("insert_field", "field_to_sparse_insert_and_map", "field_to_sparse_map", "exists_field_to_sparse",
                 "get_field_to_sparse_map", "field_to_sparse_keys", "get_coordinate_field", "interpolation_map_weight"):
        assert hasattr(ME.MinkowskiEngineBackend.CoordinateMapManagerGPU_c10, name), name
        assert hasattr(ME.CoordinateManager, name), name


def test_create_splat_coordinates():
    c = torch.tensor([[0, 0.5, -1.25], [1, 2.0, 3.75]])
    got = ME.create_splat_coordinates(c)
    want = torch.tensor([[0, 0, -2], [0, 0, -1], [0, 1, -2], [0, 1, -1],
                         [1, 2, 3], [1, 2, 4], [1, 3, 3], [1, 3, 4]], dtype=torch.int32)
    assert got.dtype == torch.int32
    assert torch.equal(got, want)


def test_field_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    for s in FIELD_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.SIGNATURES, s
    so = os.path.join(ROOT, "minkowskiengine_amd", "libme_amd.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    lib = _lib.load()
    for s in FIELD_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.me_version() >= 180


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError):
        ME.TensorField(torch.rand(4, 2), coordinates=torch.rand(4, 4))


def test_max_pool_names_missing_function():
    import inspect
    from minkowskiengine_amd import tensor_field
    assert "MinkowskiDirectMaxPoolingFunction" in inspect.getsource(tensor_field.TensorField.sparse)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "field_*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_field_fixture_self_consistency(path):
    """the reference's interpolation weights: per point at most 1, exactly 1 when every corner is present"""
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    D = int(z["D"])
    out, w = z["ref_out"], z["ref_w"].astype(np.float64)
    nq = z["queries"].shape[0]
    tot = np.bincount(out, weights=w, minlength=nq)
    cnt = np.bincount(out, minlength=nq)
    assert (w >= 0).all() and (tot <= 1 + 1e-6).all()
    full = cnt == (1 << D)
    assert full.any()
    np.testing.assert_allclose(tot[full], 1.0, atol=1e-6)
    assert (cnt[-8:] == 0).all()                      # the far queries have no present corner
    assert (cnt <= (1 << D)).all() and z["inverse_map"].max() < z["sparse_coords"].shape[0]
