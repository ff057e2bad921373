"""CPU-side checks of the dense <-> sparse conversion feature (no GPU needed): exported names and their kinds, reprs,
`dense_coordinates` against the reference's fixture, `to_sparse`'s format assertions, agreement of header, ctypes table
and both host layers on the new entry points, the fixtures themselves (they load, stay below the size limit and satisfy
the plain restatement of the rule), the host-only policy, and that CPU tensors raise (there is no CPU path)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "dense_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]
ENTRY_POINTS = ("me_dense_policy", "me_dense_cell_index", "me_dense_grid", "me_dense_rows_to_box", "me_dense_box_to_rows",
                "me_dense_occupied_workspace_bytes", "me_dense_occupied_count", "me_dense_occupied_fill",
                "me_dense_all_coords")
OPERATORS = ("DensePolicy", "DenseCellIndexGPU", "DenseGridGPU", "DenseRowsToBoxGPU", "DenseBoxToRowsGPU",
             "DenseOccupiedGPU", "DenseCoordinatesGPU")


def test_names_are_exported_and_of_the_right_kind():
    for name in ("to_sparse", "to_sparse_all", "dense_coordinates", "sum", "mean", "var", "cat"):
        assert callable(getattr(ME, name)), name
    for name in ("MinkowskiToSparseTensor", "MinkowskiToDenseTensor", "MinkowskiToFeature"):
        assert issubclass(getattr(ME, name), torch.nn.Module), name
    for name in ("MinkowskiStackCat", "MinkowskiStackSum", "MinkowskiStackMean", "MinkowskiStackVar"):
        assert issubclass(getattr(ME, name), torch.nn.Sequential), name
    for name in ("MinkowskiToDenseFunction", "MinkowskiToSparseFunction"):
        assert issubclass(getattr(ME, name), torch.autograd.Function), name
    for name in ("dense", "sparse", "double", "get_device", "coordinates_at", "features_at", "coordinates_and_features_at"):
        assert callable(getattr(ME.SparseTensor, name)), name
    for name in ("decomposition_permutations", "decomposed_coordinates_and_features"):
        assert isinstance(getattr(ME.SparseTensor, name), property), name


def test_reprs():
    assert repr(ME.MinkowskiToSparseTensor()) == "MinkowskiToSparseTensor()"
    assert repr(ME.MinkowskiToDenseTensor(torch.Size([1, 2, 3, 4]))) == "MinkowskiToDenseTensor()"
    m = ME.MinkowskiToSparseTensor(remove_zeros=False, coordinates=ME.dense_coordinates((1, 2, 3, 4)))
    assert m.remove_zeros is False and m.coordinates.shape == (12, 3)
    assert ME.MinkowskiToDenseTensor().shape is None


def test_dense_coordinates_equal_the_reference():
    z = np.load(os.path.join(GOLDEN_DIR, "dense_coordinates_4d.npz"))
    got = ME.dense_coordinates(torch.Size(z["shape"].tolist()))
    assert got.dtype == torch.int32 and not got.is_cuda and got.is_contiguous()
    assert np.array_equal(got.numpy(), z["coords"])
    assert np.array_equal(ME.dense_coordinates(z["shape"].tolist()).numpy(), z["coords"])      # a list, as the reference takes
    with pytest.raises(AssertionError):
        ME.dense_coordinates((2, 3))


def test_format_assertions():
    x = torch.zeros(2, 3, 4, 5)
    for bad in ("BCX", "CBXX", "BBXX", "BXXX", "BCCX", "XCXB"):
        with pytest.raises(AssertionError):
            ME.to_sparse(x, format=bad)
    with pytest.raises(AssertionError):
        ME.to_sparse(torch.zeros(2, 3))
    with pytest.raises(AssertionError):
        ME.to_sparse_all(torch.zeros(2, 3))


def test_cpu_tensors_raise():
    x = torch.rand(2, 3, 4, 5)
    for call in (lambda: ME.to_sparse(x), lambda: ME.to_sparse(x, format="BXXC"), lambda: ME.to_sparse_all(x),
                 lambda: ME.MinkowskiToSparseTensor()(x),
                 lambda: ME.MinkowskiToDenseFunction.apply(torch.rand(4, 3), torch.zeros(4, dtype=torch.int64), None, 2, 20),
                 lambda: ME.MinkowskiToSparseFunction.apply(x, None, 40, 2, 20)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    with pytest.raises(ValueError):
        ME.MinkowskiToSparseTensor()("not a tensor")


def test_header_prototypes_and_both_hosts_list_the_entry_points():
    from minkowskiengine_amd import _lib, backend, host
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    declared = set(re.findall(r"\b(me_dense_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(ENTRY_POINTS)
    assert {s for s in _lib.SIGNATURES if s.startswith("me_dense_")} == set(ENTRY_POINTS)
    lib = _lib.load()
    assert lib.me_version() >= 200
    for s in ENTRY_POINTS:
        assert hasattr(lib, s)
    native = host.native_module()
    assert native is not None, host.native_error()
    for op in OPERATORS:
        assert callable(getattr(backend, op)), op
        assert callable(getattr(native, op)), op
    assert (native.DENSE_ROW_STATIONARY, native.DENSE_CELL_STATIONARY) == \
        (backend.DENSE_ROW_STATIONARY, backend.DENSE_CELL_STATIONARY) == (1, 2)
    bind = open(os.path.join(ROOT, "minkowskiengine_amd", "csrc_host", "bind.cpp")).read()
    for op in OPERATORS[1:]:
        body = bind[bind.index(f'm.def("{op}"'):]
        assert "gil_scoped_release" in body[:body.index("m.def(", 10)], op
    import MinkowskiEngineBackend._C as C
    for op in OPERATORS:
        assert hasattr(C, op), op


def test_policy_is_the_byte_model_on_both_hosts():
    from minkowskiengine_amd import backend, host
    native = host.native_module()
    for n, cells, c, e in ((100000, 70 ** 3, 64, 4), (100000, 215 ** 3, 64, 4), (200000, 2 * 128 ** 3, 96, 2),
                           (1000, 10 ** 6, 1, 4), (5, 64, 3, 8)):
        for to_box in (True, False):
            box, rows = cells * c * e, n * c * e
            cell_cost = (2.5 if to_box else 1.0) * box + rows + 8 * cells
            row_cost = (box if to_box else 0) + rows + (256 if to_box else 64) * n * c
            want = 2 if cell_cost <= row_cost else 1
            assert backend.DensePolicy(n, cells, c, e, to_box) == want
            assert native.DensePolicy(n, cells, c, e, to_box) == want
    assert backend.DensePolicy(100000, 70 ** 3, 64, 4, False) == 2        # occupancy 0.29: read the box once
    assert backend.DensePolicy(100000, 215 ** 3, 64, 4, False) == 1       # occupancy 0.01: gather the rows
    assert backend.DensePolicy(100000, 70 ** 3, 64, 4, True) == 2         # one pass over the box, no zero fill
    assert backend.DensePolicy(100000, 215 ** 3, 64, 4, True) == 1        # measured: zero fill + scatter wins at 0.01
    assert backend.DensePolicy(200000, 2 * 128 ** 3, 96, 2, True) == 2    # measured: the tile kernel wins at 0.048


def _dense_np(coords, feats, shape, mn, div):
    out = np.zeros(shape, dtype=feats.dtype)
    idx = (coords[:, 1:].astype(np.int64) - mn.astype(np.int64)) // div
    for r in range(coords.shape[0]):
        out[(int(coords[r, 0]), slice(None)) + tuple(int(v) for v in idx[r])] = feats[r]
    return out


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fixture_loads_is_small_and_satisfies_the_restatement(path):
    assert os.path.getsize(path) < (1 << 20)
    z = np.load(path)
    kind, source = str(z["kind"]), str(z["source"])
    assert source in ("reference", "restatement")
    if kind == "dense":
        D = z["coords"].shape[1] - 1
        div = np.full(D, int(z["tensor_stride"]) if bool(z["contract"]) else 1, dtype=np.int64)
        want = _dense_np(z["coords"], z["feats"], z["dense"].shape, z["min_coordinate"], div)
        assert np.array_equal(want, z["dense"])
        assert z["dense"].shape[1] == z["feats"].shape[1]
        assert source == "reference" or str(z["min_arg"]) == "zero"
    elif kind in ("to_sparse", "module", "to_sparse_all"):
        x = z["x"]
        fmt = str(z["format"]) if "format" in z.files else ""
        ch = fmt.find("C") if fmt else 1
        keep_all = kind == "to_sparse_all" or (kind == "module" and not (bool(z["remove_zeros"]) and
                                                                         bool(z["with_coordinates"])))
        mask = np.ones([s for k, s in enumerate(x.shape) if k != ch], dtype=bool) if keep_all else np.abs(x).sum(ch) != 0
        assert np.array_equal(np.argwhere(mask).astype(np.int32), z["coords"])
        assert np.array_equal(np.moveaxis(x, ch, -1)[mask], z["feats"])
        assert source == "reference"
    elif kind == "dense_coordinates":
        shape = z["shape"].tolist()
        assert np.array_equal(np.argwhere(np.ones([shape[0]] + shape[2:], dtype=bool)), z["coords"])
    else:
        assert kind == "sparse" and source == "restatement"
    for k in z.files:                      # data only
        assert z[k].dtype.kind in "biufU", (k, z[k].dtype)


def test_the_fixture_set_covers_the_cases():
    kinds = [str(np.load(p)["kind"]) for p in CASES]
    assert kinds.count("dense") >= 8 and kinds.count("to_sparse") >= 5 and kinds.count("module") == 3
    channels = {np.load(p)["feats"].shape[1] for p in CASES if "feats" in np.load(p).files}
    assert {1, 3, 16, 17} <= channels
