"""CPU checks of RegionType.CUSTOM (no GPU needed): validation and normalisation of the offsets in KernelGenerator, the
kernel volume, hybrid_region_offsets, the `use_mm` rule of the convolution modules, the C ABI's region volume and the
hybrid-kernel example's command line."""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVEN = [[5, 0, 0], [-5, 1, 0], [0, 2, -1], [1, 1, 1], [0, -3, 0], [2, 0, 4], [-1, -1, -5]]


def _kg(ME, offsets, D=3, **kw):
    return ME.KernelGenerator(region_type=ME.RegionType.CUSTOM, region_offsets=offsets, dimension=D, **kw)


@pytest.mark.parametrize("bad,what", [
    ([], "empty list"),
    (torch.IntTensor(), "empty tensor"),
    (torch.zeros((0, 3), dtype=torch.int32), "no rows"),
    (None, "no offsets at all"),
    ([[1, 0], [0, 1]], "wrong width"),
    ([1, 0, 0], "one-dimensional"),
    ([[1, 0, 0], [0, 1, 0], [1, 0, 0]], "duplicate rows"),
    ([[0.5, 0.0, 0.0]], "not integers"),
])
def test_invalid_offsets_raise(bad, what):
    import minkowskiengine_amd as ME
    with pytest.raises((ValueError, RuntimeError)) as e:
        _kg(ME, bad)
    assert "region_offsets" in str(e.value) or "offset" in str(e.value), what


def test_the_messages_name_the_problem():
    import minkowskiengine_amd as ME
    with pytest.raises(ValueError, match="non-empty"):
        _kg(ME, [])
    with pytest.raises(ValueError, match="2 columns.*dimension 3"):
        _kg(ME, [[1, 0], [0, 1]])
    with pytest.raises(ValueError, match="duplicate rows"):
        _kg(ME, [[1, 0, 0], [1, 0, 0]])


@pytest.mark.parametrize("make", [
    lambda o: o,
    lambda o: np.asarray(o, np.int64),
    lambda o: torch.tensor(o, dtype=torch.int64),
    lambda o: torch.tensor(o, dtype=torch.int16),
    lambda o: torch.tensor(o, dtype=torch.int32).t().contiguous().t(),      # not contiguous
], ids=["list", "ndarray", "int64", "int16", "strided"])
def test_lists_arrays_and_tensors_are_accepted_and_normalised(make):
    import minkowskiengine_amd as ME
    kg = _kg(ME, make(SEVEN))              # (kernel_size stays at its default -1: not used by a CUSTOM region)
    assert kg.kernel_volume == 7
    t = kg.region_offsets
    assert t.dtype == torch.int32 and t.device.type == "cpu" and t.is_contiguous() and t.tolist() == SEVEN
    assert "kernel_volume=7" in repr(kg) and "CUSTOM" in repr(kg)
    # rows in any order, the origin need not be present; the built-in regions keep an empty tensor
    assert ME.KernelGenerator(kernel_size=3, dimension=3).region_offsets.numel() == 0


def test_normalised_offsets_do_not_follow_the_callers_tensor():
    import minkowskiengine_amd as ME
    src = torch.tensor(SEVEN, dtype=torch.int32)
    kg = _kg(ME, src)
    src[0, 0] = 99
    assert kg.region_offsets.tolist() == SEVEN


def _hybrid(ME, types, ks=3, D=None):
    t = {"cube": ME.RegionType.HYPER_CUBE, "cross": ME.RegionType.HYPER_CROSS}
    return ME.hybrid_region_offsets([t[a] for a in types], ks, D or len(types))


def test_hybrid_cube_cross_4d():
    import minkowskiengine_amd as ME
    o = _hybrid(ME, ["cube", "cube", "cube", "cross"])
    assert o.dtype == torch.int32 and tuple(o.shape) == (29, 4)
    rows = [tuple(r) for r in o.tolist()]
    assert len(set(rows)) == 29 and rows[0] == (0, 0, 0, 0)
    # the documented order: origin, the cube without the origin (first axis fastest, t = 0), then the temporal taps
    cube = [(x, y, z, 0) for z, y, x in itertools.product((-1, 0, 1), repeat=3) if (x, y, z) != (0, 0, 0)]
    assert rows[1:27] == cube
    assert rows[27:] == [(0, 0, 0, 1), (0, 0, 0, -1)]
    assert _kg(ME, o, D=4).kernel_volume == 29
    for word in ("origin", "HYPER_CUBE", "HYPER_CROSS", "order"):
        assert word in ME.hybrid_region_offsets.__doc__


def test_hybrid_all_cube_and_all_cross():
    import minkowskiengine_amd as ME
    cube = _hybrid(ME, ["cube"] * 3)
    assert tuple(cube.shape) == (27, 3)
    assert {tuple(r) for r in cube.tolist()} == set(itertools.product((-1, 0, 1), repeat=3))
    cross = _hybrid(ME, ["cross"] * 3)
    assert [tuple(r) for r in cross.tolist()] == [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1),
                                                  (0, 0, -1)]
    # sizes per axis; even sizes start at 0 on a cube axis and are refused on a cross axis
    o = ME.hybrid_region_offsets([ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS], [2, 5], 2)
    assert [tuple(r) for r in o.tolist()] == [(0, 0), (1, 0), (0, 1), (0, 2), (0, -2), (0, -1)]
    with pytest.raises(ValueError):
        ME.hybrid_region_offsets([ME.RegionType.HYPER_CROSS] * 2, 2, 2)
    with pytest.raises(ValueError):
        ME.hybrid_region_offsets([ME.RegionType.HYPER_CUBE] * 2, 3, 3)


def test_use_mm_only_for_the_origin():
    import minkowskiengine_amd as ME
    origin = ME.MinkowskiConvolution(4, 6, kernel_generator=_kg(ME, [[0, 0, 0]]), dimension=3)
    assert origin.use_mm and tuple(origin.kernel.shape) == (4, 6)
    shift = ME.MinkowskiConvolution(4, 6, kernel_generator=_kg(ME, [[1, 0, 0]]), dimension=3)
    assert not shift.use_mm and tuple(shift.kernel.shape) == (1, 4, 6)
    strided = ME.MinkowskiConvolution(4, 6, kernel_generator=_kg(ME, [[0, 0, 0]], stride=2), dimension=3)
    assert not strided.use_mm and tuple(strided.kernel.shape) == (1, 4, 6)
    seven = ME.MinkowskiConvolution(4, 6, kernel_generator=_kg(ME, SEVEN), dimension=3)
    assert tuple(seven.kernel.shape) == (7, 4, 6)
    assert "kernel_volume=7" in repr(seven)
    assert tuple(ME.MinkowskiChannelwiseConvolution(5, kernel_generator=_kg(ME, SEVEN), dimension=3).kernel.shape) == (7, 5)


def test_region_volume_of_a_custom_region_is_its_row_count():
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    offs = torch.tensor(SEVEN, dtype=torch.int32)
    rg = _lib.make_region(4, _lib.ME_REGION_CUSTOM, [-1] * 3, [1] * 3, [2] * 3, offs)
    assert rg.n_offsets == 7 and not rg.offsets_dev            # (no device: the volume reads no table)
    assert lib.me_region_volume(ctypes.byref(rg)) == 7
    rg.n_offsets = 0
    assert lib.me_region_volume(ctypes.byref(rg)) == -1
    # the built-in regions leave the trailing fields zero
    cube = _lib.make_region(4, 0, [3] * 3, [1] * 3, [1] * 3)
    assert cube.n_offsets == 0 and not cube.offsets_dev and lib.me_region_volume(ctypes.byref(cube)) == 27
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    assert "#define ME_REGION_CUSTOM 2" in header


def test_hybrid_example_command_line():
    """examples/hybrid_kernel_4d.py imports without a GPU; its parser and its 29-tap generator work on the host"""
    import minkowskiengine_amd as ME
    spec = importlib.util.spec_from_file_location("hybrid_kernel_4d", os.path.join(ROOT, "examples", "hybrid_kernel_4d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = mod.build_parser().format_help()
    assert "--points" in text and "--frames" in text
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    assert mod.hybrid_generator(ME).kernel_volume == 29
    net = mod.HybridNet(ME, 3, 8)
    assert tuple(net.conv1.kernel.shape) == (29, 3, 8) and tuple(net.conv2.kernel.shape) == (29, 8, 8)
    assert mod.synthetic_scene(100, 8, 3).shape[1] == 5
