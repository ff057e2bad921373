"""Arithmetic across coordinate maps and the element-wise surface, the parts that need no GPU: every name the
reference's MinkowskiNonlinearity.py and MinkowskiFunctional.py export exists here (recorded list in
tests/golden/arith_reference_names.json, re-derived from the reference's sources where they are present), repr and
state-dict keys, the C symbols, the fixture's own consistency and the CPU-tensor errors."""
import ast
import json
import os
import re

import numpy as np
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = json.load(open(os.path.join(ROOT, "tests", "golden", "arith_reference_names.json")))
FIXTURE = os.path.join(ROOT, "tests", "golden", "arith_3d.npz")
SYMBOLS = ["me_union_tables"] + [f"me_union_arith_{k}{t}" for k in ("", "backward_") for t in ("f32", "bf16", "f64")]
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(ref.reference_root(), "MinkowskiEngine")),
                               reason="needs the reference package's sources")


def test_every_nonlinearity_of_the_reference_exists():
    assert len(NAMES["MinkowskiNonlinearity"]) == 29
    for name, module in NAMES["MinkowskiNonlinearity"].items():
        cls = getattr(ME, name, None)
        assert isinstance(cls, type) and issubclass(cls, torch.nn.Module), name
        if module is not None:
            assert cls.MODULE is getattr(torch.nn, module), name


def test_every_functional_of_the_reference_exists():
    import torch.nn.functional as F
    assert len(NAMES["MinkowskiFunctional"]) == 46
    for name in NAMES["MinkowskiFunctional"]:
        assert callable(getattr(ME.MinkowskiFunctional, name, None)), name
        assert hasattr(F, name), name


@needs_ref
def test_recorded_names_are_the_references():
    src = os.path.join(ref.reference_root(), "MinkowskiEngine")
    tree = ast.parse(open(os.path.join(src, "MinkowskiNonlinearity.py")).read())
    classes = sorted(n.name for n in tree.body if isinstance(n, ast.ClassDef) and n.name != "MinkowskiNonlinearityBase")
    assert classes == sorted(NAMES["MinkowskiNonlinearity"])
    tree = ast.parse(open(os.path.join(src, "MinkowskiFunctional.py")).read())
    funcs = sorted(n.name for n in tree.body if isinstance(n, ast.FunctionDef) and not n.name.startswith("_"))
    assert funcs == sorted(NAMES["MinkowskiFunctional"])
    # and the package exports them under these names
    init = open(os.path.join(src, "__init__.py")).read()
    for name in classes:
        assert re.search(r"\b" + name + r"\b", init), name


def test_repr_and_state_dict_keys():
    layers = {"MinkowskiPReLU": ME.MinkowskiPReLU(), "MinkowskiSoftmax": ME.MinkowskiSoftmax(dim=1)}
    for name, layer in layers.items():
        assert repr(layer) == NAMES["repr"][name]
        assert sorted(layer.state_dict()) == NAMES["state_dict_keys"][name]
    assert layers["MinkowskiSoftmax"].module.dim == 1
    s = ME.MinkowskiSinusoidal(3, 5)
    assert (s.in_channel, s.out_channel) == (3, 5)
    assert {k: tuple(v.shape) for k, v in s.state_dict().items()} == {"kernel": (3, 5), "bias": (1, 5), "coef": (1, 5)}


def test_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "me_amd.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.SIGNATURES, s
    for i, name in enumerate(("ADD", "SUB", "MUL", "DIV")):
        assert re.search(rf"#define ME_UNION_{name} {i}\b", header)
    so = os.path.join(ROOT, "minkowskiengine_amd", "libme_amd.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.me_version() >= 220


def test_public_names():
    import MinkowskiEngineBackend._C as C
    from minkowskiengine_amd import host
    mods = [C, ME.MinkowskiEngineBackend] + ([host.native_module()] if host.native_module() is not None else [])
    for mod in mods:
        for name in ("union_arith_fw", "union_arith_bw"):
            assert hasattr(mod, name), (mod, name)
        assert hasattr(mod.CoordinateMapManagerGPU_c10, "union_arith_maps"), mod
    assert hasattr(ME, "MinkowskiUnionArithmeticFunction") and hasattr(ME, "union_arithmetic")


def test_fixture_is_consistent():
    """numpy over the .npz alone: the reference's rule (fn(a, b) | a | fn(0, b)) and its gradients"""
    assert os.path.getsize(FIXTURE) < 1 << 20
    z = np.load(FIXTURE)
    fns = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}
    for pair in ("overlap", "nested"):
        ca, cb, cu = z[f"{pair}/a"], z[f"{pair}/b"], z[f"{pair}/out_coords"]
        for c in (ca, cb, cu):
            assert len({tuple(r) for r in c.tolist()}) == len(c)              # unique per cloud
            assert set(c[:, 0].tolist()) == {0, 1}                            # two batches
        rows = [{tuple(r): i for i, r in enumerate(c.tolist())} for c in (ca, cb)]
        ia = np.array([rows[0].get(tuple(r), -1) for r in cu.tolist()])
        ib = np.array([rows[1].get(tuple(r), -1) for r in cu.tolist()])
        assert ((ia >= 0) | (ib >= 0)).all() and (ia >= 0).sum() == len(ca) and (ib >= 0).sum() == len(cb)
        shared = ((ia >= 0) & (ib >= 0)).sum()
        if pair == "nested":
            assert shared == len(cb) < len(ca)
        else:
            assert 0.3 * len(cb) <= shared <= 0.7 * len(cb) and (ib >= 0).sum() > shared and (ia >= 0).sum() > shared
        for c in (3, 32):
            fa, fb, w = z[f"{pair}/c{c}/fa"], z[f"{pair}/c{c}/fb"], z[f"{pair}/c{c}/w"]
            assert (np.abs(fb) >= 0.5).all() and (np.abs(fb) <= 2).all()
            x = np.where((ia >= 0)[:, None], fa[np.maximum(ia, 0)], np.float32(0))
            y = fb[np.maximum(ib, 0)]
            for op, fn in fns.items():
                want = np.where((ib >= 0)[:, None], fn(x, y), x)
                got = z[f"{pair}/c{c}/{op}/out"]
                assert got.dtype == np.float32 and np.isfinite(got).all()
                assert np.array_equal(got, want), (pair, c, op)
            # + and -: the gradients are gathers of w
            u_of_a = np.empty(len(ca), np.int64)
            u_of_a[ia[ia >= 0]] = np.nonzero(ia >= 0)[0]
            u_of_b = np.empty(len(cb), np.int64)
            u_of_b[ib[ib >= 0]] = np.nonzero(ib >= 0)[0]
            assert np.array_equal(z[f"{pair}/c{c}/add/grad_a"], w[u_of_a])
            assert np.array_equal(z[f"{pair}/c{c}/add/grad_b"], w[u_of_b])
            assert np.array_equal(z[f"{pair}/c{c}/sub/grad_b"], -w[u_of_b])
            assert np.array_equal(z[f"{pair}/c{c}/mul/grad_b"], w[u_of_b] * x[u_of_b])


def test_cpu_tensors_raise():
    B = ME.MinkowskiEngineBackend
    t = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        B.union_arith_fw(torch.rand(2, 3), torch.rand(2, 3), t, t, "add")
    with pytest.raises(RuntimeError):
        B.union_arith_bw(torch.rand(2, 3), torch.rand(2, 3), torch.rand(2, 3), t, t, t, t, "add")
    with pytest.raises(Exception):
        ME.SparseTensor(torch.rand(2, 3), torch.zeros(2, 4).int()) + ME.SparseTensor(torch.rand(2, 3), torch.ones(2, 4).int())

