"""GPU tests of arithmetic between sparse tensors on different coordinate maps (csrc/union_arith.hip through both host
layers) against the reference's own arithmetic (tests/golden/arith_3d.npz, make_golden_arith.py), and of the thin
element-wise wrappers (the rest of MinkowskiNonlinearity.py, MinkowskiFunctional.py).

Bounds.  +, -, * in fp32: every output element and every gradient element is ONE correctly rounded IEEE operation on the
operands the reference used, so the comparison is exact (np.array_equal: value equality, +0 == -0).  `/`: 1e-6 absolute
+ 1e-6 relative, the bound test_gpu_generative.py::test_union holds union features to (torch may round the division's
derivative differently).  bf16: exact against fn(a.float(), b.float()).bfloat16() row by row.  float64: gradcheck."""
import operator
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, make_cloud, placed, row_mapping

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "arith_3d.npz")
OPS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul, "div": operator.truediv}
_Z = None


def _z():
    global _Z
    if _Z is None:
        _Z = np.load(FIXTURE)
    return _Z


def _me():
    import minkowskiengine_amd as ME
    return ME


def _pair(device, ca, cb, fa, fb, requires_grad=(False, False)):
    ME = _me()
    as_t = lambda v: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(device)
    fa, fb = as_t(fa).requires_grad_(requires_grad[0]), as_t(fb).requires_grad_(requires_grad[1])
    a = ME.SparseTensor(fa, as_t(ca))
    b = ME.SparseTensor(fb, as_t(cb), coordinate_manager=a.coordinate_manager)
    assert a.coordinate_map_key != b.coordinate_map_key
    return a, b, fa, fb


def _tables(ca, cb, cu):
    """a_of_u / b_of_u of union coordinates cu, by coordinate (numpy, -1 = absent)"""
    out = []
    for c in (ca, cb):
        rows = {tuple(r): i for i, r in enumerate(np.asarray(c).tolist())}
        out.append(np.array([rows.get(tuple(r), -1) for r in np.asarray(cu).tolist()], np.int64))
    return out


def _expected(fn, fa, fb, ia, ib):
    """the reference's rule restated with torch on the CPU: fn(a, b) | a | fn(0, b)"""
    x = torch.where(torch.from_numpy(ia >= 0)[:, None], fa[np.maximum(ia, 0)], torch.zeros((), dtype=fa.dtype))
    y = fb[np.maximum(ib, 0)]
    return torch.where(torch.from_numpy(ib >= 0)[:, None], fn(x, y), x)


@pytest.mark.parametrize("c", [3, 32])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("pair", ["overlap", "nested"])
def test_reference_fixture(pair, op, c, host_layer, device):
    z = _z()
    a, b, fa, fb = _pair(device, z[f"{pair}/a"], z[f"{pair}/b"], z[f"{pair}/c{c}/fa"], z[f"{pair}/c{c}/fb"], (True, True))
    out = OPS[op](a, b)
    m = row_mapping(out.C.cpu().numpy(), z[f"{pair}/out_coords"])
    got, want = out.F.detach().cpu().numpy(), z[f"{pair}/c{c}/{op}/out"][m]
    w = torch.from_numpy(z[f"{pair}/c{c}/w"][m]).to(device)
    (out.F * w).sum().backward()
    ga, gb = fa.grad.cpu().numpy(), fb.grad.cpu().numpy()
    print(f"{pair} {op} c={c} {host_layer}: max |diff| out {np.abs(got - want).max():.3e} "
          f"grad_a {np.abs(ga - z[f'{pair}/c{c}/{op}/grad_a']).max():.3e} "
          f"grad_b {np.abs(gb - z[f'{pair}/c{c}/{op}/grad_b']).max():.3e}")
    if op == "div":
        assert_close(got, want, 1e-6, 1e-6, "out")
        assert_close(ga, z[f"{pair}/c{c}/{op}/grad_a"], 1e-6, 1e-6, "grad_a")
        assert_close(gb, z[f"{pair}/c{c}/{op}/grad_b"], 1e-6, 1e-6, "grad_b")
    else:
        assert np.array_equal(got, want)
        assert np.array_equal(ga, z[f"{pair}/c{c}/{op}/grad_a"])
        assert np.array_equal(gb, z[f"{pair}/c{c}/{op}/grad_b"])


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("pair", ["overlap", "nested"])
def test_bf16_rounds_once(pair, op, host_layer, device):
    z = _z()
    fa = torch.from_numpy(z[f"{pair}/c32/fa"]).bfloat16()
    fb = torch.from_numpy(z[f"{pair}/c32/fb"]).bfloat16()
    a, b, _, _ = _pair(device, z[f"{pair}/a"], z[f"{pair}/b"], fa, fb)
    out = OPS[op](a, b)
    assert out.F.dtype == torch.bfloat16
    ia, ib = _tables(z[f"{pair}/a"], z[f"{pair}/b"], out.C.cpu().numpy())
    want = _expected(OPS[op], fa.float(), fb.float(), ia, ib).bfloat16()
    assert torch.equal(out.F.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("c", [1, 3, 6, 32, 96, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_channel_counts(c, dtype, host_layer, device):
    """every vector width of the kernel (16-byte, 8-byte, single channels) against the rule restated with torch"""
    ca, cb = make_cloud(900, 12, seed=1, batch=2), make_cloud(700, 12, seed=2, batch=2)
    g = torch.Generator().manual_seed(c)
    fa, fb = torch.randn(ca.shape[0], c, generator=g).to(dtype), (torch.rand(cb.shape[0], c, generator=g) + 0.5).to(dtype)
    a, b, xa, xb = _pair(device, ca, cb, fa, fb, (True, True))
    up = (lambda t: t.float()) if dtype == torch.bfloat16 else (lambda t: t)
    for op, fn in OPS.items():
        out = fn(a, b)
        ia, ib = _tables(ca, cb, out.C.cpu().numpy())
        assert ((ia >= 0) | (ib >= 0)).all() and (ia >= 0).sum() == len(ca) and (ib >= 0).sum() == len(cb)
        ra, rb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
        want = _expected(fn, up(ra), up(rb), ia, ib).to(dtype)
        assert torch.equal(out.F.detach().cpu(), want.detach()), op
        w = torch.rand(out.F.shape, generator=g).to(dtype)
        xa.grad = xb.grad = None
        (out.F * w.to(device)).sum().backward()
        (want * w).sum().backward()
        tol = {torch.float32: 1e-6, torch.float64: 1e-12, torch.bfloat16: 2 ** -7}[dtype]
        assert_close(xa.grad.double().cpu().numpy(), ra.grad.double().numpy(), tol, tol, f"{op} grad_a")
        assert_close(xb.grad.double().cpu().numpy(), rb.grad.double().numpy(), tol, tol, f"{op} grad_b")


_WIDTH_CASES = [(torch.float32, 8), (torch.float32, 6), (torch.float32, 7), (torch.bfloat16, 16), (torch.bfloat16, 12),
                (torch.bfloat16, 7), (torch.float64, 4), (torch.float64, 3)]


@pytest.mark.parametrize("dtype,c", _WIDTH_CASES, ids=[f"{str(d)[6:]}-c{c}" for d, c in _WIDTH_CASES])
def test_piece_widths_and_unaligned_views(dtype, c, device):
    """The piece width of the forward and of both backward kernels follows c and the addresses (16 bytes, 8 bytes, one
    channel: fp32 c = 8 / 6 / 7, bf16 16 / 12 / 7, float64 4 / 3); the operators are element-wise, so no address may
    change a bit.  Every feature tensor of the C entry points (a, b, out; grad_out, a, b, grad_a, grad_b), one at a time
    and all together, goes 8 bytes and one element into its storage: results and gradients bit-equal to the call on
    allocator addresses, which is the backend's own."""
    from minkowskiengine_amd import _lib, backend
    lib = _lib.load()
    sfx = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64"}[dtype]
    fw, bw = getattr(lib, "me_union_arith_" + sfx), getattr(lib, "me_union_arith_backward_" + sfx)
    rng = np.random.default_rng(c)
    na = nb = 600
    nu = 900                                                # 300 rows of each input are the other's too
    u_of_a = rng.permutation(nu)[:na]
    b_only = np.setdiff1d(np.arange(nu), u_of_a)
    u_of_b = rng.permutation(np.concatenate([b_only, rng.choice(u_of_a, nb - len(b_only), replace=False)]))
    a_of_u, b_of_u = np.full(nu, -1), np.full(nu, -1)
    a_of_u[u_of_a], b_of_u[u_of_b] = np.arange(na), np.arange(nb)
    ua, ub, au, bu = (torch.from_numpy(v.astype(np.int32)).to(device) for v in (u_of_a, u_of_b, a_of_u, b_of_u))
    g = torch.Generator().manual_seed(c)
    a = torch.randn(na, c, generator=g).to(dtype).to(device)
    b = (torch.rand(nb, c, generator=g) + 0.5).to(dtype).to(device)
    go = torch.randn(nu, c, generator=g).to(dtype).to(device)
    bits = lambda t: t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])  # noqa: E731
    stream = torch.cuda.current_stream(device).cuda_stream

    def forward(code, how):
        pa, pb, out = placed(a, how["a"]), placed(b, how["b"]), placed(torch.zeros_like(go), how["out"])
        with torch.cuda.device(device):
            _lib.check(fw(pa.data_ptr(), pb.data_ptr(), c, au.data_ptr(), bu.data_ptr(), na, nb, nu, code, out.data_ptr(),
                          stream))
        return [bits(out)]

    def backward(code, how):
        pg, pa, pb = placed(go, how["g"]), placed(a, how["a"]), placed(b, how["b"])
        ga, gb = placed(torch.zeros_like(a), how["ga"]), placed(torch.zeros_like(b), how["gb"])
        with torch.cuda.device(device):
            _lib.check(bw(pg.data_ptr(), pa.data_ptr(), pb.data_ptr(), c, ua.data_ptr(), ub.data_ptr(), au.data_ptr(),
                          bu.data_ptr(), na, nb, nu, code, ga.data_ptr(), gb.data_ptr(), stream))
        return [bits(ga), bits(gb)]

    for op in OPS:
        code = backend._union_arith_op(op)
        for run, names in ((forward, ("a", "b", "out")), (backward, ("g", "a", "b", "ga", "gb"))):
            base = dict.fromkeys(names, "alloc")
            want = run(code, base)
            mine = [backend.union_arith_fw(a, b, au, bu, op)] if run is forward else \
                backend.union_arith_bw(go, a, b, ua, ub, au, bu, op)
            assert all(torch.equal(w, bits(m)) for w, m in zip(want, mine)), op
            for off in ("8", "1"):
                for how in [dict(base, **{n: off}) for n in names] + [dict.fromkeys(names, off)]:
                    got = run(code, how)
                    assert all(torch.equal(w, v) for w, v in zip(want, got)), (op, run.__name__, how)


@pytest.mark.parametrize("op", list(OPS))
def test_gradcheck_float64(op, host_layer, device):
    ca, cb = make_cloud(40, 4, seed=3, batch=2), make_cloud(30, 4, seed=4, batch=2)
    g = torch.Generator().manual_seed(5)
    fa = torch.randn(ca.shape[0], 5, generator=g, dtype=torch.float64)
    fb = torch.rand(cb.shape[0], 5, generator=g, dtype=torch.float64) + 0.5
    a, b, xa, xb = _pair(device, ca, cb, fa, fb, (True, True))
    ME = _me()

    def f(u, v):
        return OPS[op](ME.SparseTensor(u, coordinate_map_key=a.coordinate_map_key, coordinate_manager=a.coordinate_manager),
                       ME.SparseTensor(v, coordinate_map_key=b.coordinate_map_key,
                                       coordinate_manager=a.coordinate_manager)).F
    assert torch.autograd.gradcheck(f, (xa, xb), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("op", ["add", "sub"])
def test_dense_of_result_is_result_of_dense(op, host_layer, device):
    ca, cb = make_cloud(500, 10, seed=6, batch=2), make_cloud(400, 10, seed=7, batch=2)
    g = torch.Generator().manual_seed(8)
    a, b, _, _ = _pair(device, ca, cb, torch.randn(ca.shape[0], 4, generator=g), torch.randn(cb.shape[0], 4, generator=g))
    shape, lo = torch.Size([2, 4, 10, 10, 10]), torch.zeros(3, dtype=torch.int32)
    da, db, du = a.dense(shape, lo)[0], b.dense(shape, lo)[0], OPS[op](a, b).dense(shape, lo)[0]
    assert torch.equal(du, OPS[op](da, db))


def test_rows_only_one_side_holds(host_layer, device):
    """a-only rows of a * b are a (not 0); b-only rows of a / b are 0 / b: 0, and NaN where b is 0 (one planted)"""
    ca, cb = make_cloud(300, 8, seed=9, batch=2), make_cloud(300, 8, seed=10, batch=2)
    g = torch.Generator().manual_seed(11)
    fa, fb = torch.randn(ca.shape[0], 3, generator=g), torch.rand(cb.shape[0], 3, generator=g) + 0.5
    ia0, _ = _tables(ca, cb, cb)
    planted = int(np.nonzero(ia0 < 0)[0][0])                # a row of b that a does not hold
    fb[planted, 1] = 0.0
    a, b, _, _ = _pair(device, ca, cb, fa, fb)
    prod, quot = a * b, a / b
    assert prod.coordinate_map_key == quot.coordinate_map_key
    ia, ib = _tables(ca, cb, prod.C.cpu().numpy())
    a_only, b_only = (ia >= 0) & (ib < 0), (ia < 0) & (ib >= 0)
    assert a_only.any() and b_only.any()
    assert torch.equal(prod.F.cpu()[a_only], fa[ia[a_only]])
    assert torch.equal(quot.F.cpu()[a_only], fa[ia[a_only]])
    q = quot.F.cpu()[b_only]
    zero_b = fb[ib[b_only]] == 0
    assert zero_b.sum() == 1
    assert torch.isnan(q[zero_b]).all() and (q[~zero_b] == 0).all()
    assert (prod.F.cpu()[b_only] == 0).all()


def test_needs_input_grad(host_layer, device):
    ca, cb = make_cloud(200, 8, seed=12), make_cloud(200, 8, seed=13)
    g = torch.Generator().manual_seed(14)
    fa, fb = torch.randn(ca.shape[0], 8, generator=g), torch.rand(cb.shape[0], 8, generator=g) + 0.5
    from minkowskiengine_amd import host
    B = host.backend()
    for need in ((True, False), (False, True)):
        a, b, xa, xb = _pair(device, ca, cb, fa.clone(), fb.clone(), need)
        out = a * b
        out.F.sum().backward()
        assert (xa.grad is not None) == need[0] and (xb.grad is not None) == need[1]
        key, u_of_a, u_of_b, a_of_u, b_of_u = a.coordinate_manager._manager.union_arith_maps(a.coordinate_map_key,
                                                                                             b.coordinate_map_key)
        ga, gb = B.union_arith_bw(torch.ones_like(out.F), a.F.detach(), b.F.detach(), u_of_a, u_of_b, a_of_u, b_of_u, "mul",
                                  need[0], need[1])
        assert (ga is not None) == need[0] and (gb is not None) == need[1]
        assert torch.equal(ga if need[0] else gb, xa.grad if need[0] else xb.grad)


def test_degenerate_pairs(host_layer, device):
    g = torch.Generator().manual_seed(15)
    ca = make_cloud(100, 6, seed=16)
    # disjoint maps
    cb = ca.clone()
    cb[:, 1] += 100
    fa, fb = torch.randn(100, 4, generator=g), torch.randn(100, 4, generator=g)
    a, b, _, _ = _pair(device, ca, cb, fa, fb)
    out = a - b
    assert len(out) == 200
    ia, ib = _tables(ca, cb, out.C.cpu().numpy())
    assert torch.equal(out.F.cpu(), _expected(operator.sub, fa, fb, ia, ib))
    # identical coordinates under different keys
    a, b, _, _ = _pair(device, ca, ca.clone(), fa, fb)
    out = a * b
    assert len(out) == 100 and out.coordinate_map_key not in (a.coordinate_map_key, b.coordinate_map_key)
    m = row_mapping(out.C.cpu().numpy(), ca.numpy())
    assert torch.equal(out.F.cpu(), (fa * fb)[m])
    # Nb = 1
    a, b, _, _ = _pair(device, ca, ca[37:38].clone(), fa, fb[:1])
    out = a + b
    assert len(out) == 100
    m = row_mapping(out.C.cpu().numpy(), ca.numpy())
    want = fa.clone()
    want[37] += fb[0]
    assert torch.equal(out.F.cpu(), want[m])


def test_union_is_cached_per_ordered_pair(host_layer, device):
    ca, cb = make_cloud(300, 8, seed=17), make_cloud(250, 8, seed=18)
    g = torch.Generator().manual_seed(19)
    fa, fb = torch.randn(ca.shape[0], 4, generator=g), torch.randn(cb.shape[0], 4, generator=g)
    a, b, _, _ = _pair(device, ca, cb, fa, fb)
    mgr = a.coordinate_manager
    s = a + b
    n_keys = len(mgr.get_coordinate_map_keys(1))
    d = a - b
    assert d.coordinate_map_key == s.coordinate_map_key
    assert len(mgr.get_coordinate_map_keys(1)) == n_keys
    assert torch.equal(d.C, s.C)
    r = b - a                                               # the other order: b's rows first, a map of its own
    assert r.coordinate_map_key != s.coordinate_map_key
    assert len(mgr.get_coordinate_map_keys(1)) == n_keys + 1
    assert torch.equal(r.C[:len(cb)].cpu(), cb) and torch.equal(s.C[:len(ca)].cpu(), ca)
    ia, ib = _tables(cb, ca, r.C.cpu().numpy())
    assert torch.equal(r.F.cpu(), _expected(operator.sub, fb, fa, ia, ib))
    # radd / iadd follow add; iadd across maps gives a new tensor
    t = a
    t += b
    assert t is not a and t.coordinate_map_key == s.coordinate_map_key and torch.equal(t.F, s.F)
    assert torch.equal(a.__radd__(b).F, s.F)


def test_bitwise_reproducible(host_layer, device):
    ca, cb = make_cloud(20000, 40, seed=20), make_cloud(15000, 40, seed=21)
    g = torch.Generator().manual_seed(22)
    fa, fb = torch.randn(ca.shape[0], 96, generator=g), torch.rand(cb.shape[0], 96, generator=g) + 0.5
    runs = []
    for _ in range(2):
        a, b, xa, xb = _pair(device, ca, cb, fa.clone(), fb.clone(), (True, True))
        out = a / b
        (out.F * out.F).sum().backward()
        runs.append((out.C.clone(), out.F.detach().clone(), xa.grad.clone(), xb.grad.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_errors(host_layer, device):
    ME = _me()
    ca, cb = make_cloud(50, 6, seed=23), make_cloud(50, 6, seed=24)
    g = torch.Generator().manual_seed(25)
    fa, fb = torch.randn(50, 4, generator=g), torch.randn(50, 4, generator=g)
    a, b, _, _ = _pair(device, ca, cb, fa, fb)
    # channel count, dtype
    b3 = ME.SparseTensor(fb[:, :3].to(device), coordinate_map_key=b.coordinate_map_key,
                         coordinate_manager=a.coordinate_manager)
    with pytest.raises(AssertionError):
        a + b3
    bd = ME.SparseTensor(fb.double().to(device), coordinate_map_key=b.coordinate_map_key,
                         coordinate_manager=a.coordinate_manager)
    with pytest.raises(AssertionError):
        a + bd
    # another manager
    other = ME.SparseTensor(fb.to(device), cb.to(device))
    with pytest.raises(AssertionError):
        a + other
    # another tensor stride
    b2 = ME.SparseTensor(fb.to(device), (cb * 2).to(device), tensor_stride=2, coordinate_manager=a.coordinate_manager)
    with pytest.raises(Exception, match="[Ii]nvalid tensor stride"):
        a + b2
    # CPU tensors
    with pytest.raises(Exception):
        ME.SparseTensor(fa, ca) + ME.SparseTensor(fb, cb)
    # the operator entry points check their tables
    from minkowskiengine_amd import host
    B = host.backend()
    key, u_of_a, u_of_b, a_of_u, b_of_u = a.coordinate_manager._manager.union_arith_maps(a.coordinate_map_key,
                                                                                         b.coordinate_map_key)
    with pytest.raises(Exception):
        B.union_arith_fw(a.F, b.F, a_of_u[:-1], b_of_u, "add")
    with pytest.raises(Exception):
        B.union_arith_fw(a.F, b.F, a_of_u.long(), b_of_u.long(), "add")
    with pytest.raises(Exception):
        B.union_arith_fw(a.F, b.F, a_of_u, b_of_u, "pow")


def test_hosts_agree_bitwise(device):
    ME = _me()
    ca, cb = make_cloud(3000, 20, seed=26, batch=2), make_cloud(2000, 20, seed=27, batch=2)
    g = torch.Generator().manual_seed(28)
    fa, fb = torch.randn(ca.shape[0], 32, generator=g), torch.rand(cb.shape[0], 32, generator=g) + 0.5
    prev, res = ME.get_host(), {}
    try:
        for h in ("python", "native"):
            ME.set_host(h)
            a, b, xa, xb = _pair(device, ca, cb, fa.clone(), fb.clone(), (True, True))
            out = a / b
            (out.F * out.F).sum().backward()
            res[h] = (out.C.cpu(), out.F.detach().cpu(), xa.grad.cpu(), xb.grad.cpu())
    finally:
        ME.set_host(prev)
    for u, v in zip(res["python"], res["native"]):
        assert torch.equal(u, v)


# ---- the thin wrappers -------------------------------------------------------------------------------------------------
_MODULES = [("PReLU", ()), ("ReLU6", ()), ("SELU", ()), ("CELU", ()), ("GELU", ()), ("SiLU", ()), ("Hardshrink", ()),
            ("Hardsigmoid", ()), ("Hardtanh", ()), ("Hardswish", ()), ("LogSigmoid", ()), ("Softplus", ()),
            ("Softshrink", ()), ("Softsign", ()), ("Tanhshrink", ()), ("Threshold", (0.1, 20.0)), ("Softmin", (1,)),
            ("Softmax", (1,)), ("LogSoftmax", (1,))]
_FUNCTIONALS = [("threshold", (0.1, 20.0)), ("relu", ()), ("hardtanh", ()), ("hardswish", ()), ("relu6", ()), ("elu", ()),
                ("selu", ()), ("celu", ()), ("leaky_relu", ()), ("glu", ()), ("gelu", ()), ("logsigmoid", ()),
                ("hardshrink", ()), ("tanhshrink", ()), ("softsign", ()), ("softplus", ()), ("softmin", (1,)),
                ("softmax", (1,)), ("softshrink", ()), ("log_softmax", (1,)), ("tanh", ()), ("sigmoid", ()),
                ("hardsigmoid", ()), ("silu", ()), ("normalize", ())]


def _inputs(device):
    ME = _me()
    g = torch.Generator().manual_seed(29)
    coords = make_cloud(200, 8, seed=30, batch=2)
    st = ME.SparseTensor(torch.randn(coords.shape[0], 6, generator=g).to(device), coords.to(device))
    pts = torch.cat([torch.randint(0, 2, (300, 1), generator=g).float(), torch.rand(300, 3, generator=g) * 8], 1)
    tf = ME.TensorField(torch.randn(300, 6, generator=g).to(device), pts.to(device))
    return st, tf


def _same_place(y, x):
    ME = _me()
    assert type(y) is type(x)
    if isinstance(x, ME.TensorField):
        assert y.coordinate_field_map_key == x.coordinate_field_map_key
    else:
        assert y.coordinate_map_key == x.coordinate_map_key
    assert y.coordinate_manager is x.coordinate_manager


@pytest.mark.parametrize("name,args", _MODULES, ids=[m[0] for m in _MODULES])
def test_nonlinearity_modules(name, args, host_layer, device):
    ME = _me()
    layer = getattr(ME, "Minkowski" + name)(*args).to(device)
    assert isinstance(layer.module, getattr(torch.nn, name))
    for x in _inputs(device):
        y = layer(x)
        _same_place(y, x)
        assert torch.equal(y.F, layer.module(x.F))


def test_random_and_parametric_modules(host_layer, device):
    ME = _me()
    for x in _inputs(device):
        for layer in (ME.MinkowskiRReLU(), ME.MinkowskiAlphaDropout(0.3)):
            layer = layer.to(device)
            torch.manual_seed(3)
            y = layer(x)
            torch.manual_seed(3)
            assert torch.equal(y.F, layer.module(x.F))
            _same_place(y, x)
            layer.eval()
            assert torch.equal(layer(x).F, layer.module(x.F))
        sm = ME.MinkowskiSoftmax(dim=1)(x)
        assert_close(sm.F.sum(1), torch.ones(len(x.F)), 1e-6, 1e-6)
        sin = ME.MinkowskiSinusoidal(6, 9).to(device)
        y = sin(x)
        _same_place(y, x)
        assert torch.equal(y.F, torch.sin(x.F.mm(sin.kernel) + sin.bias) * sin.coef)
        assert sorted(sin.state_dict()) == ["bias", "coef", "kernel"]
        als = ME.MinkowskiAdaptiveLogSoftmaxWithLoss(6, 20, [5, 10]).to(device)
        assert isinstance(als.module, torch.nn.AdaptiveLogSoftmaxWithLoss)
        assert als.state_dict() and all(k.startswith("module.") for k in als.state_dict())


@pytest.mark.parametrize("name,args", _FUNCTIONALS, ids=[f[0] for f in _FUNCTIONALS])
def test_functionals(name, args, host_layer, device):
    import torch.nn.functional as F
    ME = _me()
    for x in _inputs(device):
        y = getattr(ME.MinkowskiFunctional, name)(x, *args)
        _same_place(y, x)
        assert torch.equal(y.F, getattr(F, name)(x.F, *args))


def test_functionals_with_parameters_and_losses(host_layer, device):
    import torch.nn.functional as F
    MF = _me().MinkowskiFunctional
    g = torch.Generator().manual_seed(31)
    for x in _inputs(device):
        w = torch.rand(1, generator=g).to(device)
        assert torch.equal(MF.prelu(x, w).F, F.prelu(x.F, w))
        lw, lb = torch.randn(4, 6, generator=g).to(device), torch.randn(4, generator=g).to(device)
        y = MF.linear(x, lw, lb)
        _same_place(y, x)
        assert torch.equal(y.F, F.linear(x.F, lw, lb))
        assert torch.equal(MF.dropout(x, 0.5, False).F, x.F) and torch.equal(MF.alpha_dropout(x, 0.5, False).F, x.F)
        assert torch.equal(MF.rrelu(x).F, F.rrelu(x.F))
        rm, rv = torch.zeros(6, device=device), torch.ones(6, device=device)
        assert torch.equal(MF.batch_norm(x, rm, rv).F, F.batch_norm(x.F, rm, rv))
        torch.manual_seed(4)
        gs = MF.gumbel_softmax(x)
        torch.manual_seed(4)
        assert torch.equal(gs.F, F.gumbel_softmax(x.F))
        target = torch.rand(x.F.shape, generator=g).to(device)
        labels = torch.randint(0, 6, (len(x.F),), generator=g).to(device)
        for name, t in (("mse_loss", target), ("l1_loss", target), ("smooth_l1_loss", target),
                        ("binary_cross_entropy_with_logits", target), ("cross_entropy", labels),
                        ("multi_margin_loss", labels), ("soft_margin_loss", target), ("kl_div", target),
                        ("poisson_nll_loss", target), ("hinge_embedding_loss", target),
                        ("multilabel_soft_margin_loss", target)):
            got = getattr(MF, name)(x, t)
            assert isinstance(got, torch.Tensor) and torch.equal(got, getattr(F, name)(x.F, t)), name
        assert torch.equal(MF.binary_cross_entropy(MF.sigmoid(x), target), F.binary_cross_entropy(torch.sigmoid(x.F), target))
        assert torch.equal(MF.nll_loss(MF.log_softmax(x, 1), labels), F.nll_loss(F.log_softmax(x.F, 1), labels))
        ml = torch.full((len(x.F), 6), -1, dtype=torch.long, device=device)
        ml[:, 0] = labels
        assert torch.equal(MF.multilabel_margin_loss(x, ml), F.multilabel_margin_loss(x.F, ml))
