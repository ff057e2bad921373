"""MinkowskiAdaLayerNorm on the GPU (csrc/ada_layer_norm.hip) against the formulas in float64 on the CPU, on the inputs as
stored:  stream = residual + gate[b] * input,  normed = norm(stream) * (1 + scale[b]) + shift[b],  b the origin row of a row.
The bound is the project's for fused kernels: per tensor E_ours <= 4 E_torch with E the largest absolute error and E_torch
that of the same formulas in the feature dtype on the GPU; where E_torch is 0 the floor is finfo(dtype).eps * max|reference|."""
import pytest
import torch
import torch.nn.functional as F

import minkowskiengine_amd as ME

pytestmark = pytest.mark.gpu
FACTOR = 4.0
KINDS, DTYPES = ("layer", "rms"), (torch.float32, torch.bfloat16)
SIZES, BATCH = (1, 33, 70), (0, 2, 5)            # rows per instance, shuffled together; batch indices with gaps
CHUNKY = (127, 128, 129)                         # runs ending one row before, on and one row after a chunk boundary at C = 64
                                                 # (16 KiB chunks: 128 bf16 rows, 64 fp32 rows)
NAMES = ("normed", "stream", "din", "dres", "dscale", "dshift", "dgate", "dgamma", "dbeta")
EPS = 1e-6


def _inputs(sizes, c, dtype, device, form="gate", affine=True, scale=True, shift=True, seed=0, draw=None, batch=None):
    """a scene of len(sizes) instances: coordinates, the origin row of every row, and every operand of the layer"""
    g = torch.Generator().manual_seed(seed)
    rnd = draw or (lambda *s: torch.randn(*s, generator=g))
    batch = batch or (BATCH[:len(sizes)] if len(sizes) <= 3 else tuple(range(len(sizes))))
    inst = torch.cat([torch.full((m,), j) for j, m in enumerate(sizes)])[torch.randperm(sum(sizes), generator=g)]
    n, nb = len(inst), len(sizes)
    coords = torch.stack([torch.tensor(batch)[inst], torch.arange(n), torch.zeros(n), torch.zeros(n)], 1).int()
    t = {"x": rnd(n, c).to(dtype), "r": rnd(n, c).to(dtype) if form != "plain" else None,
         "w": 1 + 0.1 * rnd(c) if affine else None, "b": 0.1 * rnd(c) if affine else None,
         "sc": 0.5 * rnd(nb, c) if scale else None, "sh": rnd(nb, c) if shift else None,
         "gt": rnd(nb, c) if form == "gate" else None, "dy": rnd(n, c).to(dtype),
         "ds": rnd(n, c).to(dtype) if form != "plain" else None}
    t = {k: None if v is None else v.to(device) for k, v in t.items()}
    return dict(t, coords=coords.to(device), inst=inst.to(device))


def _grads(kind, t, fn, use=("normed", "stream")):
    """the nine tensors of NAMES under the output gradients (dy, ds); `fn(leaf) -> normed | (normed, stream)`"""
    keys = ("x", "r", "sc", "sh", "gt", "w", "b")
    leaf = {k: None if t[k] is None or (k == "b" and kind == "rms") else t[k].clone().requires_grad_() for k in keys}
    out = fn(leaf)
    y, stream = out if leaf["r"] is not None else (out, None)
    pairs = [(o, go) for name, o, go in (("normed", y, t["dy"]), ("stream", stream, t["ds"])) if o is not None and name in use]
    ins = [k for k in keys if leaf[k] is not None]
    gs = dict(zip(ins, torch.autograd.grad([p[0] for p in pairs], [leaf[k] for k in ins], [p[1] for p in pairs],
                                           allow_unused=True)))
    return dict(zip(NAMES, (y, stream) + tuple(gs.get(k) for k in keys)))


def _ours(kind, t, **kw):
    def fn(leaf):
        x = ME.SparseTensor(leaf["x"], t["coords"])
        r = None if leaf["r"] is None else ME.SparseTensor(leaf["r"], coordinate_map_key=x.coordinate_map_key,
                                                           coordinate_manager=x.coordinate_manager)
        out = ME.MinkowskiFunctional.ada_layer_norm(x, leaf["sc"], leaf["sh"], r, leaf["gt"], leaf["w"], leaf["b"], EPS,
                                                    kind == "rms")
        return out.F if r is None else (out[0].F, out[1].F)
    return _grads(kind, t, fn, **kw)


def _reference(kind, t, dtype=None, device=None, **kw):
    """the formulas, indexed by batch row, in `dtype` on `device` (default: as stored)"""
    inst = t["inst"].to(device or t["inst"].device)
    t = {k: None if v is None else v.to(device=device or v.device, dtype=dtype or t["x"].dtype)
         for k, v in t.items() if k not in ("coords", "inst")}

    def fn(leaf):
        s = leaf["x"] if leaf["r"] is None else leaf["r"] + (leaf["x"] if leaf["gt"] is None else leaf["gt"][inst] * leaf["x"])
        y = F.rms_norm(s, s.shape[1:], leaf["w"], EPS) if kind == "rms" else F.layer_norm(s, s.shape[1:], leaf["w"], leaf["b"], EPS)
        y = y if leaf["sc"] is None else y * (1 + leaf["sc"][inst])
        y = y if leaf["sh"] is None else y + leaf["sh"][inst]
        return y if leaf["r"] is None else (y, s)
    return _grads(kind, t, fn, **kw)


CASES = {
    "c1": dict(c=1), "c8": dict(c=8), "c96": dict(c=96), "c96-plain": dict(c=96, form="plain"),
    "c96-residual": dict(c=96, form="residual"), "c96-no-affine": dict(c=96, affine=False),
    "c96-no-scale": dict(c=96, scale=False), "c96-no-shift": dict(c=96, shift=False), "c96-view": dict(c=96, view=True),
    "c64-chunks": dict(c=64, sizes=CHUNKY), "c2048": dict(c=2048, sizes=(2, 3), only=torch.float32),
    "offset": dict(c=96, form="plain", offset=True, only=torch.float32),
}


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in CASES.items() for d in DTYPES if v.get("only", d) == d],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("kind", KINDS)
def test_matches_the_formulas_within_torchs_error(device, host_layer, kind, dtype, case):
    kw = {k: v for k, v in CASES[case].items() if k != "only"}
    view, offset, c = kw.pop("view", False), kw.pop("offset", False), kw.pop("c")
    t = _inputs(kw.pop("sizes", SIZES), c, dtype, device, **kw)
    if offset:
        t["x"] = (1e4 + 1e-2 * t["x"].float()).to(dtype)
    ref, base = _reference(kind, t, torch.float64, "cpu"), _reference(kind, t)
    if view:                                     # a strided column view as input
        big = torch.zeros(t["x"].shape[0], c + 16, dtype=dtype, device=device)
        big[:, 8:8 + c] = t["x"]
        t["x"] = big[:, 8:8 + c]
    ours = _ours(kind, t)
    for name in NAMES:
        assert (ref[name] is None) == (ours[name] is None), name
        if ref[name] is None:
            continue
        want = ref[name].detach()
        err = lambda a: float((a.detach().double().cpu() - want).abs().max())
        e_ours, e_torch = err(ours[name]), err(base[name])
        floor = torch.finfo(dtype).eps * float(want.abs().max())
        print(f"{case} {kind} {dtype} {name}: E_ours {e_ours:.3e} E_torch {e_torch:.3e} floor {floor:.3e} "
              f"ratio {e_ours / max(e_torch, floor, 1e-300):.2f}")
        assert e_ours <= FACTOR * (e_torch if e_torch > 0 else floor), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_zero_modulation_and_unit_gate_are_the_plain_layer(device, host_layer, kind, dtype):
    t = _inputs(SIZES, 96, dtype, device)
    plain = (ME.MinkowskiRMSNorm(96, eps=EPS) if kind == "rms" else ME.MinkowskiLayerNorm(96, eps=EPS)).to(device)
    with torch.no_grad():
        plain.weight.copy_(t["w"])
        if kind == "layer":
            plain.bias.copy_(t["b"])
    ada = ME.MinkowskiAdaLayerNorm(96, elementwise_affine=True, rms=kind == "rms").to(device)
    ada.load_state_dict(plain.state_dict(), strict=True)
    zero, one = torch.zeros_like(t["sc"]), torch.ones_like(t["gt"])
    got = []
    for mod, extra in ((plain, ()), (ada, (zero, zero, one))):
        x = ME.SparseTensor(t["x"].clone().requires_grad_(), t["coords"])
        r = ME.SparseTensor(t["r"].clone(), coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
        y, s = mod.forward_residual(x, r, *extra)
        torch.autograd.backward([y.F, s.F], [t["dy"], t["ds"]])
        got.append((y.F, s.F, x.F.grad))
    for a, b, name in zip(*got, ("normed", "stream", "din")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_sums_of_small_integers_are_exact(device, host_layer, kind, dtype):
    g = torch.Generator().manual_seed(3)
    draw = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    t = _inputs(CHUNKY, 64, dtype, device, affine=False, draw=draw)
    for use, names in ((("stream",), ("din", "dres", "dgate")), (("normed", "stream"), ("dshift",))):
        ref, ours = _reference(kind, t, torch.float64, "cpu", use=use), _ours(kind, t, use=use)
        for name in names:
            assert torch.equal(ours[name].double().cpu(), ref[name]), (use, name)


def _equal(a, b, names=NAMES, rows=None):
    for name in names:
        assert (a[name] is None) == (b[name] is None), name
        if a[name] is not None:
            assert torch.equal(a[name] if rows is None else a[name][rows[0]], b[name] if rows is None else b[name][rows[1]]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_reproducible_on_both_hosts_and_local(device, kind, dtype):
    t = _inputs(CHUNKY, 64, dtype, device)
    results = {}
    for host in ("python", "native"):
        ME.set_host(host)
        try:
            results[host] = _ours(kind, t)
            _equal(results[host], _ours(kind, t))                                           # two calls
            # the rows permuted: normed and stream are permuted, bit for bit
            perm = torch.randperm(t["x"].shape[0], generator=torch.Generator().manual_seed(5)).to(device)
            moved = {k: v[perm] if k in ("x", "r", "dy", "ds", "coords", "inst") else v for k, v in t.items()}
            _equal(_ours(kind, moved), results[host], ("normed", "stream", "din", "dres"), rows=(slice(None), perm))
            # a scene of NaN / Inf next to a finite one: the finite scene gives what it gives alone
            two = _inputs((33, 70), 64, dtype, device, batch=(0, 1))
            first = two["inst"] == 0
            alone = {k: v[first] if k in ("x", "r", "dy", "ds", "coords", "inst") else v[:1] if k in ("sc", "sh", "gt")
                     else v for k, v in two.items()}
            two["x"] = torch.where(first[:, None], two["x"], torch.full_like(two["x"], float("nan")))
            two["r"][~first] = float("inf")
            bad, good = _ours(kind, two), _ours(kind, alone)
            _equal(bad, good, ("normed", "stream", "din", "dres"), rows=(first, slice(None)))
            _equal(bad, good, ("dscale", "dshift", "dgate"), rows=(slice(0, 1), slice(None)))
            assert all(bool(torch.isfinite(bad[k][:1]).all()) for k in ("dscale", "dshift", "dgate"))
            # shapes that are not (instances, C)
            x = ME.SparseTensor(t["x"], t["coords"])
            for wrong in (t["sc"][:2], t["sc"][:, :32]):
                with pytest.raises(ValueError):
                    ME.MinkowskiAdaLayerNorm(64)(x, wrong)
        finally:
            ME.set_host("python")
    _equal(results["python"], results["native"])


@pytest.mark.parametrize("kind", KINDS)
def test_float64_gradcheck(device, host_layer, kind):
    t = _inputs((3, 4), 5, torch.float64, device, batch=(0, 1))
    x = ME.SparseTensor(t["x"], t["coords"])
    keys = [k for k in ("x", "r", "w", "b", "sc", "sh", "gt") if not (k == "b" and kind == "rms")]
    ops = [t[k].double().requires_grad_() for k in keys]

    def fn(*a):
        a = dict(zip(keys, a))
        return ME.MinkowskiAdaLayerNormFunction.apply(a["x"], a["r"], a["w"], a.get("b"), a["sc"], a["sh"], a["gt"], EPS,
                                                      kind == "rms", x.coordinate_map_key, x.coordinate_manager)
    assert torch.autograd.gradcheck(fn, ops, eps=1e-6, atol=1e-6, rtol=1e-5)
