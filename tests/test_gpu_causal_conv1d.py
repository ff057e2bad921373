"""The causal conv1d on the GPU (csrc/causal_conv1d.hip) against torch.nn.functional.conv1d per instance in float64 on the
CPU, on the inputs as stored, gradients through autograd.  The bound is the project's for fused kernels: per tensor
E_ours <= 4 max(E_base, eps(dtype) max|want|), E the largest absolute error and E_base that of the same reference evaluated
in float32 and rounded to the case's dtype.  Largest ratios measured on one MI355X: see DESIGN 8.22."""
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import _lib, backend
from minkowskiengine_amd.common import get_minkowski_function
from minkowskiengine_amd.selective_scan import scan_sequence

pytestmark = pytest.mark.gpu
FACTOR = 4.0
T = int(_lib.load().me_cconv_chunk())
BATCH = (0, 2, 5)                                # batch indices with gaps
NAMES = ("y", "dx", "dweight", "dbias")
ROWS = ("y", "dx")                               # tensors in the dtype of the rows; the others are float32


def _line(sizes, g):
    """instances of `sizes` rows on a line, shuffled together: the z-order is the order of (batch, position)"""
    inst = torch.cat([torch.full((m,), j) for j, m in enumerate(sizes)])[torch.randperm(sum(sizes), generator=g)]
    n = len(inst)
    return torch.stack([torch.tensor(BATCH)[inst], torch.randperm(n, generator=g), torch.zeros(n), torch.zeros(n)], 1).int()


def _cloud(sizes, g):
    """instances of `sizes` distinct random voxels of a 12^3 box, shuffled together"""
    parts = []
    for j, m in enumerate(sizes):
        cells = torch.randperm(12 ** 3, generator=g)[:m]
        parts.append(torch.stack([torch.full((m,), BATCH[j]), cells // 144, cells // 12 % 12, cells % 12], 1))
    pts = torch.cat(parts)
    return pts[torch.randperm(len(pts), generator=g)].int()


def _inputs(sizes, d, k, dtype, device, bias=True, cloud=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    coords = (_cloud if cloud else _line)(sizes, g)
    n = len(coords)
    t = {"x": torch.randn(n, d, generator=g).to(dtype), "weight": torch.randn(d, k, generator=g) / k ** 0.5,
         "bias": 0.5 * torch.randn(d, generator=g) if bias else None, "dout": torch.randn(n, d, generator=g).to(dtype)}
    return {key: None if v is None else v.to(device) for key, v in t.items()}, coords.to(device)


KEYS = ("x", "weight", "bias")


def _grads(t, fn):
    leaf = {key: None if t[key] is None else t[key].clone().requires_grad_() for key in KEYS}
    out = fn(leaf)
    ins = [key for key in KEYS if leaf[key] is not None]
    gs = dict(zip(ins, torch.autograd.grad(out, [leaf[key] for key in ins], t["dout"].to(out.dtype))))
    return dict(zip(NAMES, (out.detach(),) + tuple(gs.get(key) for key in KEYS)))


def _ours(t, coords, activation="silu", order="z", reverse=False, offset=None):
    s = ME.SparseTensor(torch.zeros(len(coords), 1, device=coords.device), coords)

    def run(leaf):
        x = leaf["x"]
        if offset is not None:                   # a column view of a wider matrix as x
            wide = torch.zeros(x.shape[0], x.shape[1] + 16, dtype=x.dtype, device=x.device)
            wide[:, offset:offset + x.shape[1]] = x
            x = wide[:, offset:offset + x.shape[1]]
        return ME.causal_conv1d(x, leaf["weight"], leaf["bias"], activation, order, reverse, s.coordinate_map_key,
                                s.coordinate_manager, fused=True)
    return _grads(t, run), s


def _reference(t, seq, starts, work, activation="silu"):
    """conv1d instance by instance on the CPU in `work`, from the inputs as stored"""
    t = {key: None if v is None else v.detach().cpu().to(work) for key, v in t.items()}
    cuts = starts.nonzero().flatten().tolist() + [len(seq)]

    def run(leaf):
        k = leaf["weight"].shape[1]
        outs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            xi = leaf["x"][seq[a:b]].t()[None]
            out = torch.nn.functional.conv1d(xi, leaf["weight"][:, None, :], leaf["bias"], padding=k - 1,
                                             groups=xi.shape[1])[0, :, :b - a].t()
            outs.append(torch.nn.functional.silu(out) if activation == "silu" else out)
        return torch.zeros_like(leaf["x"]).index_copy(0, seq, torch.cat(outs))
    return _grads(t, run)


def _check(case, dtype, ours, ref, base, sums_of=None):
    """the bound per tensor; sums_of = m: dweight and dbias are fp32 sums of m terms in another order than the reference's"""
    for name in NAMES:
        assert (ref[name] is None) == (ours[name] is None), name
        if ref[name] is None:
            continue
        want = ref[name]
        assert ours[name].dtype == (dtype if name in ROWS else torch.float32) and ours[name].shape == want.shape, name
        err = lambda a: float((a.double().cpu() - want).abs().max())
        e_ours, e_base = err(ours[name]), err(base[name].to(dtype) if name in ROWS else base[name])
        bound = FACTOR * max(e_base, torch.finfo(dtype).eps * float(want.abs().max()))
        if sums_of is not None and name not in ROWS:
            bound = 4 * sums_of ** 0.5 * 2 ** -23 * float(want.abs().max())
        print(f"{case} {dtype} {name}: E_ours {e_ours:.3e} E_base {e_base:.3e} bound {bound:.3e} "
              f"ratio {FACTOR * e_ours / max(bound, 1e-300):.2f}")
        assert e_ours <= bound, name


F32, BOTH = (torch.float32,), (torch.float32, torch.bfloat16)
CASES = {
    "d1-k4-scalar": dict(sizes=(1, T - 1, T + 1), d=1, k=4),
    "d64-k4-start-on-boundary": dict(sizes=(T, T), d=64, k=4),
    "d65-k3-reverse": dict(sizes=(2 * T + 1,), d=65, k=3, reverse=True),
    "d96-k2-short-instances": dict(sizes=(3, 1, 2), d=96, k=2),
    "d96-k4": dict(sizes=(1, T - 1, T + 1), d=96, k=4, dtypes=BOTH),
    "d96-k4-no-bias": dict(sizes=(1, T - 1, T + 1), d=96, k=4, bias=False, dtypes=BOTH),
    "d96-k4-no-activation": dict(sizes=(1, T - 1, T + 1), d=96, k=4, activation=None, dtypes=BOTH),
    "d96-k4-view-aligned": dict(sizes=(1, T - 1, T + 1), d=96, k=4, offset=8, dtypes=BOTH),
    "d96-k4-view-offset-1": dict(sizes=(1, T - 1, T + 1), d=96, k=4, offset=1, dtypes=BOTH),
    "d300-k4-two-slabs": dict(sizes=(T - 1, T + 1), d=300, k=4),
    "d64-k4-hilbert": dict(sizes=(T + 44, 190), d=64, k=4, cloud=True, order="hilbert"),
    # one instance of (CCONV_MAX_RUNS + 1) chunks: every workgroup walks a run of two chunks and carries dweight and
    # dbias in registers from the first into the second
    "d8-k4-runs-of-two-chunks": dict(sizes=(T * (backend.CCONV_MAX_RUNS + 1),), d=8, k=4, long=True),
}


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in CASES.items() for d in v.get("dtypes", F32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_matches_conv1d_per_instance_within_fp32s_error(device, host_layer, case, dtype):
    kw = {k: v for k, v in CASES[case].items() if k != "dtypes"}
    order, reverse, offset = kw.pop("order", "z"), kw.pop("reverse", False), kw.pop("offset", None)
    activation, long = kw.pop("activation", "silu"), kw.pop("long", False)
    t, coords = _inputs(dtype=dtype, device=device, **kw)
    ours, s = _ours(t, coords, activation, order, reverse, offset)
    seq, starts = (v.cpu() for v in scan_sequence(s.coordinate_map_key, s.coordinate_manager, order, reverse))
    if not kw.get("cloud"):
        c = coords.cpu().long()
        want_seq = torch.argsort(c[:, 0] * 10_000_000 + c[:, 1])
        assert torch.equal(seq, want_seq.flip(0) if reverse else want_seq)
    assert int(starts.sum()) == len(kw["sizes"])
    ref, base = _reference(t, seq, starts, torch.float64, activation), _reference(t, seq, starts, torch.float32, activation)
    _check(case, dtype, ours, ref, base, sums_of=len(coords) if long else None)


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
def test_results_are_bitwise_reproducible_and_equal_on_both_hosts(device, dtype):
    t, coords = _inputs((T + 3, 2 * T + 1, 5), 96, 4, dtype, device, seed=4)
    results, prev = [], ME.get_host()
    try:
        for layer in ("python", "native", "native", "python"):
            ME.set_host(layer)
            results.append(_ours(t, coords, order="hilbert")[0])
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for name in NAMES:
            assert torch.equal(results[0][name], other[name]), name


@pytest.mark.parametrize("flag", range(3), ids=["dx", "dweight", "dbias"])
def test_a_gradient_asked_for_alone_is_the_same_gradient(device, host_layer, flag):
    t, coords = _inputs((T + 3, 40), 96, 4, torch.float32, device, seed=5)
    s = ME.SparseTensor(torch.zeros(len(coords), 1, device=device), coords)
    bw_fn = get_minkowski_function("CausalConv1dBackward", t["x"], s.coordinate_map_key)
    run = lambda need: bw_fn(t["x"], t["weight"], t["bias"], t["dout"], "silu", "z", False, s.coordinate_map_key,
                             s.coordinate_manager._manager, need)
    every, alone = run([True, True, True]), run([i == flag for i in range(3)])
    assert all(g is not None for g in every)
    for i in range(3):
        assert (alone[i] is None) == (i != flag)
    assert torch.equal(alone[flag], every[flag])
