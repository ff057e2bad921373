"""The SSD scan on the GPU (csrc/ssd_scan.hip) against its formulas evaluated in float64 on the CPU, position by position
and with no chunks (ssd_scan_reference), on the inputs as stored.  The bound is the project's for fused kernels: per tensor
E_ours <= 4 max(E_base, eps(dtype) max|want|), E the largest absolute error and E_base that of the same sequential formulas
in float32 on the CPU, rounded to the case's dtype.  The bf16 cases meet it against that sequential base; no
chunked bf16 base is used.  Measured largest ratios E_ours / max(E_base, floor): 2.84 in float32 (out, H = 1, P = 64,
S = 64; dA at most 1.54), 0.57 in bfloat16 (ddt, strided views)."""
import ctypes

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd.selective_scan import scan_sequence
from minkowskiengine_amd.ssd_scan import ssd_scan_reference

pytestmark = pytest.mark.gpu
FACTOR = 4.0
T = 64                                           # me_ssd_chunk()
BATCH = (0, 2, 5)                                # batch indices with gaps
KEYS = ("x", "dt", "A", "B", "C", "D", "bias")
NAMES = ("out", "dx", "ddt", "dA", "dB", "dC", "dD", "ddt_bias")
ROWS = ("out", "dx", "ddt", "dB", "dC")          # tensors in the dtype of the rows; the others are float32


def _coords(sizes, g, cloud=False):
    """instances of `sizes` rows, shuffled together: on a line, or distinct random voxels of a 12^3 box"""
    inst = torch.cat([torch.full((m,), j) for j, m in enumerate(sizes)] + [torch.zeros(0, dtype=torch.long)])
    cells = torch.cat([torch.randperm(12 ** 3, generator=g)[:m] for m in sizes]) if cloud else torch.randperm(len(inst), generator=g)
    xyz = torch.stack([cells // 144, cells // 12 % 12, cells % 12] if cloud else [cells, 0 * cells, 0 * cells], 1)
    pts = torch.cat([torch.tensor(BATCH)[inst][:, None], xyz], 1)
    return pts[torch.randperm(len(pts), generator=g)].int()


def _inputs(sizes, dtype, device, h=2, p=32, s=64, g=1, skip=True, bias=True, softplus=True, slow=False, cloud=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    coords = _coords(sizes, gen, cloud)
    n = len(coords)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    dt = 0.5 * rnd(n, h) if softplus else 0.1 + torch.rand(n, h, generator=gen)
    A = -(0.5 + torch.rand(h, generator=gen))
    if slow:                                     # see CASES["slow-decay"]
        dt, A = 0.05 + 0.02 * torch.rand(n, h, generator=gen), torch.full((h,), -0.01)
    t = {"x": rnd(n, h * p).to(dtype), "dt": dt.to(dtype), "A": A, "B": rnd(n, g * s).to(dtype), "C": rnd(n, g * s).to(dtype),
         "D": rnd(h) if skip else None, "dout": rnd(n, h * p).to(dtype),
         "bias": (0.5 * rnd(h) if softplus else 0.02 * torch.rand(h, generator=gen)) if bias else None}   # dt stays positive
    return {k: None if v is None else v.to(device) for k, v in t.items()}, coords.to(device)


def _grads(t, fn):
    leaf = {k: None if t[k] is None else t[k].clone().requires_grad_() for k in KEYS}
    out = fn(leaf)
    ins = [k for k in KEYS if leaf[k] is not None]
    gs = dict(zip(ins, torch.autograd.grad(out, [leaf[k] for k in ins], t["dout"].to(out.dtype))))
    return dict(zip(NAMES, (out.detach(),) + tuple(gs.get(k) for k in KEYS)))


def _ours(t, coords, p, g, softplus=True, order="z", reverse=False, view=False):
    sp = ME.SparseTensor(torch.zeros(len(coords), 1, device=coords.device), coords)

    def run(leaf):
        x, dt, B, C = (leaf[k] for k in ("x", "dt", "B", "C"))
        if view:                                 # x | B | C column slices of one wider matrix, dt a slice of another
            wide = torch.nn.functional.pad(torch.cat([x, B, C], 1), (8, 8))
            x, B, C = wide.split([8 + x.shape[1], B.shape[1], 8 + C.shape[1]], 1)
            x, C, dt = x[:, 8:], C[:, :-8], torch.nn.functional.pad(dt, (3, 2))[:, 3:-2]
            assert not x.is_contiguous() and not dt.is_contiguous() and x.data_ptr() + x.shape[1] * x.element_size() == B.data_ptr()
        return ME.ssd_scan(x, dt, leaf["A"], B, C, leaf["D"], leaf["bias"], softplus, p, g, order, reverse,
                           sp.coordinate_map_key, sp.coordinate_manager, fused=True)
    return _grads(t, run), sp


def _reference(t, seq, starts, work, p, g, softplus=True):
    """the sequential formulas on the CPU in `work`, from the inputs as stored"""
    t = {k: None if v is None else v.detach().cpu().to(work) for k, v in t.items()}
    return _grads(t, lambda leaf: ssd_scan_reference(leaf["x"], leaf["dt"], leaf["A"], leaf["B"], leaf["C"], leaf["D"],
                                                     leaf["bias"], softplus, p, g, seq, starts))


F32, BOTH = (torch.float32,), (torch.float32, torch.bfloat16)
CASES = {
    "h1-p64-s64-resets-in-chunk": dict(sizes=(1, T - 1, T + 1), h=1, p=64, s=64),
    "h3-p32-s128-resets-in-chunk": dict(sizes=(1, T - 1, T + 1), h=3, p=32, s=128, g=1, dtypes=BOTH),
    "h4-g2-p64-s128-reset-on-boundary": dict(sizes=(T, T), h=4, g=2, p=64, s=128),
    "h2-g2-p32-s64-carry-reverse": dict(sizes=(2 * T + 1,), h=2, g=2, p=32, s=64, reverse=True),
    "tiny-instances-no-D": dict(sizes=(3, 1, 2), skip=False),
    "no-dt-bias": dict(sizes=(5, T), bias=False),
    "plain-dt": dict(sizes=(5, T), softplus=False),
    "strided-views": dict(sizes=(T + 3, 7), h=2, g=2, p=32, s=64, view=True, dtypes=BOTH),
    # A = -0.01 and dt < 0.08: a state keeps at least 0.9 of itself over the 2 T positions between the first chunk and the
    # last row.  In float64 on the CPU, zeroing x in the first chunk moves the last row of `out` by 7.3 (its largest entry
    # is 14.1) against a bound of 9.3e-6: a chunk carry that is dropped or wrong cannot pass.
    "slow-decay": dict(sizes=(2 * T + 1,), slow=True, softplus=False),
    # ten chunks: the carry kernel composes groups of two chunks
    "slow-decay-10-chunks": dict(sizes=(9 * T + 5,), h=1, p=32, s=64, slow=True, softplus=False),
    "hilbert": dict(sizes=(190, 170), cloud=True, order="hilbert"),
}


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in CASES.items() for d in v.get("dtypes", F32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_matches_the_sequential_formulas_within_fp32s_error(device, host_layer, case, dtype):
    kw = {k: v for k, v in CASES[case].items() if k != "dtypes"}
    order, reverse, view = kw.pop("order", "z"), kw.pop("reverse", False), kw.pop("view", False)
    t, coords = _inputs(dtype=dtype, device=device, **kw)
    p, g, softplus = kw.get("p", 32), kw.get("g", 1), kw.get("softplus", True)
    ours, sp = _ours(t, coords, p, g, softplus, order, reverse, view)
    seq, starts = (v.cpu() for v in scan_sequence(sp.coordinate_map_key, sp.coordinate_manager, order, reverse))
    assert int(starts.sum()) == len(kw["sizes"])
    ref, base = (_reference(t, seq, starts, work, p, g, softplus) for work in (torch.float64, torch.float32))
    for name in NAMES:
        assert (ref[name] is None) == (ours[name] is None), name
        if ref[name] is None:
            continue
        want = ref[name]
        assert ours[name].dtype == (dtype if name in ROWS else torch.float32), name
        err = lambda a: float((a.double().cpu() - want).abs().max())
        e_ours, e_base = err(ours[name]), err(base[name].to(dtype) if name in ROWS else base[name])
        floor = torch.finfo(dtype).eps * float(want.abs().max())
        print(f"{case} {dtype} {name}: E_ours {e_ours:.3e} E_base {e_base:.3e} floor {floor:.3e} "
              f"ratio {e_ours / max(e_base, floor, 1e-300):.2f}")
        assert e_ours <= FACTOR * max(e_base, floor), name


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
def test_results_are_bitwise_reproducible_and_equal_on_both_hosts(device, dtype):
    t, coords = _inputs((T + 3, 2 * T + 1, 5), dtype, device, h=4, g=2, seed=4)
    results, prev = [], ME.get_host()
    try:
        for layer in ("python", "native", "native", "python"):
            ME.set_host(layer)
            results.append(_ours(t, coords, 32, 2, order="hilbert")[0])
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for name in NAMES:
            assert torch.equal(results[0][name], other[name]), name


def test_no_rows_and_unserved_widths(device, host_layer):
    """n = 0 at the C ABI (the serialized orders of an empty coordinate map cannot be asked for): forward launches nothing,
    backward writes zero parameter gradients; widths outside the kernels' are an error with fused=True"""
    from minkowskiengine_amd import _lib
    lib, ptr = _lib.load(), lambda v: ctypes.c_void_p(v.data_ptr())
    vec = [torch.full((2,), float("nan"), device=device) for _ in range(5)]      # D, dt_bias, dA, dD, ddt_bias
    assert lib.me_ssd_forward(None, None, None, None, 0, 64, 2, 64, 64, None, None, None, 1, None, None, 0, 0, 2, 32, 64, 1,
                              None, 64, None, None, 0, None) == 0
    assert lib.me_ssd_backward(None, None, None, None, None, 0, 64, 2, 64, 64, 64, None, ptr(vec[0]), ptr(vec[1]), 1, None,
                               None, 0, 0, 2, 32, 64, 1, None, None, None, None, None, ptr(vec[2]), ptr(vec[3]), ptr(vec[4]),
                               None, 0, None) == 0
    assert all(torch.equal(v, torch.zeros(2, device=device)) for v in vec[2:])
    for kw, p in ((dict(p=48), 48), (dict(s=16), 32)):
        t, coords = _inputs((5,), torch.float32, device, **kw)
        with pytest.raises(Exception, match="serve"):
            _ours(t, coords, p, 1)


def test_mamba2_equals_its_torch_formulation(device, host_layer):
    g = torch.Generator().manual_seed(7)
    coords = _coords((T + 9, 40), g, cloud=True).to(device)
    feats, dout = (torch.randn(len(coords), 64, generator=g).to(device) for _ in range(2))
    layer = ME.MinkowskiMamba2(64, d_state=64, headdim=32, order="hilbert").to(device)
    twin = ME.MinkowskiMamba2(64, d_state=64, headdim=32, order="hilbert").to(device).double()
    twin.load_state_dict(layer.state_dict())     # the parameters as stored, in float64: runs the torch formulation
    got = {}
    for fused, run in ((True, layer), (False, layer), ("f64", twin)):
        run.fused = None if fused == "f64" else fused
        y = run(ME.SparseTensor(feats.double() if fused == "f64" else feats, coords)).F
        got[fused] = [y.detach(), torch.autograd.grad(y, run.in_proj.weight, dout.to(y.dtype))[0]]
    for i, (ours, base, want) in enumerate(zip(got[True], got[False], got["f64"])):
        e_ours, e_base = float((ours.double() - want).abs().max()), float((base.double() - want).abs().max())
        floor = torch.finfo(torch.float32).eps * float(want.abs().max())
        print(f"mamba2 tensor {i}: E_ours {e_ours:.3e} E_base {e_base:.3e} floor {floor:.3e}")
        assert e_ours <= FACTOR * max(e_base, floor), i
