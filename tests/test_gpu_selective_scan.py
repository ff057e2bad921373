"""The selective scan on the GPU (csrc/selective_scan.hip) against its formulas evaluated in float64 on the CPU, position by
position and with no chunks (selective_scan_reference), on the inputs as stored.  The bound is the project's for fused
kernels: per tensor E_ours <= 4 max(E_base, eps(dtype) max|want|), E the largest absolute error and E_base that of the same
sequential formulas in float32 on the CPU, rounded to the case's dtype."""
import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd.selective_scan import scan_sequence, selective_scan_reference

pytestmark = pytest.mark.gpu
FACTOR = 4.0
T = 64                                           # me_sscan_chunk()
BATCH = (0, 2, 5)                                # batch indices with gaps
NAMES = ("out", "du", "ddelta", "dA", "dB", "dC", "dDskip", "dz", "ddelta_bias")
ROWS = ("out", "du", "ddelta", "dB", "dC", "dz")  # tensors in the dtype of the rows; the others are float32


def _line(sizes, g):
    """instances of `sizes` rows on a line, shuffled together"""
    inst = torch.cat([torch.full((m,), j) for j, m in enumerate(sizes)])[torch.randperm(sum(sizes), generator=g)]
    n = len(inst)
    return torch.stack([torch.tensor(BATCH)[inst], torch.randperm(n, generator=g), torch.zeros(n), torch.zeros(n)], 1).int()


def _cloud(sizes, g):
    """instances of `sizes` distinct random voxels of a 12^3 box, shuffled together"""
    parts = []
    for j, m in enumerate(sizes):
        cells = torch.randperm(12 ** 3, generator=g)[:m]
        xyz = torch.stack([cells // 144, cells // 12 % 12, cells % 12], 1)
        parts.append(torch.cat([torch.full((m, 1), BATCH[j]), xyz], 1))
    pts = torch.cat(parts)
    return pts[torch.randperm(len(pts), generator=g)].int()


def _inputs(sizes, d, s, dtype, device, z=True, skip=True, bias=True, softplus=True, slow=False, cloud=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    coords = (_cloud if cloud else _line)(sizes, g)
    n = len(coords)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    delta = 0.5 * rnd(n, d) if softplus else 0.1 + torch.rand(n, d, generator=g)
    A = -(0.5 + torch.rand(d, s, generator=g))
    if slow:                                     # see CASES["slow-decay"]
        delta, A = 0.05 + 0.01 * torch.rand(n, d, generator=g), torch.full((d, s), -0.01)
    t = {"u": rnd(n, d).to(dtype), "delta": delta.to(dtype), "A": A, "B": rnd(n, s).to(dtype), "C": rnd(n, s).to(dtype),
         "Dskip": rnd(d) if skip else None, "z": rnd(n, d).to(dtype) if z else None, "bias": (0.5 * rnd(d) if softplus else 0.02 * torch.rand(d, generator=g)) if bias else None,   # dt stays positive
         "dout": rnd(n, d).to(dtype)}
    return {k: None if v is None else v.to(device) for k, v in t.items()}, coords.to(device)


KEYS = ("u", "delta", "A", "B", "C", "Dskip", "z", "bias")


def _grads(t, fn):
    leaf = {k: None if t[k] is None else t[k].clone().requires_grad_() for k in KEYS}
    out = fn(leaf)
    ins = [k for k in KEYS if leaf[k] is not None]
    gs = dict(zip(ins, torch.autograd.grad(out, [leaf[k] for k in ins], t["dout"].to(out.dtype))))
    return dict(zip(NAMES, (out.detach(),) + tuple(gs.get(k) for k in KEYS)))


def _ours(t, coords, softplus=True, order="z", reverse=False):
    x = ME.SparseTensor(torch.zeros(len(coords), 1, device=coords.device), coords)
    return _grads(t, lambda leaf: ME.selective_scan(leaf["u"], leaf["delta"], leaf["A"], leaf["B"], leaf["C"], leaf["Dskip"],
                                                     leaf["z"], leaf["bias"], softplus, order, reverse, x.coordinate_map_key,
                                                     x.coordinate_manager, fused=True)), x


def _reference(t, seq, starts, work, softplus=True):
    """the sequential formulas on the CPU in `work`, from the inputs as stored"""
    t = {k: None if v is None else v.detach().cpu().to(work) for k, v in t.items()}
    return _grads(t, lambda leaf: selective_scan_reference(leaf["u"], leaf["delta"], leaf["A"], leaf["B"], leaf["C"],
                                                           leaf["Dskip"], leaf["z"], leaf["bias"], softplus, seq, starts))


F32, BOTH = (torch.float32,), (torch.float32, torch.bfloat16)
CASES = {
    "d1-s16": dict(sizes=(1, T - 1, T + 1), d=1, s=16),
    "d64-s8-reset-on-boundary": dict(sizes=(T, T), d=64, s=8),
    "d65-s16-carry-reverse": dict(sizes=(2 * T + 1,), d=65, s=16, reverse=True),
    "d96-s8-resets-no-z": dict(sizes=(3, 1, 2), d=96, s=8, z=False),
    "d96-s16": dict(sizes=(1, T - 1, T + 1), d=96, s=16, dtypes=BOTH),
    "d64-s16-no-skip": dict(sizes=(T, T), d=64, s=16, skip=False),
    "d65-s8-no-bias": dict(sizes=(2 * T + 1,), d=65, s=8, bias=False),
    "d96-s16-view": dict(sizes=(3, 1, 2), d=96, s=16, view=True),
    "d96-s8-plain-delta": dict(sizes=(1, T - 1, T + 1), d=96, s=8, softplus=False),
    # more than one slab of channels (256 forward, 64 or 128 backward)
    "d300-s8": dict(sizes=(T - 1, T + 1), d=300, s=8), "d300-s16": dict(sizes=(3, T), d=300, s=16),
    "hilbert": dict(sizes=(190, 170), d=64, s=16, cloud=True, order="hilbert"),
    # A = -0.01 and dt ~ 0.065: a state keeps at least 0.95 of itself over the 2 T positions between the first chunk and
    # the last row.  In float64 on the CPU, zeroing u in the first chunk moves the last row of `out` by 8.8 (its largest
    # entry is 8.7) against a bound of 1e-5: a chunk carry that is dropped or wrong cannot pass.
    "slow-decay": dict(sizes=(2 * T + 1,), d=64, s=16, slow=True, softplus=False),
    # ten chunks: the carry kernel composes groups of two chunks
    "slow-decay-10-chunks": dict(sizes=(9 * T + 5,), d=8, s=8, slow=True, softplus=False),
}


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in CASES.items() for d in v.get("dtypes", F32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_matches_the_sequential_formulas_within_fp32s_error(device, host_layer, case, dtype):
    kw = {k: v for k, v in CASES[case].items() if k != "dtypes"}
    view, order, reverse = kw.pop("view", False), kw.pop("order", "z"), kw.pop("reverse", False)
    t, coords = _inputs(dtype=dtype, device=device, **kw)
    softplus = kw.get("softplus", True)
    stored = dict(t)
    if view:                                     # a strided column view as u
        big = torch.zeros(t["u"].shape[0], kw["d"] + 16, dtype=dtype, device=device)
        big[:, 8:8 + kw["d"]] = t["u"]
        t["u"] = big[:, 8:8 + kw["d"]]
    ours, x = _ours(t, coords, softplus, order, reverse)
    seq, starts = (v.cpu() for v in scan_sequence(x.coordinate_map_key, x.coordinate_manager, order, reverse))
    if not kw.get("cloud"):                      # on a line the z-order is the order of (batch, position)
        c = coords.cpu().long()
        want_seq = torch.argsort(c[:, 0] * 10_000 + c[:, 1])
        assert torch.equal(seq, want_seq.flip(0) if reverse else want_seq)
    assert int(starts.sum()) == len(kw["sizes"])
    ref, base = _reference(stored, seq, starts, torch.float64, softplus), _reference(stored, seq, starts, torch.float32, softplus)
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
    t, coords = _inputs((T + 3, 2 * T + 1, 5), 96, 16, dtype, device, seed=4)
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


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
def test_bidirectional_mamba_equals_its_torch_formulation(device, host_layer, dtype):
    g = torch.Generator().manual_seed(7)
    coords = _cloud((T + 9, 40), g).to(device)
    feats = torch.randn(len(coords), 32, generator=g).to(device=device, dtype=dtype)
    dout = torch.randn(len(coords), 32, generator=g).to(device=device, dtype=dtype)
    layer = ME.MinkowskiMamba(32, d_state=16, order="hilbert", bidirectional=True).to(device=device, dtype=dtype)
    twin = ME.MinkowskiMamba(32, d_state=16, order="hilbert", bidirectional=True).to(device).double()
    twin.load_state_dict(layer.state_dict())     # the parameters as stored, in float64: runs the torch formulation
    params = list(layer.parameters())
    got = {}
    for fused, run in ((True, layer), (False, layer), ("f64", twin)):
        run.fused = None if fused == "f64" else fused
        y = run(ME.SparseTensor(feats.double() if fused == "f64" else feats, coords)).F
        got[fused] = [y.detach()] + list(torch.autograd.grad(y, list(run.parameters()), dout.to(y.dtype)))
    assert len(got[True]) == len(params) + 1
    for i, (ours, base, want) in enumerate(zip(got[True], got[False], got["f64"])):
        e_ours, e_base = float((ours.double() - want).abs().max()), float((base.double() - want).abs().max())
        floor = torch.finfo(dtype).eps * float(want.abs().max())
        print(f"mamba {dtype} tensor {i}: E_ours {e_ours:.3e} E_base {e_base:.3e} floor {floor:.3e}")
        assert e_ours <= FACTOR * max(e_base, floor), i


def test_parameter_gradients_of_a_batch_are_the_sums_over_its_instances(device, host_layer):
    """264 chunks: the backward workgroups walk runs of two chunks and keep dA, dDskip, ddelta_bias in registers across
    them.  Instances do not see each other, so the gradients equal the float64 sum of those of every instance alone (8
    chunks, runs of one).  Both sides are fp32 sums of m = 16896 d terms in different orders: the bound is
    4 sqrt(m) eps max|want|, the random-walk size of such a difference."""
    k, m, d, s = 33, 8 * T, 8, 8
    g = torch.Generator().manual_seed(11)
    coords = torch.stack([torch.arange(k).repeat_interleave(m), torch.randperm(k * m, generator=g), torch.zeros(k * m),
                          torch.zeros(k * m)], 1).int().to(device)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(device)
    t = {"u": rnd(k * m, d), "delta": 0.5 * rnd(k * m, d), "A": -(0.5 + torch.rand(d, s, generator=g)).to(device),
         "B": rnd(k * m, s), "C": rnd(k * m, s), "Dskip": rnd(d), "z": rnd(k * m, d), "bias": 0.5 * rnd(d), "dout": rnd(k * m, d)}
    whole = _ours(t, coords)[0]
    alone = {name: torch.zeros_like(whole[name], dtype=torch.float64) for name in ("dA", "dDskip", "ddelta_bias")}
    for j in range(k):
        rows = slice(j * m, (j + 1) * m)
        part = _ours({key: v[rows] if v.shape[0] == k * m else v for key, v in t.items()}, coords[rows])[0]
        for name in alone:
            alone[name] += part[name].double()
    for name, want in alone.items():
        err, bound = float((whole[name].double() - want).abs().max()), 4 * (k * m * d) ** 0.5 * 2 ** -23 * float(want.abs().max())
        print(f"{name}: error {err:.3e} bound {bound:.3e}")
        assert err <= bound, name
