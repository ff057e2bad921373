"""Entry-point tests of the conditional group-norm kernels (k_gnc_* in csrc/group_norm.hip) through the C ABI:
me_gnorm_cond_workspace_bytes / me_gnorm_cond_apply / me_gnorm_cond_backward after me_gnorm_stats, on tensors of the
test's own, so that `batch_row`, `n_batch`, the alignment of every matrix and the NULL arguments are chosen freely.

Expectation: float64 on the CPU (`reference`): torch.nn.functional.group_norm on the rows of every instance, then
`* (1 + scale[b]) + shift[b]`, then silu, with autograd for the gradients; an instance without rows adds nothing and gets
zero rows of grad_scale / grad_shift.  No expected value comes from a kernel.  Bound: helpers.assert_close at its
defaults, 1e-4 + 1e-4 |b| per element (the project's fp32 bound).

Before every call the workspace, allocated at exactly me_gnorm_cond_workspace_bytes, is filled with 0xFF bytes (a NaN
in every float slot): a result that depends on a word that was never written comes out as NaN.  The error paths are
host-side argument checks: nothing is launched, and the outputs keep what they held."""
import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
EPS = 1e-5
SENTINEL = 7.0
PARAMS = ("gamma", "beta", "scale", "shift")
GRADS = ("dx", "grad_gamma", "grad_beta", "grad_scale", "grad_shift")
OUTPUTS = ("out",) + GRADS


def make_inputs(sizes, c, groups, seed, order=None):
    """sizes: rows per instance (0: absent).  x = N(0, 1) + per-(instance, channel) offsets in [-2, 2]"""
    rng = np.random.default_rng([seed, c, groups])
    br = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    if order is not None:
        br = br[order]
    n, nb = len(br), len(sizes)
    x = rng.uniform(-2, 2, (nb, c))[br] + rng.standard_normal((n, c))
    return dict(x=x.astype(np.float32), dy=rng.uniform(-0.5, 0.5, (n, c)).astype(np.float32),
                gamma=rng.uniform(0.5, 1.5, c).astype(np.float32), beta=rng.uniform(-0.5, 0.5, c).astype(np.float32),
                scale=(0.5 * rng.standard_normal((nb, c))).astype(np.float32),
                shift=rng.standard_normal((nb, c)).astype(np.float32), batch_row=br, n_batch=nb, c=c, groups=groups)


def reference(inp, act=1, eps=EPS, null=()):
    """float64 with autograd: out, dx [n, c]; grad_gamma, grad_beta [c]; grad_scale, grad_shift [n_batch, c].  null: the
    parameters passed as NULL (gamma 1, the others 0); their gradients are not part of the result"""
    nb, c, G = inp["n_batch"], inp["c"], inp["groups"]
    neutral = dict(gamma=np.ones(c), beta=np.zeros(c), scale=np.zeros((nb, c)), shift=np.zeros((nb, c)))
    x = torch.tensor(inp["x"].astype(np.float64), requires_grad=True)
    p = {k: torch.tensor((neutral[k] if k in null else inp[k]).astype(np.float64), requires_grad=True) for k in PARAMS}
    br = torch.tensor(inp["batch_row"].astype(np.int64))
    out = torch.zeros_like(x)
    for b in range(nb):
        m = (br == b).nonzero().reshape(-1)
        if m.numel() == 0:
            continue
        o = torch.nn.functional.group_norm(x[m].t()[None], G, p["gamma"], p["beta"], eps)[0].t()
        o = o * (1 + p["scale"][b]) + p["shift"][b]
        out = out.index_copy(0, m, torch.nn.functional.silu(o) if act == 1 else o)
    out.backward(torch.tensor(inp["dy"].astype(np.float64)))
    res = dict(out=out.detach().numpy(), dx=x.grad.numpy())
    for k in PARAMS:
        if k not in null:
            res["grad_" + k] = p[k].grad.numpy()
    return res


def _place(a, device, offset, fill=SENTINEL):
    """-> (allocation, view): a float32 matrix on the device; offset: it begins one element (4 bytes) into its allocation
    and ends exactly at its end"""
    t = torch.tensor(np.asarray(a, dtype=np.float32)).reshape(-1)
    buf = torch.full((max(t.numel(), 1) + (1 if offset else 0),), fill, dtype=torch.float32, device=device)
    view = buf[1:] if offset else buf
    view[:t.numel()].copy_(t)
    assert view.data_ptr() % 16 == (4 if offset else 0)
    return buf, view


def run(device, inp, act=1, null=(), want=GRADS, offset=(), short_workspace=False):
    """stats -> conditional apply -> conditional backward through the C ABI on fresh buffers -> dict of CPU tensors, or,
    with short_workspace, the return codes of apply and backward given one byte less than the workspace size"""
    from minkowskiengine_amd import _lib as L
    lib = L.load()
    br_np, nb, c, G = inp["batch_row"], inp["n_batch"], inp["c"], inp["groups"]
    n = len(br_np)
    st = torch.cuda.current_stream(device).cuda_stream
    xbuf, xd = _place(inp["x"], device, "x" in offset)
    gbuf, gd = _place(inp["dy"], device, "dy" in offset)
    br = torch.tensor(br_np).to(device)
    par = {k: None if k in null else torch.tensor(inp[k]).to(device) for k in PARAMS}
    mean = torch.empty((nb * G,), dtype=torch.float32, device=device)
    rstd = torch.empty((nb * G,), dtype=torch.float32, device=device)
    ybuf, y = _place(np.full(n * c, SENTINEL), device, "y" in offset)
    dxbuf, dx = _place(np.full(n * c, SENTINEL), device, "dx" in offset)
    outs = dict(dx=dx, grad_gamma=torch.full((c,), SENTINEL, dtype=torch.float32, device=device),
                grad_beta=torch.full((c,), SENTINEL, dtype=torch.float32, device=device),
                grad_scale=torch.full((nb, c), SENTINEL, dtype=torch.float32, device=device),
                grad_shift=torch.full((nb, c), SENTINEL, dtype=torch.float32, device=device))
    need = int(lib.me_gnorm_cond_workspace_bytes(n, nb, c, G))
    assert need >= int(lib.me_gnorm_workspace_bytes(n, nb, c, G)) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    ws.fill_(0xFF)
    ptr = lambda t: None if t is None else t.data_ptr()                           # noqa: E731
    L.check(lib.me_gnorm_stats(ptr(xd), 0, ptr(br), n, nb, c, G, float(EPS), ptr(mean), ptr(rstd), ptr(ws), need, st))
    head = (n, nb, c, G, ptr(mean), ptr(rstd)) + tuple(ptr(par[k]) for k in PARAMS) + (act,)
    bwd = tuple(ptr(outs[k]) if k in want else None for k in GRADS)
    if short_workspace:
        rc = (lib.me_gnorm_cond_apply(ptr(xd), 0, ptr(br), *head, ptr(y), ptr(ws), need - 1, st),
              lib.me_gnorm_cond_backward(ptr(xd), ptr(gd), 0, ptr(br), *head, *bwd, ptr(ws), need - 1, st))
        msg = lib.me_last_error().decode()
        torch.cuda.synchronize()
        untouched = all(bool((t == SENTINEL).all()) for t in [y[:n * c]] + [outs[k][:n * c] if k == "dx" else outs[k]
                                                                             for k in GRADS])
        return rc, msg, untouched
    ws.fill_(0xFF)
    L.check(lib.me_gnorm_cond_apply(ptr(xd), 0, ptr(br), *head, ptr(y), ptr(ws), need, st))
    ws.fill_(0xFF)
    L.check(lib.me_gnorm_cond_backward(ptr(xd), ptr(gd), 0, ptr(br), *head, *bwd, ptr(ws), need, st))
    res = dict(out=y[:n * c].reshape(n, c))
    for name in GRADS:
        t = outs[name][:n * c].reshape(n, c) if name == "dx" else outs[name]
        if name in want:
            res[name] = t
        else:
            assert bool((t == SENTINEL).all()), f"{name} was not requested and was written"
    torch.cuda.synchronize()
    for buf, name in ((ybuf, "y"), (dxbuf, "dx")):
        if name in offset:      # the element in front of an offset view was not written
            assert float(buf[0]) == SENTINEL, name
    return {k: v.cpu() for k, v in res.items()}


def _check_all(got, want, what=""):
    assert set(want) <= set(got)
    for k in want:
        assert bool(torch.isfinite(torch.as_tensor(got[k])).all()), f"{what}{k}"
        assert_close(got[k], want[k], what=f"{what}{k}")


@pytest.mark.parametrize("act", [1, 0], ids=["silu", "identity"])
def test_parity_with_an_absent_instance(device, act):
    """batch_row given directly, shuffled, using {0, 2, 3} of 4: the absent instance gets zero rows of grad_scale /
    grad_shift, written"""
    n = 300 + 257 + 40
    order = np.random.default_rng(11).permutation(n)
    inp = make_inputs([300, 0, 257, 40], 12, 4, seed=1, order=order)
    got = run(device, inp, act=act)
    _check_all(got, reference(inp, act=act))
    assert bool((got["grad_scale"][1] == 0).all()) and bool((got["grad_shift"][1] == 0).all())
    again = run(device, inp, act=act)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("c,groups", [(16, 4), (12, 4)])
@pytest.mark.parametrize("offset", [("x",), ("y",), ("dy",), ("dx",), ("x", "y", "dy", "dx")], ids="+".join)
def test_misaligned_views(device, offset, c, groups):
    """matrices that begin 4 bytes into a 16-byte line fall back to one-element pieces: no vector access at such an
    address, the same results within the fp32 bound"""
    inp = make_inputs([700, 40, 1], c, groups, seed=3)
    want = reference(inp)
    aligned = run(device, inp)
    got = run(device, inp, offset=offset)
    _check_all(aligned, want, what="aligned ")
    _check_all(got, want, what="misaligned ")
    _check_all(got, {k: v.numpy() for k, v in aligned.items()}, what="misaligned vs aligned ")


@pytest.mark.parametrize("null", PARAMS)
def test_one_null_parameter(device, null):
    inp = make_inputs([300, 257], 12, 4, seed=4)
    want = reference(inp, null=(null,))
    got = run(device, inp, null=(null,), want=tuple(k for k in GRADS if k != "grad_" + null))
    _check_all(got, want, what=f"no {null} ")
    assert "grad_" + null not in got


def test_all_parameters_null_is_the_normalisation_and_silu(device):
    inp = make_inputs([300, 257], 12, 4, seed=4)
    got = run(device, inp, null=PARAMS, want=("dx",))
    _check_all(got, reference(inp, null=PARAMS))


def test_subsets_of_the_gradients(device):
    """only the requested outputs are written (the others keep their guard value, checked in run), and each is bit for
    bit what the full call gives"""
    inp = make_inputs([300, 257], 12, 4, seed=5)
    full = run(device, inp)
    _check_all(full, reference(inp))
    for want in (("dx",), ("grad_gamma",), ("grad_beta",), ("grad_scale",), ("grad_shift",), ("grad_scale", "grad_shift"),
                 ("dx", "grad_shift"), ("grad_gamma", "grad_beta"), ()):
        got = run(device, inp, want=want)
        assert set(got) == {"out"} | set(want)
        for k in got:
            assert torch.equal(got[k], full[k]), (want, k)


@pytest.mark.parametrize("act", [1, 0], ids=["silu", "identity"])
def test_one_row(device, act):
    """n = 1: variance 0, xhat = 0 -> out = act(be); cg = 4 values in a group, so dx is small, not zero"""
    inp = make_inputs([1], 8, 2, seed=6)
    got = run(device, inp, act=act)
    _check_all(got, reference(inp, act=act))


def test_widest_rows(device):
    """3225 channels: the 64 KiB of LDS of the partial kernel with one row lane (5 c + 256 floats); 3226 are refused
    before any launch"""
    from minkowskiengine_amd import _lib as L
    inp = make_inputs([40, 24], 3225, 1, seed=7)
    assert len(inp["batch_row"]) == 64
    _check_all(run(device, inp), reference(inp))
    lib = L.load()
    c, big = 3226, 1 << 30
    st = torch.cuda.current_stream(device).cuda_stream
    for rc in (lib.me_gnorm_cond_apply(None, 0, None, 64, 2, c, 1, None, None, None, None, None, None, 1, None, None, big,
                                       st),
               lib.me_gnorm_cond_backward(None, None, 0, None, 64, 2, c, 1, None, None, None, None, None, None, 1, None,
                                          None, None, None, None, None, big, st)):
        assert rc != 0
        assert "channel count too large" in lib.me_last_error().decode()
    torch.cuda.synchronize()


def test_short_workspace_is_an_argument_error(device):
    inp = make_inputs([300, 257], 12, 4, seed=8)
    rc, msg, untouched = run(device, inp, short_workspace=True)
    assert rc[0] != 0 and rc[1] != 0
    assert "workspace too small" in msg
    assert untouched, "an entry point that returned an error wrote an output"


def test_unknown_act_is_an_argument_error(device):
    from minkowskiengine_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream(device).cuda_stream
    assert lib.me_gnorm_cond_apply(None, 0, None, 64, 2, 8, 2, None, None, None, None, None, None, 2, None, None, 1 << 30,
                                   st) != 0
    assert "act must be" in lib.me_last_error().decode()
