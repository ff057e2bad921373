"""Entry-point tests of the group-norm kernels (csrc/group_norm.hip and the shared csrc/segment_norm.hpp) through the C ABI:
me_gnorm_workspace_bytes / me_gnorm_stats / me_gnorm_apply / me_gnorm_backward, on tensors of the test's own, so that
`batch_row`, `n_batch`, the alignment of every matrix and the NULL arguments are chosen freely.

Expectation: one plain float64 restatement on the CPU (`reference`), segmented by batch_row and by group; an instance
without rows has mean 0, rstd 1 / sqrt(eps) and adds nothing to the parameter gradients.  No expected value comes from a
kernel.  Bound: helpers.assert_close at its defaults, 1e-4 + 1e-4 |b| per element (the project's fp32 bound).

Before every stats / backward call the workspace, allocated at exactly me_gnorm_workspace_bytes, is filled with 0xFF
bytes (a NaN in every float slot): a result that depends on a word that was never written comes out as NaN.  The error
paths are host-side argument checks: nothing is launched, and the outputs keep what they held."""
import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
EPS = 1e-5
SENTINEL = 7.0
NO_ROWS_RSTD = float(np.float32(1) / np.sqrt(np.float32(EPS)))       # 1 / sqrt(eps) in fp32, as the kernel forms it
OUTPUTS = ("mean", "rstd", "out", "dx", "grad_gamma", "grad_beta")


def make_inputs(sizes, c, groups, seed, order=None):
    """sizes: rows per instance (0: absent).  x = N(0, 1) + per-(instance, channel) offsets in [-2, 2]"""
    rng = np.random.default_rng([seed, c, groups])
    br = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    if order is not None:
        br = br[order]
    n = len(br)
    x = rng.uniform(-2, 2, (len(sizes), c))[br] + rng.standard_normal((n, c))
    return dict(x=x.astype(np.float32), dy=rng.uniform(-0.5, 0.5, (n, c)).astype(np.float32),
                gamma=rng.uniform(0.5, 1.5, c).astype(np.float32), beta=rng.uniform(-0.5, 0.5, c).astype(np.float32),
                batch_row=br, n_batch=len(sizes), c=c, groups=groups)


def reference(inp, eps=EPS, gamma=True, beta=True, x=None):
    """float64: mean, rstd [n_batch, groups]; out, dx [n, c]; grad_gamma, grad_beta [c]"""
    x = (inp["x"] if x is None else x).astype(np.float64)
    dy, br, nb, c, G = inp["dy"].astype(np.float64), inp["batch_row"], inp["n_batch"], inp["c"], inp["groups"]
    cg = c // G
    ga = inp["gamma"].astype(np.float64) if gamma else np.ones(c)
    be = inp["beta"].astype(np.float64) if beta else np.zeros(c)
    mean, rstd = np.zeros((nb, G)), np.full((nb, G), 1.0 / np.sqrt(eps))
    out, dx = np.zeros_like(x), np.zeros_like(x)
    gg, gb = np.zeros(c), np.zeros(c)
    for b in range(nb):
        rows = np.nonzero(br == b)[0]
        if len(rows) == 0:
            continue
        xb = x[rows].reshape(len(rows), G, cg)
        mu = xb.mean(axis=(0, 2))
        rs = 1.0 / np.sqrt(((xb - mu[None, :, None]) ** 2).mean(axis=(0, 2)) + eps)
        mean[b], rstd[b] = mu, rs
        xhat = ((xb - mu[None, :, None]) * rs[None, :, None]).reshape(len(rows), c)
        out[rows] = xhat * ga + be
        t1, t2 = dy[rows].sum(0), (dy[rows] * xhat).sum(0)
        gb += t1
        gg += t2
        m = len(rows) * cg
        T1 = np.repeat((ga * t1).reshape(G, cg).sum(1), cg) / m
        T2 = np.repeat((ga * t2).reshape(G, cg).sum(1), cg) / m
        dx[rows] = np.repeat(rs, cg) * (ga * dy[rows] - T1 - xhat * T2)
    return dict(mean=mean, rstd=rstd, out=out, dx=dx, grad_gamma=gg, grad_beta=gb)


def _place(a, device, offset, fill=SENTINEL):
    """-> (allocation, view): a float32 matrix on the device; offset: it begins one element (4 bytes) into its allocation
    and ends exactly at its end"""
    t = torch.tensor(np.asarray(a, dtype=np.float32)).reshape(-1)
    buf = torch.full((max(t.numel(), 1) + (1 if offset else 0),), fill, dtype=torch.float32, device=device)
    view = buf[1:] if offset else buf
    view[:t.numel()].copy_(t)
    assert view.data_ptr() % 16 == (4 if offset else 0)
    return buf, view


def run(device, inp, eps=EPS, gamma=True, beta=True, want=("dx", "grad_gamma", "grad_beta"), offset=(), x=None,
        short_workspace=False):
    """stats -> apply -> backward through the C ABI on fresh buffers -> dict of CPU tensors, or, with short_workspace,
    the return codes of stats and backward given one byte less than me_gnorm_workspace_bytes"""
    from minkowskiengine_amd import _lib as L
    lib = L.load()
    br_np, nb, c, G = inp["batch_row"], inp["n_batch"], inp["c"], inp["groups"]
    n = len(br_np)
    st = torch.cuda.current_stream(device).cuda_stream
    xbuf, xd = _place(inp["x"] if x is None else x, device, "x" in offset)
    gbuf, gd = _place(inp["dy"], device, "dy" in offset)
    br = torch.tensor(br_np if n else np.zeros(1, np.int32)).to(device)
    ga = torch.tensor(inp["gamma"]).to(device) if gamma else None
    be = torch.tensor(inp["beta"]).to(device) if beta else None
    mean = torch.full((nb * G,), SENTINEL, dtype=torch.float32, device=device)
    rstd = torch.full((nb * G,), SENTINEL, dtype=torch.float32, device=device)
    ybuf, y = _place(np.full(n * c, SENTINEL), device, "y" in offset)
    dxbuf, dx = _place(np.full(n * c, SENTINEL), device, "dx" in offset)
    gg = torch.full((c,), SENTINEL, dtype=torch.float32, device=device)
    gb = torch.full((c,), SENTINEL, dtype=torch.float32, device=device)
    need = int(lib.me_gnorm_workspace_bytes(n, nb, c, G))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    ws.fill_(0xFF)
    ptr = lambda t: None if t is None else t.data_ptr()                           # noqa: E731
    bwd = (ptr(mean), ptr(rstd), ptr(ga), ptr(dx) if "dx" in want else None, ptr(gg) if "grad_gamma" in want else None,
           ptr(gb) if "grad_beta" in want else None, ptr(ws))
    if short_workspace:
        rc = (lib.me_gnorm_stats(ptr(xd), 0, ptr(br), n, nb, c, G, float(eps), ptr(mean), ptr(rstd), ptr(ws), need - 1, st),
              lib.me_gnorm_backward(ptr(xd), ptr(gd), 0, ptr(br), n, nb, c, G, *bwd, need - 1, st))
        msg = lib.me_last_error().decode()
        torch.cuda.synchronize()
        untouched = all(bool((t == SENTINEL).all()) for t in (mean, rstd, dx[:n * c], gg, gb))
        return rc, msg, untouched
    L.check(lib.me_gnorm_stats(ptr(xd), 0, ptr(br), n, nb, c, G, float(eps), ptr(mean), ptr(rstd), ptr(ws), need, st))
    L.check(lib.me_gnorm_apply(ptr(xd), 0, ptr(br), n, nb, c, G, ptr(mean), ptr(rstd), ptr(ga), ptr(be), ptr(y), st))
    res = dict(mean=mean.reshape(nb, G), rstd=rstd.reshape(nb, G), out=y[:n * c].reshape(n, c))
    if n > 0:
        ws.fill_(0xFF)
        L.check(lib.me_gnorm_backward(ptr(xd), ptr(gd), 0, ptr(br), n, nb, c, G, *bwd, need, st))
    for name, t in (("dx", dx[:n * c].reshape(n, c)), ("grad_gamma", gg), ("grad_beta", gb)):
        if name in want and n > 0:
            res[name] = t
        else:
            assert bool((t == SENTINEL).all()), f"{name} was not requested and was written"
    torch.cuda.synchronize()
    for buf, name in ((ybuf, "y"), (dxbuf, "dx")):
        if name in offset:      # the element in front of an offset view was not written
            assert float(buf[0]) == SENTINEL, name
    return {k: v.cpu() for k, v in res.items()}


def _check_all(got, want, names=OUTPUTS, what=""):
    for k in names:
        assert_close(got[k], want[k], what=f"{what}{k}")


def test_more_instances_than_indices_present(device):
    """batch_row uses only {0, 2} of 4: the absent instances get mean 0 and rstd 1 / sqrt(eps) exactly"""
    inp = make_inputs([300, 0, 257, 0], 12, 4, seed=1)
    got = run(device, inp)
    _check_all(got, reference(inp))
    absent = torch.tensor([1, 3])
    assert bool((got["mean"][absent] == 0).all())
    assert torch.equal(got["rstd"][absent], torch.full((2, 4), NO_ROWS_RSTD, dtype=torch.float32))
    # the present instances do not see the absent ones: the same rows as instances {0, 1} of 2, bit for bit
    dense = dict(inp, batch_row=(inp["batch_row"] // 2).astype(np.int32), n_batch=2)
    alone = run(device, dense)
    for k in ("out", "dx", "grad_gamma", "grad_beta"):
        assert torch.equal(got[k], alone[k]), k
    assert torch.equal(got["mean"][[0, 2]], alone["mean"]) and torch.equal(got["rstd"][[0, 2]], alone["rstd"])


def test_no_rows(device):
    """n == 0: the "no rows" statistics for every instance, apply writes nothing, backward is an argument error"""
    from minkowskiengine_amd import _lib as L
    inp = make_inputs([0, 0, 0], 8, 2, seed=2)
    got = run(device, inp)
    assert bool((got["mean"] == 0).all())
    assert torch.equal(got["rstd"], torch.full((3, 2), NO_ROWS_RSTD, dtype=torch.float32))
    lib = L.load()
    assert lib.me_gnorm_backward(None, None, 0, None, 0, 3, 8, 2, None, None, None, None, None, None, None, 1 << 30,
                                 None) != 0
    assert "at least one row" in lib.me_last_error().decode()


@pytest.mark.parametrize("offset", [("x",), ("y",), ("dy",), ("dx",), ("x", "y", "dy", "dx")], ids="+".join)
def test_misaligned_views(device, offset):
    """matrices that begin 4 bytes into a 16-byte line fall back to one-element pieces: no vector access at such an
    address, the same results within the fp32 bound"""
    inp = make_inputs([700, 40, 1], 16, 4, seed=3)
    want = reference(inp)
    aligned = run(device, inp)
    got = run(device, inp, offset=offset)
    _check_all(aligned, want, what="aligned ")
    _check_all(got, want, what="misaligned ")
    _check_all(got, {k: v.numpy() for k, v in aligned.items()}, what="misaligned vs aligned ")


def test_null_arguments(device):
    inp = make_inputs([300, 257], 12, 4, seed=4)
    full = run(device, inp)
    _check_all(full, reference(inp))
    # gamma / beta NULL: 1 / 0
    plain = run(device, inp, gamma=False, beta=False)
    _check_all(plain, reference(inp, gamma=False, beta=False), what="no affine ")
    only_beta = run(device, inp, gamma=False)
    _check_all(only_beta, reference(inp, gamma=False), what="no gamma ")
    # each output of the backward pass on its own, and none: the others bit for bit what the full call gives
    for want in (("dx",), ("grad_gamma",), ("grad_beta",), ("grad_gamma", "grad_beta"), ("dx", "grad_beta"), ()):
        got = run(device, inp, want=want)
        assert set(got) == {"mean", "rstd", "out"} | set(want)
        for k in got:
            assert torch.equal(got[k], full[k]), (want, k)


def test_short_workspace_is_an_argument_error(device):
    inp = make_inputs([300, 257], 12, 4, seed=5)
    rc, msg, untouched = run(device, inp, short_workspace=True)
    assert rc[0] != 0 and rc[1] != 0
    assert "workspace too small" in msg
    assert untouched, "an entry point that returned an error wrote an output"


def test_nan_stays_in_its_instance_and_group(device):
    inp = make_inputs([300, 257, 40], 12, 4, seed=6)
    x = inp["x"].copy()
    x[300 + 17, 7] = np.nan                    # instance 1, channel 7: group 2
    got = run(device, inp, x=x)
    clean = run(device, inp)
    want = reference(inp)
    br = torch.tensor(inp["batch_row"].astype(np.int64))
    hit = (br == 1)[:, None] & (torch.arange(12) // 3 == 2)[None, :]
    assert bool(torch.isnan(got["out"][hit]).all()), "every element of the (instance, group) is NaN"
    assert bool(torch.isfinite(got["out"][~hit]).all())
    assert_close(got["out"][~hit], want["out"][~hit.numpy()], what="out of the other (instance, group)s")
    assert bool(torch.isnan(got["rstd"][1, 2])) and bool(torch.isnan(got["mean"][1, 2])), "not clamped"
    keep = torch.ones(3, 4, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(got["rstd"][keep], clean["rstd"][keep]) and torch.equal(got["mean"][keep], clean["mean"][keep])
    assert bool(torch.isfinite(got["dx"][~hit]).all())
    assert_close(got["dx"][~hit], want["dx"][~hit.numpy()], what="dx of the other (instance, group)s")


def test_widest_rows(device):
    """3225 channels: the 64 KiB of LDS of the partial kernels with one row lane (5 c + 256 floats); 3232 do not fit"""
    from minkowskiengine_amd import _lib as L
    inp = make_inputs([20, 13, 7], 3225, 1, seed=7)
    _check_all(run(device, inp), reference(inp))
    lib = L.load()
    c, big = 3232, 1 << 30
    st = torch.cuda.current_stream(device).cuda_stream
    keep = torch.full((3,), SENTINEL, dtype=torch.float32, device=device)
    p = keep.data_ptr()
    for rc in (lib.me_gnorm_stats(None, 0, None, 40, 3, c, 1, EPS, p, p, None, big, st),
               lib.me_gnorm_apply(None, 0, None, 40, 3, c, 1, None, None, None, None, None, st),
               lib.me_gnorm_backward(None, None, 0, None, 40, 3, c, 1, None, None, None, None, None, None, None, big, st)):
        assert rc != 0
        assert "channel count too large" in lib.me_last_error().decode()
    torch.cuda.synchronize()
    assert bool((keep == SENTINEL).all())
