"""Operator-level tests of the per-instance attention kernels (csrc/attention.hip) through AttentionForwardGPU /
AttentionBackwardGPU of both host layers.

Yardstick: float64 arithmetic written out here with torch (`reference`): softmax(Q K^T * scale) V per instance and head, with
autograd for the gradients.  No expected value comes from a kernel.  Exact cases (uniform weights, one-hot attention, a
one-row instance) are the lane-map checks: integer data and asymmetric operands, so a transposed or permuted fragment
cannot pass.  Bitwise cases (independence, strided operands, reproducibility, gradient subsets) compare two runs of the
kernels.

Error bound for fp32 and bf16 (`within_bound`): for each case E_torch is the maximum absolute error, against the float64
result, of torch's own attention in the same dtype on the same rows per instance (scaled_dot_product_attention under
sdpa_kernel(SDPBackend.MATH), autograd for the gradients); the kernels must stay within FACTOR * E_torch per tensor (out,
dq, dk, dv).  Every figure is printed before it is asserted (pytest -s)."""
import math

import pytest
import torch

import minkowskiengine_amd as ME
from minkowskiengine_amd import host as _host

pytestmark = pytest.mark.gpu

BQ = BK = 64   # kAttnBlock of csrc/attn_block.hpp: the stationary rows of a workgroup, forward and backward
# A blocked online softmax sums in another order than torch's single pass, and on draws of a hundred rows the error of
# either fluctuates by about a factor of two: 4 covers both.  Measured ratios E_kernel / E_torch (one run, the maximum
# over d, layouts and hosts; out / dq / dk / dv): block edges fp32 1.12 / 1.45 / 1.75 / 1.24, bf16 1.00 / 1.83 / 1.67 / 1.67;
# large logits fp32 0.78 / 0.58 / 1.17 / 1.04, bf16 1.08 / 1.35 / 2.30 / 1.16; two maps fp32 1.13 / 1.93 / 1.52 / 0.96, bf16
# 1.00 / 1.91 / 1.70 / 1.44; strided <= 1.67; module level <= 2.79.
FACTOR = 4.0
DTYPES = (torch.float32, torch.bfloat16)
NAMES = ("out", "dq", "dk", "dv")


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def make_tensor(sizes, device, shuffle=False, seed=0):
    """a sparse tensor with sizes[b] voxels in instance b on one line; -> (tensor, batch index of every row (int64))"""
    g = torch.Generator().manual_seed(seed)
    coords = torch.cat([torch.stack([torch.full((n,), b), torch.arange(n), torch.zeros(n), torch.zeros(n)], 1)
                        for b, n in enumerate(sizes)]).int()
    if shuffle:
        coords = coords[torch.randperm(coords.shape[0], generator=g)]
    x = ME.SparseTensor(torch.zeros(coords.shape[0], 1), coordinates=coords, device=device)
    assert x.F.shape[0] == coords.shape[0]
    return x, x.C[:, 0].long()


def draw(n, c, dtype, device, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    return (amp * torch.randn(n, c, generator=g)).to(dtype).to(device)


# ---- the operators ----------------------------------------------------------------------------------------------------------
def run(xq, xkv, q, k, v, dout, heads, scale=None, need=(True, True, True), backward=True):
    """forward (+ backward) through the operators of the current host -> dict of device tensors"""
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    qk, kk, mgr = xq.coordinate_map_key, xkv.coordinate_map_key, xq._manager._manager
    fw = ME.get_minkowski_function("AttentionForward", q, qk)
    bw = ME.get_minkowski_function("AttentionBackward", q, qk)
    glob = _host.key_like(qk)
    out, lse = fw(q, k, v, heads, scale, qk, kk, glob, mgr)
    res = dict(out=out, lse=lse)
    if backward:
        res["dq"], res["dk"], res["dv"] = bw(q, k, v, out, lse, dout, heads, scale, qk, kk, glob, mgr, need_grad_q=need[0],
                                             need_grad_k=need[1], need_grad_v=need[2])
    return res


# ---- yardsticks -------------------------------------------------------------------------------------------------------------
def _heads(t, rows, heads):
    return t[rows].view(rows.numel(), heads, -1).transpose(0, 1)   # [H, n, d]


def reference(q, k, v, dout, bq, bk, heads, scale=None):
    """float64, written out: softmax(Q K^T scale) V per instance and head, autograd for the gradients; lse too"""
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    q64, k64, v64 = (t.detach().double().requires_grad_() for t in (q, k, v))
    out = torch.zeros_like(q64)
    lse = torch.full((q.shape[0], heads), -math.inf, dtype=torch.float64, device=q.device)
    for b in torch.unique(bq).tolist():
        mq, mk = (bq == b).nonzero().reshape(-1), (bk == b).nonzero().reshape(-1)
        if mk.numel() == 0:
            continue
        s = _heads(q64, mq, heads) @ _heads(k64, mk, heads).transpose(1, 2) * scale
        o = torch.softmax(s, -1) @ _heads(v64, mk, heads)
        out = out.index_copy(0, mq, o.transpose(0, 1).reshape(mq.numel(), -1))
        lse[mq] = torch.logsumexp(s.detach(), -1).t()
    out.backward(dout.double())
    z = torch.zeros_like
    return dict(out=out.detach(), lse=lse, dq=q64.grad if q64.grad is not None else z(q64),
                dk=k64.grad if k64.grad is not None else z(k64), dv=v64.grad if v64.grad is not None else z(v64))


def torch_attention(q, k, v, dout, bq, bk, heads, scale=None):
    """torch's own attention in the dtype of q on the rows of every instance: the yardstick of the error bound"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    d = q.shape[1] // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    q_, k_, v_ = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = torch.zeros_like(q_)
    with sdpa_kernel(SDPBackend.MATH):
        for b in torch.unique(bq).tolist():
            mq, mk = (bq == b).nonzero().reshape(-1), (bk == b).nonzero().reshape(-1)
            if mk.numel() == 0:
                continue
            o = torch.nn.functional.scaled_dot_product_attention(
                _heads(q_, mq, heads)[None], _heads(k_, mk, heads)[None], _heads(v_, mk, heads)[None], scale=scale)[0]
            out = out.index_copy(0, mq, o.transpose(0, 1).reshape(mq.numel(), -1))
        out.backward(dout)
    z = torch.zeros_like
    return dict(out=out.detach(), dq=q_.grad if q_.grad is not None else z(q_),
                dk=k_.grad if k_.grad is not None else z(k_), dv=v_.grad if v_.grad is not None else z(v_))


def within_bound(ours, q, k, v, dout, bq, bk, heads, scale=None, what=""):
    ref = reference(q, k, v, dout, bq, bk, heads, scale)
    theirs = torch_attention(q, k, v, dout, bq, bk, heads, scale)
    bad = []
    for name in NAMES:
        assert torch.isfinite(ours[name].float()).all(), f"{what} {name}: not finite"
        e = float((ours[name].double() - ref[name]).abs().max())
        et = float((theirs[name].double() - ref[name]).abs().max())
        print(f"{what} {name}: E_kernel {e:.3e}  E_torch {et:.3e}  ratio {e / et if et > 0 else float('inf') if e > 0 else 0:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    finite = torch.isfinite(ref["lse"])
    assert torch.equal(torch.isfinite(ours["lse"]), finite)
    assert float((ours["lse"].double()[finite] - ref["lse"][finite]).abs().max()) <= 1e-5 * max(1.0, float(ref["lse"][finite].abs().max()))
    assert not bad, f"{what}: beyond {FACTOR} x E_torch: {bad}"


# ---- exact data: the lane-map checks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_uniform_weights_give_the_column_mean_exactly(device, host_layer, d, dtype):
    """q = k = 0: every weight is 1 / n_b.  v = small asymmetric integers and n_b a power of two (half a block, a block, two
    blocks): the per-instance, per-head column mean is exact in fp32, so out must EQUAL it."""
    heads = 2
    x, b = make_tensor([BK // 2, BK, 2 * BK], device, shuffle=True, seed=d)
    n, c = b.numel(), heads * d
    rows, cols = torch.arange(n, device=device)[:, None], torch.arange(c, device=device)[None]
    v = ((rows * 7 + cols * 3) % 17).to(dtype)
    q = torch.zeros(n, c, dtype=dtype, device=device)
    r = run(x, x, q, q.clone(), v, None, heads, backward=False)
    want = torch.zeros(n, c, dtype=torch.float32, device=device)
    for i in range(3):
        m = b == i
        want[m] = v[m].float().mean(0, keepdim=True)   # integers below 2^24 and a power-of-two count: exact
    assert torch.equal(r["out"], want.to(dtype))
    for i, nb in enumerate((BK // 2, BK, 2 * BK)):
        assert float((r["lse"][b == i] - math.log(nb)).abs().max()) <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_one_hot_attention_gives_the_class_mean(device, host_layer, d, dtype):
    """q and k are one-hot rows times 64: a row attends to the keys of its own class only (the other scores are
    4096 / sqrt(d) >= 362 lower, exp underflows to 0).  The classes are spread unevenly over the key blocks."""
    heads, classes = 2, 5
    x, b = make_tensor([2 * BK + 2, BK - 1], device, shuffle=True, seed=100 + d)
    n, c = b.numel(), heads * d
    idx = torch.arange(n, device=device)
    cls = (idx * idx + idx // 7) % classes
    q = torch.zeros(n, heads, d, dtype=dtype, device=device)
    q[idx, 0, cls] = 64.0
    q[idx, 1, (cls * 3 + 1) % d] = 64.0          # another one-hot position per head, the same classes
    q = q.view(n, c)
    v = ((idx[:, None] * 7 + torch.arange(c, device=device)[None] * 3) % 17).to(dtype)
    r = run(x, x, q, q.clone(), v, None, heads, backward=False)
    want = torch.zeros(n, c, dtype=torch.float64, device=device)
    for i in range(2):
        for k in range(classes):
            m = (b == i) & (cls == k)
            want[m] = v[m].double().mean(0, keepdim=True)
    tol = 16.0 * (2.0 ** -22 if dtype == torch.float32 else 2.0 ** -8)   # max |v| times a few roundings of the dtype
    err = float((r["out"].double() - want).abs().max())
    print(f"one-hot d={d} {dtype}: max error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_one_row_instance_is_exact(device, host_layer, dtype):
    heads, d = 2, 32
    x, b = make_tensor([3, 1, BK + 1], device, shuffle=True, seed=5)
    n, c = b.numel(), heads * d
    q, k, v, dout = (draw(n, c, dtype, device, s) for s in (1, 2, 3, 4))
    r = run(x, x, q, k, v, dout, heads)
    m = b == 1
    assert int(m.sum()) == 1
    assert torch.equal(r["out"][m], v[m])
    assert torch.equal(r["dq"][m], torch.zeros_like(q[m])) and torch.equal(r["dk"][m], torch.zeros_like(k[m]))
    assert torch.equal(r["dv"][m], dout[m])


# ---- block edges, bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shuffle", [False, True], ids=["grouped", "shuffled"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_block_edges(device, host_layer, d, shuffle, dtype):
    """instances of 1, BK - 1, BK, BK + 1 and 2 BK + 2 rows in one tensor: forward and all three gradients"""
    heads = 3
    x, b = make_tensor([1, BK - 1, BK, BK + 1, 2 * BK + 2], device, shuffle=shuffle, seed=d)
    n, c = b.numel(), heads * d
    q, k, v, dout = (draw(n, c, dtype, device, 10 * d + s) for s in range(4))
    r = run(x, x, q, k, v, dout, heads)
    within_bound(r, q, k, v, dout, b, b, heads, what=f"edges d={d} shuffle={shuffle} {dtype} {host_layer}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_large_logits_stay_finite(device, host_layer, dtype):
    """|s| reaches a few hundred: without the running maximum fp32 exp overflows"""
    heads, d = 2, 64
    x, b = make_tensor([BK + 5, 2 * BK + 1], device, shuffle=True, seed=9)
    n, c = b.numel(), heads * d
    q, k, v, dout = (draw(n, c, dtype, device, 40 + s, amp=(30.0, 4.0, 1.0, 1.0)[s]) for s in range(4))
    s = (q.double().view(n, heads, d).transpose(0, 1) @ k.double().view(n, heads, d).transpose(0, 1).transpose(1, 2)) / 8.0
    assert float(s.abs().max()) > 200.0
    r = run(x, x, q, k, v, dout, heads)
    within_bound(r, q, k, v, dout, b, b, heads, what=f"large logits {dtype} {host_layer}")


# ---- different maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_queries_and_keys_on_different_maps(device, host_layer, dtype):
    """queries on the stride-2 map, keys / values on a pruned stride-1 map of the same manager; instance 1 is present on
    the query map and absent on the key map: zero rows, lse = -inf, zero gradients"""
    heads, d = 2, 32
    x, b1 = make_tensor([BK + 7, 9, 2 * BK - 3], device, shuffle=True, seed=21)
    xq = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)(x)
    xkv = ME.MinkowskiPruning()(x, b1 != 1)
    bq, bk = xq.C[:, 0].long(), xkv.C[:, 0].long()
    assert xq.tensor_stride[0] == 2 and int((bq == 1).sum()) > 0 and int((bk == 1).sum()) == 0
    c = heads * d
    q, dout = draw(bq.numel(), c, dtype, device, 1), draw(bq.numel(), c, dtype, device, 2)
    k, v = draw(bk.numel(), c, dtype, device, 3), draw(bk.numel(), c, dtype, device, 4)
    r = run(xq, xkv, q, k, v, dout, heads)
    m = bq == 1
    assert torch.equal(r["out"][m], torch.zeros_like(q[m])) and torch.equal(r["dq"][m], torch.zeros_like(q[m]))
    assert bool(torch.isneginf(r["lse"][m]).all())
    within_bound(r, q, k, v, dout, bq, bk, heads, what=f"two maps {dtype} {host_layer}")


# ---- bitwise properties -------------------------------------------------------------------------------------------------------
def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_instance_does_not_see_its_neighbour(device, host_layer, dtype):
    """instance A (BK + 1 rows: it ends one slot into a block) next to an instance of Inf and NaN, rows interleaved, must
    give bit for bit what the same rows give alone: a difference means a padded slot or a neighbour's row leaks"""
    heads, d, na = 2, 64, BK + 1
    c = heads * d
    qa, ka, va, da = (draw(na, c, dtype, device, 70 + s) for s in range(4))
    xa, _ = make_tensor([na], device)
    alone = run(xa, xa, qa, ka, va, da, heads)
    x, b = make_tensor([na, BK + 3], device, shuffle=True, seed=33)
    n = b.numel()
    bad = torch.full((n, c), math.inf, dtype=dtype, device=device)
    bad[::2] = math.nan
    bad[1::4] = -math.inf
    ma = b == 0
    q, k, v, dout = (bad.clone().index_put_((ma.nonzero().reshape(-1),), t) for t in (qa, ka, va, da))
    both = run(x, x, q, k, v, dout, heads)
    for name in NAMES + ("lse",):
        assert torch.isfinite(alone[name].float()).all()
        assert _equal(both[name][ma], alone[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_strided_operands_equal_contiguous_copies(device, host_layer, dtype):
    heads, d = 2, 32
    c = heads * d
    x, b = make_tensor([BK + 1, 17], device, shuffle=True, seed=3)
    n = b.numel()
    qkv, dout = draw(n, 3 * c, dtype, device, 1), draw(n, c, dtype, device, 2)
    views = [qkv[:, i * c:(i + 1) * c] for i in range(3)]
    assert not views[0].is_contiguous()
    strided = run(x, x, *views, dout, heads)
    copied = run(x, x, *(t.contiguous() for t in views), dout, heads)
    for name in NAMES + ("lse",):
        assert _equal(strided[name], copied[name]), name
    within_bound(strided, *views, dout, b, b, heads, what=f"strided {dtype} {host_layer}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_calls_and_two_hosts_are_bitwise_equal(device, dtype):
    heads, d = 2, 64
    c = heads * d
    results = []
    prev = ME.get_host()
    try:
        for layer in ("python", "native", "python"):
            ME.set_host(layer)
            x, b = make_tensor([2 * BK + 2, BK - 1, 5], device, shuffle=True, seed=12)
            q, k, v, dout = (draw(b.numel(), c, dtype, device, 90 + s) for s in range(4))
            results.append(run(x, x, q, k, v, dout, heads))
            results.append(run(x, x, q, k, v, dout, heads))
    finally:
        ME.set_host(prev)
    for other in results[1:]:
        for name in NAMES + ("lse",):
            assert _equal(results[0][name], other[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gradient_subsets(device, host_layer, dtype):
    """each of the seven non-empty need-flag subsets returns exactly the wanted gradients, bit for bit those of the
    all-three call"""
    heads, d = 2, 32
    c = heads * d
    x, b = make_tensor([BK + 2, 30], device, shuffle=True, seed=8)
    q, k, v, dout = (draw(b.numel(), c, dtype, device, 50 + s) for s in range(4))
    full = run(x, x, q, k, v, dout, heads)
    for mask in range(1, 8):
        need = tuple(bool(mask >> i & 1) for i in range(3))
        r = run(x, x, q, k, v, dout, heads, need=need)
        for name, wanted in zip(("dq", "dk", "dv"), need):
            if wanted:
                assert _equal(r[name], full[name]), (need, name)
            else:
                assert r[name] is None, (need, name)
