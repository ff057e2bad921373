"""MinkowskiCrossAttention, MinkowskiCrossAttentionFunction and MinkowskiFunctional.cross_attention on the GPU, under both
host layers.

Yardsticks: torch.nn.MultiheadAttention with key_padding_mask in float64 on the same weights, applied to every instance on
its own (module level), and the float64 attention written out in tests/test_gpu_attention_kernels.py (`reference`,
function level).  Error bound: the rule of that module — per tensor E_kernel <= FACTOR * E_torch, E_torch being the error
of torch's own math-backend attention in the dtype of the case against the same float64 result.  Every figure is printed
before it is asserted (pytest -s); measured maxima: DESIGN 8.14."""
import copy
import os
import sys

import pytest
import torch
from torch.nn.attention import SDPBackend, sdpa_kernel

import minkowskiengine_amd as ME
from test_gpu_attention_kernels import FACTOR, make_tensor, reference, torch_attention

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.bfloat16)
SIZES = (1, 70, 200)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def check_bound(ours, ref, theirs, what):
    bad = []
    for name in ours:
        assert torch.isfinite(ours[name].float()).all(), f"{what} {name}: not finite"
        e = float((ours[name].double() - ref[name]).abs().max())
        et = float((theirs[name].double() - ref[name]).abs().max())
        print(f"{what} {name}: E_kernel {e:.3e}  E_torch {et:.3e}  ratio {e / et if et > 0 else float('inf') if e > 0 else 0:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"{what}: beyond {FACTOR} x E_torch: {bad}"


def context_batch(batch, tokens, lengths):
    """the instance of every context row, -1 for a token beyond the length: the bk of `reference`"""
    t = torch.arange(tokens, device=batch.device)
    n_batch = int(batch.max()) + 1
    lens = [tokens] * n_batch if lengths is None else lengths
    return torch.cat([torch.where(t < int(lens[b]), b, -1) for b in range(n_batch)])


# ---- the module against torch.nn.MultiheadAttention ---------------------------------------------------------------------------
def mha_per_instance(mha, feats, batch, context, values, lengths):
    """torch's module on every instance as one sequence, the padding masked; -> the rows in the order of `feats`"""
    out = torch.zeros(feats.shape[0], mha.embed_dim, dtype=feats.dtype, device=feats.device)
    tokens = torch.arange(context.shape[1], device=feats.device)
    with sdpa_kernel(SDPBackend.MATH):
        for b in range(context.shape[0]):
            rows = (batch == b).nonzero().reshape(-1)
            o, _ = mha(feats[rows][None], context[b:b + 1], values[b:b + 1], need_weights=False,
                       key_padding_mask=(tokens >= int(lengths[b]))[None])
            out = out.index_copy(0, rows, o[0])
    return out


def module_run(module, runner, feats, context, values, dout):
    """forward + backward -> {out, every parameter gradient, dF, dcontext, dvalues}"""
    f, c, v = (t.detach().clone().requires_grad_() for t in (feats, context, values))
    module.zero_grad()
    out = runner(module, f, c, v)
    out.backward(dout.to(out.dtype))
    res = dict(out=out.detach(), dF=f.grad, dcontext=c.grad, dvalues=v.grad)
    res.update({"d" + n: p.grad.clone() for n, p in module.named_parameters()})
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kw", [dict(), dict(kdim=48, vdim=80)], ids=["same_dims", "kdim48_vdim80"])
def test_module_matches_multihead_attention_with_key_padding_mask(device, host_layer, kw, dtype):
    torch.manual_seed(5)
    embed, heads, tokens, lengths = 64, 2, 77, (77, 1, 40)
    x, batch = make_tensor(SIZES, device, shuffle=True, seed=7)
    ours = ME.MinkowskiCrossAttention(embed, heads, **kw).to(device)
    with torch.no_grad():
        ours.in_proj_bias.normal_(std=0.1)
        ours.out_proj.bias.normal_(std=0.1)
    ours = ours.to(dtype)
    mha = torch.nn.MultiheadAttention(embed, heads, batch_first=True, **kw).to(device).to(dtype)
    mha.load_state_dict(ours.state_dict(), strict=True)
    mha64 = copy.deepcopy(mha).double()                           # the rounded weights of the case, in float64
    feats = torch.randn(batch.numel(), embed, device=device).to(dtype)
    context = torch.randn(3, tokens, ours.kdim, device=device).to(dtype)
    values = torch.randn(3, tokens, ours.vdim, device=device).to(dtype)
    dout = torch.randn(batch.numel(), embed, device=device).to(dtype)
    len_dev = torch.tensor(lengths, device=device)

    def run_ours(m, f, c, v):
        xs = ME.SparseTensor(f, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
        y = m(xs, c, len_dev, value_context=v)
        assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == x.coordinate_map_key
        return y.F

    def run_torch(m, f, c, v):
        return mha_per_instance(m, f, batch, c, v, lengths)
    got = module_run(ours, run_ours, feats, context, values, dout)
    ref = module_run(mha64, run_torch, feats.double(), context.double(), values.double(), dout.double())
    theirs = module_run(mha, run_torch, feats, context, values, dout)
    assert sorted(got) == sorted(ref)
    check_bound(got, ref, theirs, f"module {kw} {dtype} {host_layer}")
    for name in ("dcontext", "dvalues"):                          # the padding of instances 1 and 2: exactly zero
        assert float(got[name][1, 1:].abs().max()) == 0.0 and float(got[name][2, 40:].abs().max()) == 0.0, name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_module_shares_one_context_projection_between_keys_and_values(device, host_layer, dtype):
    """kdim == vdim == embed_dim and no value_context: k and v are the column views of ONE projection of the context"""
    torch.manual_seed(6)
    embed, heads, tokens, lengths = 64, 2, 20, (20, 7)
    x, batch = make_tensor((40, 9), device, shuffle=True, seed=2)
    ours = ME.MinkowskiCrossAttention(embed, heads).to(device).to(dtype)
    mha = torch.nn.MultiheadAttention(embed, heads, batch_first=True).to(device).to(dtype)
    mha.load_state_dict(ours.state_dict(), strict=True)
    mha64 = copy.deepcopy(mha).double()
    feats, dout = (torch.randn(batch.numel(), embed, device=device).to(dtype) for _ in range(2))
    context = torch.randn(2, tokens, embed, device=device).to(dtype)

    def run_ours(m, f, c, v):
        xs = ME.SparseTensor(f, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
        return m(xs, c, torch.tensor(lengths)).F                  # lengths on the host: moved by the function

    def run_torch(m, f, c, v):
        return mha_per_instance(m, f, batch, c, c, lengths)
    got = module_run(ours, run_ours, feats, context, context, dout)
    ref = module_run(mha64, run_torch, feats.double(), context.double(), context.double(), dout.double())
    theirs = module_run(mha, run_torch, feats, context, context, dout)
    for r in (got, ref, theirs):
        assert r.pop("dvalues") is None
    check_bound(got, ref, theirs, f"module shared projection {dtype} {host_layer}")


# ---- the function ---------------------------------------------------------------------------------------------------------------
def function_run(x, q, k, v, dout, heads, lengths=None, scale=None, kv_splits=None):
    q_, k_, v_ = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = ME.MinkowskiCrossAttentionFunction.apply(q_, k_, v_, lengths, heads, scale, x.coordinate_map_key,
                                                   x.coordinate_manager, kv_splits)
    out.backward(dout)
    return dict(out=out.detach(), dq=q_.grad, dk=k_.grad, dv=v_.grad)


def draw_case(device, dtype, sizes, tokens, heads, d, seed, shuffle=True):
    x, batch = make_tensor(sizes, device, shuffle=shuffle, seed=seed)
    g = torch.Generator().manual_seed(seed)
    c = heads * d
    q, dout = (torch.randn(batch.numel(), c, generator=g).to(dtype).to(device) for _ in range(2))
    k, v = (torch.randn(len(sizes), tokens, c, generator=g).to(dtype).to(device) for _ in range(2))
    return x, batch, q, k, v, dout


def function_yardsticks(batch, q, k, v, dout, heads, lengths, scale=None):
    bk = context_batch(batch, k.shape[1], lengths)
    flat = lambda t: t.reshape(-1, t.shape[-1])          # noqa: E731
    ref = reference(q, flat(k), flat(v), dout, batch, bk, heads, scale)
    theirs = torch_attention(q, flat(k), flat(v), dout, batch, bk, heads, scale)
    ref.pop("lse")
    for r in (ref, theirs):
        r["dk"], r["dv"] = r["dk"].view(k.shape), r["dv"].view(v.shape)
    return ref, theirs


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_functional_with_scale_lengths_and_an_empty_context(device, host_layer, dtype):
    heads, d, tokens, lengths = 2, 32, 77, (77, 0, 3)
    x, batch, q, k, v, dout = draw_case(device, dtype, SIZES, tokens, heads, d, seed=1)
    ref, theirs = function_yardsticks(batch, q, k, v, dout, heads, lengths, scale=0.3)
    q_, k_, v_ = (t.detach().clone().requires_grad_() for t in (q, k, v))
    xs = ME.SparseTensor(q_, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
    y = ME.MinkowskiFunctional.cross_attention(xs, k_, v_, heads, context_lengths=torch.tensor(lengths), scale=0.3)
    assert isinstance(y, ME.SparseTensor) and y.coordinate_map_key == x.coordinate_map_key
    y.F.backward(dout)
    got = dict(out=y.F.detach(), dq=q_.grad, dk=k_.grad, dv=v_.grad)
    check_bound(got, ref, theirs, f"functional scale=0.3 {dtype} {host_layer}")
    empty = batch == 1                                              # the instance of length 0: zero rows, zero gradients
    assert float(got["out"][empty].abs().max()) == 0.0 and float(got["dq"][empty].abs().max()) == 0.0
    for name in ("dk", "dv"):
        assert float(got[name][1].abs().max()) == 0.0 and float(got[name][2, 3:].abs().max()) == 0.0, name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_no_lengths_equal_full_lengths_bitwise(device, host_layer, dtype):
    x, batch, q, k, v, dout = draw_case(device, dtype, SIZES, 77, 2, 64, seed=2)
    a = function_run(x, q, k, v, dout, 2)
    b = function_run(x, q, k, v, dout, 2, lengths=torch.tensor([77, 77, 77], device=device))
    c = function_run(x, q, k, v, dout, 2, lengths=[90, 77, 1000])                    # clamped on the device
    for name in a:
        assert _same(a[name], b[name]) and _same(a[name], c[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_policy_and_forced_splits_agree_within_the_bound(device, host_layer, dtype, monkeypatch):
    """2 x 2,100 queries under 77 tokens: few workgroups, at least 2,048 queries per instance — a shape the policy may
    split.  The policy's S, a forced S = 1, a forced S = 4 and S = 3 from the environment: each within the bound; the
    forward pass and dq do not depend on S at all; forcing the policy's own S changes nothing."""
    from minkowskiengine_amd import _lib
    heads, d, tokens, lengths = 2, 32, 77, (77, 50)
    x, batch, q, k, v, dout = draw_case(device, dtype, (2100, 2100), tokens, heads, d, seed=4)
    ref, theirs = function_yardsticks(batch, q, k, v, dout, heads, lengths)
    s = _lib.load().me_attn_kv_splits(batch.numel(), 2 * tokens, 2, heads * d, heads)
    print(f"the policy's S for 2 x 2100 queries, 2 x 77 tokens, {heads} heads: {s}")
    runs = dict(policy=function_run(x, q, k, v, dout, heads, lengths),
                one=function_run(x, q, k, v, dout, heads, lengths, kv_splits=1),
                four=function_run(x, q, k, v, dout, heads, lengths, kv_splits=4),
                same=function_run(x, q, k, v, dout, heads, lengths, kv_splits=s))
    monkeypatch.setenv("ME_AMD_ATTN_KV_SPLITS", "3")
    runs["env"] = function_run(x, q, k, v, dout, heads, lengths)
    monkeypatch.delenv("ME_AMD_ATTN_KV_SPLITS")
    for name, r in runs.items():
        check_bound(r, ref, theirs, f"S={name} {dtype} {host_layer}")
        assert _same(r["out"], runs["one"]["out"]) and _same(r["dq"], runs["one"]["dq"]), name
        assert float(r["dk"][1, 50:].abs().max()) == 0.0 and float(r["dv"][1, 50:].abs().max()) == 0.0, name
    for name in ("dk", "dv"):
        assert _same(runs["policy"][name], runs["same"][name]), name
        if dtype == torch.float32:              # another partition of the sum: another rounding somewhere in 154 x 64 sums
            assert not _same(runs["four"][name], runs["one"][name]) and not _same(runs["env"][name], runs["four"][name]), name
    with pytest.raises(RuntimeError, match="kv_splits"):
        function_run(x, q, k, v, dout, heads, lengths, kv_splits=33)


def test_gradcheck_float64(device, host_layer):
    """2 instances, 5 tokens, d = 5 (the float64 twins take any head dimension), lengths (5, 3)"""
    x, batch = make_tensor((4, 3), device, shuffle=True, seed=3)
    g = torch.Generator().manual_seed(0)
    q = torch.randn(7, 10, generator=g, dtype=torch.float64).to(device).requires_grad_()
    k, v = (torch.randn(2, 5, 10, generator=g, dtype=torch.float64).to(device).requires_grad_() for _ in range(2))
    lengths = torch.tensor([5, 3], device=device)

    def fn(q, k, v):
        return ME.MinkowskiCrossAttentionFunction.apply(q, k, v, lengths, 2, None, x.coordinate_map_key,
                                                        x.coordinate_manager)
    assert torch.autograd.gradcheck(fn, (q, k, v), eps=1e-6, atol=1e-7, rtol=1e-5)
    fn(q, k, v).sum().backward()
    assert float(k.grad[1, 3:].abs().max()) == 0.0 and float(v.grad[1, 3:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_hosts_are_bitwise_equal(device, dtype):
    results = []
    prev = ME.get_host()
    try:
        for layer in ("python", "native", "python"):
            ME.set_host(layer)
            x, batch, q, k, v, dout = draw_case(device, dtype, (2100, 70, 2100), 77, 2, 64, seed=12)
            for lengths in (None, (77, 1, 30)):
                for splits in (None, 1, 3):
                    results.append((layer, lengths, splits, function_run(x, q, k, v, dout, 2, lengths, kv_splits=splits)))
    finally:
        ME.set_host(prev)
    first = {(le, s): r for la, le, s, r in results[:6]}
    for layer, lengths, splits, r in results[6:]:
        for name in r:
            assert _same(first[(lengths, splits)][name], r[name]), (layer, lengths, splits, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_shuffled_rows_equal_grouped_rows_after_unpermuting(device, host_layer, dtype):
    heads, d, tokens, lengths = 2, 64, 77, (30, 77, 2)
    xg, bg, q, k, v, dout = draw_case(device, dtype, SIZES, tokens, heads, d, seed=9, shuffle=False)
    xs, bs = make_tensor(SIZES, device, shuffle=True, seed=9)
    key = lambda x: x.C[:, 0].long() * 1000 + x.C[:, 1].long()          # noqa: E731
    perm = torch.argsort(key(xs))[torch.argsort(torch.argsort(key(xg)))]   # row i of xg is row perm[i] of xs
    assert torch.equal(xs.C[perm], xg.C) and not torch.equal(perm, torch.arange(perm.numel(), device=device))
    qs, ds = torch.empty_like(q), torch.empty_like(dout)
    qs[perm], ds[perm] = q, dout
    grouped = function_run(xg, q, k, v, dout, heads, lengths)
    shuffled = function_run(xs, qs, k, v, ds, heads, lengths)
    shuffled["out"], shuffled["dq"] = shuffled["out"][perm], shuffled["dq"][perm]
    ref, theirs = function_yardsticks(bg, q, k, v, dout, heads, lengths)
    check_bound(grouped, ref, theirs, f"grouped {dtype} {host_layer}")
    check_bound(shuffled, ref, theirs, f"shuffled {dtype} {host_layer}")
    for name in ("out", "dq"):                  # a query's own arithmetic does not depend on where its row sits
        assert _same(grouped[name], shuffled[name]), name


# ---- the example, the errors ------------------------------------------------------------------------------------------------------
def test_example_block_runs_a_step(device, host_layer):
    import cross_attention_block as CB
    torch.manual_seed(0)
    x, batch = make_tensor((90, 40), device, shuffle=True, seed=1)
    x = ME.SparseTensor(torch.randn(batch.numel(), 64, device=device), coordinate_map_key=x.coordinate_map_key,
                        coordinate_manager=x.coordinate_manager)
    block = CB.CrossAttentionBlock(64, 2, emb_channels=16, context_channels=48).to(device)
    emb = torch.randn(2, 16, device=device)
    context = torch.randn(2, 9, 48, device=device, requires_grad=True)
    out = block(x, emb, context, torch.tensor([9, 4]))
    assert isinstance(out, ME.SparseTensor) and tuple(out.F.shape) == (130, 64)
    out.F.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in block.parameters())
    assert float(context.grad[1, 4:].abs().max()) == 0.0 and float(context.grad[1, :4].abs().max()) > 0.0


def test_errors_come_before_any_launch(device, host_layer):
    x, batch = make_tensor((5, 4), device)
    x = ME.SparseTensor(torch.randn(9, 64, device=device), coordinate_map_key=x.coordinate_map_key,
                        coordinate_manager=x.coordinate_manager)
    m = ME.MinkowskiCrossAttention(64, 2).to(device)
    ctx = torch.randn(2, 6, 64, device=device)
    field = ME.TensorField(torch.randn(9, 64, device=device), coordinates=x.C.float())
    with pytest.raises(TypeError, match="TensorField"):
        m(field, ctx)
    with pytest.raises(TypeError, match="SparseTensor"):
        m(x.F, ctx)
    with pytest.raises(ValueError, match="instances, tokens"):
        m(x, ctx.reshape(12, 64))                                            # not 3-D
    with pytest.raises(ValueError, match="2 instances"):
        m(x, torch.randn(3, 6, 64, device=device))                           # a wrong B
    with pytest.raises(ValueError, match="dtype and device"):
        ME.MinkowskiFunctional.cross_attention(x, ctx.double(), ctx.double(), 2)
    with pytest.raises(ValueError, match="dtype and device"):
        ME.MinkowskiFunctional.cross_attention(x, ctx.cpu(), ctx.cpu(), 2)
    with pytest.raises(ValueError, match="head dimension"):
        ME.MinkowskiFunctional.cross_attention(x, ctx, ctx, 4)               # d = 16
    with pytest.raises(ValueError, match="context_lengths"):
        m(x, ctx, torch.tensor([6, 6, 6]))
    assert tuple(m(x, ctx, torch.tensor([6, 2])).F.shape) == (9, 64)
