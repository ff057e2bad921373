"""The batch-norm kernels (csrc/norm.hip) at the places where they could be wrong without tests/test_gpu_norm.py or
tests/test_gpu_sync_norm_kernels.py noticing, through backend.py's wrappers (bn_stats, bn_apply, bn_apply_residual,
bn_backward, bn_backward_residual, bn_local_moments, bn_backward_sums, bn_backward_apply) and, for the tile merge,
through the C ABI itself.  The reference throughout is torch.nn.BatchNorm1d in float64 on the CPU.

The five gaps and the tests that close them:

1. k_bn_final with tile_rows > 0 and more than kBnMaxChunks (512) tiles — second and third pass of the g0 loop, the row
   count of the partial last tile, lanes past the end clamped and masked: test_tile_merge, test_tile_merge_offset_rows,
   test_tile_merge_passes_agree_with_one_pass.
2. The chunk cap of bn_chunks — chunks == 512 with n % 512 != 0, chunk sizes q + extra, a thread walking more than one
   batch of rows: test_capped_chunks, test_backward_cap_alone, test_module_capped_chunks_on_both_host_layers.
3. More than 256 pieces per row (the p0 loop with R = 1) and the 64 KiB LDS limit of the batch-norm launchers:
   test_wide_rows, test_rows_past_the_lds_limit_are_refused.
4. The three piece widths (16 bytes, 4 channels, 1 channel) chosen from the channel count and from the pointers each
   wrapper looks at: test_piece_widths_and_unaligned_views.
5. Degenerate statistics — n = 1, n = 2, a constant column, a column whose M2 overflows fp32, one NaN / +inf in one
   channel: test_one_and_two_rows, test_constant_column, test_column_whose_m2_overflows,
   test_non_finite_value_stays_in_its_channel.

Bounds (the project's own): close(..., 1e-5) relative to 1 + max |ref| for mean, rstd, y and dx, 10 x that for the
parameter gradients, 2e-4 for rows offset by +300, bf16 outputs within 2^-8 |ref| + 1e-3 max |ref|.  Bit-identity and
guard checks take no tolerance.

The ReLU-fused and residual forms are checked in two steps.  Forward: the fused output equals, bit for bit, torch's
relu / addition applied to the plain output (the kernels' stated contract); the plain output is what is compared with
float64.  Backward: float64 batch-norm backward of the masked gradient; the mask of the ReLU-fused form is the
reference's own (y > 0 in float64), that of the residual form is the stored output's, which is what the kernel reads."""
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
F32, BF16 = torch.float32, torch.bfloat16

_COMMON = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "minkowskiengine_amd", "csrc",
                            "norm_common.hpp")).read()
K_MAX_CHUNKS = int(re.search(r"constexpr int kBnMaxChunks = (\d+);", _COMMON).group(1))
K_ROWS_PER_THREAD = int(re.search(r"constexpr int kBnRowsPerThread = (\d+);", _COMMON).group(1))
K_LDS_LIMIT = 64 * 1024


def geometry(dtype, c, aligned=True):
    """(V, P, R) of the partial kernels' launch (bn_partials / bn_backward_width in norm.hip)"""
    w = 4 if dtype == F32 else 8
    v = w if (aligned and c % w == 0) else (4 if (aligned and c % 4 == 0) else 1)
    p = c // v
    return v, p, (1 if p >= 256 else 256 // p)


def lds_bytes(c, r):
    return (r * 2 * c + 2 * c + 256 + c) * 4          # bn_partial_lds_bytes


def close(a, b, tol=1e-5):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


def within_bf16(got, ref):
    err = (got.double().cpu() - ref).abs()
    return bool((err <= 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().max()).all())


def _inputs(n, c, offset=0.0, dtype=F32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + n + c)
    x = ((torch.randn(n, c, generator=g) * (1.0 + torch.arange(c) % 5) * scale) + offset).to(dtype)
    gy = torch.randn(n, c, generator=g).to(dtype)
    skip = torch.randn(n, c, generator=g).to(dtype)
    w, b = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    return x, gy, skip, w, b


def _reference(x64, w, b, gy64):
    bn = torch.nn.BatchNorm1d(x64.shape[1], eps=EPS, momentum=MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(w.double())
        bn.bias.copy_(b.double())
    x = x64.clone().requires_grad_(True)
    y = bn(x)
    y.backward(gy64)
    mean = x64.mean(0)
    rstd = torch.rsqrt(x64.var(0, unbiased=False) + EPS)
    return dict(mean=mean, rstd=rstd, y=y.detach(), dx=x.grad, dw=bn.weight.grad, db=bn.bias.grad,
                rm=bn.running_mean, rv=bn.running_var)


class _GuardedTorch:
    """Stands in for the `torch` name inside backend.py while a wrapper runs: every tensor the wrapper allocates (outputs,
    statistics, workspace) is the middle of a larger buffer filled with a sentinel, PAD elements in front of and behind
    it (a multiple of 16 bytes in every dtype: the alignment the wrapper sees is the allocator's).  Everything else is
    torch's.  The wrapper itself runs unchanged."""
    PAD, SENTINEL = 512, 7

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        numel = math.prod(int(s) for s in size)
        buf = torch.full((numel + 2 * self.PAD,), self.SENTINEL, dtype=dtype, device=device)
        self.bufs.append((buf, numel))
        return buf[self.PAD:self.PAD + numel].view(tuple(size))

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def guards_intact(self):
        return all(bool((b[:self.PAD] == self.SENTINEL).all()) and bool((b[self.PAD + n:] == self.SENTINEL).all())
                   for b, n in self.bufs)

    def untouched(self):
        return all(bool((b == self.SENTINEL).all()) for b, _ in self.bufs)


def _guarded(numel, dtype, device, fill):
    """(buffer, view of `numel` elements set to `fill` in its middle) for outputs this file hands to the C ABI itself"""
    pad = _GuardedTorch.PAD
    buf = torch.full((numel + 2 * pad,), _GuardedTorch.SENTINEL, dtype=dtype, device=device)
    buf[pad:pad + numel] = fill
    return buf, buf[pad:pad + numel]


def _guards_of(buf, numel):
    pad = _GuardedTorch.PAD
    return bool((buf[:pad] == _GuardedTorch.SENTINEL).all()) and bool((buf[pad + numel:] == _GuardedTorch.SENTINEL).all())


def _run_all(x, gy, skip, w, b):
    """every wrapper once on device tensors (x, gy and skip may be views) -> all results"""
    from minkowskiengine_amd import backend as MEB
    dev, c, n = x.device, x.shape[1], x.shape[0]
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    mean, rstd = MEB.bn_stats(x, EPS, MOMENTUM, rm, rv, nbt)
    r = dict(mean=mean, rstd=rstd, rm=rm, rv=rv, nbt=nbt)
    r["record"] = MEB.bn_local_moments(x)
    r["y"] = MEB.bn_apply(x, mean, rstd, w, b, False)
    r["y_relu"] = MEB.bn_apply(x, mean, rstd, w, b, True)
    r["y_res"] = MEB.bn_apply_residual(x, skip, mean, rstd, w, b, True)
    r["dx"], r["dw"], r["db"] = MEB.bn_backward(x, gy, mean, rstd, w, b, False)
    r["dx_relu"], r["dw_relu"], r["db_relu"] = MEB.bn_backward(x, gy, mean, rstd, w, b, True)
    r["dx_res"], r["dskip"], r["dw_res"], r["db_res"] = MEB.bn_backward_residual(x, gy, r["y_res"], mean, rstd, w, b, True)
    r["sums"] = MEB.bn_backward_sums(x, gy, mean, rstd, w, b, False)
    r["dx_two"], _ = MEB.bn_backward_apply(x, gy, n, mean, rstd, w, b, r["sums"], False)
    r["sums_res"] = MEB.bn_backward_sums(x, gy, mean, rstd, w, b, True, r["y_res"])
    r["dx_res_two"], r["dskip_two"] = MEB.bn_backward_apply(x, gy, n, mean, rstd, w, b, r["sums_res"], True, r["y_res"],
                                                            need_dskip=True)
    return r


def _assert_all(got, x, gy, skip, w, b, tol=1e-5):
    """`got` of _run_all against float64 (x, gy, skip: the CPU tensors in the kernels' dtype)"""
    bf16 = x.dtype == BF16
    n, c = x.shape
    x64, gy64 = x.double(), gy.double()
    ref = _reference(x64, w, b, gy64)
    near = (lambda a, r_: within_bf16(a, r_)) if bf16 else (lambda a, r_: close(a, r_, tol))
    assert got["y"].dtype == x.dtype and got["dx"].dtype == x.dtype and got["dw"].dtype == F32
    assert close(got["mean"], ref["mean"], tol) and close(got["rstd"], ref["rstd"], tol)
    assert close(got["rm"], ref["rm"], tol) and close(got["rv"], ref["rv"], 10 * tol) and int(got["nbt"]) == 1
    # the record of synchronised batch norm is the same merge: count, the mean's bits, M2 = n * biased variance
    rec = got["record"]
    assert int(rec[:2].contiguous().view(torch.int64)) == n
    assert torch.equal(rec[2:2 + c], got["mean"])
    assert close(rec[2 + c:] / n, x64.var(0, unbiased=False), tol)
    assert near(got["y"], ref["y"]) and near(got["dx"], ref["dx"])
    assert close(got["dw"], ref["dw"], 10 * tol) and close(got["db"], ref["db"], 10 * tol)
    # the two halves of the backward pass are the one-call form's kernels
    assert torch.equal(got["sums"][0], got["db"]) and torch.equal(got["sums"][1], got["dw"])
    assert torch.equal(got["dx_two"], got["dx"])
    # fused ReLU: forward bits, backward against float64 with the reference's mask
    assert torch.equal(got["y_relu"], torch.relu(got["y"]))
    ref_relu = _reference(x64, w, b, gy64 * (ref["y"] > 0))
    assert near(got["dx_relu"], ref_relu["dx"])
    assert close(got["dw_relu"], ref_relu["dw"], 10 * tol) and close(got["db_relu"], ref_relu["db"], 10 * tol)
    # residual form: forward bits, backward against float64 with the stored output's mask
    assert torch.equal(got["y_res"], torch.relu(got["y"] + skip.to(got["y"].device)))
    if not bf16:
        assert close(got["y_res"], torch.relu(ref["y"] + skip.double()), tol)
    mask = (got["y_res"] > 0).cpu()
    assert 0.2 < float(mask.double().mean()) < 0.8                      # the ReLU does mask something
    assert torch.equal(got["dskip"].cpu(), gy * mask)
    ref_res = _reference(x64, w, b, gy64 * mask)
    assert near(got["dx_res"], ref_res["dx"])
    assert close(got["dw_res"], ref_res["dw"], 10 * tol) and close(got["db_res"], ref_res["db"], 10 * tol)
    assert torch.equal(got["sums_res"][0], got["db_res"]) and torch.equal(got["sums_res"][1], got["dw_res"])
    assert torch.equal(got["dx_res_two"], got["dx_res"]) and torch.equal(got["dskip_two"], got["dskip"])


def _case(device, n, c, dtype, tol=1e-5, offset=0.0, repeat=False, seed=0):
    x, gy, skip, w, b = _inputs(n, c, offset, dtype, seed)
    dev = [t.to(device) for t in (x, gy, skip, w, b)]
    got = _run_all(*dev)
    _assert_all(got, x, gy, skip, w, b, tol)
    if repeat:
        again = _run_all(*dev)
        assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"
    return got


# ---- A. tile merge: me_bn_stats_from_tiles ---------------------------------------------------------------------------
TILE_ROWS = 3


def _tile_partials(x64, tile_rows):
    """(mean, M2) of rows [g * tile_rows, min((g + 1) * tile_rows, n)) per tile g, float64 rounded to fp32"""
    n, c = x64.shape
    full = n // tile_rows
    body = x64[:full * tile_rows].view(full, tile_rows, c)
    pm = body.mean(1)
    pq = ((body - pm[:, None]) ** 2).sum(1)
    if n % tile_rows:
        tail = x64[full * tile_rows:]
        pm = torch.cat([pm, tail.mean(0, keepdim=True)])
        pq = torch.cat([pq, ((tail - tail.mean(0)) ** 2).sum(0, keepdim=True)])
    return pm.float().contiguous(), pq.float().contiguous()


def _from_tiles(device, pm, pq, n, c, tile_rows, calls=1):
    """-> mean, rstd, running_mean, running_var, num_batches_tracked after `calls` calls on fresh running statistics;
    every output lies between guard elements"""
    from minkowskiengine_amd import _lib
    lib = _lib.load()
    pm, pq = pm.to(device), pq.to(device)
    outs = [_guarded(c, F32, device, fill) for fill in (-3.0, -3.0, 0.0, 1.0)]
    nbt_buf, nbt = _guarded(1, torch.int64, device, 0)
    (_, mean), (_, rstd), (_, rm), (_, rv) = outs
    for i in range(calls):
        if i:                                   # the running statistics start over: the calls are to be identical
            rm.fill_(0.0)
            rv.fill_(1.0)
        _lib.check(lib.me_bn_stats_from_tiles(pm.data_ptr(), pq.data_ptr(), n, c, tile_rows, EPS, MOMENTUM,
                                              mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                              nbt.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    torch.cuda.synchronize()
    assert all(_guards_of(buf, c) for buf, _ in outs) and _guards_of(nbt_buf, 1), "the merge wrote outside its outputs"
    return dict(mean=mean.clone(), rstd=rstd.clone(), rm=rm.clone(), rv=rv.clone(), nbt=int(nbt))


def _assert_stats(got, ref, tol):
    assert close(got["mean"], ref["mean"], tol) and close(got["rstd"], ref["rstd"], tol)
    assert close(got["rm"], ref["rm"], tol) and close(got["rv"], ref["rv"], 10 * tol)


@pytest.mark.parametrize("c", [1, 4, 5, 96])                       # 5: the last block of four channel waves is partly idle
@pytest.mark.parametrize("tiles", [1, 2, 511, 512, 513, 1024, 1025, 1100])
def test_tile_merge(device, tiles, c):
    """gap 1: tiles of 3 rows with a partial last tile (n = 3 tiles - 1), up to three passes of the g0 loop"""
    n = TILE_ROWS * tiles - 1
    x = _inputs(n, c, seed=3)[0]
    pm, pq = _tile_partials(x.double(), TILE_ROWS)
    assert pm.shape == (tiles, c)
    ref = _reference(x.double(), torch.ones(c), torch.zeros(c), torch.zeros(n, c).double())
    got = _from_tiles(device, pm, pq, n, c, TILE_ROWS)
    _assert_stats(got, ref, 1e-5)
    assert got["nbt"] == 1
    twice = _from_tiles(device, pm, pq, n, c, TILE_ROWS, calls=2)
    assert twice["nbt"] == 2
    assert all(torch.equal(got[k], twice[k]) for k in ("mean", "rstd", "rm", "rv")), "two calls differ"


def test_tile_merge_offset_rows(device):
    """gap 1 with |mean| >> std (rows offset by +300): the shift is tile 0's mean in every pass; 2e-4 is the project's
    bound for this input (tests/test_gpu_norm.py)"""
    tiles, c = 1100, 96
    n = TILE_ROWS * tiles - 1
    x = _inputs(n, c, offset=300.0, seed=4)[0]
    pm, pq = _tile_partials(x.double(), TILE_ROWS)
    ref = _reference(x.double(), torch.ones(c), torch.zeros(c), torch.zeros(n, c).double())
    _assert_stats(_from_tiles(device, pm, pq, n, c, TILE_ROWS), ref, 2e-4)


@pytest.mark.parametrize("c", [5, 96])
def test_tile_merge_passes_agree_with_one_pass(device, c):
    """gap 1, the multi-pass loop alone: 513 tiles of 3 rows (two passes) against the same matrix cut into 257 tiles of 6
    rows (one pass)"""
    n = TILE_ROWS * 513 - 1
    x64 = _inputs(n, c, seed=5)[0].double()
    two = _from_tiles(device, *_tile_partials(x64, TILE_ROWS), n, c, TILE_ROWS)
    pm6, pq6 = _tile_partials(x64, 2 * TILE_ROWS)
    assert pm6.shape[0] == 257
    one = _from_tiles(device, pm6, pq6, n, c, 2 * TILE_ROWS)
    _assert_stats(two, one, 1e-5)


# ---- B. capped chunks -------------------------------------------------------------------------------------------------
# (dtype, c, rows above the forward cap kBnMaxChunks * R * kBnRowsPerThread): with the constants 512 and 8 these are
# n = 4200, 8300, 4200 and 512 * 256 * 8 + 77
CAPPED = [(F32, 1024, 104), (F32, 512, 108), (BF16, 2048, 104), (F32, 4, 77)]


@pytest.mark.parametrize("dtype,c,above", CAPPED, ids=lambda v: str(v).replace("torch.", ""))
def test_capped_chunks(device, dtype, c, above):
    """gap 2: the smallest row counts above the cap with n % 512 != 0 — 512 chunks of q and q + 1 rows (`extra` of
    k_bn_final), a second batch of rows per thread in the forward and the backward partial kernels"""
    r = geometry(dtype, c)[2]
    n = K_MAX_CHUNKS * r * K_ROWS_PER_THREAD + above
    assert n % K_MAX_CHUNKS != 0 and math.ceil(n / (r * K_ROWS_PER_THREAD)) > K_MAX_CHUNKS
    _case(device, n, c, dtype, repeat=True)


def test_backward_cap_alone(device):
    """gap 2: the backward partial kernel keeps half as many rows in flight, so its cap is lower: n = 2100 at c = 1024 has
    263 forward chunks and 512 backward chunks of 4 and 5 rows"""
    c, r = 1024, geometry(F32, 1024)[2]
    n = K_MAX_CHUNKS * r * (K_ROWS_PER_THREAD // 2) + 52
    assert n % K_MAX_CHUNKS != 0 and math.ceil(n / (r * K_ROWS_PER_THREAD)) < K_MAX_CHUNKS
    _case(device, n, c, F32, repeat=True)


def test_module_capped_chunks_on_both_host_layers(device, host_layer):
    """gap 2 through MinkowskiBatchNorm on the ctypes twin and the native host layer (which has its own call sites)"""
    import minkowskiengine_amd as ME
    from helpers import make_cloud
    c = 1024
    n = K_MAX_CHUNKS * geometry(F32, c)[2] * K_ROWS_PER_THREAD + 104
    coords = make_cloud(n, 40, 3, seed=1)
    x, gy, _, w, b = _inputs(n, c, seed=6)
    ref = _reference(x.double(), w, b, gy.double())
    bn = ME.MinkowskiBatchNorm(c, eps=EPS, momentum=MOMENTUM).to(device)
    with torch.no_grad():
        bn.bn.weight.copy_(w)
        bn.bn.bias.copy_(b)
    f = x.to(device).requires_grad_(True)
    y = bn(ME.SparseTensor(f, coords.to(device)))
    y.F.backward(gy.to(device))
    assert close(y.F.detach(), ref["y"]) and close(f.grad, ref["dx"])
    assert close(bn.bn.weight.grad, ref["dw"], 1e-4) and close(bn.bn.bias.grad, ref["db"], 1e-4)
    assert close(bn.bn.running_mean, ref["rm"]) and close(bn.bn.running_var, ref["rv"], 1e-4)


# ---- C. wide rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,v,p", [(F32, 1028, 4, 257),      # second p0 pass with one active thread
                                         (F32, 3224, 4, 806),      # four-channel pieces at the edge of the LDS limit
                                         (F32, 3225, 1, 3225),     # one-channel pieces, the last 12 bytes short of 64 KiB
                                         (BF16, 3225, 1, 3225),
                                         (BF16, 2056, 8, 257)], ids=lambda v: str(v).replace("torch.", ""))
def test_wide_rows(device, dtype, c, v, p):
    """gap 3: more than 256 pieces per row — the p0 loop of the partial kernels and the piece loop of the apply kernels
    with one row lane — up to the widest row whose sums fit into 64 KiB of LDS"""
    assert geometry(dtype, c) == (v, p, 1) and lds_bytes(c, 1) <= K_LDS_LIMIT
    if c == 3225:
        assert lds_bytes(c + 1, 1) > K_LDS_LIMIT           # the widest row that fits
    _case(device, 301, c, dtype, repeat=True)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_rows_past_the_lds_limit_are_refused(device, monkeypatch, dtype):
    """gap 3: c = 3226 needs more than 64 KiB: every entry point that sizes LDS by c returns the library's error, and
    neither the running statistics handed in nor anything the wrapper had allocated for the call is written.  Only the
    refusal is asserted."""
    from minkowskiengine_amd import backend as MEB
    c, n = 3226, 40
    assert lds_bytes(c, geometry(dtype, c)[2]) > K_LDS_LIMIT
    x, gy, skip, w, b = [t.to(device) for t in _inputs(n, c, dtype=dtype)]
    mean, rstd = torch.zeros(c, device=device), torch.ones(c, device=device)
    rm, rv = torch.full((c,), 0.25, device=device), torch.full((c,), 2.0, device=device)
    nbt = torch.full((), 7, dtype=torch.int64, device=device)
    alloc = _GuardedTorch()
    monkeypatch.setattr(MEB, "torch", alloc)
    calls = [lambda: MEB.bn_stats(x, EPS, MOMENTUM, rm, rv, nbt),
             lambda: MEB.bn_local_moments(x),
             lambda: MEB.bn_backward(x, gy, mean, rstd, w, b, False),
             lambda: MEB.bn_backward(x, gy, mean, rstd, w, b, True),
             lambda: MEB.bn_backward_residual(x, gy, skip, mean, rstd, w, b, True),
             lambda: MEB.bn_backward_sums(x, gy, mean, rstd, w, b, False),
             lambda: MEB.bn_backward_sums(x, gy, mean, rstd, w, b, True, skip)]
    for call in calls:
        with pytest.raises(RuntimeError, match="channel count too large"):
            call()
    torch.cuda.synchronize()
    assert len(alloc.bufs) >= 2 * len(calls) and alloc.untouched(), "a refused call wrote to its outputs"
    assert bool((rm == 0.25).all()) and bool((rv == 2.0).all()) and int(nbt) == 7


# ---- D. piece widths and alignment ------------------------------------------------------------------------------------
def _tight_view(t, device):
    """a copy of `t` that starts one element into its storage and ends exactly at the storage's end"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert view.data_ptr() + view.numel() * view.element_size() == base.data_ptr() + base.numel() * base.element_size()
    return view


WIDTH_CASES = [(F32, 96, 4), (F32, 20, 4), (F32, 7, 1), (BF16, 96, 8), (BF16, 12, 4), (BF16, 7, 1)]


@pytest.mark.parametrize("unaligned", ["none", "x", "dy", "skip", "all"])
@pytest.mark.parametrize("dtype,c,v", WIDTH_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_piece_widths_and_unaligned_views(device, monkeypatch, dtype, c, v, unaligned):
    """gap 4: one channel count per piece width, on tensors from the allocator and on views that start one element into
    their storage and end at its end — x, dy, skip, each alone and all three.  The wrappers accept such a view as it is
    (it is contiguous; they neither copy nor refuse it) and the launchers fall back to one-channel pieces for every
    kernel that is handed the unaligned pointer: bn_stats / bn_local_moments look at x, bn_apply at x, y and skip, the
    backward at x, dy, dx, the stored output and dskip.  Every tensor the wrappers allocate lies between guard elements."""
    from minkowskiengine_amd import backend as MEB
    n = 1001
    assert geometry(dtype, c)[0] == v and geometry(dtype, c, aligned=False)[0] == 1
    x, gy, skip, w, b = _inputs(n, c, dtype=dtype, seed=8)
    place = lambda t, name: _tight_view(t, device) if unaligned in (name, "all") else t.to(device)
    dev = [place(x, "x"), place(gy, "dy"), place(skip, "skip"), w.to(device), b.to(device)]
    for t, name in zip(dev[:3], ("x", "dy", "skip")):
        assert (t.data_ptr() % 16 != 0) == (unaligned in (name, "all"))
    alloc = _GuardedTorch()
    monkeypatch.setattr(MEB, "torch", alloc)
    got = _run_all(*dev)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(alloc.bufs) > 20 and alloc.guards_intact(), "a kernel wrote outside a tensor its wrapper allocated"
    _assert_all(got, x, gy, skip, w, b)


# ---- E. degenerate and non-finite -------------------------------------------------------------------------------------
RSQRT_EPS_TOL = 2.0 ** -21      # rstd of an exactly zero variance: eps rounded to fp32 (2^-25 of rstd) and a reciprocal
                                # square root within two units in the last place (2^-22)


@pytest.mark.parametrize("dtype,c,v", WIDTH_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_one_and_two_rows(device, dtype, c, v):
    """gap 5: n = 2 against BatchNorm1d; n = 1, which BatchNorm1d refuses in training mode, against the formulas: mean =
    the row, variance 0, y = beta, dx = 0, grad_gamma = 0, grad_beta = dy, and running_var takes the biased variance
    (k_bn_final's convention where n - 1 = 0).
    With one row every reference output but grad_beta is 0 or beta while the kernels' terms are of the size of a = gamma /
    sqrt(eps) <= 475: the apply kernel evaluates x * a + (beta - mean * a), the backward dy * a - (sum dy / n) * a, and
    each rounds one such term, an error of 2^-24 a |x| and 2^-24 a |dy|.  The row stays within |x| <= 0.5 and |dy| <= 0.25
    so that this is at most 7.6e-6, inside the 1e-5 bound; it grows with the values beyond it.
    With two rows dx is itself a cancellation residue of order eps / var, far below one fp32 rounding of its terms: bf16
    rows get the fp32 bound on top of the bf16 bound there (the output carries the fp32 arithmetic and one bf16 rounding)."""
    from minkowskiengine_amd import backend as MEB
    g = torch.Generator().manual_seed(c)
    w, b = (torch.rand(c, generator=g) + 0.5).to(device), (torch.rand(c, generator=g) - 0.5).to(device)
    # n = 2: the two rows differ by 1 .. 3 in every channel (rstd <= 2)
    x0 = torch.rand(1, c, generator=g) - 0.5
    x2 = torch.cat([x0, x0 + 1.0 + torch.arange(c) % 3]).to(dtype)
    gy2 = torch.randn(2, c, generator=g).to(dtype)
    ref = _reference(x2.double(), w.cpu(), b.cpu(), gy2.double())
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    mean, rstd = MEB.bn_stats(x2.to(device), EPS, MOMENTUM, rm, rv)
    y = MEB.bn_apply(x2.to(device), mean, rstd, w, b)
    dx, dw, db = MEB.bn_backward(x2.to(device), gy2.to(device), mean, rstd, w, b)
    assert close(mean, ref["mean"]) and close(rstd, ref["rstd"]) and close(rm, ref["rm"]) and close(rv, ref["rv"], 1e-4)
    assert close(dw, ref["dw"], 1e-4) and close(db, ref["db"], 1e-4)
    if dtype == BF16:
        assert within_bf16(y, ref["y"])
        err = (dx.double().cpu() - ref["dx"]).abs()
        top = float(ref["dx"].abs().max())
        assert bool((err <= 2.0 ** -8 * ref["dx"].abs() + 1e-3 * top + 1e-5 * (1.0 + top)).all())
    else:
        assert close(y, ref["y"]) and close(dx, ref["dx"])
    # n = 1
    x1 = (torch.rand(1, c, generator=g) - 0.5).to(dtype)
    gy1 = ((torch.rand(1, c, generator=g) - 0.5) * 0.5).to(dtype)
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    mean, rstd = MEB.bn_stats(x1.to(device), EPS, MOMENTUM, rm, rv)
    y = MEB.bn_apply(x1.to(device), mean, rstd, w, b)
    dx, dw, db = MEB.bn_backward(x1.to(device), gy1.to(device), mean, rstd, w, b)
    assert torch.equal(mean.cpu(), x1[0].float())
    assert float((rstd.double().cpu() * math.sqrt(EPS) - 1.0).abs().max()) <= RSQRT_EPS_TOL
    assert close(rm, MOMENTUM * x1[0].double()) and close(rv, torch.full((c,), 1.0 - MOMENTUM, dtype=torch.float64))
    beta = b.double().cpu()[None, :]
    assert within_bf16(y, beta) if dtype == BF16 else close(y, beta)
    assert close(dx, torch.zeros(1, c, dtype=torch.float64))
    assert bool((dw == 0).all()) and torch.equal(db.cpu(), gy1[0].float())
    rec = MEB.bn_local_moments(x1.to(device))
    assert int(rec[:2].contiguous().view(torch.int64)) == 1 and torch.equal(rec[2:2 + c], mean) and not bool(rec[2 + c:].any())


@pytest.mark.parametrize("dtype,c,v", WIDTH_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_constant_column(device, dtype, c, v):
    """gap 5: a column of one value (0.5; the bound on |mean| of test_one_and_two_rows applies) among ordinary ones, over
    several chunks: its M2 is exactly 0 in every chunk and in the merge, so mean is the value itself, rstd is rsqrt(eps)
    to the rounding of eps and of the reciprocal square root (RSQRT_EPS_TOL), and dx is finite and matches float64 like
    every other column"""
    n, col = 1001, c - 2
    x, gy, skip, w, b = _inputs(n, c, dtype=dtype, seed=9)
    x[:, col] = 0.5
    got = _run_all(*[t.to(device) for t in (x, gy, skip, w, b)])
    assert float(got["mean"][col]) == 0.5 and float(got["record"][2 + c + col]) == 0.0
    assert abs(float(got["rstd"][col]) * math.sqrt(EPS) - 1.0) <= RSQRT_EPS_TOL
    assert bool(torch.isfinite(got["dx"].float()).all()) and bool(torch.isfinite(got["dx_res"].float()).all())
    _assert_all(got, x, gy, skip, w, b)


def test_column_whose_m2_overflows(device):
    """gap 5: a column of +-1e18 whose sum of squared deviations, 7.2e38 in float64, is +inf once rounded to fp32 (the
    format M2 is kept in).  Pinned to what follows from that rounded M2: the record's M2 is +inf, the variance is +inf,
    rstd = rsqrt(inf) = 0, running_var = +inf; the mean is finite and matches float64; y = beta and dx = 0 in that column
    (x * 0), grad_gamma = 0, grad_beta = sum dy.  Every other column has the bits of a run in which that column is
    ordinary.  One row in ten is -1e18 and row 0 is +1e18, so that of the two terms of M2 = B - A^2 / n only B
    overflows: with both infinite their difference is NaN, which is not what this case is about."""
    n, c, col = 2000, 4, 1
    x, gy, skip, w, b = _inputs(n, c, seed=10)
    big = x.clone()
    big[:, col] = torch.where(torch.arange(n) % 10 == 5, -1e18, 1e18)
    m2 = float(((big[:, col].double() - big[:, col].double().mean()) ** 2).sum())
    assert m2 > 3.5e38 and math.isinf(float(torch.tensor(m2).float()))
    plain = _run_all(*[t.to(device) for t in (x, gy, skip, w, b)])
    got = _run_all(*[t.to(device) for t in (big, gy, skip, w, b)])
    others = [j for j in range(c) if j != col]
    for k in ("mean", "rstd", "rm", "rv", "y", "y_relu", "y_res", "dx", "dw", "db", "dx_relu", "dx_res", "dskip"):
        assert torch.equal(got[k][..., others], plain[k][..., others]), k
    ref_mean = big[:, col].double().mean()
    assert abs(float(got["mean"][col]) - float(ref_mean)) <= 1e-5 * float(ref_mean)
    assert abs(float(got["rm"][col]) - MOMENTUM * float(ref_mean)) <= 1e-5 * float(ref_mean)
    assert float(got["record"][2 + c + col]) == math.inf and float(got["rv"][col]) == math.inf
    assert float(got["rstd"][col]) == 0.0
    assert bool((got["y"][:, col] == b[col].to(device)).all())
    assert bool((got["dx"][:, col] == 0).all()) and float(got["dw"][col]) == 0.0
    assert torch.equal(got["db"], plain["db"])


@pytest.mark.parametrize("bad", [math.nan, math.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype,c,v", WIDTH_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_non_finite_value_stays_in_its_channel(device, dtype, c, v, bad):
    """gap 5: one NaN / +inf in one channel, at a row of chunk 0 and at a row of the last chunk (all loads are
    unconditional and masked by multiplication).  As in float64, that channel's rstd is NaN (inf - inf for +inf), its
    mean and running statistics are not finite, y, dx and grad_gamma are NaN in every row — also behind the fused ReLU
    and the residual addition, where relu(NaN) is NaN and the gradient of the residual branch is 0; grad_beta is sum dy,
    which does not depend on x.  Every other channel has the bits of the run without the bad value, in all three forms."""
    n, col = 2001, c // 2
    x, gy, skip, w, b = _inputs(n, c, dtype=dtype, seed=11)
    _, _, r = geometry(dtype, c)
    assert n > 2 * r * K_ROWS_PER_THREAD                                # several chunks
    clean = _run_all(*[t.to(device) for t in (x, gy, skip, w, b)])
    others = [j for j in range(c) if j != col]
    for row in (3, n - 2):
        xb = x.clone()
        xb[row, col] = bad
        ref = _reference(xb.double(), w, b, gy.double())
        assert bool(ref["rstd"][col].isnan()) and bool(ref["y"][:, col].isnan().all()) and bool(ref["dx"][:, col].isnan().all())
        assert bool(ref["dw"][col].isnan()) and bool(ref["db"][col].isfinite()) and bool(ref["rv"][col].isnan())
        got = _run_all(*[t.to(device) for t in (xb, gy, skip, w, b)])
        for k in got:
            if k in ("nbt", "record"):
                continue
            assert torch.equal(got[k][..., others], clean[k][..., others]), (k, row)
        rec, rec0 = got["record"], clean["record"]
        keep = torch.ones(rec.numel(), dtype=torch.bool)
        keep[2 + col] = keep[2 + c + col] = False
        assert torch.equal(rec[keep], rec0[keep]), row
        assert bool(got["rstd"][col].isnan()) and bool(got["rv"][col].isnan()) and bool(rec[2 + c + col].isnan()), row
        assert not bool(got["mean"][col].isfinite()) and not bool(got["rm"][col].isfinite()), row
        assert bool(got["y"][:, col].isnan().all()) and bool(got["dx"][:, col].isnan().all()), row
        # the fused forms: relu(NaN) is NaN, no gradient passes a NaN output, dx is NaN through the statistics
        assert bool(got["y_relu"][:, col].isnan().all()) and bool(got["y_res"][:, col].isnan().all()), row
        assert bool(got["dx_relu"][:, col].isnan().all()) and bool(got["dx_res"][:, col].isnan().all()), row
        assert bool((got["dskip"][:, col] == 0).all()), row
        assert bool(got["dw"][col].isnan()) and torch.equal(got["db"], clean["db"]), row
