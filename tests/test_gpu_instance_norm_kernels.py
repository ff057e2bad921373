"""Entry-point tests of the instance-norm kernels (csrc/instance_norm.hip and the shared csrc/norm_common.hpp) through the
C ABI: me_inorm_workspace_bytes / me_inorm_stats / me_inorm_apply / me_inorm_backward and the float64 twins, on tensors
of the test's own.  The module tests (test_gpu_instance_norm.py) reach these kernels only with sorted batches of 2 - 4
instances and c <= 64; here `batch_row` and `n_batch` are chosen freely, so a chunk mixes many batch indices, instances
have no rows at all, the 512-chunk cap is reached, rows are wider than one pass of 256 threads and views are unaligned.

Expectation: one plain float64 restatement on the CPU (`reference`), segmented by batch_row; rstd = 1 / sqrt(biased
variance + eps); an instance without rows has mean 0, rstd 1 / sqrt(eps) and adds nothing to the parameter gradients.
For bf16 the formula is applied to the bf16-rounded inputs.  No expected value comes from a kernel.

Bounds (none measured from the kernels).  fp32 mean / rstd / out / dx / grad_gamma / grad_beta: helpers.assert_close at
its defaults, 1e-4 + 1e-4 |b| per element.  bf16 out / dx: 1e-4 + 2^-8 |b| (one round-to-nearest to an 8-bit significand
at the store, derived in test_gpu_instance_norm.py); bf16 statistics and parameter gradients: the fp32 bar (fp32 sums of
exactly widened bf16 values).  float64: 1e-10 absolute.

Inputs: x = per-(instance, channel) offset uniform in [-4, 4] + 0.3 randn, dy uniform in [-0.5, 0.5], gamma in
[0.5, 1.5], beta in [-0.5, 0.5], fixed seeds, built on the CPU by cached builders.  One addition: the rows of an instance
of fewer than 16 rows also get +1 / -1 (times spread / 0.3) alternating by their rank within the instance.  Two or three Gaussian rows are
arbitrarily close together with a probability that the hundreds of (instance, channel) pairs of these tests do reach, and
there no fp32 computation can meet the bar: with the mean of a 2-row instance off by e (half an ulp of |x| <= 4.5,
2.4e-7) and the rows d apart, dx — analytically 0 — comes out as 2 e gamma (dy1 + dy2 + 2 (dy1 - dy2) / 2) / d^2, about
e / d^2, which passes 1e-4 below d = 0.05.  The alternating term keeps d near 2.  Two more departures, both because the
naive float32 restatement below did not stay within half the bar otherwise: matrices of 2000 rows or more (the capped
shapes cannot have fewer) use a spread of 3.0 instead of 0.3 — an error e of a mean reaches grad_gamma as
e rstd |sum dy|, which grows with the rows and shrinks with the spread — and the constant-instance cases pass
eps = 1e-5, so that rstd = 316 and not 1e4 multiplies the rounding of sum dy / n in dx.  The smaller matrices keep the
spread of 0.3, channel means up to 13 spreads from zero.  tests/test_instance_norm_inputs_cpu.py
checks without a GPU that a naive two-pass float32 restatement in row order — less accurate than the kernels — stays within
HALF the bar of the float64 reference for every fp32 case here, so a failure on the GPU is the kernel's; it also checks
the piece widths, row lanes, chunk counts and reduce branches that the case tables below claim.

Before every stats / backward call the workspace, allocated at exactly me_inorm_workspace_bytes, is filled with 0xFF
bytes (a NaN in every float slot): a result that depends on a partial that was never written comes out as NaN."""
import functools
import itertools
import math
import zlib

import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
EPS = 1e-8                                  # MinkowskiInstanceNorm's eps
BF16_OUT = dict(atol=1e-4, rtol=2.0 ** -8)
SMALL_INSTANCE = 16                         # instances below this many rows get the alternating +-1 term
SPREAD, WIDE_SPREAD, WIDE_SPREAD_ROWS = 0.3, 3.0, 2000
CONST_EPS = 1e-5

# ---- the launch geometry, restated from csrc/instance_norm.hip (in_piece, in_stats, in_backward) and
# csrc/norm_common.hpp (bn_chunks, bn_reduce_lanes, bn_partial_lds_bytes) -----------------------------------------------
K_MAX_CHUNKS = 512
K_ROWS_PER_THREAD = 8
K_LDS_LIMIT = 64 * 1024


def piece(dtype, c, aligned=True):
    """in_piece: 16 bytes where every address is 16-byte aligned and c divides, else 4 elements, else 1"""
    w = 4 if dtype == "f32" else 8
    if aligned and c % w == 0:
        return w
    return 4 if aligned and c % 4 == 0 else 1


def geometry(dtype, c, n, aligned=True):
    """-> dict(V, P, R, chunk_rows, chunks, bwd_chunks, branch, G, lds) of the statistics / backward partial kernels"""
    v = piece(dtype, c, aligned)
    p = c // v
    r = 1 if p >= 256 else 256 // p
    chunks = lambda rows: min(max(-(-n // (r * rows)), 1), K_MAX_CHUNKS)          # noqa: E731
    nv = 2 * c
    grouped = nv * 2 <= 256
    return dict(V=v, P=p, R=r, chunk_rows=K_ROWS_PER_THREAD * r, chunks=chunks(K_ROWS_PER_THREAD),
                bwd_chunks=chunks(K_ROWS_PER_THREAD // 2), branch="grouped" if grouped else "direct",
                G=256 // nv if grouped else None, lds=(r * 2 * c + 2 * c + 256 + c) * 4)


def _several(dtype, c, chunks=5):
    return chunks * geometry(dtype, c, 1)["chunk_rows"] + 3


# (dtype, c, n, pattern); n is ignored by the patterns that set their own row count ("many300*")
def _edge_ns(c):
    r8 = geometry("f32", c, 1)["chunk_rows"]
    return [r8 - 1, r8, r8 + 1, 5 * r8 + 3]


SHAPE_CASES = (
    # grouped reduce, G = 128 / 42 / 32 / 10 / 2: one chunk less a row, one chunk, one chunk and a row, about 5 chunks
    [("f32", c, n, "sorted3") for c in (1, 3, 4, 12, 64) for n in _edge_ns(c)] +
    # direct reduce with R = 3 / 15 / 10 row lanes, none of which divides 256
    [("f32", c, _several("f32", c), "sorted3") for c in (65, 68, 96)] +
    [("f32", 1024, 40, "sorted3"),              # P = 256: R = 1, 5 chunks of 8 rows
     ("f32", 1024, 5000, "sorted3"),            # P = 256, 512 chunks forward and backward: 9 - 10 rows each
     ("f32", 257, 40, "sorted3"),               # P = 257, V = 1: the p0 loop / p += W loop
     ("f32", 1028, 40, "sorted3"),              # P = 257, V = 4
     ("bf16", 2056, 40, "sorted3"),             # P = 257, V = 8
     ("f32", 64, 70000, "sorted35")] +          # R = 16: the cap at 65 536 rows, 136 - 137 rows per chunk
    # bf16 piece widths: V = 4 (c % 8 != 0), V = 8, V = 1
    [("bf16", c, _several("bf16", c), "sorted3") for c in (4, 12, 8, 24, 64, 3)] +
    [("f32", 3224, 24, "sorted3"),              # the widest rows the LDS of the partial kernels holds: V = 4
     ("f32", 3225, 24, "sorted3"),              # and V = 1
     ("f32", 4, 1, "sorted3"), ("f32", 5, 1, "sorted3"), ("bf16", 4, 1, "sorted3"), ("bf16", 5, 1, "sorted3")])

PATTERNS = ("sorted3", "gapped", "rr3", "rr7", "perm3", "many300", "many300_shuffled", "one", "only37")
PATTERN_SHAPES = [("f32", 4, _several("f32", 4, 3)), ("f32", 12, _several("f32", 12, 3)), ("f32", 96, _several("f32", 96)),
                  ("bf16", 24, _several("bf16", 24, 3)), ("f32", 1024, 5000)]
PATTERN_CASES = [(d, c, n, p) for (d, c, n) in PATTERN_SHAPES for p in PATTERNS]
GAPPED_ABSENT = (0, 5, 8)
UNALIGNED_CASES = [("f32", 8, 3 * 1024 + 3, "gapped"), ("bf16", 16, 3 * 1024 + 3, "gapped")]
F64_CASES = [(c, n, p) for c in (3, 5) for (n, p) in ((1999, "sorted3"), (1500, "gapped"), (1000, "rr7"),
                                                      (0, "many300"), (0, "many300_shuffled"))]
CONST_VALUE, CONST_ROWS = 1000.25, 3000
CONST_CASES = [(c, layout) for c in (12, 96) for layout in ("sorted", "interleaved")]


def segments(pattern, n):
    """-> (batch_row int32 [n'], n_batch); every index in [0, n_batch)"""
    rng = np.random.default_rng(zlib.crc32(pattern.encode()) + n)
    if pattern.startswith("sorted"):                      # equal sizes: the boundaries fall inside chunks
        nb = int(pattern[6:])
        br = np.repeat(np.arange(nb), [len(a) for a in np.array_split(np.arange(n), nb)])
    elif pattern == "gapped":                             # absent at index 0, in the middle and at the end; 1-row ones
        big = (n - 7) // 2
        sizes = [0, 1, 2, big, 1, 0, n - 7 - big, 3, 0]
        assert big > 0
        nb, br = len(sizes), np.repeat(np.arange(len(sizes)), sizes)
    elif pattern in ("rr3", "rr7"):
        nb = int(pattern[2:])
        br = np.arange(n) % nb
    elif pattern == "perm3":
        nb = 3
        br = rng.permutation(segments("sorted3", n)[0])
    elif pattern in ("many300", "many300_shuffled"):      # 1 - 8 rows each: hundreds of indices in one chunk
        nb = 300
        br = np.repeat(np.arange(nb), np.random.default_rng(300).integers(1, 9, nb))
        if pattern.endswith("shuffled"):
            br = np.random.default_rng(301).permutation(br)
    elif pattern == "one":
        nb, br = 1, np.zeros(n)
    elif pattern == "only37":
        nb, br = 64, np.full(n, 37)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(br, dtype=np.int32), nb


def _segment_index(br, nb):
    """rows in instance order (stable), first row of every instance in that order, rows per instance"""
    order = np.argsort(br, kind="stable")
    cnt = np.bincount(br, minlength=nb)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    return order, starts, cnt


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def make_inputs(dtype, c, br, nb, seed, const_instance=None, spread=SPREAD):
    """the project's instance-norm input construction -> dict of read-only float32 arrays (bf16: already rounded)"""
    n = len(br)
    rng = np.random.default_rng([seed, c, n])
    offset = rng.uniform(-4, 4, (nb, c))
    x = offset[br] + spread * rng.standard_normal((n, c))
    order, starts, cnt = _segment_index(br, nb)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - starts[br[order]]
    small = cnt[br] < SMALL_INSTANCE
    x[small] += np.where(rank[small] % 2 == 0, 1.0, -1.0)[:, None] * (spread / SPREAD)
    if const_instance is not None:
        x[br == const_instance] = CONST_VALUE
    out = dict(x=x.astype(np.float32), dy=rng.uniform(-0.5, 0.5, (n, c)).astype(np.float32),
               gamma=rng.uniform(0.5, 1.5, c).astype(np.float32), beta=rng.uniform(-0.5, 0.5, c).astype(np.float32),
               batch_row=br, n_batch=nb, c=c, dtype=dtype)
    if dtype == "bf16":
        out["x"], out["dy"] = _bf16_round(out["x"]), _bf16_round(out["dy"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=6)
def inputs(dtype, c, n, pattern):
    br, nb = segments(pattern, n)
    return make_inputs(dtype, c, br, nb, zlib.crc32(pattern.encode()) % 1000,
                       spread=SPREAD if len(br) < WIDE_SPREAD_ROWS else WIDE_SPREAD)


@functools.lru_cache(maxsize=4)
def const_inputs(c, layout):
    """3 instances; every row of instance 1 equals CONST_VALUE (CONST_ROWS rows: many chunks at c = 12 and 96)"""
    br = np.repeat(np.arange(3), [500, CONST_ROWS, 700])
    if layout == "interleaved":
        br = np.random.default_rng(5).permutation(br)
    return make_inputs("f32", c, np.ascontiguousarray(br, dtype=np.int32), 3, 77, const_instance=1, spread=WIDE_SPREAD)


def reference(inp, eps=EPS, gamma=True, beta=True):
    """float64: mean, rstd [n_batch, c]; out, dx [n, c]; grad_gamma, grad_beta [c]"""
    x, dy, br, nb = inp["x"].astype(np.float64), inp["dy"].astype(np.float64), inp["batch_row"], inp["n_batch"]
    n, c = x.shape
    ga = inp["gamma"].astype(np.float64) if gamma else np.ones(c)
    be = inp["beta"].astype(np.float64) if beta else np.zeros(c)
    order, starts, cnt = _segment_index(br, nb)
    present = cnt > 0

    def seg_sum(a):
        out = np.zeros((nb, c))
        if n:
            out[present] = np.add.reduceat(a[order], starts[present], axis=0)
        return out
    div = np.maximum(cnt, 1)[:, None].astype(np.float64)
    mean = seg_sum(x) / div
    d = x - mean[br]
    rstd = 1.0 / np.sqrt(seg_sum(d * d) / div + eps)
    xhat = d * rstd[br]
    t1, t2 = seg_sum(dy), seg_sum(dy * xhat)
    dx = ga * rstd[br] * (dy - (t1 / div)[br] - xhat * (t2 / div)[br])
    return dict(mean=mean, rstd=rstd, out=xhat * ga + be, dx=dx, grad_gamma=t2.sum(0), grad_beta=t1.sum(0))


def naive_f32(inp, eps=EPS):
    """the same formula with every sum a running float32 sum in row order and every intermediate float32: two passes,
    no shift, no tree — what the bar has to leave room for at the least"""
    f = np.float32
    x, dy, br, nb = inp["x"], inp["dy"], inp["batch_row"], inp["n_batch"]
    n, c = x.shape
    order, starts, cnt = _segment_index(br, nb)

    def seg_sum(a):
        out = np.zeros((nb, c), f)
        for b in np.nonzero(cnt)[0]:
            out[b] = np.cumsum(a[order[starts[b]:starts[b] + cnt[b]]], axis=0, dtype=f)[-1]
        return out
    div = np.maximum(cnt, 1)[:, None].astype(f)
    mean = seg_sum(x) / div
    d = x - mean[br]
    rstd = (f(1) / np.sqrt(seg_sum(d * d) / div + f(eps))).astype(f)
    xhat = d * rstd[br]
    t1, t2 = seg_sum(dy), seg_sum(dy * xhat)
    dx = inp["gamma"] * rstd[br] * (dy - (t1 / div)[br] - xhat * (t2 / div)[br])
    out = dict(mean=mean, rstd=rstd, out=xhat * inp["gamma"] + inp["beta"], dx=dx, grad_gamma=t2.sum(0, dtype=f),
               grad_beta=t1.sum(0, dtype=f))
    assert all(v.dtype == f for v in out.values())
    return out


# ---- running the entry points ---------------------------------------------------------------------------------------
OUTPUTS = ("mean", "rstd", "out", "dx", "grad_gamma", "grad_beta")
SENTINEL = 7.0          # what an output buffer holds before a call that must not write it


def _lib():
    from minkowskiengine_amd import _lib as L
    return L


def _tdtype(dtype):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[dtype]


def _upload(a, tdtype, device, offset):
    """the matrix on the device; offset: it begins one element into its allocation and ends exactly at its end"""
    t = torch.tensor(np.asarray(a)).to(tdtype)
    buf = torch.full((max(t.numel(), 1) + (1 if offset else 0),), SENTINEL, dtype=tdtype, device=device)
    view = buf[1:] if offset else buf
    view[:t.numel()].copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == (view.element_size() if offset else 0)
    return buf, view


def _blank(numel, tdtype, device, offset):
    buf = torch.full((max(numel, 1) + (1 if offset else 0),), float("nan"), dtype=tdtype, device=device)
    if offset:
        buf[0] = SENTINEL
    view = buf[1:] if offset else buf
    assert view.data_ptr() % 16 == (view.element_size() if offset else 0)
    return buf, view


def run(device, inp, eps=EPS, gamma=True, beta=True, want=("dx", "grad_gamma", "grad_beta"), offset=(), ws_byte=0xFF,
        x=None, dy=None):
    """stats -> apply -> backward through the C ABI on fresh buffers -> dict of CPU tensors (None: not requested).
    offset: which of "x", "dy", "y", "dx" begin one element into their allocation.  x / dy: replacements of the
    case's matrices (the non-finite runs)."""
    L = _lib()
    lib = L.load()
    dtype = inp["dtype"]
    td = _tdtype(dtype)
    pd = torch.float64 if dtype == "f64" else torch.float32
    br_np, nb, c = inp["batch_row"], inp["n_batch"], inp["c"]
    n = len(br_np)
    st = torch.cuda.current_stream(device).cuda_stream
    _, xd = _upload(inp["x"] if x is None else x, td, device, "x" in offset)
    _, gd = _upload(inp["dy"] if dy is None else dy, td, device, "dy" in offset)
    br = torch.tensor(br_np if n else np.zeros(1, np.int32)).to(device)
    ga = torch.tensor(inp["gamma"]).to(pd).to(device) if gamma else None
    be = torch.tensor(inp["beta"]).to(pd).to(device) if beta else None
    _, mean = _blank(nb * c, pd, device, False)
    _, rstd = _blank(nb * c, pd, device, False)
    ybuf, y = _blank(n * c, td, device, "y" in offset)
    dxbuf, dxv = _blank(n * c, td, device, "dx" in offset)
    gg = torch.full((c,), SENTINEL, dtype=pd, device=device)
    gb = torch.full((c,), SENTINEL, dtype=pd, device=device)
    if "dx" not in want:
        dxv.fill_(SENTINEL)
    need = int(lib.me_inorm_workspace_bytes(n, nb, c))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    ptr = lambda t: None if t is None else t.data_ptr()                           # noqa: E731
    ws.fill_(ws_byte)
    if dtype == "f64":
        L.check(lib.me_inorm_stats_f64(ptr(xd), ptr(br), n, nb, c, float(eps), ptr(mean), ptr(rstd), st))
        L.check(lib.me_inorm_apply_f64(ptr(xd), ptr(br), n, nb, c, ptr(mean), ptr(rstd), ptr(ga), ptr(be), ptr(y), st))
    else:
        bf = 1 if dtype == "bf16" else 0
        L.check(lib.me_inorm_stats(ptr(xd), bf, ptr(br), n, nb, c, float(eps), ptr(mean), ptr(rstd), ptr(ws), need, st))
        L.check(lib.me_inorm_apply(ptr(xd), bf, ptr(br), n, nb, c, ptr(mean), ptr(rstd), ptr(ga), ptr(be), ptr(y), st))
    stats = mean.clone(), rstd.clone()
    res = dict(mean=mean, rstd=rstd, out=y[:n * c].reshape(n, c), dx=None, grad_gamma=None, grad_beta=None)
    if n > 0:
        ws.fill_(ws_byte)
        args = (ptr(mean), ptr(rstd), ptr(ga), ptr(dxv) if "dx" in want else None,
                ptr(gg) if "grad_gamma" in want else None, ptr(gb) if "grad_beta" in want else None, ptr(ws), need, st)
        if dtype == "f64":
            L.check(lib.me_inorm_backward_f64(ptr(xd), ptr(gd), ptr(br), n, nb, c, *args))
        else:
            L.check(lib.me_inorm_backward(ptr(xd), ptr(gd), bf, ptr(br), n, nb, c, *args))
        for name, t in (("dx", dxv[:n * c].reshape(n, c)), ("grad_gamma", gg), ("grad_beta", gb)):
            if name in want:
                res[name] = t
            else:
                assert bool((t == SENTINEL).all()), f"{name} was not requested and was written"
    torch.cuda.synchronize()
    if n == 0:      # apply without rows returns 0 and writes nothing
        assert bool(torch.isnan(ybuf.float()).all()), "apply wrote y without rows"
    # backward only reads the statistics; the element in front of an offset output is not touched
    assert _same_bits(mean, stats[0]) and _same_bits(rstd, stats[1]), "backward changed mean / rstd"
    for name, buf in (("y", ybuf), ("dx", dxbuf)):
        if name in offset:
            assert float(buf[0]) == SENTINEL, f"the element in front of {name} was written"
    res = {k: (None if v is None else v.detach().cpu()) for k, v in res.items()}
    res["mean"], res["rstd"] = res["mean"][:nb * c].reshape(nb, c), res["rstd"][:nb * c].reshape(nb, c)
    return res


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def check_close(got, want, dtype, tag=""):
    for name in OUTPUTS:
        if got[name] is None:
            continue
        g = got[name].double().numpy()
        w = want[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if dtype == "f64":
            err = float(np.abs(g - w).max()) if g.size else 0.0
            assert err <= 1e-10, f"{tag} {name}: max abs err {err}"
        elif dtype == "bf16" and name in ("out", "dx"):
            assert_close(g, w, what=f"{tag} {name}", **BF16_OUT)
        else:
            assert_close(g, w, what=f"{tag} {name}")


def check_structure(got, inp, eps=EPS):
    """what must hold exactly: an absent instance has mean 0; a one-row instance has out == beta; all is finite"""
    br, nb = inp["batch_row"], inp["n_batch"]
    cnt = np.bincount(br, minlength=nb)
    for name in OUTPUTS:
        assert got[name] is None or bool(torch.isfinite(got[name]).all()), f"{name} is not finite"
    absent = torch.from_numpy(cnt == 0)
    assert bool((got["mean"][absent] == 0).all()), "mean of an instance without rows"
    assert_close(got["rstd"][absent], np.full((int(absent.sum()), inp["c"]), 1 / math.sqrt(eps)), what="absent rstd")
    rows = torch.from_numpy(cnt[br] == 1) if len(br) else torch.zeros(0, dtype=torch.bool)
    if bool(rows.any()):
        one = torch.from_numpy(cnt == 1)
        assert_close(got["rstd"][one], np.full((int(one.sum()), inp["c"]), 1 / math.sqrt(eps)), what="one-row rstd")
        beta = torch.tensor(inp["beta"]).to(got["out"].dtype)
        assert _same_bits(got["out"][rows], beta.expand(int(rows.sum()), -1).contiguous()), "one-row instance: out"
        assert bool((got["dx"][rows] == 0).all()), "one-row instance: dx"


def _id(case):
    return "-".join(str(v) for v in case)


# ---- the tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPE_CASES, ids=_id)
def test_shapes(device, case):
    inp = inputs(*case)
    got = run(device, inp)
    check_close(got, reference(inp), case[0], _id(case))
    check_structure(got, inp)


@pytest.mark.parametrize("case", PATTERN_CASES, ids=_id)
def test_segment_patterns(device, case):
    inp = inputs(*case)
    got = run(device, inp)
    check_close(got, reference(inp), case[0], _id(case))
    check_structure(got, inp)


@pytest.mark.parametrize("c,layout", CONST_CASES)
def test_constant_instance(device, c, layout):
    """every row of instance 1 equals 1000.25, over many chunks: the shifted sums are exactly 0, so mean is the value,
    rstd is 1 / sqrt(eps) and out == beta bit for bit"""
    inp = const_inputs(c, layout)
    got = run(device, inp, eps=CONST_EPS)
    check_close(got, reference(inp, eps=CONST_EPS), "f32", f"const {c} {layout}")
    assert bool((got["mean"][1] == CONST_VALUE).all())
    assert_close(got["rstd"][1], np.full(c, 1 / math.sqrt(CONST_EPS)), what="rstd of the constant instance")
    rows = torch.from_numpy(inp["batch_row"] == 1)
    assert int(rows.sum()) == CONST_ROWS
    assert _same_bits(got["out"][rows], torch.tensor(inp["beta"]).expand(CONST_ROWS, -1).contiguous())
    for name in OUTPUTS:
        assert bool(torch.isfinite(got[name]).all()), name


ISOLATION_CASES = [("f32", 12, _several("f32", 12), "sorted3"), ("f32", 12, _several("f32", 12), "rr3"),
                   ("bf16", 24, _several("bf16", 24), "sorted3"), ("bf16", 24, _several("bf16", 24), "rr3"),
                   ("f32", 1028, 40, "sorted3")]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", ISOLATION_CASES, ids=_id)
def test_non_finite_rows_stay_in_their_instance_and_channel(device, case, bad):
    """channel q of the rows of instance k holds NaN / +Inf (k shares chunks with its neighbours in the sorted layout
    and every chunk in the round-robin layout; q sits inside a vector piece), once in x alone and once in x and dy.
    Everything that does not belong to (k, q) is bit-identical to the clean run; mean, rstd, out and dx of (k, q) and
    grad_gamma[q] are NaN, as in the float64 formula.  grad_beta[q] = sum dy does not depend on x: with x alone
    poisoned it is bit-identical to the clean run, with dy poisoned too it is NaN for NaN and +Inf for +Inf."""
    inp = inputs(*case)
    k, q = 1, 5
    x, dy = inp["x"].copy(), inp["dy"].copy()
    rows = inp["batch_row"] == k
    x[rows, q] = bad
    dy[rows, q] = bad
    clean = run(device, inp)
    other_ch = torch.ones(inp["c"], dtype=torch.bool)
    other_ch[q] = False
    rows_t = torch.from_numpy(rows)
    inst = torch.arange(inp["n_batch"]) == k
    for what, dirty in (("x", run(device, inp, x=x)), ("x and dy", run(device, inp, x=x, dy=dy))):
        for name in ("mean", "rstd"):
            assert _same_bits(clean[name][~inst], dirty[name][~inst]), f"{what}: {name} of the other instances"
            assert _same_bits(clean[name][inst][:, other_ch], dirty[name][inst][:, other_ch]), f"{what}: {name}, other channels"
            assert bool(torch.isnan(dirty[name][k, q])), f"{what}: {name} of the poisoned instance and channel"
        for name in ("out", "dx"):
            assert _same_bits(clean[name][~rows_t], dirty[name][~rows_t]), f"{what}: {name} of the other instances"
            assert _same_bits(clean[name][rows_t][:, other_ch], dirty[name][rows_t][:, other_ch]), \
                f"{what}: {name}, other channels"
            assert bool(torch.isnan(dirty[name][rows_t][:, q].float()).all()), f"{what}: {name} of the poisoned channel"
        for name in ("grad_gamma", "grad_beta"):
            assert _same_bits(clean[name][other_ch], dirty[name][other_ch]), f"{what}: {name}"
        assert bool(torch.isnan(dirty["grad_gamma"][q])), what
        if what == "x":
            assert _same_bits(clean["grad_beta"], dirty["grad_beta"]), "grad_beta does not depend on x"
        else:
            gb = float(dirty["grad_beta"][q])
            assert math.isnan(gb) if math.isnan(bad) else gb == math.inf


REPRO_CASES = [("f32", 12, _several("f32", 12), "many300_shuffled"), ("f32", 96, _several("f32", 96), "gapped"),
               ("bf16", 24, _several("bf16", 24), "rr7"), ("f32", 1024, 5000, "perm3")]


@pytest.mark.parametrize("case", REPRO_CASES, ids=_id)
def test_runs_are_bit_identical_whatever_the_workspace_held(device, case):
    inp = inputs(*case)
    first = run(device, inp)
    for ws_byte in (0xFF, 0x00):
        again = run(device, inp, ws_byte=ws_byte)
        for name in OUTPUTS:
            assert _same_bits(first[name], again[name]), (name, ws_byte)


ARG_CASES = [("f32", 12, _several("f32", 12), "gapped"), ("bf16", 24, _several("bf16", 24), "gapped"),
             ("f64", 5, 1500, "gapped")]


@pytest.mark.parametrize("case", ARG_CASES, ids=_id)
def test_argument_combinations(device, case):
    """gamma / beta NULL mean 1 / 0; every subset of {dx, grad_gamma, grad_beta} may be NULL: what is requested is
    bit-identical to the run that requests everything, what is not requested is never written (checked in run)"""
    inp = inputs(*case)
    full = run(device, inp)
    check_close(full, reference(inp), case[0], "all")
    names = ("dx", "grad_gamma", "grad_beta")
    for k in range(len(names)):
        for want in itertools.combinations(names, k):
            got = run(device, inp, want=want)
            for name in ("mean", "rstd", "out") + want:
                assert _same_bits(full[name], got[name]), (want, name)
            for name in set(names) - set(want):
                assert got[name] is None
    ones = dict(inp, gamma=np.ones_like(inp["gamma"]), beta=np.zeros_like(inp["beta"]))
    for gamma, beta in ((False, True), (True, False), (False, False)):
        got = run(device, inp, gamma=gamma, beta=beta)
        check_close(got, reference(inp, gamma=gamma, beta=beta), case[0], f"gamma={gamma} beta={beta}")
        explicit = run(device, dict(inp, gamma=inp["gamma"] if gamma else ones["gamma"],
                                    beta=inp["beta"] if beta else ones["beta"]))
        for name in OUTPUTS:
            assert _same_bits(explicit[name], got[name]), (gamma, beta, name)


@pytest.mark.parametrize("which", ["x", "dy", "y", "dx"])
@pytest.mark.parametrize("case", UNALIGNED_CASES, ids=_id)
def test_unaligned_views(device, case, which):
    """one of the four matrices begins one element into a larger allocation and ends exactly at its end: the calls that
    get it fall back to V = 1 while the others keep the 16-byte pieces (stats looks at x alone, apply at x and y,
    backward at x, dy and dx)"""
    inp = inputs(*case)
    got = run(device, inp, offset=(which,))
    check_close(got, reference(inp), case[0], f"{which} offset")
    check_structure(got, inp)


@pytest.mark.parametrize("c", [3226, 4096])
def test_rows_wider_than_the_lds_are_refused(device, c):
    """the partial kernels keep 5 c + 256 floats in LDS: above c = 3225 stats and backward return an error that names the
    channel count before any launch, and write nothing"""
    L = _lib()
    lib = L.load()
    n, nb = 24, 2
    st = torch.cuda.current_stream(device).cuda_stream
    x = torch.zeros(n, c, device=device)
    br = torch.zeros(n, dtype=torch.int32, device=device)
    mean = torch.full((nb, c), SENTINEL, device=device)
    rstd = torch.full((nb, c), SENTINEL, device=device)
    dx = torch.full((n, c), SENTINEL, device=device)
    gg = torch.full((c,), SENTINEL, device=device)
    need = int(lib.me_inorm_workspace_bytes(n, nb, c))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
    with pytest.raises(RuntimeError, match="channel count"):
        L.check(lib.me_inorm_stats(x.data_ptr(), 0, br.data_ptr(), n, nb, c, EPS, mean.data_ptr(), rstd.data_ptr(),
                                   ws.data_ptr(), need, st))
    with pytest.raises(RuntimeError, match="channel count"):
        L.check(lib.me_inorm_backward(x.data_ptr(), x.data_ptr(), 0, br.data_ptr(), n, nb, c, mean.data_ptr(),
                                      rstd.data_ptr(), None, dx.data_ptr(), gg.data_ptr(), gg.data_ptr(), ws.data_ptr(),
                                      need, st))
    torch.cuda.synchronize()
    for t in (mean, rstd, dx, gg):
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize("dtype,c", [("f32", 4), ("f32", 5), ("bf16", 4), ("bf16", 5), ("f64", 4), ("f64", 5)])
def test_no_rows(device, dtype, c):
    """n = 0: every instance is absent (mean 0, rstd 1 / sqrt(eps)), apply is a no-op that returns 0 and backward
    returns its documented error (the float64 twin: zero parameter gradients)"""
    inp = make_inputs(dtype, c, np.zeros(0, np.int32), 3, 0)
    got = run(device, inp)                      # stats + apply; run() skips backward without rows
    assert bool((got["mean"] == 0).all())
    want = 1 / math.sqrt(EPS)
    if dtype == "f64":
        assert float((got["rstd"] - want).abs().max()) <= 1e-10
    else:
        assert_close(got["rstd"], np.full((3, c), want), what="rstd")
    L = _lib()
    lib = L.load()
    st = torch.cuda.current_stream(device).cuda_stream
    td, pd = _tdtype(dtype), (torch.float64 if dtype == "f64" else torch.float32)
    x = torch.zeros(1, c, dtype=td, device=device)
    br = torch.zeros(1, dtype=torch.int32, device=device)
    dx = torch.full((1, c), SENTINEL, dtype=td, device=device)
    gg, gb = (torch.full((c,), SENTINEL, dtype=pd, device=device) for _ in range(2))
    need = int(lib.me_inorm_workspace_bytes(0, 3, c))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
    mean, rstd = got["mean"].to(device), got["rstd"].to(device)
    if dtype == "f64":
        L.check(lib.me_inorm_backward_f64(x.data_ptr(), x.data_ptr(), br.data_ptr(), 0, 3, c, mean.data_ptr(),
                                          rstd.data_ptr(), None, dx.data_ptr(), gg.data_ptr(), gb.data_ptr(),
                                          ws.data_ptr(), need, st))
        torch.cuda.synchronize()
        assert bool((gg == 0).all()) and bool((gb == 0).all())
    else:
        with pytest.raises(RuntimeError, match="at least one row"):
            L.check(lib.me_inorm_backward(x.data_ptr(), x.data_ptr(), 1 if dtype == "bf16" else 0, br.data_ptr(), 0, 3, c,
                                          mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(), gg.data_ptr(),
                                          gb.data_ptr(), ws.data_ptr(), need, st))
        torch.cuda.synchronize()
        assert bool((gg == SENTINEL).all()) and bool((gb == SENTINEL).all())
    assert bool((dx == SENTINEL).all())


def test_workspace_contract(device):
    """the size covers both partial arrays of the most chunks either pass uses, never shrinks with n, and a claim of one
    byte less is refused before any launch (the buffer itself is whole)"""
    L = _lib()
    lib = L.load()
    n, nb, c = 3000, 5, 12
    sizes = [int(lib.me_inorm_workspace_bytes(m, nb, c)) for m in (0, 1, 4, 5, 2048, 3000, 10 ** 6)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[3] > sizes[2] and sizes[4] > sizes[3]
    assert sizes[6] >= 2 * K_MAX_CHUNKS * nb * c * 4 + K_MAX_CHUNKS * nb * 4
    for dtype, m in (("f32", n), ("bf16", n), ("f32", 70000)):
        g = geometry(dtype, c, m)
        need = int(lib.me_inorm_workspace_bytes(m, nb, c))
        assert need >= (2 * c + 1) * nb * 4 * max(g["chunks"], g["bwd_chunks"]) + (2 * c + 1) * nb * 4
    st = torch.cuda.current_stream(device).cuda_stream
    need = int(lib.me_inorm_workspace_bytes(n, nb, c))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
    x = torch.zeros(n, c, device=device)
    br = torch.zeros(n, dtype=torch.int32, device=device)
    mean = torch.full((nb, c), SENTINEL, device=device)
    rstd = torch.full((nb, c), SENTINEL, device=device)
    dx = torch.full((n, c), SENTINEL, device=device)
    with pytest.raises(RuntimeError, match="workspace too small"):
        L.check(lib.me_inorm_stats(x.data_ptr(), 0, br.data_ptr(), n, nb, c, EPS, mean.data_ptr(), rstd.data_ptr(),
                                   ws.data_ptr(), need - 1, st))
    with pytest.raises(RuntimeError, match="workspace too small"):
        L.check(lib.me_inorm_backward(x.data_ptr(), x.data_ptr(), 0, br.data_ptr(), n, nb, c, mean.data_ptr(),
                                      rstd.data_ptr(), None, dx.data_ptr(), None, None, ws.data_ptr(), need - 1, st))
    with pytest.raises(RuntimeError, match="workspace too small"):
        L.check(lib.me_inorm_backward_f64(x.data_ptr(), x.data_ptr(), br.data_ptr(), n, nb, c, mean.data_ptr(),
                                          rstd.data_ptr(), None, dx.data_ptr(), None, None, ws.data_ptr(), need - 1, st))
    torch.cuda.synchronize()
    for t in (mean, rstd, dx):
        assert bool((t == SENTINEL).all())
    assert bool((ws == 0xFF).all())


@pytest.mark.parametrize("c,n,pattern", F64_CASES, ids=lambda v: str(v))
def test_float64_twins(device, c, n, pattern):
    inp = inputs("f64", c, n, pattern)
    assert len(inp["batch_row"]) <= 2000
    got = run(device, inp)
    assert got["out"].dtype == torch.float64 and got["grad_gamma"].dtype == torch.float64
    check_close(got, reference(inp), "f64", f"f64 {c} {n} {pattern}")
    check_structure(got, inp)
