"""The tile-plan convolution launches themselves (csrc/conv_bf16.hip k_conv_tile_bf16 and its split-K reduce,
csrc/conv_bf16_ws.hip, csrc/conv_f32x3.hip k_conv_tile_f32x3 / _ws) on synthetic neighbour tables, through the C ABI:
a table tbl [volume, n_tgt] (source row of (offset, target row), -1: none) -> me_plan_build / me_plan_build_multi ->
me_conv_pack_weights_{bf16,f32x3} -> me_conv_target_bf16 / _fused / _ex (statistics, split-K) and me_conv_target_f32x3:
    dst[r] = sum over offsets k of src[tbl[k][r]] @ W[k]        for EVERY target row r (no entry: zeros),
the tiles being the rows order[t T .. (t + 1) T) (order NULL: the rows themselves).

tests/test_gpu_conv.py, test_gpu_bf16.py and test_gpu_conv_backward_tail.py drive these kernels through whole layers on
uniform random clouds with the policy's geometry.  Here the claims the kernels rest on are the subject: padding slots
gather source row 0 into a dummy accumulator row; the 64-slot index window of a batch is read to its end; (tile, offset)
items on the group (16) and batch (64) edges under every batch_groups; tile heights and row counts on the tile edges;
every shipped (slab width, chunk depth); poisoned rows 0 and n_src - 1 that no entry names; non-finite rows that are
named; the batch-norm partials against their fp32 error bound; split-K with its workspace; the argument checks.

Oracle: numpy float64 on the operands as the kernel sees them (bf16: features and weights rounded to bf16; f32x3: the
fp32 values).  EXACT data — integer features in [-8, 8], weights that round to multiples of 2^-6 in [-2, 2] — make every
fp32 partial sum exact in any order (precondition sum|products| 2^6 < 2^24, asserted): the bf16 dst must equal the bf16
rounding of the float64 sum BIT FOR BIT, the f32x3 dst the sum itself.  RANDOM data: assert_bf16_close, and for f32x3
|err| <= 2e-6 sum|x||w| per element (test_gpu_conv.py::test_split_bf16_pipe_is_fp32_grade).  Every buffer is a view into
the MIDDLE of a larger tensor: NaN around features and weights, a bit pattern around dst, the partials, the packed
weights and the split-K workspace (NaN inside before every launch), guard-row indices around tbl and order."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import (DEBUG_BUILD_ONLY, GUARD_PAD, Guarded, assert_tile_partials, exact_weights_bf16, int_view, middle,
                     same_nonfinite_class)
from test_gpu_bf16 import assert_bf16_close, bf16_round

pytestmark = pytest.mark.gpu

# (name, switches) of the bf16 launches that the header promises to agree bit for bit with me_conv_target_bf16:
# k_conv_tile_bf16, the wave-specialised kernel, batch fusion, no deep pipeline, two stage buffers, 64-bit gather
# addresses (conv variant 6: the general instantiation), no batch fusion inside the kernel (variant 7)
BF16_KERNELS = [("tile", dict(ws=0)), ("ws", dict(ws=1)), ("fused", dict(ws=0, fused=1)), ("no-deep", dict(ws=0, deep=0)),
                ("twobuf", dict(ws=0, deep=1, twobuf=1)), ("addr64", dict(ws=0, variant=6)), ("variant7", dict(ws=1, variant=7))]
# f32x3: the shipped choice (wave-specialised on 64 / 128 columns, k_conv_tile_f32x3 on 32 / 96), conv variant 30 (the
# ping-pong kernel where the build has it), variant 6 (64-bit addresses: the general instantiation)
X3_KERNELS = [("shipped", 0), ("variant30", 30), ("addr64", 6)]


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _restore(lib):
    lib.me_debug_set_bf16_ws(-1)
    lib.me_debug_set_bf16_shape(0, 0)
    lib.me_debug_set_bf16_deep(-1)
    lib.me_debug_set_bf16_twobuf(-1)
    lib.me_debug_set_bf16_splitk(-1)
    lib.me_debug_set_bf16_splitk_mode(0)
    lib.me_debug_set_bf16_offsync(0)
    lib.me_debug_set_tile_dispatch(0)
    lib.me_debug_set_conv_variant(0)


@pytest.fixture
def lib():
    _, lib = _lib()
    _restore(lib)
    try:
        yield lib
    finally:
        _restore(lib)


# ---- tables -----------------------------------------------------------------------------------------------------------------
def make_table(rng, kind, volume, n_tgt, n_src, tile_rows=128, first_row=0, last_row=None):
    """int32 [volume, n_tgt] of source rows in [first_row, last_row), -1 = no neighbour"""
    last_row = n_src if last_row is None else last_row
    rows = rng.integers(first_row, max(last_row, first_row + 1), size=(volume, n_tgt)).astype(np.int32)
    none = np.full((volume, n_tgt), -1, np.int32)
    if kind == "dense":
        return rows
    if kind == "absent":
        return none
    if kind in ("last_offset", "first_offset"):
        k = volume - 1 if kind == "last_offset" else 0
        half = rng.random(n_tgt) < 0.5
        none[k, half] = rows[k, half]
        return none
    if kind == "one_row":                        # one target row holds every entry of the table
        r = n_tgt // 2
        none[:, r] = rows[:, r]
        return none
    if kind == "same_source":                    # every entry of a (tile, offset) item names one source row
        for t in range(-(-n_tgt // tile_rows)):
            none[:, t * tile_rows:(t + 1) * tile_rows] = rows[:, t:t + 1]
        return none
    tbl = np.where(rng.random((volume, n_tgt)) < 0.3, rows, -1).astype(np.int32)
    if kind == "tail_last_col":                  # the last, partial tile present at its last column only
        start = (n_tgt - 1) // tile_rows * tile_rows
        assert start < n_tgt - 1 and n_tgt % tile_rows
        tbl[:, start:n_tgt - 1] = -1
        tbl[:, n_tgt - 1] = rows[:, n_tgt - 1]
    else:
        assert kind == "random", kind
    return tbl


ITEM_SIZES = (15, 16, 17, 63, 64, 65, 80)       # group edge, batch edge (4 x 16), 5 groups -> 3 + 2


def item_size_table(rng, tile_rows, n_tgt, n_src, order=None):
    """offset k of tiles 0 and 1 holds exactly ITEM_SIZES[k] entries (the rows of a tile are order[t T ..]); one more
    offset that is empty in tile 0; a random rest"""
    assert tile_rows >= max(ITEM_SIZES) and n_tgt >= 2 * tile_rows
    volume = len(ITEM_SIZES) + 1
    tbl = make_table(rng, "random", volume, n_tgt, n_src)
    pos = np.arange(n_tgt) if order is None else np.asarray(order)
    for t in (0, 1):
        tile = pos[t * tile_rows:(t + 1) * tile_rows]
        tbl[:, tile] = -1
        for k, size in enumerate(ITEM_SIZES):
            chosen = rng.choice(tile, size, replace=False)
            tbl[k, chosen] = rng.integers(0, n_src, size)
    counts = [(tbl[k, pos[:tile_rows]] >= 0).sum() for k in range(volume)]
    assert tuple(counts[:-1]) == ITEM_SIZES and counts[-1] == 0
    return tbl


# ---- one problem on the device ------------------------------------------------------------------------------------------------
class Case:
    """features, weights and table of one problem on the device (views into guard tensors) and its float64 oracle"""

    def __init__(self, device, tbl, x, w_fed, w_used, pipe):
        L, self.lib = _lib()
        self.check, self.device, self.pipe = L.check, device, pipe
        self.volume, self.n_tgt = tbl.shape
        self.n_src, self.c_src = x.shape
        self.c_dst = w_fed.shape[2]
        assert w_fed.shape == (self.volume, self.c_src, self.c_dst) and tbl.max() < self.n_src and tbl.min() >= -1
        if pipe == "bf16":
            assert torch.equal(bf16_round(x).nan_to_num(7.0, 8.0, 9.0), x.nan_to_num(7.0, 8.0, 9.0))
            assert torch.equal(bf16_round(w_fed), w_used)
        else:
            assert torch.equal(w_fed, w_used)
        self.tbl_host, self.x_host, self.w_fed, self.w_used = tbl, x, w_fed, w_used
        self.n_pairs = int((tbl >= 0).sum())
        # ---- the oracle ----
        x64, w64 = x.numpy().astype(np.float64), w_used.numpy().astype(np.float64)
        ref, mag = np.zeros((self.n_tgt, self.c_dst)), np.zeros((self.n_tgt, self.c_dst))
        xa = np.abs(np.nan_to_num(x64, nan=0.0, posinf=0.0, neginf=0.0))
        with np.errstate(invalid="ignore"):
            if self.volume <= 256:
                for k in range(self.volume):
                    m = tbl[k] >= 0
                    if m.any():
                        ref[m] += x64[tbl[k][m]] @ w64[k]
                        mag[m] += xa[tbl[k][m]] @ np.abs(np.nan_to_num(w64[k], nan=0.0, posinf=0.0, neginf=0.0))
            else:                                   # a sparse table over very many offsets: pair by pair
                ks, rs = np.nonzero(tbl >= 0)
                ss = tbl[ks, rs]
                np.add.at(ref, rs, np.einsum("pc,pcd->pd", x64[ss], w64[ks]))
                np.add.at(mag, rs, np.einsum("pc,pcd->pd", xa[ss], np.abs(w64[ks])))
        self.ref, self.mag = ref, mag
        # ---- device buffers ----
        nan = float("nan")
        dt = torch.bfloat16 if pipe == "bf16" else torch.float32
        self.src_big, self.src = middle(self.n_src * self.c_src, dt, device, nan)
        self.src.copy_(x.to(dt).reshape(-1))
        self.w_big, self.w = middle(w_fed.numel(), torch.float32, device, nan)
        self.w.copy_(w_fed.reshape(-1))
        self.wt_big, self.wt = middle(w_fed.numel(), torch.float32, device, nan)       # [K, c_dst, c_src]: transposed = 1
        self.wt.copy_(w_fed.permute(0, 2, 1).contiguous().reshape(-1))
        # a stray table read gives source row n_src: the NaN behind the features
        self.tbl_big, self.tbl = middle(tbl.size, torch.int32, device, self.n_src)
        self.tbl.copy_(torch.from_numpy(np.ascontiguousarray(tbl)).reshape(-1))
        self.dst = Guarded(self.n_tgt * self.c_dst, 2 if pipe == "bf16" else 4, device)
        self.packed = {}
        self.inputs = [self.src_big, self.w_big, self.wt_big, self.tbl_big]
        self.inputs_before = [t.clone() for t in self.inputs]
        self.outputs = [self.dst]
        assert self.src.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    # ---- expectations ----
    def exact_precondition(self, scale=64.0):
        assert np.isfinite(self.mag).all() and (self.mag * scale < 2.0 ** 24).all(), \
            "exact data: sum|products| / quantum must stay below 2^24"
        fin = np.isfinite(self.ref)
        assert (np.where(fin, self.ref, 0.0) * scale % 1 == 0).all()

    def exact_bits_bf16(self):
        self.exact_precondition()
        return int_view(torch.from_numpy(self.ref).to(torch.bfloat16))

    # ---- weights ----
    def pack(self, transposed=0):
        """the packed image for the kernel shape in force (the chunk depth follows me_debug_set_bf16_shape)"""
        lib, bf16, mfma = self.lib, self.pipe == "bf16", self.pipe == "f32mfma"
        chunk = 0 if mfma else int((lib.me_conv_pack_chunk_bf16 if bf16 else lib.me_conv_pack_chunk_f32x3)(self.c_src, self.c_dst))
        key = (transposed, chunk)
        if key not in self.packed:
            elems = int((lib.me_conv_packed_weight_elems if mfma else lib.me_conv_packed_weight_elems_bf16 if bf16 else
                         lib.me_conv_packed_weight_elems_f32x3)(self.volume, self.c_src, self.c_dst))
            g = Guarded(elems, 4 if mfma else 2, self.device, base=7)
            g.fill()
            w = self.wt if transposed else self.w
            if mfma:
                self.check(lib.me_conv_pack_weights_f32(w.data_ptr(), self.volume, self.c_src, self.c_dst, transposed,
                                                        g.ptr(), None))
            elif bf16:
                self.check(lib.me_conv_pack_weights_bf16(w.data_ptr(), 1, self.volume, self.c_src, self.c_dst, transposed,
                                                         g.ptr(), None))
            else:
                self.check(lib.me_conv_pack_weights_f32x3(w.data_ptr(), self.volume, self.c_src, self.c_dst, transposed,
                                                          g.ptr(), None))
            torch.cuda.synchronize()
            assert g.intact(), "the weight pack wrote outside the image"
            self.packed[key] = (g, g.bits.clone())
            self.outputs.append(g)
        return self.packed[key][0]

    def intact(self):
        ok = all(torch.equal(int_view(a), int_view(b)) for a, b in zip(self.inputs, self.inputs_before))
        ok = ok and all(torch.equal(g.bits, before) for g, before in self.packed.values())
        return ok and all(g.intact() for g in self.outputs)


class Plan:
    """me_plan_build (or me_plan_build_multi) of a case's table; the arrays sit in guard tensors whose surroundings name
    source row n_src (NaN) and local target row 0"""

    def __init__(self, case, tile_rows, batch_groups, order=None, multi=False, dispatch=0, expect_error=False):
        L, lib = _lib()
        self.case, self.T, self.bg = case, tile_rows, batch_groups
        dev, n_tgt, volume = case.device, case.n_tgt, case.volume
        self.order_host = None if order is None else np.asarray(order)
        self.order = None
        if order is not None:       # a stray order read gives target row n_tgt: the pattern behind dst
            self.order_big, self.order = middle(n_tgt, torch.int32, dev, n_tgt)
            self.order.copy_(torch.from_numpy(self.order_host.astype(np.int32)))
        self.rc = None
        if not 1 <= tile_rows <= 4096:
            return
        self.tiles = int(lib.me_plan_num_tiles(n_tgt, tile_rows))
        mg = int(lib.me_plan_max_groups(n_tgt, volume, case.n_pairs, tile_rows))
        sizes = [16 * mg, 16 * mg, 2 * mg, int(lib.me_plan_tile_bptr_elems(n_tgt, tile_rows)), self.tiles * volume + 1]
        fills = [case.n_src, 0, 0, 0, 0]
        self.bigs, self.arrays = zip(*[middle(n, torch.int32, dev, f) for n, f in zip(sizes, fills)])
        self.arrays[0].fill_(case.n_src)            # unwritten slots inside: the NaN row into local row 0
        self.arrays[1].fill_(0)
        guards = [b.clone() for b in self.bigs]
        lib.me_debug_set_tile_dispatch(dispatch)
        optr = None if self.order is None else self.order.data_ptr()
        try:
            if not multi:
                ws = torch.empty(int(lib.me_plan_workspace_bytes(n_tgt, volume, tile_rows)), dtype=torch.uint8, device=dev)
                self.rc = lib.me_plan_build(case.tbl.data_ptr(), optr, n_tgt, volume, tile_rows, batch_groups,
                                            *[a.data_ptr() for a in self.arrays], ws.data_ptr(), ws.numel(), None)
            else:
                jobs = (L.MePlanJob * 1)()
                j = jobs[0]
                j.tbl, j.order, j.n_tgt, j.volume = case.tbl.data_ptr(), optr, n_tgt, volume
                j.tile_rows, j.batch_groups = tile_rows, batch_groups
                j.plan_src, j.plan_dst, j.batch_desc, j.tile_bptr, j.item_gptr = [a.data_ptr() for a in self.arrays]
                total = int(lib.me_plan_jobs_init(ctypes.byref(jobs), 1))
                assert total == self.tiles * volume
                raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
                ws = torch.empty(int(lib.me_plan_multi_workspace_bytes(total)), dtype=torch.uint8, device=dev)
                self.rc = lib.me_plan_build_multi(ctypes.byref(jobs), raw.data_ptr(), 1, ws.data_ptr(), ws.numel(), None)
        finally:
            lib.me_debug_set_tile_dispatch(0)
        torch.cuda.synchronize()
        if expect_error:
            return
        L.check(self.rc)
        for b, g, a in zip(self.bigs, guards, self.arrays):
            assert torch.equal(b[:GUARD_PAD], g[:GUARD_PAD]) and torch.equal(b[GUARD_PAD + a.numel():], g[GUARD_PAD + a.numel():]), \
                "the plan build wrote outside its arrays"
        self.before = [b.clone() for b in self.bigs]
        perm = self.arrays[3][self.tiles + 1:2 * self.tiles + 1].cpu().numpy()
        assert sorted(perm.tolist()) == list(range(self.tiles)), "the dispatch order is no permutation of the tiles"
        self.dispatch_order = perm
        self.parts = [Guarded(self.tiles * case.c_dst, 4, dev, base=1000 * (i + 1)) for i in range(2)]
        self.workspaces = {}

    def ptrs(self):
        return [a.data_ptr() for a in self.arrays[:4]] + [None if self.order is None else self.order.data_ptr()]

    def intact(self):
        return (all(torch.equal(a, b) for a, b in zip(self.bigs, self.before)) and all(p.intact() for p in self.parts) and
                all(w.intact() for w in self.workspaces.values()))

    def workspace(self, split_k):
        lib, c = self.case.lib, self.case
        if split_k not in self.workspaces:
            nbytes = int(lib.me_conv_splitk_workspace_bytes(c.n_tgt, self.T, c.c_dst, split_k))
            assert nbytes == split_k * self.tiles * self.T * c.c_dst * 4
            self.workspaces[split_k] = Guarded(nbytes // 4, 4, c.device, base=77)
        return self.workspaces[split_k]

    def position_rows(self):
        """target row of every tile position"""
        return np.arange(self.case.n_tgt) if self.order_host is None else self.order_host


def _switches(lib, ws=-1, deep=-1, twobuf=-1, variant=0, fused=0):
    lib.me_debug_set_bf16_ws(ws)
    lib.me_debug_set_bf16_deep(deep)
    lib.me_debug_set_bf16_twobuf(twobuf)
    assert lib.me_debug_set_conv_variant(variant) == 0
    return fused


def call_bf16(case, plan, entry="ex", fused=0, split_k=1, stats=False, workspace="auto", **over):
    """one launch; dst, the partials and the workspace hold NaN before it.  Returns the return code."""
    lib = case.lib
    case.dst.fill()
    for p in plan.parts:
        p.fill()
    ws = None
    if split_k > 1 and workspace == "auto" and 1 <= split_k <= 8:
        ws = plan.workspace(split_k)
        ws.fill()
    wp = case.pack(over.pop("transposed", 0))
    a = dict(src=case.src.data_ptr(), wp=wp.ptr(), dst=case.dst.ptr(), T=plan.T, bg=plan.bg,
             mean=plan.parts[0].ptr() if stats else None, m2=plan.parts[1].ptr() if stats else None,
             ws=None if ws is None else ws.ptr())
    a.update(over)
    head = (a["src"], case.n_src, case.c_src, a["wp"], case.volume, case.c_dst, *plan.ptrs(), a["dst"], case.n_tgt, a["T"],
            a["bg"])
    if entry == "ex":
        rc = lib.me_conv_target_bf16_ex(*head, fused, split_k, a["ws"], a["mean"], a["m2"], None)
    elif entry == "stats":
        rc = lib.me_conv_target_bf16_stats(*head, fused, a["mean"], a["m2"], None)
    else:
        rc = (lib.me_conv_target_bf16_fused if fused else lib.me_conv_target_bf16)(*head, None)
    torch.cuda.synchronize()
    return rc


def run_bf16(case, plan, what="", **kw):
    """-> (dst bf16 [n_tgt, c_dst], (mean, m2) float64 numpy [tiles, c_dst] or None); guards checked"""
    stats = kw.get("stats", False)
    case.check(call_bf16(case, plan, **kw))
    assert case.intact() and plan.intact(), f"{what}: the launch wrote outside its outputs, or into an input"
    out = case.dst.as_dtype(torch.bfloat16, (case.n_tgt, case.c_dst))
    if not stats:
        assert all(p.untouched() for p in plan.parts), f"{what}: partials written without being asked"
        return out, None
    return out, tuple(p.as_dtype(torch.float32, (plan.tiles, case.c_dst)).double().cpu().numpy() for p in plan.parts)


def call_f32x3(case, plan, **over):
    lib = case.lib
    case.dst.fill()
    wp = case.pack(over.pop("transposed", 0))
    a = dict(src=case.src.data_ptr(), wp=wp.ptr(), dst=case.dst.ptr(), T=plan.T, bg=plan.bg)
    a.update(over)
    rc = lib.me_conv_target_f32x3(a["src"], case.n_src, case.c_src, a["wp"], case.volume, case.c_dst, *plan.ptrs(),
                                  a["dst"], case.n_tgt, a["T"], a["bg"], None)
    torch.cuda.synchronize()
    return rc


def run_f32x3(case, plan, what="", **kw):
    case.check(call_f32x3(case, plan, **kw))
    assert case.intact() and plan.intact(), f"{what}: the launch wrote outside dst, or into an input"
    return case.dst.as_dtype(torch.float32, (case.n_tgt, case.c_dst))


def _same_bits(a, b):
    return torch.equal(int_view(a), int_view(b))


def check_partials(case, plan, out, parts, what):
    stored = out.double().cpu().numpy()[plan.position_rows()]
    assert_tile_partials(stored, plan.T, parts[0], parts[1], what)


def check_bf16(case, plans, exact, what, kernels=BF16_KERNELS, stats=True):
    """every plan x every kernel: the first launch against the oracle (bit for bit on exact data), all others against the
    first launch's bits; the statistics launch stores the same bits and partials within their bound.  Returns dst."""
    lib = case.lib
    expect = case.exact_bits_bf16() if exact else None
    first = None
    for plan in plans:
        for name, sw in kernels:
            w = f"{what} T={plan.T} bg={plan.bg} {name}"
            fused = _switches(lib, **sw)
            out, _ = run_bf16(case, plan, w, entry="plain", fused=fused)
            if first is None:
                first = out
                if exact:
                    bad = int_view(out).cpu() != expect
                    assert not bool(bad.any()), f"{w}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result"
                else:
                    assert bool(torch.isfinite(out.float()).all()), f"{w}: rows not written, or computed from the surroundings"
                    assert_bf16_close(out.float().cpu().numpy(), case.ref, w)
            else:
                assert _same_bits(out, first), f"{w}: bits differ from the first launch"
            if stats and name in ("tile", "ws", "fused"):
                assert lib.me_conv_stats_supported_bf16(case.c_src, case.c_dst) == 1
                out2, parts = run_bf16(case, plan, w + " stats", entry="ex", fused=fused, stats=True)
                assert _same_bits(out2, first), f"{w}: dst differs with the statistics epilogue"
                check_partials(case, plan, out2, parts, w)
    _switches(lib)
    return first


def check_f32x3(case, plans, exact, what, kernels=X3_KERNELS):
    lib = case.lib
    first = None
    for plan in plans:
        for name, variant in kernels:
            w = f"{what} T={plan.T} bg={plan.bg} {name}"
            assert lib.me_debug_set_conv_variant(variant) == 0
            out = run_f32x3(case, plan, w)
            if first is None:
                first = out
                got = out.double().cpu().numpy()
                if exact:
                    bad = got != case.ref
                    assert not bad.any(), f"{w}: {int(bad.sum())} of {bad.size} elements differ from the exact sum"
                else:
                    assert np.isfinite(got).all(), f"{w}: rows not written, or computed from the surroundings"
                    excess = np.abs(got - case.ref) - 2e-6 * case.mag
                    assert (excess <= 0).all(), f"{w}: error {np.abs(got - case.ref).max():.3g} above 2e-6 sum|x||w|"
            else:
                assert _same_bits(out, first), f"{w}: bits differ from the first launch"
    lib.me_debug_set_conv_variant(0)
    return first


# ---- data -------------------------------------------------------------------------------------------------------------------
def exact_case(device, pipe, tbl, n_src, c_src, c_dst, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-8, 9, size=(n_src, c_src)).astype(np.float32))
    fed, rounded = exact_weights_bf16(rng, (tbl.shape[0], c_src, c_dst))
    return Case(device, tbl, x, fed if pipe == "bf16" else rounded, rounded, pipe)


def random_case(device, pipe, tbl, n_src, c_src, c_dst, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n_src, c_src, generator=g) - 0.3
    w = torch.rand(tbl.shape[0], c_src, c_dst, generator=g) - 0.5
    if pipe == "bf16":
        x, w = bf16_round(x), bf16_round(w)
    return Case(device, tbl, x, w, w, pipe)


def both_pipes(device, tbl, n_src, c_src, c_dst, seed, plans_of, what, exact_only=False, kernels=None):
    """the table on both pipes, exact and random data; plans_of(case) -> list of plans.  Returns the exact bf16 dst."""
    kw = {} if kernels is None else dict(kernels=kernels)
    case = exact_case(device, "bf16", tbl, n_src, c_src, c_dst, seed)
    out = check_bf16(case, plans_of(case), True, f"{what} bf16 exact", **kw)
    case = exact_case(device, "f32", tbl, n_src, c_src, c_dst, seed)
    check_f32x3(case, plans_of(case), True, f"{what} f32x3 exact")
    if not exact_only:
        case = random_case(device, "bf16", tbl, n_src, c_src, c_dst, seed + 1)
        check_bf16(case, plans_of(case)[:2], False, f"{what} bf16 random", **kw)
        case = random_case(device, "f32", tbl, n_src, c_src, c_dst, seed + 1)
        check_f32x3(case, plans_of(case)[:2], False, f"{what} f32x3 random")
    return out


# ---- items on the group and batch edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_src,c_dst", [(32, 64), (64, 128)])
def test_item_sizes_on_group_and_batch_edges_under_every_batch_size(device, lib, c_src, c_dst):
    """(tile, offset) items of 15 / 16 / 17 / 63 / 64 / 65 / 80 entries and an empty one, under batch_groups 1 - 4 (one
    group per batch ... the 5 groups of 80 entries dealt 3 + 2), order NULL and permuted, both dispatch orders: the same
    bits from every plan and every kernel"""
    T, n_tgt, n_src = 128, 2 * 128 + 1, 300
    rng = np.random.default_rng(c_src)
    for order in (None, rng.permutation(n_tgt)):
        tbl = item_size_table(rng, T, n_tgt, n_src, order)

        def plans_of(case):
            plans = [Plan(case, T, bg, order) for bg in (4, 1, 2, 3)] + [Plan(case, T, 4, order, dispatch=1)]
            desc = plans[0].arrays[2].cpu().numpy()
            first_tile = desc[2 * int(plans[0].arrays[3][0]):2 * int(plans[0].arrays[3][1])].reshape(-1, 2)
            groups = [int((first_tile[first_tile[:, 1] >> 8 == k, 1] & 255).sum()) for k in range(len(ITEM_SIZES) + 1)]
            assert groups == [1, 1, 2, 4, 4, 5, 5, 0], groups
            sizes80 = sorted((first_tile[first_tile[:, 1] >> 8 == 6, 1] & 255).tolist())
            assert sizes80 == [2, 3], sizes80                       # 5 groups -> 3 + 2
            return plans
        both_pipes(device, tbl, n_src, c_src, c_dst, 10 + c_src, plans_of, f"items order={'perm' if order is not None else 'none'}")


def test_fused_launches_on_plans_of_small_batches(device, lib):
    """A fused super-batch holds up to four single-group batches and the stage buffer batch_groups groups: with
    batch_groups < 4 me_conv_target_bf16_fused (and the fp32-MFMA kernel's me_conv_target_f32_fused, which shares the
    scheme) lost the groups beyond the buffer and returned wrong sums.  Tables whose items are single groups (39-row tiles
    of a 30 % table; one row holding every entry: 27 single-entry items in a row), exact data: every launch must give the
    float64 sum exactly."""
    n_src = 150
    for kind, volume, n_tgt, T in (("random", 27, 3 * 39 + 5, 39), ("one_row", 27, 100, 64), ("random", 8, 200, 16)):
        tbl = make_table(np.random.default_rng(volume + T), kind, volume, n_tgt, n_src)
        for c_src, c_dst in ((8, 8), (32, 64), (96, 96)):
            case = exact_case(device, "bf16", tbl, n_src, c_src, c_dst, 5)
            check_bf16(case, [Plan(case, T, bg) for bg in (1, 2, 3, 4)], True, f"{kind} T={T} {c_src}->{c_dst}", BF16_KERNELS[:3])
            case = exact_case(device, "f32mfma", tbl, n_src, c_src, c_dst, 5)
            case.exact_precondition()
            for bg in (1, 2, 3, 4):
                plan = Plan(case, T, bg)
                for fused in (0, 1):
                    case.dst.fill()
                    fn = lib.me_conv_target_f32_fused if fused else lib.me_conv_target_f32
                    case.check(fn(case.src.data_ptr(), n_src, c_src, case.pack(0).ptr(), volume, c_dst, *plan.ptrs(),
                                  case.dst.ptr(), n_tgt, T, bg, None))
                    torch.cuda.synchronize()
                    assert case.intact() and plan.intact()
                    got = case.dst.as_dtype(torch.float32, (n_tgt, c_dst)).double().cpu().numpy()
                    bad = got != case.ref
                    assert not bad.any(), (f"fp32 MFMA {kind} T={T} bg={bg} fused={fused} {c_src}->{c_dst}: "
                                           f"{int(bad.sum())} of {bad.size} elements differ from the exact sum")


# ---- occupancy of the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_src", [("dense", 200), ("absent", 1), ("random", 200), ("last_offset", 200),
                                        ("first_offset", 200), ("one_row", 200), ("same_source", 200), ("random", 1),
                                        ("tail_last_col", 200)],
                         ids=["dense", "absent", "random", "last-offset-only", "offset-0-only", "one-row-holds-all",
                              "one-source-per-item", "n_src-1", "tail-last-column"])
def test_table_occupancy(device, lib, kind, n_src):
    """"absent": every row is still written, with +0; "n_src-1": every entry is source row 0, the row the padding slots
    gather as well; "one-source-per-item": one source row in all 16 slots of every group; "tail-last-column": what the
    slots beyond the last row compute must reach neither dst nor the partials"""
    T, n_tgt = 64, 2 * 64 + 37
    for volume, c_src, c_dst in ((27, 32, 64), (8, 64, 128)):
        tbl = make_table(np.random.default_rng(volume), kind, volume, n_tgt, n_src, T)
        out = both_pipes(device, tbl, n_src, c_src, c_dst, 300 + volume, lambda case: [Plan(case, T, 4), Plan(case, T, 2)],
                         f"{kind} K={volume}", exact_only=(volume == 8))
        if kind == "absent":
            assert not bool(int_view(out).any()), "no entry anywhere: +0 everywhere"
        else:
            assert bool((out.float() != 0).any())


# ---- row counts, tile heights, orders -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 39, 128, 131, 256])
def test_row_counts_on_the_tile_edges(device, lib, T):
    """n_tgt = 1, T - 1, T, T + 1, 2 T + 1 at tile heights 16 ... 256 (39 and 131: no multiple of the group), order NULL and
    a random permutation: the permuted launch stores the same rows (other tiles, the same sums on exact data)"""
    n_src, c_src, c_dst = 150, 32, 64
    for n_tgt in (1, T - 1, T, T + 1, 2 * T + 1):
        rng = np.random.default_rng(1000 * T + n_tgt)
        tbl = make_table(rng, "random", 8, n_tgt, n_src)
        perm = rng.permutation(n_tgt)
        plans_of = lambda case: [Plan(case, T, 4), Plan(case, T, 3, perm), Plan(case, T, 1, perm, multi=True)]   # noqa: E731
        both_pipes(device, tbl, n_src, c_src, c_dst, T + n_tgt, plans_of, f"n={n_tgt}", exact_only=(n_tgt not in (T + 1, 1)),
                   kernels=BF16_KERNELS[:3])


def test_tile_heights_out_of_range_are_refused(device, lib):
    tbl = make_table(np.random.default_rng(3), "random", 8, 100, 50)
    for pipe in ("bf16", "f32"):
        case = random_case(device, pipe, tbl, 50, 32, 64, 5)
        good = Plan(case, 64, 4)
        for T in (15, 257):
            assert Plan(case, T, 4, expect_error=True).rc != 0, f"me_plan_build took tile_rows {T}"
            call = call_bf16 if pipe == "bf16" else call_f32x3
            assert call(case, good, T=T) != 0 and case.dst.untouched() and case.intact(), (pipe, T)
            assert case.lib.me_last_error()


# ---- volumes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", [1, 2, 8, 27, 125])
def test_volumes(device, lib, volume):
    n_tgt, n_src = 150, 100
    tbl = make_table(np.random.default_rng(volume), "random", volume, n_tgt, n_src)
    both_pipes(device, tbl, n_src, 32, 64, 40 + volume, lambda case: [Plan(case, 64, 4), Plan(case, 39, 2)], f"K={volume}",
               kernels=BF16_KERNELS[:3])


def test_largest_volume_and_one_more(device, lib):
    """volume 65535 is the largest the plan and the launches take (me_plan_build: "kernel volume out of range"; a batch
    descriptor holds the offset above 8 bits of group count); 65536 is refused by return code.  A sparse table: the first,
    the last and a few hundred offsets in between hold entries."""
    volume, n_tgt, n_src = 65535, 40, 30
    rng = np.random.default_rng(9)
    tbl = np.full((volume, n_tgt), -1, np.int32)
    ks = np.unique(np.concatenate([[0, 1, 255, 256, 257, 32767, 32768, volume - 2, volume - 1], rng.integers(0, volume, 300)]))
    for k in ks:
        m = rng.random(n_tgt) < 0.4
        tbl[k, m] = rng.integers(0, n_src, int(m.sum()))
    tbl[volume - 1, n_tgt - 1] = n_src - 1
    both_pipes(device, tbl, n_src, 8, 8, 77, lambda case: [Plan(case, 16, 4)], f"K={volume}", exact_only=True,
               kernels=BF16_KERNELS[:2])
    small = Case(device, np.full((2, n_tgt), -1, np.int32), torch.zeros(n_src, 8), torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), "bf16")
    small.volume = volume + 1                        # only the argument check may look at it
    assert Plan(small, 16, 4, expect_error=True).rc != 0


# ---- channels -----------------------------------------------------------------------------------------------------------------
CHANNELS = [(8, 8), (32, 24), (40, 32), (96, 32), (128, 8), (8, 40), (64, 64), (96, 96), (72, 136), (192, 128), (128, 96),
            (32, 128), (64, 128), (128, 256), (256, 256), (256, 128), (72, 128), (96, 128), (128, 64), (96, 64), (32, 96)]
# (slab width, chunk depth) the shipped dispatch reaches, from conv_variant_bf16 and conv_variant_f32x3
BF16_SHAPES = {(32, 32), (32, 64), (32, 96), (32, 128), (64, 32), (64, 64), (64, 96), (64, 128), (128, 32), (128, 64),
               (128, 128), (128, 256)}
X3_SHAPES = {(32, 32), (32, 64), (32, 96), (32, 128), (64, 32), (64, 64), (64, 96), (64, 128), (96, 32), (96, 64), (96, 96),
             (128, 32), (128, 64), (128, 96)}


def _shape_bf16(c_src, c_dst):
    """conv_variant_bf16 of the shipped policy"""
    kc = 128 if c_src % 128 == 0 else 96 if c_src % 96 == 0 else 32 if c_src <= 32 else 64 if c_src <= 64 else 128
    nc = 32 if c_dst <= 32 else 64
    if c_dst % 128 == 0 and kc != 96:
        nc = 128
    if nc == 128 and c_src % 256 == 0 and c_dst <= 256:
        kc = 256
    return nc, kc


def _shape_f32x3(c_src, c_dst):
    nc = 128 if c_dst % 128 == 0 else 96 if c_dst % 96 == 0 else 32 if c_dst <= 32 else 64
    kc = (128 if c_src % 128 == 0 and nc <= 64 else 64 if c_src % 64 == 0 else 96 if c_src % 96 == 0 else
          32 if c_src <= 32 else 64)
    return nc, kc


def test_channel_list_reaches_every_shipped_shape():
    """(host only) every (slab width, chunk depth) of both dispatches, source channels that are no multiple of the chunk,
    output channels that are no multiple of 16, and the chunk depth the library reports for each"""
    _, lib = _lib()
    assert {_shape_bf16(*c) for c in CHANNELS} == BF16_SHAPES
    assert {_shape_f32x3(*c) for c in CHANNELS} == X3_SHAPES
    for c_src, c_dst in CHANNELS:
        assert int(lib.me_conv_pack_chunk_bf16(c_src, c_dst)) == _shape_bf16(c_src, c_dst)[1], (c_src, c_dst)
        assert int(lib.me_conv_pack_chunk_f32x3(c_src, c_dst)) == _shape_f32x3(c_src, c_dst)[1], (c_src, c_dst)
    assert {c for c, _ in CHANNELS} >= {8, 32, 40, 64, 72, 96, 128, 192, 256}
    assert {c for _, c in CHANNELS} >= {8, 24, 32, 40, 64, 96, 128, 136, 256}
    assert any(s % _shape_bf16(s, d)[1] for s, d in CHANNELS) and any(d % 16 for _, d in CHANNELS)


@pytest.mark.parametrize("c_src,c_dst", CHANNELS)
def test_channels(device, lib, c_src, c_dst):
    """every shipped instantiation, with a partial last tile and padded groups; the transposed weight form ([K, c_dst,
    c_src], the input gradient's) packs to the same image"""
    n_tgt, n_src, volume = 150, 90, 8
    tbl = make_table(np.random.default_rng(c_src + c_dst), "random", volume, n_tgt, n_src)
    plans_of = lambda case: [Plan(case, 64, 4), Plan(case, 48, 2)]   # noqa: E731
    both_pipes(device, tbl, n_src, c_src, c_dst, c_src * 300 + c_dst, plans_of, f"{c_src}->{c_dst}")
    for pipe in ("bf16", "f32"):
        case = random_case(device, pipe, tbl, n_src, c_src, c_dst, 5)
        assert torch.equal(case.pack(0).bits, case.pack(1).bits), f"{pipe}: the transposed form packs another image"
        if c_src != c_dst:
            # ... and is not ignored: the same bytes read as [K, c_src, c_dst] are another kernel
            w = case.w_fed.permute(0, 2, 1).contiguous().reshape(case.w_fed.shape)
            other = Case(device, tbl, case.x_host, w, w, pipe)
            assert not torch.equal(other.pack(0).bits, case.pack(0).bits)


def test_forced_kernel_shapes(device, lib):
    """me_debug_set_bf16_shape: the instantiations the policy does not choose (128 columns on 96-channel chunks, narrow
    chunks under wide rows) give the bits of the policy's kernel on exact data"""
    n_tgt, n_src = 150, 90
    tbl = make_table(np.random.default_rng(1), "random", 8, n_tgt, n_src)
    for (c_src, c_dst), shapes in (((96, 128), [(0, 0), (128, 96), (64, 32)]), ((64, 64), [(0, 0), (64, 32), (32, 64)]),
                                   ((256, 128), [(0, 0), (128, 128), (128, 64), (64, 128)])):
        outs = []
        for nc, kc in shapes:
            lib.me_debug_set_bf16_shape(nc, kc)
            case = exact_case(device, "bf16", tbl, n_src, c_src, c_dst, 21)
            outs.append(check_bf16(case, [Plan(case, 64, 4)], True, f"{c_src}->{c_dst} shape=({nc},{kc})", BF16_KERNELS[:3]))
            lib.me_debug_set_bf16_shape(0, 0)
        assert all(_same_bits(o, outs[0]) for o in outs)


def test_shapes_of_the_tuning_build(device, lib):
    """96-column slabs (no statistics epilogue: refused) and the offset-synchronous schedule exist in a tuning build only"""
    if not lib.me_debug_variants_compiled():
        pytest.skip("96-column slabs and the offset-synchronous kernel are " + DEBUG_BUILD_ONLY)
    tbl = make_table(np.random.default_rng(1), "random", 8, 150, 90)
    lib.me_debug_set_bf16_shape(96, 32)
    case = exact_case(device, "bf16", tbl, 90, 32, 96, 21)
    plan = Plan(case, 64, 4)
    assert lib.me_conv_stats_supported_bf16(32, 96) == 0
    assert call_bf16(case, plan, stats=True) != 0 and case.dst.untouched() and all(p.untouched() for p in plan.parts)
    check_bf16(case, [plan], True, "96 columns", BF16_KERNELS[:1], stats=False)
    lib.me_debug_set_bf16_shape(0, 0)
    lib.me_debug_set_bf16_offsync(1)
    case = exact_case(device, "bf16", tbl, 90, 64, 64, 22)
    check_bf16(case, [Plan(case, 64, 4)], True, "offset-synchronous", BF16_KERNELS[:1])


def test_source_channels_the_split_kernel_refuses(device, lib):
    """c_src = 12 is no multiple of 8: me_conv_f32x3_supported says so, the launch is refused, dst stays untouched"""
    assert lib.me_conv_f32x3_supported(12, 16) == 0 and lib.me_conv_f32x3_supported(8, 16) == 1
    tbl = make_table(np.random.default_rng(1), "random", 8, 100, 50)
    case = random_case(device, "f32", tbl, 50, 12, 16, 3)
    plan = Plan(case, 64, 4)
    assert call_f32x3(case, plan) != 0 and case.dst.untouched() and case.intact()


# ---- the second exact set of the split kernel ---------------------------------------------------------------------------------
def test_f32x3_exact_with_all_three_planes(device, lib):
    """features of 17 significant bits — +-(2^16 + 2^8 + 1 + more): the second and third bf16 plane of the split are both
    non-zero — in two channels per row, weights +-2^e with e in {-2, -1, 0}: every product is a multiple of 2^-2 below
    2^17, every partial sum of a target row exact in fp32 (precondition sum|products| 2^2 < 2^24, asserted); the result
    must be the float64 sum exactly.  A kernel that dropped a plane would be off by 2^-8 or 2^-16 relative."""
    n_tgt, n_src, volume = 150, 90, 8
    rng = np.random.default_rng(4)
    tbl = make_table(rng, "random", volume, n_tgt, n_src)
    for c_src, c_dst in ((32, 64), (64, 128), (96, 96), (128, 32)):
        m = (2 ** 16 + 2 ** 8 + 1 + (rng.integers(0, 2 ** 15, size=(n_src, 2)) & ~0x101)) * rng.choice([-1, 1], size=(n_src, 2))
        x = np.zeros((n_src, c_src), np.float32)
        cols = np.stack([rng.choice(c_src, 2, replace=False) for _ in range(n_src)])
        x[np.arange(n_src)[:, None], cols] = m
        xt = torch.from_numpy(x)
        a1 = xt.view(torch.int32).bitwise_and(-65536).view(torch.float32)
        r = xt - a1
        a2 = r.view(torch.int32).bitwise_and(-65536).view(torch.float32)
        nz = xt != 0
        assert bool((a2[nz] != 0).all()) and bool(((r - a2)[nz] != 0).all()), "planes 2 and 3 must be non-zero"
        w = np.ldexp(rng.choice([-1.0, 1.0], size=(volume, c_src, c_dst)), rng.integers(-2, 1, size=(volume, c_src, c_dst)))
        wt = torch.from_numpy(w.astype(np.float32))
        case = Case(device, tbl, xt, wt, wt, "f32")
        case.exact_precondition(scale=4.0)
        check_f32x3(case, [Plan(case, 64, 4), Plan(case, 39, 1)], True, f"three planes {c_src}->{c_dst}")


# ---- poisoned rows behind the padding ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["row0", "last_row"])
def test_poisoned_rows_that_no_entry_names(device, lib, which):
    """padding slots gather source row 0 into the dummy accumulator row; index windows and clamped loads may touch the last
    row.  With no entry naming the row, NaN or +Inf there must give, bit for bit, the result of zeros there — in dst, in
    the partials, through split-K (0 x finite = 0 would hide a missing mask)"""
    n_tgt, n_src, volume, T = 2 * 64 + 21, 120, 8, 64
    rng = np.random.default_rng(7)
    tbl = make_table(rng, "random", volume, n_tgt, n_src, first_row=1, last_row=n_src - 1)
    tbl[:, T:T + 8] = -1                                # rows without any entry inside a tile
    tbl[3, :T] = -1
    tbl[3, rng.choice(T, 17, replace=False)] = rng.integers(1, n_src - 1, 17)      # a group with 15 padding slots
    row = 0 if which == "row0" else n_src - 1
    assert not (tbl == row).any() and (tbl >= 0).any()
    for pipe, (c_src, c_dst) in (("bf16", (64, 128)), ("bf16", (32, 64)), ("f32", (64, 128)), ("f32", (32, 24))):
        base = exact_case(device, pipe, tbl, n_src, c_src, c_dst, 31)
        outs, parts_seen = {}, {}
        for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
            x = base.x_host.clone()
            x[row] = fill
            case = Case(device, tbl, x, base.w_fed, base.w_used, pipe)
            assert np.isfinite(case.ref).all()
            plans = [Plan(case, T, 4), Plan(case, T, 1, rng.permutation(n_tgt))]
            if pipe == "bf16":
                outs[name] = check_bf16(case, plans, True, f"{which}={name} {c_src}->{c_dst}")
                _switches(lib, ws=0)
                parts_seen[name] = run_bf16(case, plans[0], name, stats=True)[1]
                if c_dst == 128:
                    for g in (2, 4):
                        out, parts = run_bf16(case, plans[0], f"{which}={name} split_k={g}", split_k=g, stats=True)
                        assert torch.equal(int_view(out).cpu(), case.exact_bits_bf16()), f"{which}={name} split_k={g}"
                        check_partials(case, plans[0], out, parts, f"{which}={name} split_k={g}")
                _switches(lib)
            else:
                outs[name] = check_f32x3(case, plans, True, f"{which}={name} {c_src}->{c_dst}")
        assert _same_bits(outs["nan"], outs["zero"]) and _same_bits(outs["inf"], outs["zero"])
        for name in parts_seen:
            assert all(np.array_equal(a, b) for a, b in zip(parts_seen[name], parts_seen["zero"]))


# ---- non-finite rows that are named -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["bf16", "f32"])
def test_non_finite_rows_propagate_as_in_fp32(device, lib, pipe):
    """source rows with +Inf, -Inf and NaN in one channel, named from padded groups (an item of 17 entries), from every
    group of a full batch (an item of 64), from the last batch of the tile (the last offset) and met by the opposite
    infinity in one sum.  Where the float64 oracle gives NaN / +Inf / -Inf so does the kernel — the row-side rule of
    conv_common.hpp: a non-finite feature times a weight is what fp32 arithmetic makes of it — and everything else is
    finite and (exact data) exact."""
    n_tgt, n_src, volume, T = 2 * 64 + 21, 120, 8, 64
    inf = float("inf")
    for c_src, c_dst in ((64, 128), (32, 64), (40, 24)):
        rng = np.random.default_rng(c_src)
        tbl = make_table(rng, "random", volume, n_tgt, n_src, first_row=4)
        tbl[0, :T] = -1
        tbl[0, rng.choice(T, 17, replace=False)] = rng.integers(4, n_src, 17)
        tbl[1, :T] = rng.integers(4, n_src, T)
        for k in (0, 1, volume - 1):                   # every fifth entry of those items names a special row
            present = np.flatnonzero(tbl[k, :T] >= 0)
            tbl[k, present[::5]] = 1 + (np.arange(len(present[::5])) % 3)
        tbl[volume - 1, n_tgt - 1] = 1                 # the last row of the partial tile, at the last offset
        both = np.flatnonzero(tbl[0, :T] == 1)[0]      # +Inf at offset 0 and -Inf at offset 2 in one sum
        tbl[2, both] = 2
        base = exact_case(device, pipe, tbl, n_src, c_src, c_dst, 61)
        x = base.x_host.clone()
        x[1, 2], x[2, 2], x[3, 0] = inf, -inf, float("nan")
        w_fed = base.w_fed.clone()
        w_fed[:, :, :4] = w_fed[:, :, :4].abs() + 0.25     # columns that keep the sign of the infinity ...
        w_fed[:, :, 4:8] = 0.0                             # ... and columns of 0 x Inf = NaN
        w_used = bf16_round(w_fed)
        case = Case(device, tbl, x, w_fed if pipe == "bf16" else w_used, w_used, pipe)
        ref = case.ref
        assert np.isnan(ref[both, :4]).all() and np.isposinf(ref).any() and np.isneginf(ref).any()
        assert np.isnan(ref[:, 4:8]).any() and np.isfinite(ref).mean() > 0.3
        case.exact_precondition()
        fin = np.isfinite(ref)
        first = None
        for plan in (Plan(case, T, 4), Plan(case, T, 1), Plan(case, 39, 3, rng.permutation(n_tgt))):
            for name, sw in (BF16_KERNELS if pipe == "bf16" else X3_KERNELS):
                what = f"{pipe} {c_src}->{c_dst} T={plan.T} bg={plan.bg} {name}"
                if pipe == "bf16":
                    out = run_bf16(case, plan, what, entry="plain", fused=_switches(lib, **sw))[0]
                else:
                    assert lib.me_debug_set_conv_variant(sw) == 0
                    out = run_f32x3(case, plan, what)
                got = out.double().cpu().numpy()
                same_nonfinite_class(got, ref, what)
                want = torch.from_numpy(ref).to(out.dtype).double().numpy()
                assert np.array_equal(got[fin], want[fin]), f"{what}: finite elements differ from the exact result"
                if first is None:
                    first = out
                assert torch.equal(torch.isnan(out), torch.isnan(first)) and _same_bits(out.nan_to_num(0.0), first.nan_to_num(0.0)), what
        _switches(lib)
        assert case.intact()


def test_non_finite_weight_gives_nan_in_the_split_kernel(device, lib):
    """the one divergence from fp32 arithmetic the header documents: an infinite WEIGHT makes every output it reaches NaN
    (fp32 would keep the sign); no other output changes"""
    n_tgt, n_src = 150, 90
    tbl = make_table(np.random.default_rng(2), "random", 8, n_tgt, n_src)
    base = exact_case(device, "f32", tbl, n_src, 32, 64, 8)
    w = base.w_fed.clone()
    w[5, 6, 9] = float("inf")
    case = Case(device, tbl, base.x_host.abs() + 1.0, w, w, "f32")
    out = run_f32x3(case, Plan(case, 64, 4)).double().cpu().numpy()
    reached = tbl[5] >= 0
    assert reached.any() and np.isnan(out[reached, 9]).all() and np.isposinf(case.ref[reached, 9]).all()
    rest = np.ones_like(out, bool)
    rest[reached, 9] = False
    assert np.array_equal(out[rest], case.ref[rest])


# ---- the statistics partials --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_src,c_dst", [(32, 24), (32, 64), (64, 40), (72, 136), (64, 128), (256, 256)])
def test_statistics_partials(device, lib, c_src, c_dst):
    """part_mean / part_m2 against the float64 mean / M2 of the bf16 values actually stored, within the fp32 bound derived
    at helpers.assert_tile_partials: 32-, 64- and 128-column slabs (the last slab partial for 24, 40, 136 columns), tiles
    whose rows are all empty (exact zeros), a constant tile (M2 == 0 exactly), partial last tiles of 1 and 5 rows, fused on
    and off, the wave-specialised kernel, a permuted order, split-K (the reduce kernel forms them)"""
    n_src, volume = 100, 8
    for T, n_tgt in ((64, 4 * 64 + 1), (39, 4 * 39 + 5)):
        rng = np.random.default_rng(n_tgt + c_dst)
        tbl = make_table(rng, "random", volume, n_tgt, n_src)
        tbl[:, T:2 * T] = -1                               # tile 1: no entry at all
        tbl[:, 2 * T:3 * T] = -1
        tbl[3, 2 * T:3 * T] = 17                           # tile 2: every row sees the same neighbour
        case = random_case(device, "bf16", tbl, n_src, c_src, c_dst, n_tgt)
        for order in (None, rng.permutation(n_tgt)):
            plan = Plan(case, T, 4, order)
            first = None
            for name, sw in BF16_KERNELS[:3]:
                what = f"{c_src}->{c_dst} T={T} {name} order={'perm' if order is not None else 'none'}"
                fused = _switches(lib, **sw)
                for entry in ("ex", "stats"):
                    out, parts = run_bf16(case, plan, what, entry=entry, fused=fused, stats=True)
                    assert_bf16_close(out.float().cpu().numpy(), case.ref, what)
                    check_partials(case, plan, out, parts, what)
                    if first is None:
                        first = (out, parts)
                    assert _same_bits(out, first[0]), what
                if order is None:
                    o = out.float()
                    mean, m2 = parts
                    assert not mean[1].any() and not m2[1].any(), f"{what}: a tile of empty rows"
                    assert bool((o[2 * T:3 * T] == o[2 * T]).all()) and bool((o[2 * T] != 0).any())
                    assert np.array_equal(mean[2], o[2 * T].double().cpu().numpy()) and not m2[2].any(), f"{what}: a constant tile"
                    if n_tgt % T == 1:
                        assert np.array_equal(mean[-1], o[-1].double().cpu().numpy()) and not m2[-1].any(), f"{what}: a tile of one row"
                    else:
                        tail = o[n_tgt // T * T:].cpu().numpy()
                        assert (tail != tail[0]).any(), "the partial tile must hold different rows"
            if c_dst % 128 == 0:
                _switches(lib, ws=0)
                for g in (2, 4):
                    what = f"{c_src}->{c_dst} T={T} split_k={g}"
                    out, parts = run_bf16(case, plan, what, split_k=g, stats=True)
                    assert_bf16_close(out.float().cpu().numpy(), case.ref, what)
                    check_partials(case, plan, out, parts, what)
        _switches(lib)


# ---- split-K ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_src,c_dst", [(64, 128), (128, 128), (256, 256), (128, 256)])
def test_split_k_against_the_oracle(device, lib, c_src, c_dst):
    """G = 2, 4 (and 3, 8) offset groups through the fp32 workspace and the reduce kernel: compared with the oracle only
    (the header: not the bits of the unsplit launch) — bit for bit on exact data; volumes that G does not divide, a volume
    below G (the launch then runs unsplit), a partial last tile, a permuted order, the workspace NaN before the launch"""
    n_src = 100
    for volume, n_tgt, T in ((27, 2 * 64 + 21, 64), (8, 3 * 39 + 1, 39), (3, 70, 48)):
        rng = np.random.default_rng(volume + c_src)
        tbl = make_table(rng, "random", volume, n_tgt, n_src)
        exact = exact_case(device, "bf16", tbl, n_src, c_src, c_dst, volume)
        rnd = random_case(device, "bf16", tbl, n_src, c_src, c_dst, volume + 1)
        for case in (exact, rnd):
            for order in (None, rng.permutation(n_tgt)):
                plan = Plan(case, T, 4, order)
                for g in (2, 4, 3, 8):
                    for twobuf in ((-1, 1) if g == 2 else (-1,)):
                        what = f"{c_src}->{c_dst} K={volume} split_k={g} twobuf={twobuf}"
                        _switches(lib, ws=0, twobuf=twobuf)
                        out, _ = run_bf16(case, plan, what, split_k=g)
                        if case is exact:
                            assert torch.equal(int_view(out).cpu(), case.exact_bits_bf16()), what
                        else:
                            assert_bf16_close(out.float().cpu().numpy(), case.ref, what)
    _switches(lib)
    # the policy switch: me_conv_plan_config_bf16_ex answers the forced group count with taller tiles
    T, bg, sk = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for g in (2, 4):
        lib.me_debug_set_bf16_splitk(g)
        assert lib.me_conv_plan_config_bf16_ex(1000, 27, 8000, c_src, c_dst, ctypes.byref(T), ctypes.byref(bg), ctypes.byref(sk)) == 0
        assert sk.value in (1, g) and 16 <= T.value <= 256 and 1 <= bg.value <= 4
    lib.me_debug_set_bf16_splitk(0)
    assert lib.me_conv_plan_config_bf16_ex(1000, 27, 8000, c_src, c_dst, ctypes.byref(T), ctypes.byref(bg), ctypes.byref(sk)) == 0
    assert sk.value == 1


# ---- me_plan_build_multi ------------------------------------------------------------------------------------------------------
def test_plan_build_multi_feeds_the_kernels_identically(device, lib):
    T, n_tgt, n_src = 128, 2 * 128 + 1, 300
    rng = np.random.default_rng(12)
    order = rng.permutation(n_tgt)
    tbl = item_size_table(rng, T, n_tgt, n_src, order)
    for pipe in ("bf16", "f32"):
        case = random_case(device, pipe, tbl, n_src, 64, 128, 3)
        single, multi = Plan(case, T, 3, order), Plan(case, T, 3, order, multi=True)
        for a, b, name in zip(single.arrays[:3], multi.arrays[:3], ("plan_src", "plan_dst", "batch_desc")):
            assert torch.equal(a, b), name
        assert torch.equal(single.arrays[3][:single.tiles + 1], multi.arrays[3][:single.tiles + 1])
        assert torch.equal(single.arrays[4], multi.arrays[4])
        if pipe == "bf16":
            a, pa = run_bf16(case, single, "single", stats=True)
            b, pb = run_bf16(case, multi, "multi", stats=True)
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        else:
            a, b = run_f32x3(case, single, "single"), run_f32x3(case, multi, "multi")
        assert _same_bits(a, b)


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_dst_untouched(device, lib):
    tbl = make_table(np.random.default_rng(1), "random", 8, 150, 90)
    case = random_case(device, "bf16", tbl, 90, 64, 128, 1)
    plan = Plan(case, 64, 4)
    _switches(lib, ws=0)
    src, dst, wp = case.src.data_ptr(), case.dst.ptr(), case.pack(0).ptr()
    bad = {
        "source pointer off by 2 bytes": dict(src=src + 2),
        "dst pointer off by 8 bytes": dict(dst=dst + 8),
        "packed weights off by 8 bytes": dict(wp=wp + 8),
        "batch_groups 0": dict(bg=0),
        "batch_groups 5": dict(bg=5),
        "split_k 0": dict(split_k=0),
        "split_k 9": dict(split_k=9),
        "split-K without workspace": dict(split_k=2, workspace=None),
        "part_mean alone": dict(stats=True, m2=None),
        "part_m2 alone": dict(stats=True, mean=None),
    }
    for name, over in bad.items():
        assert call_bf16(case, plan, **over) != 0, name
        assert case.dst.untouched() and all(p.untouched() for p in plan.parts), f"{name}: refused, yet something was written"
        assert case.intact() and plan.intact() and lib.me_last_error(), name
    assert call_bf16(case, plan, entry="stats", stats=True, m2=None) != 0 and case.dst.untouched()
    # every shipped slab width has the epilogue: no channel count is refused for the statistics
    assert all(lib.me_conv_stats_supported_bf16(s, d) == 1 for s, d in CHANNELS)
    # ... and the same arguments, unchanged, run
    out, parts = run_bf16(case, plan, "good arguments", split_k=2, stats=True)
    assert_bf16_close(out.float().cpu().numpy(), case.ref, "good arguments")
    # the split kernel's checks
    case = random_case(device, "f32", tbl, 90, 64, 128, 1)
    plan = Plan(case, 64, 4)
    src, dst, wp = case.src.data_ptr(), case.dst.ptr(), case.pack(0).ptr()
    for name, over in {"source pointer off by 4 bytes": dict(src=src + 4), "dst pointer off by 8 bytes": dict(dst=dst + 8),
                       "packed weights off by 8 bytes": dict(wp=wp + 8), "batch_groups 0": dict(bg=0),
                       "batch_groups 5": dict(bg=5)}.items():
        assert call_f32x3(case, plan, **over) != 0, name
        assert case.dst.untouched() and case.intact() and plan.intact() and lib.me_last_error(), name
    out = run_f32x3(case, plan, "good arguments").double().cpu().numpy()
    assert (np.abs(out - case.ref) <= 2e-6 * case.mag).all()
