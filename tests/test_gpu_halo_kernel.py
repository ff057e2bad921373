"""The halo convolution launch itself (csrc/conv_halo.hip: k_halo_plan<N>, k_conv_halo_bf16) on synthetic neighbour
tables, through the C ABI, on the library as it ships: a table tbl [volume, n_tgt] (source row of (offset, column), -1:
none) -> me_halo_plan_build -> me_conv_pack_weights_bf16 -> me_conv_halo_bf16:
    dst[out_order[p]] = sum over offsets k of src[tbl[k][col_order[p]]] @ W[k]      for every tile position p < n_tgt,
the tiles being T consecutive positions (a NULL order: the identity; no entry: zeros).

tests/test_gpu_halo.py drives the kernel through whole layers, mostly in the forced mode of a -DME_DEBUG_VARIANTS build.
Here nothing is forced: in auto mode (me_debug_halo_mode() == -1, ME_AMD_HALO unset) me_conv_halo_bf16 takes the three
channel shapes of the policy — 192 -> 128, 256 -> 384 (three 128-column slabs, four 64-channel chunks), 64 -> 32 (64-row
tiles, four row waves, no group masks) — at any volume in [2, 32], and the subject is what the hand-scheduled walk rests
on: tiles with an empty halo, waves without any neighbour beside active ones, walks of 0 ... 5 offsets (the unroll
boundaries of the two-weight-set loop and the surplus request behind the last offset), offset 31 of 32, halos of
s_cap - 1 / s_cap / s_cap + 1 / 3 s_cap rows (staged image against direct gather, mixed in one launch), single row
groups per offset, col_order != out_order, row counts on the tile edges, the statistics epilogue, every instantiation
of the plan kernel, the argument checks.

Oracle: Case.ref of test_gpu_conv_tile_kernels.py — numpy float64 on the bf16-rounded operands, in table-column space;
the orders are applied on the host (expected()).  EXACT data (integer features in [-8, 8], weights that round to
multiples of 2^-6 in [-2, 2]; precondition sum|products| 2^6 < 2^24 asserted, largest case here 32 offsets x 256
channels x 8 x 2 x 64 = 8.4 M) make every fp32 partial sum exact in any order: the bf16 dst must equal the bf16 rounding
of the float64 sum BIT FOR BIT, on the staged path and on the direct path, which associate differently.  RANDOM data:
assert_bf16_close; partials: assert_tile_partials.  The plan arrays are compared bit for bit with numpy_halo_plan.  Every
buffer is a view into the middle of a larger tensor (helpers.middle / Guarded)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from helpers import GUARD_PAD, Guarded, assert_tile_partials, int_view, middle, same_nonfinite_class
from test_gpu_bf16 import assert_bf16_close
from test_gpu_conv_tile_kernels import Case, Plan, call_bf16, exact_case, make_table, random_case
from test_gpu_halo import numpy_halo_plan

pytestmark = pytest.mark.gpu

SHAPES = [(192, 128), (256, 384), (64, 32)]
CONFIG = {(192, 128): (128, 383), (256, 384): (128, 383), (64, 32): (64, 319)}     # (tile_rows, s_cap) of the policy
ROW_WAVES = {128: 2, 64: 4}                     # waves along the rows of a tile: 2 x 2 waves on 128 rows, 4 x 1 on 64
shapes = pytest.mark.parametrize("shape", SHAPES, ids=[f"{s}to{d}" for s, d in SHAPES])
PATTERN16, PATTERN32 = 0x5a5a, 0x5a5a5a5a       # around and (before the build) inside lidx, kmask and halo_cnt
WINDOW = 300                                    # source rows of the tables whose halos fit: below both capacities
FAR = 1500                                      # source rows of the tables that overflow


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def config(shape, volume=27):
    """(tile_rows, s_cap) from me_conv_halo_config_bf16; a forced variant fails here"""
    _, lib = _lib()
    t, cap = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.me_debug_halo_mode() == -1, "a halo variant is forced: these tests are about the policy's kernels"
    assert lib.me_conv_halo_config_bf16(1000, volume, 8000, shape[0], shape[1], ctypes.byref(t), ctypes.byref(cap)) == 1
    assert (t.value, cap.value) == CONFIG[shape], f"{shape}: config {(t.value, cap.value)} (ME_AMD_HALO set?)"
    return t.value, cap.value


# ---- data -------------------------------------------------------------------------------------------------------------------
_EXACT = {}


def exact_data(device, volume, n_src, shape):
    """(features, weights fed, weights rounded) of exact_case, drawn once per (volume, n_src, shape)"""
    key = (volume, n_src, shape)
    if key not in _EXACT:
        b = exact_case(device, "bf16", np.full((volume, 1), -1, np.int32), n_src, shape[0], shape[1], 50 + len(_EXACT))
        _EXACT[key] = (b.x_host, b.w_fed, b.w_used)
    return _EXACT[key]


def exact(device, tbl, n_src, shape, x=None):
    """exact data on the table `tbl`; x: other features under the same weights"""
    x0, fed, used = exact_data(device, tbl.shape[0], n_src, shape)
    return Case(device, tbl, x0 if x is None else x, fed, used, "bf16")


def inverse(perm):
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


# ---- the plan ---------------------------------------------------------------------------------------------------------------
class HaloPlan:
    """me_halo_plan_build of a case's table (col_order: tile position -> table column; src_perm: source row -> slot
    position, with its inverse).  The arrays sit in guard tensors: the source row n_src (NaN) around and inside
    halo_rows, a pattern around and inside the others; compared bit for bit with numpy_halo_plan."""

    def __init__(self, case, tile_rows, s_cap, col_order=None, src_perm=None, expect_error=False):
        L, lib = _lib()
        self.case, self.T, self.s_cap = case, tile_rows, s_cap
        dev, n_tgt, volume, n_src = case.device, case.n_tgt, case.volume, case.n_src
        self.tiles = -(-n_tgt // tile_rows)
        assert int(lib.me_halo_plan_num_tiles(n_tgt, tile_rows)) == self.tiles
        self.col_host = None if col_order is None else np.asarray(col_order, np.int64)
        self.pos_host = None if src_perm is None else np.asarray(src_perm, np.int64)
        self.inputs = []
        self.col = self.index_array(self.col_host, n_tgt)          # a stray read: column n_tgt
        self.src_pos = self.index_array(self.pos_host, n_src)      # a stray read: position n_src -> (guard) row n_src
        self.src_order = self.index_array(None if src_perm is None else inverse(self.pos_host), n_src)
        sizes = [self.tiles, self.tiles * s_cap, self.tiles * volume * tile_rows, self.tiles * volume]
        dtypes = [torch.int32, torch.int32, torch.int16, torch.int32]
        self.fills = [PATTERN32, n_src, PATTERN16, PATTERN32]
        self.bigs, self.arrays = zip(*[middle(n, dt, dev, f) for n, dt, f in zip(sizes, dtypes, self.fills)])
        self.parts = None
        self.rc = lib.me_halo_plan_build(case.tbl.data_ptr(), *[None if a is None else a.data_ptr() for a in
                                                                (self.col, self.src_pos, self.src_order)],
                                         n_tgt, volume, tile_rows, s_cap, *[a.data_ptr() for a in self.arrays], None)
        torch.cuda.synchronize()
        for b, a, f in zip(self.bigs, self.arrays, self.fills):
            assert bool((b[:GUARD_PAD] == f).all()) and bool((b[GUARD_PAD + a.numel():] == f).all()), \
                "the plan build wrote outside its arrays"
        if expect_error:
            assert all(bool((a == f).all()) for a, f in zip(self.arrays, self.fills)), "refused, yet something was written"
            return
        L.check(self.rc)
        cnt, rows, lidx, kmask = [a.cpu().numpy() for a in self.arrays]
        r_cnt, r_rows, r_lidx, r_kmask = numpy_halo_plan(case.tbl_host, self.col_host, n_tgt, tile_rows, s_cap, self.pos_host)
        assert np.array_equal(cnt, r_cnt), "halo_cnt"
        assert np.array_equal(rows.reshape(self.tiles, s_cap), np.where(r_rows < 0, n_src, r_rows)), "halo_rows"
        assert np.array_equal(lidx.view(np.uint16).reshape(r_lidx.shape), r_lidx), "lidx"
        assert np.array_equal(kmask.view(np.uint32).reshape(r_kmask.shape), r_kmask), "kmask"
        self.cnt, self.lidx, self.kmask = r_cnt, r_lidx, r_kmask
        self.before = [b.clone() for b in self.bigs]

    def index_array(self, host, fill):
        """an int32 index array of the launch in a guard tensor of `fill`; None stays None"""
        if host is None:
            return None
        big, view = middle(len(host), torch.int32, self.case.device, fill)
        view.copy_(torch.from_numpy(np.asarray(host).astype(np.int32)))
        self.inputs.append((big, big.clone()))
        return view

    def partials(self):
        if self.parts is None:
            self.parts = [Guarded(self.tiles * self.case.c_dst, 4, self.case.device, base=1000 * (i + 1)) for i in range(2)]
        return self.parts

    def intact(self):
        return (all(torch.equal(a, b) for a, b in zip(self.bigs, self.before)) and
                all(torch.equal(a, b) for a, b in self.inputs) and all(p.intact() for p in self.partials()))

    def overflowing(self):
        return self.cnt > self.s_cap


def table_only(device, tbl, n_src):
    """what HaloPlan needs of a case, for the plan build alone"""
    big, view = middle(tbl.size, torch.int32, device, n_src)
    view.copy_(torch.from_numpy(np.ascontiguousarray(tbl)).reshape(-1))
    return types.SimpleNamespace(device=device, tbl=view, tbl_big=big, tbl_host=tbl, n_src=n_src, volume=tbl.shape[0],
                                 n_tgt=tbl.shape[1], c_dst=0)


# ---- the launch -------------------------------------------------------------------------------------------------------------
def call_halo(case, plan, stats=False, transposed=0, out_order=None, **over):
    """one launch; dst and the partials hold NaN before it.  Returns the return code."""
    lib = case.lib
    case.dst.fill()
    parts = plan.partials()
    for p in parts:
        p.fill()
    oo = plan.index_array(out_order, case.n_tgt)                   # a stray read: row n_tgt, the pattern behind dst
    cnt, rows, lidx, kmask = [a.data_ptr() for a in plan.arrays]
    a = dict(src=case.src.data_ptr(), n_src=case.n_src, c_src=case.c_src, wp=case.pack(transposed).ptr(), volume=case.volume,
             c_dst=case.c_dst, cnt=cnt, rows=rows, lidx=lidx, kmask=kmask, tbl=case.tbl.data_ptr(),
             col=None if plan.col is None else plan.col.data_ptr(), out=None if oo is None else oo.data_ptr(),
             dst=case.dst.ptr(), n_tgt=case.n_tgt, T=plan.T, s_cap=plan.s_cap,
             mean=parts[0].ptr() if stats else None, m2=parts[1].ptr() if stats else None)
    a.update(over)
    rc = lib.me_conv_halo_bf16(a["src"], a["n_src"], a["c_src"], a["wp"], a["volume"], a["c_dst"], a["cnt"], a["rows"],
                               a["lidx"], a["kmask"], a["tbl"], a["col"], a["out"], a["dst"], a["n_tgt"], a["T"], a["s_cap"],
                               a["mean"], a["m2"], None)
    torch.cuda.synchronize()
    return rc


def run_halo(case, plan, stats=False, transposed=0, out_order=None, what=""):
    """-> (dst bf16 [n_tgt, c_dst], (mean, m2) float64 numpy [tiles, c_dst] or None); guards checked"""
    case.check(call_halo(case, plan, stats, transposed, out_order))
    assert case.intact() and plan.intact(), f"{what}: the launch wrote outside its outputs, or into an input"
    out = case.dst.as_dtype(torch.bfloat16, (case.n_tgt, case.c_dst))
    if not stats:
        assert all(p.untouched() for p in plan.partials()), f"{what}: partials written without being asked"
        return out, None
    return out, tuple(p.as_dtype(torch.float32, (plan.tiles, case.c_dst)).double().cpu().numpy() for p in plan.partials())


def expected(case, plan, out_order=None):
    """the oracle in dst row space: dst[out_order[p]] = ref[col_order[p]]"""
    n = case.n_tgt
    cols = np.arange(n) if plan.col_host is None else plan.col_host
    rows = np.arange(n) if out_order is None else np.asarray(out_order)
    assert sorted(cols.tolist()) == list(range(n)) and sorted(rows.tolist()) == list(range(n))
    exp = np.empty_like(case.ref)
    exp[rows] = case.ref[cols]
    return exp


def assert_exact(case, plan, out, what, out_order=None):
    case.exact_precondition()
    want = int_view(torch.from_numpy(expected(case, plan, out_order)).to(torch.bfloat16))
    bad = (int_view(out).cpu() != want).numpy()
    rows = np.unique(np.nonzero(bad)[0])
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, in {len(rows)} rows "
                           f"{rows[:6].tolist()}..., columns {np.unique(np.nonzero(bad)[1])[:6].tolist()}...")


def check_exact(device, tbl, n_src, shape, what, col_order=None, src_perm=None, out_order=None, x=None):
    """plan, launch, bit-exact dst -> (case, plan, dst)"""
    T, s_cap = config(shape, tbl.shape[0])
    case = exact(device, tbl, n_src, shape, x)
    plan = HaloPlan(case, T, s_cap, col_order, src_perm)
    out, _ = run_halo(case, plan, out_order=out_order, what=what)
    assert_exact(case, plan, out, what, out_order)
    return case, plan, out


# ---- table constructors (numpy only) ----------------------------------------------------------------------------------------
def capacity_table(rng, volume, T, n_src, counts, rows_last):
    """tile t names exactly counts[t] distinct source rows — each once, then up to 100 repeats — at random entries; the
    last tile holds rows_last rows"""
    n_tgt = (len(counts) - 1) * T + rows_last
    tbl = np.full((volume, n_tgt), -1, np.int32)
    for t, c in enumerate(counts):
        rows_here = T if t < len(counts) - 1 else rows_last
        entries = volume * rows_here
        assert c <= entries and c <= n_src
        chosen = rng.choice(n_src, c, replace=False)
        extra = min(entries - c, 100)
        where = rng.choice(entries, c + extra, replace=False)
        tbl[where // rows_here, t * T + where % rows_here] = np.concatenate([chosen, rng.choice(chosen, extra)])
        v = tbl[:, t * T:t * T + rows_here]
        assert len(np.unique(v[v >= 0])) == c
    return tbl


WALKS = [(), (31,), (0, 31), (30, 31), (7,), (), (1, 2, 29), (0, 15, 16, 31), (4, 9, 20, 27, 30), (0, 1, 2, 3, 4)]


def walks_table(rng, T, row_waves, walks, n_src):
    """volume 32; the rows of wave range i (rows [i T / row_waves, ...): range i % row_waves of tile i // row_waves)
    have neighbours at exactly the offsets walks[i], at a fifth of the rows"""
    span = T // row_waves
    tiles = -(-len(walks) // row_waves)
    tbl = np.full((32, tiles * T), -1, np.int32)
    for i, ks in enumerate(walks):
        for k in ks:
            m = rng.random(span) < 0.2
            m[rng.integers(span)] = True
            tbl[k, i * span:(i + 1) * span][m] = rng.integers(0, n_src, int(m.sum()))
    return tbl


def walks_of_plan(kmask, T, row_waves):
    """the offsets every wave walks, as the kernel derives them from kmask"""
    R = T // 16 // row_waves
    out = []
    for t in range(kmask.shape[0]):
        for w in range(row_waves):
            out.append(tuple(np.flatnonzero((kmask[t] >> np.uint32(w * R)) & np.uint32((1 << R) - 1)).tolist()))
    return out


def group_table(rng, volume, T, n_tgt, n_src):
    """offset k of tile t has neighbours in the 16-row group (k + t) % groups of the tile only -> (tbl, kmask)"""
    tiles = -(-n_tgt // T)
    tbl = np.full((volume, n_tgt), -1, np.int32)
    want = np.zeros((tiles, volume), np.uint32)
    for t in range(tiles):
        groups = -(-(min(n_tgt, (t + 1) * T) - t * T) // 16)
        for k in range(volume):
            g = (k + t) % groups
            lo, hi = t * T + g * 16, min(t * T + g * 16 + 16, n_tgt)
            m = rng.random(hi - lo) < 0.6
            m[rng.integers(hi - lo)] = True
            tbl[k, lo:hi][m] = rng.integers(0, n_src, int(m.sum()))
            want[t, k] = 1 << g
    return tbl, want


def mixed_table(rng, volume, T, n_tgt):
    """tile 0 from a window of source rows that fits, every other tile dense over FAR rows: they overflow"""
    tbl = make_table(rng, "dense", volume, n_tgt, FAR)
    tbl[:, :T] = make_table(rng, "random", volume, n_tgt, FAR, last_row=WINDOW)[:, :T]
    return tbl


# ---- 1. config and refusals -------------------------------------------------------------------------------------------------
def test_config_and_refusals(device):
    """auto mode; the three shapes' geometry; every refused call returns non-zero with its message and leaves dst behind
    its NaN fill; n_tgt == 0 is no error and writes nothing"""
    _, lib = _lib()
    assert lib.me_debug_halo_mode() == -1
    for shape in SHAPES:
        for volume in (2, 8, 27, 32):
            assert config(shape, volume) == CONFIG[shape]
        for volume in (1, 33):
            assert lib.me_conv_halo_config_bf16(1000, volume, 8000, shape[0], shape[1], None, None) == 0
        T, s_cap = CONFIG[shape]
        rng = np.random.default_rng(shape[0])
        case = exact(device, make_table(rng, "random", 2, T + 5, 50), 50, shape)
        plan = HaloPlan(case, T, s_cap)
        parts = plan.partials()
        bad = {
            "volume 1": (dict(volume=1), b"no halo kernel"),
            "volume 33": (dict(volume=33), b"no halo kernel"),
            "another tile height": (dict(T=192 - T), b"another geometry"),
            "another capacity": (dict(s_cap=s_cap - 1), b"another geometry"),
            "part_mean alone": (dict(mean=parts[0].ptr()), b"statistics"),
            "part_m2 alone": (dict(m2=parts[1].ptr()), b"statistics"),
        }
        for name in ("src", "wp", "cnt", "rows", "lidx", "kmask", "tbl", "dst"):
            bad[f"NULL {name}"] = ({name: None}, b"null argument")
        for name, (over, text) in bad.items():
            assert call_halo(case, plan, **over) != 0, f"{shape} {name}: accepted"
            assert text in lib.me_last_error(), (shape, name, lib.me_last_error())
            assert case.dst.untouched() and all(p.untouched() for p in parts), f"{shape} {name}: refused, yet something was written"
            assert case.intact() and plan.intact(), (shape, name)
        assert call_halo(case, plan, stats=True, n_tgt=0) == 0
        assert case.dst.untouched() and all(p.untouched() for p in parts) and case.intact() and plan.intact()
        # ... and the same arguments, unchanged, run
        out, _ = run_halo(case, plan, what=f"{shape} good arguments")
        assert_exact(case, plan, out, f"{shape} good arguments")
    if not lib.me_debug_variants_compiled():
        for shape in ((128, 128), (128, 32)):
            assert lib.me_conv_halo_config_bf16(1000, 27, 8000, shape[0], shape[1], None, None) == 0
            tbl = make_table(np.random.default_rng(1), "random", 2, 133, 50)
            case = exact_case(device, "bf16", tbl, 50, shape[0], shape[1], 3)
            plan = HaloPlan(case, 128, 383)
            assert call_halo(case, plan) != 0 and b"no halo kernel" in lib.me_last_error(), shape
            assert case.dst.untouched() and case.intact() and plan.intact(), shape


# ---- 2. row counts on the tile edges ----------------------------------------------------------------------------------------
@shapes
def test_row_counts_on_the_tile_edges(device, shape):
    """n_tgt = 1, 15, 16, 17, T - 1, T, T + 1, 2 T + 5 at volume 27 on halos that fit; the partial last tile also present at
    its last column only (what the rows beyond n_tgt compute must not reach dst)"""
    T, _ = CONFIG[shape]
    for n_tgt in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5):
        rng = np.random.default_rng(100 * T + n_tgt)
        check_exact(device, make_table(rng, "random", 27, n_tgt, WINDOW), WINDOW, shape, f"n_tgt={n_tgt}")
        if n_tgt in (17, 2 * T + 5):
            check_exact(device, make_table(rng, "tail_last_col", 27, n_tgt, WINDOW, T), WINDOW, shape, f"n_tgt={n_tgt} last column")


# ---- 3. table occupancy -----------------------------------------------------------------------------------------------------
@shapes
@pytest.mark.parametrize("kind", ["dense", "absent", "first_offset", "last_offset", "one_row", "same_source", "random"])
def test_table_occupancy(device, shape, kind):
    """"absent": tiles with an empty halo (S == 0): every row still written, with +0; "one_row" / "first_offset" /
    "last_offset": walks of one offset and waves without any beside an active one; "same_source": a halo of one row"""
    T, _ = CONFIG[shape]
    n_tgt = 2 * T + 37
    tbl = make_table(np.random.default_rng(len(kind)), kind, 27, n_tgt, WINDOW, T)
    _, plan, out = check_exact(device, tbl, WINDOW, shape, kind)
    assert not plan.overflowing().any()
    if kind == "absent":
        assert not plan.cnt.any() and not plan.kmask.any() and not bool(int_view(out).any()), "no entry anywhere: +0 everywhere"
    else:
        assert plan.cnt.any() and bool((out.float() != 0).any())


# ---- 4. the two kernels of the policy ---------------------------------------------------------------------------------------
@shapes
def test_tile_plan_kernel_gives_the_same_bits_on_exact_data(device, shape):
    """the policy switches a launch side between me_conv_target_bf16 and the halo kernel from one use to the next"""
    T, _ = CONFIG[shape]
    tbl = make_table(np.random.default_rng(4), "random", 27, 2 * T + 37, WINDOW)
    case, _, out = check_exact(device, tbl, WINDOW, shape, "halo")
    tile_plan = Plan(case, T, 4)
    case.check(call_bf16(case, tile_plan, entry="plain"))
    assert case.intact() and tile_plan.intact()
    assert torch.equal(case.dst.bits, int_view(out).reshape(-1)), "me_conv_target_bf16 and me_conv_halo_bf16 differ"


# ---- 5. halo sizes on the capacity edge -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,volume", [(s, 27) for s in SHAPES] + [((64, 32), 8)],
                         ids=[f"{s}to{d}" for s, d in SHAPES] + ["64to32-volume8"])
def test_halo_sizes_on_the_capacity_edge(device, shape, volume):
    """five tiles in one launch: s_cap - 1 and s_cap rows (staged), s_cap + 1 and 3 s_cap (volume 8: all 512 entries
    distinct) and a partial tile of s_cap + 40 (direct gather off the table); slots by row and by a permutation"""
    T, s_cap = CONFIG[shape]
    counts = [s_cap - 1, s_cap, s_cap + 1, min(3 * s_cap, volume * T), s_cap + 40]
    rng = np.random.default_rng(volume)
    tbl = capacity_table(rng, volume, T, FAR, counts, T - 3)
    for src_perm in (None, rng.permutation(FAR)):
        what = f"capacity edge, slots by {'row' if src_perm is None else 'position'}"
        _, plan, _ = check_exact(device, tbl, FAR, shape, what, src_perm=src_perm)
        assert plan.cnt.tolist() == counts, what
        assert plan.overflowing().tolist() == [False, False, True, True, True]
        assert (plan.lidx == 0xffff).any(axis=(1, 2)).tolist() == plan.overflowing().tolist(), what
        assert int((plan.lidx[2] == 0xffff).sum()) >= 1 and int((plan.lidx[1] == s_cap).sum()) >= 1


# ---- 6. active-offset counts and the last offset ----------------------------------------------------------------------------
@shapes
def test_walks_of_zero_to_five_offsets_and_offset_31(device, shape):
    """volume 32; per wave row range walks of 0 ... 5 offsets — {31}, {0, 31}, {30, 31} among them —, different in the
    waves of one workgroup (a wave without any offset beside active ones); then the list rotated by one, so that every
    walk is taken by another wave"""
    T, _ = CONFIG[shape]
    waves = ROW_WAVES[T]
    assert sorted({len(w) for w in WALKS}) == [0, 1, 2, 3, 4, 5]
    for rot in (0, 1):
        walks = WALKS[rot:] + WALKS[:rot]
        walks = walks + [()] * (-len(walks) % waves)
        tbl = walks_table(np.random.default_rng(rot), T, waves, walks, WINDOW)
        _, plan, _ = check_exact(device, tbl, WINDOW, shape, f"walks rotated by {rot}")
        assert walks_of_plan(plan.kmask, T, waves) == [tuple(sorted(w)) for w in walks]
        assert not plan.overflowing().any()


# ---- 7. row groups ----------------------------------------------------------------------------------------------------------
@shapes
def test_one_row_group_per_offset(device, shape):
    """per (tile, offset) neighbours in one 16-row group only, every group in turn, the 5-row last group of the partial
    tile included: the skip masks of the 128-row shapes, zero rows multiplied on 64 -> 32 — the same exact answer"""
    T, _ = CONFIG[shape]
    n_tgt = 2 * T + 21
    tbl, want = group_table(np.random.default_rng(7), 27, T, n_tgt, WINDOW)
    assert set(want[0].tolist()) == {1 << g for g in range(T // 16)} and set(want[2].tolist()) == {1, 2}
    _, plan, out = check_exact(device, tbl, WINDOW, shape, "row groups")
    assert np.array_equal(plan.kmask, want)
    assert bool((out[n_tgt - 5:].float() != 0).any())


# ---- 8. orders --------------------------------------------------------------------------------------------------------------
@shapes
def test_column_and_output_orders(device, shape):
    """col_order (tile position -> table column) and out_order (tile position -> dst row) as two different
    permutations — a position-space table in production —, and each alone"""
    T, _ = CONFIG[shape]
    n_tgt = 2 * T + 37
    rng = np.random.default_rng(8)
    tbl = make_table(rng, "random", 27, n_tgt, WINDOW)
    col, out = rng.permutation(n_tgt), rng.permutation(n_tgt)
    assert (col != out).any()
    for c, o in ((col, out), (col, None), (None, out), (col, col)):
        check_exact(device, tbl, WINDOW, shape, f"col_order={c is not None} out_order={o is not None}", col_order=c, out_order=o)


# ---- 9. poisoned and non-finite rows ----------------------------------------------------------------------------------------
@shapes
@pytest.mark.parametrize("path", ["staged", "direct"])
def test_poisoned_and_non_finite_rows(device, shape, path):
    """NaN in source rows 0, n_src - 1 and every other row no entry names (the clamped staging loads, the zero slot, the
    predicated direct loads) must not reach dst; +Inf, -Inf and NaN in three rows that are named give what float64 gives
    in the rows that name them, and nothing else changes"""
    T, s_cap = CONFIG[shape]
    n_tgt, n_src = 2 * T + 37, (WINDOW if path == "staged" else FAR)
    rng = np.random.default_rng(9)
    tbl = make_table(rng, "dense", 27, n_tgt, n_src, first_row=4, last_row=n_src - 1)
    tbl[rng.random(tbl.shape) < (0.7 if path == "staged" else 0.2)] = -1
    named = np.zeros(n_src, bool)
    named[tbl[tbl >= 0]] = True
    assert not named[0] and not named[n_src - 1] and not named[1:4].any()
    x0 = exact_data(device, 27, n_src, shape)[0]
    x = x0.clone()
    x[~named] = float("nan")
    case, plan, out = check_exact(device, tbl, n_src, shape, f"{path}: NaN in unnamed rows", x=x)
    assert plan.overflowing().all() == (path == "direct") and plan.overflowing().any() == (path == "direct")
    assert bool(torch.isfinite(out.float()).all())
    # three named rows
    special = tbl.copy()
    present = np.flatnonzero((special >= 0).reshape(-1))
    pick = present[::15]
    special.reshape(-1)[pick] = 1 + np.arange(len(pick)) % 3
    special[26, n_tgt - 1] = 1                                  # the last row of the partial tile, at the last offset
    x[1:4] = x0[1:4]
    x[1, 2], x[2, 2], x[3, 0] = float("inf"), -float("inf"), float("nan")
    case = exact(device, special, n_src, shape, x)
    plan = HaloPlan(case, T, s_cap)
    assert plan.overflowing().all() == (path == "direct") and plan.overflowing().any() == (path == "direct")
    out, _ = run_halo(case, plan, what=f"{path}: non-finite rows")
    got, ref = out.double().cpu().numpy(), case.ref
    fin = np.isfinite(ref)
    touched = np.isin(special, (1, 2, 3)).any(0)
    assert np.array_equal(~fin.all(1), touched), "the oracle: exactly the rows that name a special row are non-finite"
    assert np.isposinf(ref).any() and np.isneginf(ref).any() and np.isnan(ref).any() and fin.all(1).any()
    same_nonfinite_class(got, ref, f"{path}: non-finite rows")
    case.exact_precondition()
    want = torch.from_numpy(ref).to(torch.bfloat16).double().numpy()
    assert np.array_equal(got[fin], want[fin]), f"{path}: finite elements differ from the exact result"


# ---- 10. statistics ---------------------------------------------------------------------------------------------------------
@shapes
def test_statistics_partials(device, shape):
    """part_mean / part_m2 of a full tile, an all-absent tile (exact zeros), an overflowing tile and a partial tile
    against the float64 mean / M2 of the stored values (assert_tile_partials); with out_order the rows of tile t are
    dst[out_order[t T ...]]; dst does not change with the partials"""
    T, s_cap = CONFIG[shape]
    n_tgt = 3 * T + T // 2 + 3
    rng = np.random.default_rng(10)
    tbl = make_table(rng, "random", 27, n_tgt, FAR, last_row=WINDOW)
    tbl[:, T:2 * T] = -1
    tbl[:, 2 * T:3 * T] = make_table(rng, "dense", 27, n_tgt, FAR)[:, 2 * T:3 * T]
    for case in (random_case(device, "bf16", tbl, FAR, shape[0], shape[1], 11), exact(device, tbl, FAR, shape)):
        plan = HaloPlan(case, T, s_cap)
        assert plan.cnt[1] == 0 and plan.overflowing().tolist() == [False, False, True, False]
        for order in (None, rng.permutation(n_tgt)):
            what = f"statistics out_order={order is not None}"
            plain, _ = run_halo(case, plan, out_order=order, what=what)
            out, (mean, m2) = run_halo(case, plan, stats=True, out_order=order, what=what)
            assert torch.equal(int_view(out), int_view(plain)), f"{what}: dst differs with the statistics epilogue"
            assert_bf16_close(out.float().cpu().numpy(), expected(case, plan, order), what)
            rows = np.arange(n_tgt) if order is None else order
            stored = out.double().cpu().numpy()[rows]
            assert_tile_partials(stored, T, mean, m2, what)
            assert not mean[1].any() and not m2[1].any() and not stored[T:2 * T].any(), f"{what}: the tile of empty rows"
            assert (stored[:T] != stored[0]).any() and (stored[3 * T:] != stored[3 * T]).any()


# ---- 11. transposed pack ----------------------------------------------------------------------------------------------------
@shapes
def test_transposed_weights_give_the_same_bits(device, shape):
    """the [K, c_dst, c_src] form of the weights (how the input-gradient shapes are launched) packs to the same image"""
    T, _ = CONFIG[shape]
    tbl = mixed_table(np.random.default_rng(11), 27, T, 2 * T + 37)
    case, plan, out = check_exact(device, tbl, FAR, shape, "pack(0)")
    assert torch.equal(case.pack(0).bits, case.pack(1).bits)
    out_t, _ = run_halo(case, plan, transposed=1, what="pack(1)")
    assert torch.equal(int_view(out_t), int_view(out))


# ---- 12. random data --------------------------------------------------------------------------------------------------------
@shapes
def test_random_data_against_the_bf16_bound(device, shape):
    T, s_cap = CONFIG[shape]
    n_tgt = 2 * T + 37
    rng = np.random.default_rng(12)
    for name, tbl in (("fits", make_table(rng, "random", 27, n_tgt, FAR, last_row=WINDOW)), ("mixed", mixed_table(rng, 27, T, n_tgt))):
        case = random_case(device, "bf16", tbl, FAR, shape[0], shape[1], 13)
        plan = HaloPlan(case, T, s_cap, src_perm=rng.permutation(FAR))
        assert plan.overflowing().tolist() == ([False] * 3 if name == "fits" else [False, True, True])
        out, _ = run_halo(case, plan, what=name)
        assert bool(torch.isfinite(out.float()).all()), f"{name}: rows not written, or computed from the surroundings"
        assert_bf16_close(out.float().cpu().numpy(), expected(case, plan), name)


# ---- 13. plan kernel instantiations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume,T", [(3, 16), (2, 128), (4, 128), (8, 128), (16, 128), (32, 128), (64, 64)])
def test_plan_kernel_instantiations(device, volume, T):
    """k_halo_plan<256> ... <4096> by volume x tile_rows, alone, against numpy_halo_plan: s_cap 8 with a first tile of five
    entries (fits) and tiles that overflow, a partial last tile, with and without col_order and slot positions"""
    n_src, n_tgt, s_cap = 200, 3 * T + 5, 8
    rng = np.random.default_rng(volume * T)
    tbl = make_table(rng, "random", volume, n_tgt, n_src)
    tbl[:, :T] = -1
    tbl[:, T:2 * T] = make_table(rng, "dense", volume, n_tgt, n_src)[:, T:2 * T]
    where = rng.choice(volume * T, 5, replace=False)
    tbl[where // T, where % T] = rng.integers(0, n_src, 5)
    for col_order, src_perm in ((None, None), (rng.permutation(n_tgt), None), (None, rng.permutation(n_src)),
                                (rng.permutation(n_tgt), rng.permutation(n_src))):
        by_column = tbl.copy()
        if col_order is not None:
            by_column[:, col_order] = tbl                # tile position p reads column col_order[p]
        case = table_only(device, by_column, n_src)
        before = case.tbl_big.clone()
        plan = HaloPlan(case, T, s_cap, col_order, src_perm)
        assert plan.overflowing().any() and not plan.overflowing().all() and plan.cnt.all()
        assert torch.equal(case.tbl_big, before) and all(torch.equal(a, b) for a, b in plan.inputs)


def test_plan_sizes_out_of_range_are_refused(device):
    _, lib = _lib()
    for volume, T in ((65, 16), (33, 128), (64, 80), (8, 24), (0, 16)):
        case = table_only(device, np.full((max(volume, 1), 40), -1, np.int32), 10)
        case.volume = volume
        assert HaloPlan(case, T, 8, expect_error=True).rc != 0, f"me_halo_plan_build took volume {volume} x tile_rows {T}"
        assert lib.me_last_error()
