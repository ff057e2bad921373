"""The coordinate kernels of csrc/coords.hip through the C ABI, on synthetic inputs: hash insert (fused and the scan
pipeline), Z-order keys and the radix sort, the spatial index, the flat-table and the LDS-bucketed kernel-map probes with
their compaction, counting and transpose kernels, and the small entry points (stride, expand_region, quantize_labels).

tests/test_gpu_coords.py drives the same kernels through the coordinate manager, which sizes the buffers itself, on
random clouds of a few thousand rows.  Here every buffer has exactly its documented size:
  * every output and every workspace is a helpers.GuardedBytes (the byte-typed sibling of helpers.Guarded: the 8-byte
    arrays and the workspaces need it, and one type keeps the harness in one piece) — a pattern of 4096 bytes on either
    side that must be intact after the call; workspaces are exactly *_workspace_bytes(...) long;
  * every call runs twice, the workspace pre-filled with zeros and then with the suite's poison word 0x7f817f81, the
    outputs pre-filled with a sentinel: all outputs must be bit-identical (the library never reads workspace it has not
    written).  The one exception is the hash TABLE of an insert: which of two colliding coordinates gets the earlier slot
    follows the race of their atomicCAS, so its bits are checked through me_coords_find instead;
  * every input sits in the middle of a larger tensor of the poison word (helpers.middle);
  * a workspace one byte short is refused: non-zero return, me_last_error() set, outputs and guards untouched.
All comparisons are integer and bit-exact.  References: tests/coords_reference.py (numpy, checked on its own by
tests/test_coords_reference_cpu.py) and the C oracle (oracle.me_oracle)."""
import ctypes

import numpy as np
import pytest
import torch

import coords_reference as R
from helpers import GuardedBytes, middle
from oracle import me_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0x7f817f81          # conftest._poison_device_memory
SENTINEL = 0x7fc00001        # what an output holds before a launch (helpers.Guarded.NAN[4])
CUBE, CROSS, CUSTOM = 0, 1, 2
ME_MAX_DIM = 7


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


@pytest.fixture
def lib():
    _, lib = _lib()
    lib.me_debug_set_insert_fused(1)
    try:
        yield lib
    finally:
        lib.me_debug_set_insert_fused(1)


# ---- harness ----------------------------------------------------------------------------------------------------------------
class In:
    """a host array on the device, in the middle of a tensor of the poison word"""

    def __init__(self, a, device):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.int32, np.int64), a.dtype
        t = torch.from_numpy(a.reshape(-1))
        self.big, self.view = middle(t.numel(), t.dtype, device, POISON)
        self.view.copy_(t)
        self.snapshot = self.big.clone()
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return torch.equal(self.big, self.snapshot)


def out_buf(n_elems, elem_bytes, device):
    return GuardedBytes(int(n_elems) * elem_bytes, device)


def run_guarded(lib, launch, outs, ws, racy=()):
    """launch(ws_ptr, ws_bytes) -> (rc, host values), twice: workspace of zeros, workspace of the poison word.  Outputs
    (but those in `racy`) and host values must agree bit for bit, every guard band must be intact.  Leaves the second
    run's results in `outs`; -> the host values."""
    seen = []
    for word in (0, POISON):
        for o in outs:
            o.fill(SENTINEL)
        if ws is not None:
            ws.fill(word)
        rc, host = launch(ws.ptr() if ws is not None else None, ws.n if ws is not None else 0)
        torch.cuda.synchronize()
        assert rc == 0, lib.me_last_error()
        for i, o in enumerate(list(outs) + ([ws] if ws is not None else [])):
            assert o.intact(), f"guard band of buffer {i} overwritten (workspace pre-filled with {word:#x})"
        seen.append(([None if o in racy else o.bytes.clone() for o in outs], host))
    for i, (a, b) in enumerate(zip(seen[0][0], seen[1][0])):
        assert a is None or torch.equal(a, b), f"output {i} depends on what the workspace held before the call"
    assert seen[0][1] == seen[1][1], f"host results depend on the workspace: {seen[0][1]} vs {seen[1][1]}"
    return seen[1][1]


def refused_when_short(lib, launch, outs, ws):
    """the documented refusal of a workspace one byte short"""
    for o in outs:
        o.fill(SENTINEL)
    ws.fill(POISON)
    rc, _ = launch(ws.ptr(), ws.n - 1)
    torch.cuda.synchronize()
    assert rc != 0 and lib.me_last_error(), "a workspace one byte short must be refused"
    assert b"workspace" in lib.me_last_error()
    for o in outs:
        assert o.holds(SENTINEL) and o.intact(), "a refused call touched an output"
    assert ws.holds(POISON) and ws.intact(), "a refused call touched the workspace"


def np_of(buf, dtype, shape=(-1,)):
    return buf.view(dtype, shape).cpu().numpy().copy()


def ints(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def cloud(rng, n, D, lo, hi, batches=(0,)):
    """n UNIQUE rows (batch, x_1 .. x_D) with x in [lo, hi], shuffled"""
    cells = (hi - lo + 1) ** D * len(batches)
    assert cells >= n, (cells, n)
    if cells <= 4 * n:                                  # dense: choose among all cells
        lin = rng.choice(cells, n, replace=False)
        cols = []
        for _ in range(D):
            cols.append(lin % (hi - lo + 1) + lo)
            lin = lin // (hi - lo + 1)
        c = np.column_stack([np.asarray(batches)[lin]] + cols[::-1])
    else:
        c = np.zeros((0, D + 1), np.int64)
        while len(c) < n:
            more = np.column_stack([rng.choice(batches, 2 * n)] + [rng.integers(lo, hi + 1, 2 * n) for _ in range(D)])
            c = np.unique(np.concatenate((c, more)), axis=0)
        c = c[rng.permutation(len(c))[:n]]
    return np.ascontiguousarray(c[rng.permutation(n)].astype(np.int32))


def unique_rows(c):
    c = np.asarray(c, np.int32)
    return np.ascontiguousarray(c[R.first_occurrence(c)[0]])


# =============================================================================================================================
# 1. me_coords_insert_and_map_bbox + me_coords_find
# =============================================================================================================================
class Insert:
    """one guarded insert: buffers of exactly the documented sizes"""

    def __init__(self, lib, device, coords, capacity=None):
        self.lib, self.device = lib, device
        self.n, self.ncol = coords.shape
        n, ncol = self.n, self.ncol
        self.cap = int(capacity or lib.me_hash_capacity(n))
        self.coords = In(coords, device)
        self.table = out_buf(self.cap, 8, device)
        self.cu = out_buf(n * ncol, 4, device)
        self.um = out_buf(n, 8, device)
        self.inv = out_buf(n, 8, device)
        self.ws = GuardedBytes(int(lib.me_insert_workspace_bytes(n)), device)
        self.outs = [self.table, self.cu, self.um, self.inv]

    def launch(self, ws_ptr, ws_bytes):
        nu = ctypes.c_int64(-7)
        bbox = ints([77] * (2 * self.ncol))
        rc = self.lib.me_coords_insert_and_map_bbox(self.coords.ptr(), self.n, self.ncol, self.table.ptr(), self.cap,
                                                    self.cu.ptr(), self.um.ptr(), self.inv.ptr(), ctypes.byref(nu), bbox,
                                                    ws_ptr, ws_bytes, None)
        return rc, (nu.value, tuple(bbox))

    def run(self):
        self.n_unique, self.bbox = run_guarded(self.lib, self.launch, self.outs, self.ws, racy=(self.table,))
        assert self.coords.intact()
        return self

    def results(self):
        nu = self.n_unique
        return (np_of(self.um, torch.int64)[:nu], np_of(self.inv, torch.int64),
                np_of(self.cu, torch.int32, (self.n, self.ncol))[:nu])

    def find(self, queries):
        """me_coords_find of int32 [nq, ncol] rows on the table of this insert -> int32 [nq]"""
        q = In(queries, self.device)
        rows = out_buf(len(queries), 4, self.device)

        def launch(_p, _b):
            return self.lib.me_coords_find(self.table.ptr(), self.cap, self.cu.ptr(), self.ncol, q.ptr(), len(queries),
                                           rows.ptr(), None), ()
        run_guarded(self.lib, launch, [rows], None)
        return np_of(rows, torch.int32)


def check_insert(lib, device, coords, capacity=None):
    """fused and pipeline insert of `coords` against the first-occurrence reference and against each other"""
    um_ref, inv_ref = R.first_occurrence(coords)
    got = {}
    for fused in (1, 0):
        lib.me_debug_set_insert_fused(fused)
        try:
            ins = Insert(lib, device, coords, capacity).run()
        finally:
            lib.me_debug_set_insert_fused(1)
        um, inv, cu = ins.results()
        what = f"{'fused' if fused else 'pipeline'} insert of {coords.shape}"
        assert ins.n_unique == len(um_ref), f"{what}: n_unique {ins.n_unique}, want {len(um_ref)}"
        assert np.array_equal(um, um_ref), f"{what}: unique_map"
        assert np.array_equal(inv, inv_ref), f"{what}: inverse_map"
        assert np.array_equal(cu, coords[um_ref]), f"{what}: coords_unique"
        assert np.array_equal(np.asarray(ins.bbox), R.bounding_box(coords)), f"{what}: bbox {ins.bbox}"
        if len(coords):
            absent = coords[:min(len(coords), 70)].copy()
            absent[:, -1] += np.int32(coords[:, -1].max() - coords[:, -1].min() + 1)     # beyond the last column's range
            rows = ins.find(np.concatenate((coords, absent)))
            assert np.array_equal(rows[:len(coords)], inv_ref.astype(np.int32)), f"{what}: me_coords_find of the input rows"
            assert (rows[len(coords):] == -1).all(), f"{what}: me_coords_find of absent rows"
        got[fused] = [o.bytes.clone() for o in ins.outs[1:]]
    for a, b in zip(got[1], got[0]):
        assert torch.equal(a, b), "the fused and the pipeline insert differ"
    return ins


INSERT_LAYOUTS = ("unique", "all_equal", "dist64", "dist1024", "winner_last_of_block", "reversed", "negative")


def insert_rows(layout, n, ncol, seed=0):
    """n rows of `ncol` columns in one of the duplicate layouts of k_insert / k_insert_flags / k_insert_emit"""
    rng = np.random.default_rng(seed + 1000 * n + ncol)
    u = np.zeros((n, ncol), np.int64)                   # n distinct rows in a shuffled order, a few columns busy
    ids = rng.permutation(n)
    u[:, 0] = ids % 3
    u[:, 1] = ids // 3
    if ncol > 2:
        u[:, 2:] = rng.integers(-4, 5, size=(n, ncol - 2))
    if layout == "unique":
        c = u
    elif layout == "all_equal":
        c = np.repeat(u[:1], n, axis=0)
    elif layout in ("dist64", "dist1024", "reversed"):
        d = 1024 if layout == "dist1024" else 64        # row i == row i - d: the winner is in the previous 64-row ballot
        c = u[np.arange(n) % d]                         # group (kInsJ groups per thread) / the previous 1024-row block
        if layout == "reversed":
            c = c[::-1]
    elif layout == "winner_last_of_block":
        # the last row of a 1024-row block of k_insert_flags (or of a 256-thread block / a 64-row group when n is
        # smaller) wins against every second row after it
        w = max([e for e in (1023, 255, 63) if e < n - 1] or [0])
        c = u.copy()
        c[w + 1::2] = u[w]
    else:
        assert layout == "negative", layout
        c = u - np.array([0] + [n + 5] * (ncol - 1))
        c[rng.integers(0, n, n // 3)] = c[rng.integers(0, n, n // 3)]
    return np.ascontiguousarray(c.astype(np.int32))


INSERT_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("layout", INSERT_LAYOUTS)
@pytest.mark.parametrize("n", INSERT_N)
def test_insert_block_edges_and_duplicate_layouts(device, lib, n, layout):
    """k_insert / k_insert_flags / k_insert_emit (fused) and k_insert_resolve / k_scan_single / k_insert_finalize / k_bbox
    (me_debug_set_insert_fused(0)) on the 64-row ballot group, the 256-thread block and the kInsBlockRows = 1024 block
    edges, capacity = me_hash_capacity(n) (the 50 % load limit when n is a power of two); the column count walks
    2 .. ME_MAX_DIM + 1 over the cases."""
    ncol = 2 + (INSERT_N.index(n) + INSERT_LAYOUTS.index(layout)) % ME_MAX_DIM
    check_insert(lib, device, insert_rows(layout, n, ncol))


@pytest.mark.parametrize("ncol", range(2, ME_MAX_DIM + 2))
def test_insert_every_column_count(device, lib, ncol):
    """every instantiation of ME_DISPATCH_NCOL (2 .. 8 columns; 2 and 4 take the vector loads) on 1025 rows with
    duplicates at distance 64 and a workspace one byte short"""
    coords = insert_rows("dist64", 1025, ncol, seed=3)
    ins = check_insert(lib, device, coords)
    refused_when_short(lib, ins.launch, ins.outs, ins.ws)


def test_insert_sparse_table_and_nothing(device, lib):
    """a capacity far beyond me_hash_capacity (2^16 slots for 257 rows), and n = 0: n_unique 0, the bounding box all
    zeros, the table all empty slots"""
    check_insert(lib, device, insert_rows("negative", 257, 4), capacity=1 << 16)
    ins = Insert(lib, device, np.zeros((0, 4), np.int32)).run()
    assert ins.n_unique == 0 and ins.bbox == (0,) * 8
    assert bool((ins.table.view(torch.int64) == -1).all())


@pytest.mark.parametrize("n,layout,ncol", [(32768, "dist1024", 4), (32768, "unique", 2), (32769, "dist1024", 4),
                                           (32769, "negative", 3), (32768 + 1025, "dist64", 4),
                                           (32768 + 1025, "winner_last_of_block", 5)])
def test_insert_scan_edges(device, lib, n, layout, ncol):
    """kScanSingleMax = 32768 flags: k_scan_single below and at it, k_scan_block_sums / k_scan_of_sums / k_scan_apply
    beyond it (32769: a last scan block of one item; 32768 + 1025: 34 blocks of kScanBlock = 1024, the last one with one
    item) in the pipeline insert; the fused insert runs the same rows through 33 / 34 blocks of k_insert_flags"""
    check_insert(lib, device, insert_rows(layout, n, ncol))


@pytest.mark.parametrize("n", [1 << 23, (1 << 23) + 1], ids=["2^23_fused_8192_blocks", "2^23+1_pipeline_by_the_library"])
def test_insert_path_switch_at_2_23_rows(device, lib, n):
    """kInsMaxBlocks * kInsBlockRows = 2^23 rows: the last size of the fused insert (k_insert_emit scans all 8192 block
    counts in LDS) and the first one the library itself hands to the scan pipeline.  D = 1, coords[i] = (0, i), the last
    4099 rows copies of chosen rows: the answer is known without a reference sort and is checked on the device."""
    ndup = 4099
    base = n - ndup
    g = torch.Generator().manual_seed(n)
    src = torch.randint(0, base, (ndup,), generator=g)
    src[:4] = torch.tensor([0, 1023, 1024, base - 1])
    rows = torch.cat((torch.arange(base), src))
    cap = int(lib.me_hash_capacity(n))
    big, coords = middle(2 * n, torch.int32, device, POISON)
    coords.view(n, 2)[:, 0] = 0
    coords.view(n, 2)[:, 1] = rows.to(device=device, dtype=torch.int32)
    table, cu, um, inv = out_buf(cap, 8, device), out_buf(2 * n, 4, device), out_buf(n, 8, device), out_buf(n, 8, device)
    ws = GuardedBytes(int(lib.me_insert_workspace_bytes(n)), device)

    def launch(ws_ptr, ws_bytes):
        nu = ctypes.c_int64(-7)
        bbox = ints([77] * 4)
        rc = lib.me_coords_insert_and_map_bbox(coords.data_ptr(), n, 2, table.ptr(), cap, cu.ptr(), um.ptr(), inv.ptr(),
                                               ctypes.byref(nu), bbox, ws_ptr, ws_bytes, None)
        return rc, (nu.value, tuple(bbox))
    n_unique, bbox = run_guarded(lib, launch, [table, cu, um, inv], ws, racy=(table,))
    assert n_unique == base and bbox == (0, 0, 0, base - 1)
    want_inv = rows.to(device)
    assert torch.equal(inv.view(torch.int64), want_inv), "inverse_map"
    assert torch.equal(um.view(torch.int64)[:base], torch.arange(base, device=device)), "unique_map"
    assert torch.equal(cu.view(torch.int32)[:2 * base], coords[:2 * base]), "coords_unique"
    found = out_buf(n, 4, device)
    found.fill(SENTINEL)
    rc = lib.me_coords_find(table.ptr(), cap, cu.ptr(), 2, coords.data_ptr(), n, found.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.me_last_error()
    assert found.intact() and torch.equal(found.view(torch.int32), want_inv.int()), "me_coords_find of every input row"


# =============================================================================================================================
# 2. me_coords_spatial_keys, me_coords_zorder
# =============================================================================================================================
def gpu_keys(lib, device, coords, ts):
    n, ncol = coords.shape
    cin, keys = In(coords, device), out_buf(n, 8, device)

    def launch(_p, _b):
        return lib.me_coords_spatial_keys(cin.ptr(), n, ncol, ints(ts), keys.ptr(), None), ()
    run_guarded(lib, launch, [keys], None)
    assert cin.intact()
    return np_of(keys, torch.int64).view(np.uint64)


def gpu_zorder(lib, device, coords, ts, bbox, refuse=False):
    n, ncol = coords.shape
    cin, order = In(coords, device), out_buf(n, 4, device)
    ws = GuardedBytes(int(lib.me_coords_zorder_workspace_bytes(n)), device)
    bb = ints(bbox) if bbox is not None else None

    def launch(ws_ptr, ws_bytes):
        return lib.me_coords_zorder(cin.ptr(), n, ncol, ints(ts), bb, order.ptr(), ws_ptr, ws_bytes, None), ()
    run_guarded(lib, launch, [order], ws)
    got = np_of(order, torch.int32)
    if refuse:
        refused_when_short(lib, launch, [order], ws)
    assert cin.intact()
    return got


ZORDER_N = (1, 1023, 1024, 1025, 2049)      # kRsTile = 1024 rows per block of k_rs_hist / k_rs_scatter
ZORDER_TS = (1, 2, (2, 4, 1))


def zorder_rows(kind, rng, n, D, ts):
    """-> (coords int32 [n, D + 1], bbox or None, branch the box must reach, parity of the pass count or None)"""
    kbits = R.key_bits(D)
    half = 1 << (kbits - 1)
    tsa = np.asarray(ts, np.int64)
    batch = np.zeros(n, np.int64)
    want_branch, parity = "plain", None
    if kind in ("no_box", "exact_box"):
        x = rng.integers(-41, 42, size=(n, D))                           # negative, not multiples of the stride
    elif kind == "all_keys_equal":
        x = np.repeat(rng.integers(-41, 42, size=(1, D)), n, axis=0)
    elif kind == "several_batches":
        x = rng.integers(0, 16, size=(n, D)) * tsa
        batch = rng.integers(0, 3, n)
        batch[:2] = (0, 2)[:n]
    elif kind in ("even_passes", "odd_passes"):
        # one batch, 2^b cells per axis with both ends present: ceil(b * D / 8) passes over the coordinate bits
        parity = 0 if kind == "even_passes" else 1
        b = min(b for b in range(2, kbits) if -(-b * D // 8) % 2 == parity)
        x = rng.integers(0, 1 << b, size=(n, D)) * tsa
        x[0], x[-1] = 0, ((1 << b) - 1) * tsa
    elif kind == "batches_0_and_128":
        x = rng.integers(-9, 10, size=(n, D))
        batch = rng.choice([0, 128], n)
        batch[:2] = (0, 128)[:n]
    elif kind == "wrap_box":
        x = rng.integers(half - 3, half + 3, size=(n, D)) * tsa + rng.integers(0, tsa)
        x[0], x[-1] = (half - 3) * tsa, (half + 2) * tsa
        want_branch = "wrap"
    else:
        assert kind == "wide_box", kind
        x = rng.integers(-half, half, size=(n, D)) * tsa + rng.integers(0, tsa)
        x[0], x[-1] = -half * tsa, (half - 1) * tsa
        want_branch = "wide"
    c = np.column_stack((batch, x)).astype(np.int32)
    if n == 1 and kind in ("wrap_box", "wide_box", "even_passes", "several_batches", "odd_passes", "batches_0_and_128"):
        want_branch, parity = "plain", None                              # one row cannot span a box
    return np.ascontiguousarray(c), (None if kind == "no_box" else R.bounding_box(c)), want_branch, parity


ZORDER_KINDS = ("no_box", "exact_box", "all_keys_equal", "several_batches", "batches_0_and_128", "even_passes",
                "odd_passes", "wrap_box", "wide_box")


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ZORDER_KINDS)
def test_spatial_keys_and_zorder(device, lib, kind, D):
    """k_spatial_keys against the numpy restatement of the documented key, me_coords_zorder (k_rs_hist, the scan,
    k_rs_scatter per key byte) against numpy's stable argsort of the REFERENCE keys; row counts on the kRsTile = 1024
    edges, tensor strides 1, 2 and (2, 4, 1) with negative coordinates off the stride's multiples.  Boxes: none (every
    key byte), exact, all keys equal (np == 0: the one pass at shift 0), one / several batches (the pass at shift 56),
    batches 0 and 128 (equal in the 7-bit batch byte), an even and an odd pass count (which of `order` / vbuf the first
    pass writes), a box across +2^(kbits-1) cells (`a > b`) and one 2^kbits cells wide (`hi - lo >= mask`)."""
    rng = np.random.default_rng(100 * D + ZORDER_KINDS.index(kind))
    for n in ZORDER_N:
        for ts_spec in ZORDER_TS:
            ts = [ts_spec] * D if np.isscalar(ts_spec) else [ts_spec[d % 3] for d in range(D)]
            coords, bbox, want_branch, parity = zorder_rows(kind, rng, n, D, ts)
            shifts, branches = R.zorder_passes(bbox, ts, D)
            what = f"{kind} D={D} n={n} ts={ts} passes at {shifts}"
            if kind == "no_box":
                assert len(shifts) == -(-R.key_bits(D) * D // 8) + 1, what
            else:
                assert want_branch in branches, f"{what}: the box takes {branches}"
            if kind == "all_keys_equal":
                assert shifts == [0], what
            if parity is not None:
                assert len(shifts) % 2 == parity, what
            ref = R.morton_keys(coords, ts)
            keys = gpu_keys(lib, device, coords, ts)
            assert np.array_equal(keys, ref), f"{what}: keys differ first at row {np.flatnonzero(keys != ref)[:1]}"
            order = gpu_zorder(lib, device, coords, ts, bbox, refuse=(n == 1025 and ts_spec == 2))
            assert np.array_equal(order, np.argsort(ref, kind="stable")), f"{what}: order"


# =============================================================================================================================
# 3. me_spatial_index_build
# =============================================================================================================================
def make_grid(ncol, shift, sc_min, sc_dim, ts):
    L, _ = _lib()
    g = L.MeSpatialGrid()
    g.ncol = ncol
    for d in range(ncol - 1):
        g.shift[d], g.tensor_stride[d] = int(shift[d]), int(ts[d])
    for d in range(ncol):
        g.sc_min[d], g.sc_dim[d] = int(sc_min[d]), int(sc_dim[d])
    return g


class SpatialIndex:
    """one guarded me_spatial_index_build, checked against coords_reference.spatial_index"""

    def __init__(self, lib, device, coords, grid_lists, refuse=False):
        shift, sc_min, sc_dim, ts = grid_lists
        n, ncol = coords.shape
        self.n, self.ncol, self.coords = n, ncol, coords
        self.grid = make_grid(ncol, shift, sc_min, sc_dim, ts)
        self.m = int(lib.me_spatial_cells(ctypes.byref(self.grid)))
        assert self.m == int(np.prod(sc_dim))
        self.cin = In(coords, device)
        self.order, self.pos = out_buf(n, 4, device), out_buf(n, 4, device)
        self.sorted, self.dir = out_buf(n * ncol, 4, device), out_buf(self.m + 1, 4, device)
        ws = GuardedBytes(int(lib.me_spatial_index_workspace_bytes(n, self.m)), device)
        outs = [self.order, self.pos, self.sorted, self.dir]

        def launch(ws_ptr, ws_bytes):
            return lib.me_spatial_index_build(self.cin.ptr(), n, ctypes.byref(self.grid), self.order.ptr(), self.pos.ptr(),
                                              self.sorted.ptr(), self.dir.ptr(), ws_ptr, ws_bytes, None), ()
        run_guarded(lib, launch, outs, ws)
        assert self.cin.intact()
        self.order_np, self.pos_np = np_of(self.order, torch.int32), np_of(self.pos, torch.int32)
        dir_np = np_of(self.dir, torch.int32)
        what = f"spatial index of {coords.shape} rows in {self.m} supercells"
        if n == 0:
            assert (dir_np == 0).all(), f"{what}: dir_start of an empty map"
        else:
            order, pos, dir_start = R.spatial_index(coords, shift, sc_min, sc_dim, ts)
            assert np.array_equal(self.order_np, order), f"{what}: order"
            assert np.array_equal(self.pos_np, pos), f"{what}: pos_of_row"
            assert np.array_equal(np_of(self.sorted, torch.int32, (n, ncol)), coords[order]), f"{what}: coords_sorted"
            assert np.array_equal(dir_np, dir_start) and dir_np[self.m] == n, f"{what}: dir_start"
        if refuse:
            refused_when_short(lib, launch, outs, ws)


def rows_in_supercells(rng, n, grid_lists, batch0, allowed):
    """n rows (duplicates allowed: the sort is stable) whose supercells are drawn from the linear indices `allowed`"""
    shift, sc_min, sc_dim, ts = grid_lists
    D = len(shift)
    lin = rng.choice(allowed, n)
    cols = []
    for d in range(D - 1, -1, -1):
        sc = lin % sc_dim[1 + d] + sc_min[1 + d]
        lin = lin // sc_dim[1 + d]
        cell = (sc << shift[d]) + rng.integers(0, 1 << shift[d], n)
        cols.append(cell * ts[d] + rng.integers(0, ts[d], n))             # anywhere inside the cell of ts[d] units
    assert (lin < sc_dim[0]).all()
    return np.ascontiguousarray(np.column_stack([lin + batch0] + cols[::-1]).astype(np.int32))


SPATIAL_GRIDS = {
    # name: (shift, sc_min (batch first), sc_dim, ts)
    "m=1_no_radix_pass": ([4, 4, 4], [2, -1, 0, 3], [1, 1, 1, 1], [1, 2, 1]),
    "m=255_one_pass": ([2], [0, -100], [1, 255], [2]),
    "m=256_one_pass_directory_of_257": ([2], [0, -100], [1, 256], [3]),
    "m=257_two_passes": ([1], [5, -300], [1, 257], [2]),
    "m=80000_three_passes": ([1, 2], [0, -90, 7], [2, 200, 200], [2, 1]),
    "m=1260_4d": ([1, 1, 2, 1], [1, -3, 0, -2, 4], [3, 5, 4, 3, 7], [1, 2, 1, 3]),
}


@pytest.mark.parametrize("name", list(SPATIAL_GRIDS))
def test_spatial_index_build(device, lib, name):
    """k_sp_keys, the radix passes (ceil(log2 m / 8): none for m = 1, one up to m = 256, two from 257, three beyond
    65,536), k_sp_directory (m + 1 entries: 256 / 257 / 258 on the 256-thread edge) and k_sp_finish; row counts 0, 1 and
    the kRsTile = 1024 edges; the first, the last and a middle run of supercells empty; negative coordinates off the
    multiples of a tensor stride > 1."""
    grid_lists = SPATIAL_GRIDS[name]
    m = int(np.prod(grid_lists[2]))
    rng = np.random.default_rng(m)
    allowed = np.arange(m)
    if m > 4:                                        # empty supercells first, last and in the middle
        allowed = np.concatenate((np.arange(2, m // 2 - m // 8), np.arange(m // 2 + m // 8, m - 2)))
    for n in (0, 1, 1023, 1024, 1025, 2049):
        coords = rows_in_supercells(rng, n, grid_lists, grid_lists[1][0], allowed) if n else \
            np.zeros((0, len(grid_lists[0]) + 1), np.int32)
        SpatialIndex(lib, device, coords, grid_lists, refuse=(n == 1025))


# =============================================================================================================================
# 4. me_kernel_map_probe / _compact / _count / _transpose (flat table)
# =============================================================================================================================
def me_region(device, D, kind, ks=3, dil=1, ts=1, offsets=None):
    """(me_region of the library, numpy function (in_coords, out_coords) -> reference nbr [volume, n_out])"""
    L, lib = _lib()
    as_list = lambda v: [int(v)] * D if np.isscalar(v) else [int(x) for x in v]       # noqa: E731
    ks, dil, ts = as_list(ks), as_list(dil), as_list(ts)
    if kind == CUSTOM:
        offs = torch.tensor(offsets, dtype=torch.int32)
        rg = L.make_region(D + 1, CUSTOM, ks, dil, ts, offs, device)
        step = np.asarray(dil) * np.asarray(ts)

        def ref(in_c, out_c):
            nbr = np.empty((len(offsets), len(out_c)), np.int32)
            for k, off in enumerate(offsets):
                q = out_c.copy()
                q[:, 1:] += (np.asarray(off) * step).astype(np.int32)
                nbr[k] = O.find(in_c, q)
            return nbr
    else:
        rg = L.make_region(D + 1, kind, ks, dil, ts)
        org = O.make_region(D, ks, dil, ts, kind)

        def ref(in_c, out_c):
            return O.kernel_map(in_c, out_c, org)[0]
    volume = int(lib.me_region_volume(ctypes.byref(rg)))
    return rg, volume, ref


def check_flat_kernel_map(lib, device, in_c, out_c, rg, volume, ref, pointers, refuse=False):
    """probe -> compact on one workspace, then count on a second one, then transpose; `pointers`: which of the host
    k_offsets / the device k_offsets_dev the probe gets"""
    n_out, n_in = len(out_c), len(in_c)
    nbr_ref = ref(in_c, out_c)
    in_ref, out_ref, koffs_ref = R.pair_lists(nbr_ref)
    n_pairs = int(koffs_ref[-1])
    ins = Insert(lib, device, in_c).run()
    assert ins.n_unique == n_in, "the in map of a kernel-map case must hold unique rows"
    oc = In(out_c, device)
    nbr = out_buf(volume * n_out, 4, device)
    koffs_dev = out_buf(volume + 1, 8, device) if pointers in ("dev", "both") else None
    in_pairs, out_pairs = out_buf(n_pairs, 4, device), out_buf(n_pairs, 4, device)
    ws = GuardedBytes(int(lib.me_kernel_map_workspace_bytes(n_out, volume)), device)
    outs = [nbr, in_pairs, out_pairs] + ([koffs_dev] if koffs_dev is not None else [])

    def probe(ws_ptr, ws_bytes):
        host = (ctypes.c_int64 * (volume + 1))(*[-5] * (volume + 1)) if pointers in ("host", "both") else None
        rc = lib.me_kernel_map_probe(ins.table.ptr(), ins.cap, ins.cu.ptr(), oc.ptr(), n_out, ctypes.byref(rg), nbr.ptr(),
                                     host, koffs_dev.ptr() if koffs_dev is not None else None, ws_ptr, ws_bytes, None)
        return rc, (tuple(host) if host is not None else ())

    def probe_and_compact(ws_ptr, ws_bytes):
        rc, host = probe(ws_ptr, ws_bytes)
        if rc == 0:
            rc = lib.me_kernel_map_compact(nbr.ptr(), n_out, volume, in_pairs.ptr(), out_pairs.ptr(), ws_ptr, ws_bytes, None)
        return rc, host
    host = run_guarded(lib, probe_and_compact, outs, ws)
    what = f"flat kernel map {n_in} -> {n_out} rows, volume {volume}, k_offsets: {pointers}"
    assert np.array_equal(np_of(nbr, torch.int32, (volume, n_out)), nbr_ref), f"{what}: nbr"
    if host:
        assert np.array_equal(np.asarray(host), koffs_ref), f"{what}: host k_offsets {host}"
    if koffs_dev is not None:
        assert np.array_equal(np_of(koffs_dev, torch.int64), koffs_ref), f"{what}: k_offsets_dev"
    assert np.array_equal(np_of(in_pairs, torch.int32), in_ref), f"{what}: in_pairs"
    assert np.array_equal(np_of(out_pairs, torch.int32), out_ref), f"{what}: out_pairs (per offset, by output row)"
    if refuse:
        refused_when_short(lib, probe, outs, ws)

        def compact(ws_ptr, ws_bytes):
            return lib.me_kernel_map_compact(nbr.ptr(), n_out, volume, in_pairs.ptr(), out_pairs.ptr(), ws_ptr, ws_bytes,
                                             None), ()
        refused_when_short(lib, compact, [in_pairs, out_pairs], ws)
    # me_kernel_map_count on the finished table, with a workspace of its own
    tbl = In(nbr_ref, device)
    count_dev = out_buf(volume + 1, 8, device)
    ws2 = GuardedBytes(int(lib.me_kernel_map_workspace_bytes(n_out, volume)), device)

    def count(ws_ptr, ws_bytes):
        host = (ctypes.c_int64 * (volume + 1))(*[-5] * (volume + 1)) if pointers != "dev" else None
        return lib.me_kernel_map_count(tbl.ptr(), n_out, volume, host, count_dev.ptr(), ws_ptr, ws_bytes, None), \
            (tuple(host) if host is not None else ())
    host = run_guarded(lib, count, [count_dev], ws2)
    assert np.array_equal(np_of(count_dev, torch.int64), koffs_ref), f"{what}: me_kernel_map_count"
    assert not host or np.array_equal(np.asarray(host), koffs_ref), f"{what}: me_kernel_map_count (host)"
    if refuse:
        refused_when_short(lib, count, [count_dev], ws2)
    # transpose of the reference pair lists
    ip, op, kd = In(in_ref, device), In(out_ref, device), In(koffs_ref, device)
    nbrT = out_buf(volume * n_in, 4, device)

    def transpose(_p, _b):
        return lib.me_kernel_map_transpose(ip.ptr(), op.ptr(), kd.ptr(), volume, n_pairs, n_in, nbrT.ptr(), None), ()
    run_guarded(lib, transpose, [nbrT], None)
    assert np.array_equal(np_of(nbrT, torch.int32, (volume, n_in)), R.transposed_table(in_ref, out_ref, koffs_ref, n_in)), \
        f"{what}: nbrT"
    return n_pairs


FLAT_N_OUT = (1, 63, 64, 65, 255, 256, 257, 1025)
FLAT_REGIONS = {
    # name: (kind, kernel size, dilation, out coordinates on multiples of)
    "volume_1": (CUBE, 1, 1, 1),
    "volume_8_even_kernel_stride_2_out": (CUBE, 2, 1, 2),
    "volume_27": (CUBE, 3, 1, 1),
    "cross_7_dilation_2": (CROSS, 3, 2, 1),
    "custom_5_offsets": (CUSTOM, 1, 1, 1),
}
CUSTOM_OFFSETS = [[0, 0, 0], [1, 0, -1], [-2, 3, 0], [0, 0, 4], [-1, -1, -1]]


@pytest.mark.parametrize("region", list(FLAT_REGIONS))
@pytest.mark.parametrize("n_out", FLAT_N_OUT)
def test_flat_kernel_map(device, lib, n_out, region):
    """k_kmap_probe (<NCOL, CUSTOM>), k_kmap_koffsets, k_kmap_compact, k_kmap_count and k_kmap_transpose on the 64-row
    wave and the 256-row block edges of the out map; the in map differs from the out map (for the even kernel the out
    rows lie on the stride-2 lattice); the probe gets the host k_offsets, k_offsets_dev (koffs then lives in the caller's
    array, nothing in the workspace slot, no synchronisation) or both, walking over the cases."""
    kind, ks, dil, lattice = FLAT_REGIONS[region]
    idx = FLAT_N_OUT.index(n_out) + list(FLAT_REGIONS).index(region)
    rng = np.random.default_rng(idx)
    D = 3
    side = max(4, int(round((3 * n_out) ** (1 / 3))) + 1)
    in_c = cloud(rng, min(2 * n_out + 40, (2 * side) ** 3 // 2), D, -side, side - 1, batches=(0, 1))
    out_c = cloud(rng, n_out, D, -side // lattice, (side - 1) // lattice, batches=(0, 1))
    out_c[:, 1:] *= lattice
    if kind == CUBE and ks == 1:
        out_c[::2] = in_c[:len(out_c[::2])]             # volume 1 only hits where the coordinates coincide
        out_c = unique_rows(out_c)
        out_c = np.ascontiguousarray(np.concatenate((out_c, cloud(rng, n_out, D, side, 2 * side))[:n_out]))
    rg, volume, ref = me_region(device, D, kind, ks, dil, 1, CUSTOM_OFFSETS)
    n_pairs = check_flat_kernel_map(lib, device, in_c, out_c, rg, volume, ref, ("host", "dev", "both")[idx % 3],
                                    refuse=(n_out == 257))
    assert n_pairs > 0 or n_out == 1, "the case is meant to have hits"


@pytest.mark.parametrize("pattern", ["no_hit", "every_probe_hits", "hits_only_in_the_last_wave"])
def test_flat_kernel_map_hit_patterns(device, lib, pattern):
    """n_pairs = 0 (empty pair lists, k_kmap_transpose not launched), every (row, offset) probe a hit (the pair lists at
    their bound n_out * volume), hits in the last wave of the last block only (rows 256 .. 299 of 300)"""
    rng = np.random.default_rng(5)
    full = cloud(rng, 1000, 3, 0, 9)                    # the whole 10^3 cube
    rg, volume, ref = me_region(device, 3, CUBE, 3)
    if pattern == "no_hit":
        out_c = cloud(rng, 300, 3, 1000, 1009)
    elif pattern == "every_probe_hits":
        out_c = cloud(rng, 512, 3, 1, 8)                # the whole interior
    else:
        out_c = np.concatenate((cloud(rng, 256, 3, 1000, 1009), cloud(rng, 44, 3, 1, 8)))
    n_pairs = check_flat_kernel_map(lib, device, full, out_c, rg, volume, ref, "dev")
    assert n_pairs == {"no_hit": 0, "every_probe_hits": 27 * 512, "hits_only_in_the_last_wave": 27 * 44}[pattern]


def test_transpose_grid_cap(device, lib):
    """k_kmap_transpose / k_kmap_transpose_ordered beyond the x-grid cap (bx > 4096): volume 1, 4096 * 256 + 1 pairs of
    the identity map — ceil(n / 256) = 4097 blocks are capped to 4096, and the last pair is the one that thread 0 of
    block 0 takes in a second step of the grid-stride loop; the ordered form writes through a reversed pos_in"""
    n = 4096 * 256 + 1
    rows = torch.arange(n, dtype=torch.int32, device=device)
    koffs = torch.tensor([0, n], dtype=torch.int64, device=device)
    for ordered in (False, True):
        nbrT = out_buf(n, 4, device)
        pos = rows.flip(0).contiguous()

        def launch(_p, _b):
            if ordered:
                return lib.me_kernel_map_transpose_ordered(rows.data_ptr(), rows.data_ptr(), koffs.data_ptr(), 1, n, n,
                                                           pos.data_ptr(), nbrT.ptr(), None), ()
            return lib.me_kernel_map_transpose(rows.data_ptr(), rows.data_ptr(), koffs.data_ptr(), 1, n, n, nbrT.ptr(),
                                               None), ()
        run_guarded(lib, launch, [nbrT], None)
        assert torch.equal(nbrT.view(torch.int32), pos if ordered else rows)


# =============================================================================================================================
# 5. me_kernel_map_probe_lds, me_kernel_map_compact_ordered, me_kernel_map_transpose_ordered
# =============================================================================================================================
def lds_bytes_formula(D, shift, halo, volume):
    """(halo grid + own cells + offset deltas + 2 * 3^D neighbour ranges + 2) int32 (me_kernel_map_probe_lds_bytes)"""
    return (int(np.prod([(1 << shift) + 2 * h for h in halo])) + (1 << shift) ** D + volume + 2 * 3 ** D + 2) * 4


def check_lds_kernel_map(lib, device, q_c, l_c, D, kind, ks, dil, shift, ts=1, with_offsets=True, refuse=False):
    """spatial indices of both maps (checked against their reference on the way), the LDS probe and the ordered
    compaction on one workspace, the ordered transpose; everything mapped back to row space against O.kernel_map.
    -> (launch cap, supercells of the query grid, LDS bytes, pair count)"""
    L, _ = _lib()
    tsl = [ts] * D
    rg = L.make_region(D + 1, kind, [ks] * D, [dil] * D, tsl)
    volume = int(lib.me_region_volume(ctypes.byref(rg)))
    iq = SpatialIndex(lib, device, q_c, R.grid_of(q_c, shift, tsl))
    il = SpatialIndex(lib, device, l_c, R.grid_of(l_c, shift, tsl))
    halo = [((ks - 1) if ks % 2 == 0 else ks // 2) * dil] * D
    lds = int(lib.me_kernel_map_probe_lds_bytes(ctypes.byref(rg), ctypes.byref(iq.grid), ctypes.byref(il.grid)))
    assert lds == lds_bytes_formula(D, shift, halo, volume), (lds, lds_bytes_formula(D, shift, halo, volume))
    n_q, n_l = len(q_c), len(l_c)
    nbr_ref = O.kernel_map(l_c, q_c, O.make_region(D, ks, dil, ts, kind))[0]            # row space
    pos_ref = nbr_ref[:, iq.order_np]                                                   # [k, query position]
    in_ref, out_ref, koffs_ref = R.pair_lists(pos_ref, out_rows=iq.order_np)
    n_pairs = int(koffs_ref[-1])
    nbr = out_buf(volume * n_q, 4, device)
    what = f"LDS kernel map {n_l} -> {n_q} rows, D={D} ks={ks} dil={dil} shift={shift}, {lds} bytes of LDS"
    if not with_offsets:                                 # k_offsets_dev == NULL: no counting, no workspace
        def probe_only(_p, _b):
            return lib.me_kernel_map_probe_lds(ctypes.byref(iq.grid), iq.sorted.ptr(), iq.dir.ptr(), n_q,
                                               ctypes.byref(il.grid), il.sorted.ptr(), il.order.ptr(), il.dir.ptr(),
                                               ctypes.byref(rg), nbr.ptr(), None, None, 0, None), ()
        run_guarded(lib, probe_only, [nbr], None)
        assert np.array_equal(np_of(nbr, torch.int32, (volume, n_q)), pos_ref), f"{what}: nbr_pos without counting"
        return None, iq.m, lds, n_pairs
    koffs_dev = out_buf(volume + 1, 8, device)
    in_pairs, out_pairs = out_buf(n_pairs, 4, device), out_buf(n_pairs, 4, device)
    ws = GuardedBytes(int(lib.me_kernel_map_workspace_bytes(n_q, volume)), device)
    outs = [nbr, koffs_dev, in_pairs, out_pairs]

    def probe(ws_ptr, ws_bytes):
        return lib.me_kernel_map_probe_lds(ctypes.byref(iq.grid), iq.sorted.ptr(), iq.dir.ptr(), n_q, ctypes.byref(il.grid),
                                           il.sorted.ptr(), il.order.ptr(), il.dir.ptr(), ctypes.byref(rg), nbr.ptr(),
                                           koffs_dev.ptr(), ws_ptr, ws_bytes, None), ()

    def compact(ws_ptr, ws_bytes):
        return lib.me_kernel_map_compact_ordered(nbr.ptr(), iq.order.ptr(), n_q, volume, in_pairs.ptr(), out_pairs.ptr(),
                                                 ws_ptr, ws_bytes, None), ()

    def probe_and_compact(ws_ptr, ws_bytes):
        rc, _ = probe(ws_ptr, ws_bytes)
        return (rc, ()) if rc else compact(ws_ptr, ws_bytes)
    run_guarded(lib, probe_and_compact, outs, ws)
    got = np_of(nbr, torch.int32, (volume, n_q))
    assert np.array_equal(got, pos_ref), f"{what}: nbr_pos"
    back = np.empty_like(got)
    back[:, iq.order_np] = got
    assert np.array_equal(back, nbr_ref), f"{what}: the table in row space"
    assert np.array_equal(np_of(koffs_dev, torch.int64), koffs_ref), f"{what}: k_offsets_dev against the table"
    assert np.array_equal(np_of(in_pairs, torch.int32), in_ref), f"{what}: in_pairs"
    assert np.array_equal(np_of(out_pairs, torch.int32), out_ref), f"{what}: out_pairs"
    if refuse:
        refused_when_short(lib, probe, outs, ws)
        refused_when_short(lib, compact, [in_pairs, out_pairs], ws)
    ip, op, kd = In(in_ref, device), In(out_ref, device), In(koffs_ref, device)
    nbrT = out_buf(volume * n_l, 4, device)

    def transpose(_p, _b):
        return lib.me_kernel_map_transpose_ordered(ip.ptr(), op.ptr(), kd.ptr(), volume, n_q * volume, n_l, il.pos.ptr(),
                                                   nbrT.ptr(), None), ()
    run_guarded(lib, transpose, [nbrT], None)
    assert np.array_equal(np_of(nbrT, torch.int32, (volume, n_l)),
                          R.transposed_table(in_ref, out_ref, koffs_ref, n_l, pos_in=il.pos_np)), f"{what}: nbrT"
    cap = 4 * 256 * (1 if lds > 40 * 1024 else 2)
    return cap, iq.m, lds, n_pairs


def two_maps(rng, D, inner, outer, n_pool, n_extra):
    """query and lookup maps of one tensor stride that overlap without coinciding: the lookup map is 70 % of a pool in
    [inner) with batches 2 and 3, the query map another 70 % of the pool plus rows in the wider [outer) with batches
    1, 2 and 3 — bounding boxes that differ on every axis and in the batch column, query supercells whose neighbours lie
    below and above the lookup directory, a query batch the lookup map does not have."""
    pool = cloud(rng, n_pool, D, inner[0], inner[1], batches=(2, 3))
    l_c = pool[rng.random(n_pool) < 0.7]
    extra = cloud(rng, n_extra, D, outer[0], outer[1], batches=(1, 2, 3))
    corners = np.array([[1] + [outer[0]] * D, [3] + [outer[1]] * D, [2] + [inner[0]] * D, [3] + [inner[1]] * D], np.int32)
    q_c = unique_rows(np.concatenate((pool[rng.random(n_pool) < 0.7], extra, corners)))
    l_c = unique_rows(np.concatenate((l_c, corners[2:])))
    return np.ascontiguousarray(q_c[rng.permutation(len(q_c))]), np.ascontiguousarray(l_c)


@pytest.mark.parametrize("D,shift,inner,outer,n_pool,n_extra", [(3, 2, (-3, 14), (-11, 25), 1500, 600),
                                                                (4, 1, (-2, 5), (-6, 9), 1200, 500)], ids=["3d", "4d"])
def test_lds_probe_two_different_maps(device, lib, D, shift, inner, outer, n_pool, n_extra):
    """k_kmap_probe_lds with gq != gl: the decode of the supercell uses gq.sc_min / gq.sc_dim, the 3^D neighbour ranges
    gl.sc_min / gl.sc_dim and the `inside` test (low and high side, a missing batch index)"""
    rng = np.random.default_rng(D)
    q_c, l_c = two_maps(rng, D, inner, outer, n_pool, n_extra)
    gq, gl = R.grid_of(q_c, shift, 1), R.grid_of(l_c, shift, 1)
    assert all(a != b for a, b in zip(gq[1], gl[1])) and all(a != b for a, b in zip(gq[2], gl[2])), (gq, gl)
    _, _, _, n_pairs = check_lds_kernel_map(lib, device, q_c, l_c, D, CUBE, 3, 1, shift, refuse=True)
    assert n_pairs > 0
    check_lds_kernel_map(lib, device, q_c, l_c, D, CROSS, 3, 1, shift)
    check_lds_kernel_map(lib, device, q_c, l_c, D, CUBE, 3, 1, shift, with_offsets=False)      # k_offsets_dev == NULL


@pytest.mark.parametrize("direction", ["query_is_a_subset", "lookup_is_a_subset"])
def test_lds_probe_strict_subset(device, lib, direction):
    """a pruned map against its parent and the other way round (_build_kernel_map_lds takes this path for any two maps
    of equal tensor stride), with a tensor stride of 2"""
    rng = np.random.default_rng(11)
    parent = cloud(rng, 1400, 3, -9, 12, batches=(0, 1))
    parent[:, 1:] *= 2
    child = np.ascontiguousarray(parent[rng.random(len(parent)) < 0.4][::-1])
    q_c, l_c = (child, parent) if direction == "query_is_a_subset" else (parent, child)
    _, _, _, n_pairs = check_lds_kernel_map(lib, device, q_c, l_c, 3, CUBE, 3, 1, 2, ts=2)
    assert n_pairs >= len(child)


def test_lds_probe_more_supercells_than_the_cap_of_2048(device, lib):
    """the grid-stride loop of k_kmap_probe_lds with at most 40 KiB of LDS (cap 4 * 256 * 2 = 2048 workgroups): 3-D, ks =
    3, supercells of 2^3 cells, 20^3 = 8000 directory entries and 3000 rows — most supercells empty (the `rows == 0`
    skip), s_grid / s_rng / s_qlin refilled for every further supercell of a workgroup; sparse rows: many supercells
    share one 64-position chunk (the atomicAdd count path)"""
    rng = np.random.default_rng(12)
    l_c = unique_rows(np.concatenate((cloud(rng, 3000, 3, 0, 39), [[0, 0, 0, 0], [0, 39, 39, 39]])))
    q_c = unique_rows(np.concatenate((l_c[rng.random(len(l_c)) < 0.6], cloud(rng, 800, 3, 0, 39),
                                      [[0, 0, 0, 0], [0, 39, 39, 39]])))
    cap, m_q, lds, n_pairs = check_lds_kernel_map(lib, device, q_c, l_c, 3, CUBE, 3, 1, 1)
    assert lds <= 40 * 1024 and cap == 2048 and m_q == 8000 and n_pairs > 0


def test_lds_probe_more_supercells_than_the_cap_of_1024(device, lib):
    """the same loop above 40 KiB of LDS (cap 4 * 256 = 1024): ks = 5 on supercells of 16^3 cells (halo grid 20^3: 49,108
    bytes), 11^3 = 1331 directory entries, rows in clusters"""
    rng = np.random.default_rng(13)
    centres = rng.integers(4, 172, size=(70, 3))
    pts = (centres[:, None, :] + rng.integers(-3, 4, size=(70, 45, 3))).reshape(-1, 3)
    rows = np.column_stack((np.zeros(len(pts), np.int64), pts))
    l_c = unique_rows(np.concatenate((rows, [[0, 0, 0, 0], [0, 175, 175, 175]])))
    q_c = np.ascontiguousarray(l_c[rng.permutation(len(l_c))])
    cap, m_q, lds, n_pairs = check_lds_kernel_map(lib, device, q_c, l_c, 3, CUBE, 5, 1, 4)
    assert lds == 49108 > 40 * 1024 and cap == 1024 and m_q == 1331 and n_pairs > len(q_c)


def test_lds_probe_largest_halo_and_refusals(device, lib):
    """me_kernel_map_probe_lds_bytes on the documented formula: 3-D, ks = 3 on 16^3 supercells is eligible up to dilation
    8 (halo grid 32^3: 147,788 bytes, beyond 48 KiB: the hipFuncAttributeMaxDynamicSharedMemorySize path, run here) and not at dilation 9 (173,932 bytes > 160 KiB - 256); a halo equal to
    the supercell side in 1-D is eligible (run); grids of different `shift` and a CUSTOM region are refused, by the size
    function (-1) and by the probe (non-zero, nothing written)"""
    L, _ = _lib()
    rng = np.random.default_rng(14)
    c = cloud(rng, 2500, 3, 0, 40)
    c[:40, 1:] = c[40:80, 1:] + 8                        # some rows exactly one dilated step apart
    c = unique_rows(c)
    _, _, lds, n_pairs = check_lds_kernel_map(lib, device, c, c, 3, CUBE, 3, 8, 4)
    assert lds == 147788 and n_pairs > len(c)
    g = make_grid(4, *R.grid_of(c, 4, [1] * 3))
    rg9 = L.make_region(4, CUBE, [3] * 3, [9] * 3, [1] * 3)
    assert lds_bytes_formula(3, 4, [9] * 3, 27) == 173932 > 160 * 1024 - 256
    assert lib.me_kernel_map_probe_lds_bytes(ctypes.byref(rg9), ctypes.byref(g), ctypes.byref(g)) == -1
    # 1-D: supercells of 2 cells, ks = 5 -> halo 2 == side
    c1 = cloud(rng, 70, 1, -50, 50, batches=(0, 1))
    _, _, lds, n_pairs = check_lds_kernel_map(lib, device, c1, c1, 1, CUBE, 5, 1, 1)
    assert lds == (6 + 2 + 5 + 6 + 2) * 4 and n_pairs > len(c1)
    rg7 = L.make_region(2, CUBE, [7], [1], [1])          # halo 3 > side 2
    g1 = make_grid(2, *R.grid_of(c1, 1, [1]))
    assert lib.me_kernel_map_probe_lds_bytes(ctypes.byref(rg7), ctypes.byref(g1), ctypes.byref(g1)) == -1
    # refusals of the probe itself: mismatched shift, CUSTOM region
    idx = SpatialIndex(lib, device, c, R.grid_of(c, 4, [1] * 3))
    g3 = make_grid(4, *R.grid_of(c, 3, [1] * 3))
    rg = L.make_region(4, CUBE, [3] * 3, [1] * 3, [1] * 3)
    custom = L.make_region(4, CUSTOM, [1] * 3, [1] * 3, [1] * 3, torch.tensor([[0, 0, 0], [1, 0, 0]], dtype=torch.int32),
                           device)
    nbr = out_buf(27 * len(c), 4, device)
    for region, lookup_grid in ((rg, g3), (custom, idx.grid)):
        assert lib.me_kernel_map_probe_lds_bytes(ctypes.byref(region), ctypes.byref(idx.grid), ctypes.byref(lookup_grid)) == -1
        nbr.fill(SENTINEL)
        rc = lib.me_kernel_map_probe_lds(ctypes.byref(idx.grid), idx.sorted.ptr(), idx.dir.ptr(), len(c),
                                         ctypes.byref(lookup_grid), idx.sorted.ptr(), idx.order.ptr(), idx.dir.ptr(),
                                         ctypes.byref(region), nbr.ptr(), None, None, 0, None)
        torch.cuda.synchronize()
        assert rc != 0 and b"not eligible" in lib.me_last_error()
        assert nbr.holds(SENTINEL) and nbr.intact()


def test_lds_probe_counts_on_dense_supercells(device, lib):
    """the plain-store count path of k_kmap_probe_lds: 3-D supercells of 8^3 cells, 92 % full, so a supercell owns whole
    64-position chunks (`*w = cnt`) and shares its first and last one (atomicAdd); k_offsets_dev against the table"""
    rng = np.random.default_rng(15)
    c = cloud(rng, int(0.92 * 16 ** 3), 3, 0, 15)
    _, m_q, _, n_pairs = check_lds_kernel_map(lib, device, c, c, 3, CUBE, 3, 1, 3)
    assert m_q == 8 and n_pairs > 20 * len(c)
    full = cloud(rng, 16 ** 3, 3, 0, 15)                 # every supercell exactly 512 rows: only owned chunks
    check_lds_kernel_map(lib, device, full, full, 3, CUBE, 2, 1, 3)


@pytest.mark.parametrize("n_q", [1, 64, 65])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_lds_probe_dimensions_and_small_queries(device, lib, D, n_q):
    """every instantiation k_kmap_probe_lds<2 .. 5> with 1, 64 and 65 query rows (one position, one whole chunk, a chunk
    and one position) taken from a lookup map of a few hundred rows with negative coordinates"""
    rng = np.random.default_rng(10 * D + n_q)
    hi = {1: 150, 2: 12, 3: 5, 4: 3}[D]
    l_c = cloud(rng, 250, D, -hi, hi, batches=(0, 1))
    q_c = np.ascontiguousarray(l_c[rng.permutation(len(l_c))[:n_q]])
    _, _, _, n_pairs = check_lds_kernel_map(lib, device, q_c, l_c, D, CUBE, 3, 1, 1)
    assert n_pairs >= n_q


# =============================================================================================================================
# 6. me_coords_stride, me_coords_expand_region, me_coords_quantize_labels
# =============================================================================================================================
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("ncol,ts", [(2, (3,)), (4, (2, 4, 1)), (5, (2, 2, 3, 5))])
def test_stride(device, lib, n, ncol, ts):
    """k_stride on the 256-thread edge: floor to the multiple of a per-axis stride for negative coordinates"""
    rng = np.random.default_rng(n + ncol)
    coords = rng.integers(-50, 50, size=(n, ncol)).astype(np.int32)
    coords[:4, 1:] = [[-1] * (ncol - 1), [0] * (ncol - 1), [-ts[0]] * (ncol - 1), [-ts[0] - 1] * (ncol - 1)]
    cin, out = In(coords, device), out_buf(n * ncol, 4, device)

    def launch(_p, _b):
        return lib.me_coords_stride(cin.ptr(), n, ncol, ints(ts), out.ptr(), None), ()
    run_guarded(lib, launch, [out], None)
    assert np.array_equal(np_of(out, torch.int32, (n, ncol)), O.stride_coordinates(coords, ts))
    assert cin.intact()


@pytest.mark.parametrize("aligned", [False, True], ids=["no_align_stride", "align_stride"])
@pytest.mark.parametrize("region", ["cube_3", "cube_2_ts_2", "cross_3_dilation_2", "custom"])
def test_expand_region(device, lib, region, aligned):
    """k_expand_region<NCOL, CUSTOM>: candidate (row, k) at row * volume + k, the `aligned` flags (one byte each: an
    output whose length is no multiple of 4) against O.region_coordinates, and its first-occurrence dedup against
    O.stride_region; 3-D and 2-D rows, n * volume on no block edge"""
    rng = np.random.default_rng(7)
    kind, ks, dil, ts = {"cube_3": (CUBE, 3, 1, 1), "cube_2_ts_2": (CUBE, 2, 1, 2), "cross_3_dilation_2": (CROSS, 3, 2, 1),
                         "custom": (CUSTOM, 1, 2, 1)}[region]
    for D, n in ((3, 67), (2, 1)):
        coords = cloud(rng, n, D, -6, 6, batches=(0, 1))
        coords[:, 1:] *= ts
        offsets = [o[:D] for o in CUSTOM_OFFSETS][:4 if D == 2 else 5]
        rg, volume, _ = me_region(device, D, kind, ks, dil, ts, offsets)
        if kind == CUSTOM:
            want = np.concatenate([coords + np.array([0] + [v * dil * ts for v in off], np.int32) for off in offsets], 1)
            want = want.reshape(n * volume, D + 1)
        else:
            want = O.region_coordinates(coords, O.make_region(D, ks, dil, ts, kind))
        align = [2 * ts] * D
        cin = In(coords, device)
        out, flags = out_buf(n * volume * (D + 1), 4, device), out_buf(n * volume, 1, device)

        def launch(_p, _b):
            return lib.me_coords_expand_region(cin.ptr(), n, D + 1, ctypes.byref(rg), ints(align) if aligned else None,
                                               out.ptr(), flags.ptr() if aligned else None, None), ()
        run_guarded(lib, launch, [out] + ([flags] if aligned else []), None)
        got = np_of(out, torch.int32, (n * volume, D + 1))
        assert np.array_equal(got, want), f"{region} D={D}: candidates"
        if aligned:
            keep = np_of(flags, torch.uint8).astype(bool)
            assert np.array_equal(keep, (want[:, 1:] % np.asarray(align) == 0).all(1)), f"{region} D={D}: aligned flags"
            got = got[keep]
        if kind != CUSTOM:
            assert np.array_equal(unique_rows(got) if len(got) else got,
                                  O.stride_region(coords, O.make_region(D, ks, dil, ts, kind), align if aligned else None))


@pytest.mark.parametrize("case", ["agree", "disagree", "disagree_in_the_last_row_only", "ignore_label_as_input"])
def test_quantize_labels(device, lib, case):
    """k_quantize_labels_init / _mark against O.quantize_label: 700 points in 257 voxels (the 256-thread edge of both
    kernels)"""
    rng = np.random.default_rng(9)
    n_vox, n, ignore = 257, 700, 255
    vox = cloud(rng, n_vox, 3, -4, 4)
    which = np.concatenate((rng.permutation(n_vox), rng.integers(0, n_vox - 1, n - n_vox)))    # every voxel; the last once
    which[-1] = which[0]                                                                     # the last row: a second point
    coords = np.ascontiguousarray(vox[which])
    vox_label = rng.integers(0, 20, n_vox).astype(np.int32)
    labels = vox_label[which].copy()
    if case == "disagree":
        labels[rng.random(n) < 0.3] += 1
    elif case == "disagree_in_the_last_row_only":
        labels[-1] += 1
    elif case == "ignore_label_as_input":
        labels[rng.random(n) < 0.2] = ignore             # as a voxel's first label and as a later, disagreeing one
        labels[0] = ignore
    um, inv, want = O.quantize_label(coords, labels, ignore)
    assert len(um) == n_vox
    if case == "disagree_in_the_last_row_only":
        assert (want == ignore).sum() == 1 and want[inv[-1]] == ignore
    um_d, inv_d, lab_d = In(um, device), In(inv, device), In(labels, device)
    out = out_buf(n_vox, 4, device)

    def launch(_p, _b):
        return lib.me_coords_quantize_labels(um_d.ptr(), n_vox, inv_d.ptr(), lab_d.ptr(), n, ignore, out.ptr(), None), ()
    run_guarded(lib, launch, [out], None)
    assert np.array_equal(np_of(out, torch.int32), want), case
