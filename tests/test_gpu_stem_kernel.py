"""The stacked-offset kernel itself (csrc/conv_stem.hip, k_conv_stem_bf16) on synthetic neighbour tables, through the C ABI:
dst[out_order[p]] = sum over offsets k of src[tbl[k][col_order[p]]] @ W[k]  (tbl entry -1: no neighbour), batch-norm
partials (mean, M2) per tile of me_conv_stem_tile_rows() tile POSITIONS p.

tests/test_gpu_stem.py drives the kernel through whole layers, where a workgroup walks one tile, both orders are the map's
own and every feature is finite.  Here the control flow around the walk is the subject: several tiles per workgroup
(me_debug_set_stem_tiles_per_wg: rings and statistics buffers reused, workgroups with one tile fewer), row counts on the
tile edges, offset counts on the quad / unroll edges (the walk covers the volume rounded up to 16: padded slots) up to the
largest volume the LDS admits, every weight form, col_order / out_order permutations, empty / dense / one-sided tables, a
poisoned row 0 behind the "no neighbour" mask, Inf / NaN rows, the partials against their fp32 error bound, the argument
checks.

Oracle: numpy float64 on the operands as the kernel sees them (bf16 features, weights rounded to bf16 by torch).  Two data
sets: EXACT data (integer features in [-8, 8], weights that round to multiples of 2^-6 in [-2, 2]: every fp32 partial sum
is exact in any order, so dst must equal the bf16 rounding of the fp64 sum BIT FOR BIT; the precondition
sum|products| * 2^6 < 2^24 is asserted) and RANDOM data (assert_bf16_close).  Besides the values: dst is bitwise the same
under every (G, tiles per workgroup), the partials under every tiles per workgroup at a fixed G, and nothing around the
buffers was touched: every buffer is a view into the MIDDLE of a larger tensor, NaN around the features and the weights, a
bit pattern around dst and both partial arrays, NaN inside them before every launch.  The surroundings of tbl, col_order
and out_order hold indices of those guard rows: a stray index read shows as a NaN or a damaged guard, never as an access
outside the tensors."""
import numpy as np
import pytest
import torch

from test_gpu_bf16 import assert_bf16_close, bf16_round

pytestmark = pytest.mark.gpu

PAD = 4096             # elements around every buffer (16-byte alignment kept; wider than any row here)
DST_SHIFT = 4          # dst starts 8 bytes off a 16-byte boundary: the kernel asks for 8-byte alignment only
NAN_BITS16 = 0x7fc1
SETTINGS = [(4, 0), (1, 2), (2, 3), (4, 2)]      # (G, tiles per workgroup; 0 = policy) of the tests away from the tile walk
WEIGHT_FORMS = [(1, 0), (0, 0), (1, 1), (0, 1)]  # (w_is_f32, transposed)


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


@pytest.fixture
def stem():
    """the kernel wherever its shape is supported (mode 1); the policy and both knobs restored afterwards"""
    _, lib = _lib()
    lib.me_debug_set_stem(1, 0)
    try:
        yield lib
    finally:
        lib.me_debug_set_stem(-1, 0)
        lib.me_debug_set_stem_tiles_per_wg(0)


# ---- data -------------------------------------------------------------------------------------------------------------
def exact_features(rng, n_src):
    return torch.from_numpy(rng.integers(-8, 9, size=(n_src, 8)).astype(np.float32))


def exact_weights(rng, volume, c_dst):
    """fp32 weights [K, 8, C] that round (RNE) to multiples of 2^-6 in [-2, 2]: such a value plus a perturbation below half
    a bf16 ulp — a quarter ulp at most, since below a power of two the spacing halves — and a few exact ties: value + half
    an ulp away from zero, which round back to the (even) value.  Returns (fed, rounded)."""
    m = rng.integers(-128, 129, size=(volume, 8, c_dst))
    w = (m / 64.0).astype(np.float32)
    _, e = np.frexp(np.abs(w))
    ulp = np.where(m != 0, np.ldexp(1.0, e - 8), 0.0)          # |w| in [2^(e-1), 2^e): 8 significant bits
    pert = rng.uniform(-0.24, 0.24, size=w.shape) * ulp
    ties = np.zeros(w.shape, bool)
    ties.reshape(-1)[rng.choice(np.flatnonzero(m), max(3, w.size // 50), replace=False)] = True
    pert[ties] = (np.sign(w) * 0.5 * ulp)[ties]
    fed = torch.from_numpy((w.astype(np.float64) + pert).astype(np.float32))
    assert not torch.equal(fed, torch.from_numpy(w))
    rounded = fed.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(rounded, torch.from_numpy(w)), "the perturbed weights must round to the multiples of 2^-6"
    return fed, rounded


def random_features(g, n_src):
    return bf16_round(torch.rand(n_src, 8, generator=g) - 0.3)


def random_weights(g, volume, c_dst):
    w = bf16_round(torch.rand(volume, 8, c_dst, generator=g) - 0.5)
    return w, w


def make_table(rng, kind, volume, n_tgt, n_src, tile_rows=256, first_row=0):
    """int32 [volume, n_tgt] of source rows in [first_row, n_src), -1 = no neighbour"""
    rows = rng.integers(first_row, n_src, size=(volume, n_tgt)).astype(np.int32)
    if kind == "dense":
        return rows
    if kind == "absent":
        return np.full((volume, n_tgt), -1, np.int32)
    if kind == "last_offset":                # the only present entries sit at offset volume - 1
        tbl = np.full((volume, n_tgt), -1, np.int32)
        half = rng.random(n_tgt) < 0.5
        tbl[volume - 1, half] = rows[volume - 1, half]
        return tbl
    tbl = np.where(rng.random((volume, n_tgt)) < 0.3, rows, -1).astype(np.int32)
    if kind == "tail_last_col":
        # the last, partial tile present at the last table column only — the column the lanes beyond n_tgt are clamped to
        start = (n_tgt - 1) // tile_rows * tile_rows
        assert start < n_tgt - 1 and n_tgt % tile_rows
        tbl[:, start:n_tgt - 1] = -1
        tbl[:, n_tgt - 1] = rows[:, n_tgt - 1]
    else:
        assert kind == "random", kind
    return tbl


def _middle(n, dtype, device, fill, pad=PAD, shift=0):
    """a view of n elements into the middle of a tensor of pad + shift + n + pad, everything set to `fill`"""
    big = torch.full((pad + shift + n + pad,), fill, dtype=dtype, device=device)
    return big, big[pad + shift:pad + shift + n]


def _pattern(n, dtype, device, base):
    return ((torch.arange(n, device=device) % 251) + base).to(dtype)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class _Case:
    """inputs of one launch shape on the device, and the float64 oracle — built once, launched many times"""

    def __init__(self, device, tbl, x, w_fed, w_rounded, form=(1, 0), col_order=None, out_order=None):
        L, lib = _lib()
        self.lib, self.check, self.device = lib, L.check, device
        volume, n_tgt = tbl.shape
        n_src, c_dst = x.shape[0], w_fed.shape[2]
        assert x.shape[1] == 8 and w_fed.shape[:2] == (volume, 8) and tbl.max() < n_src and tbl.min() >= -1
        assert torch.equal(x.to(torch.bfloat16).to(torch.float32).nan_to_num(7.0, 8.0, 9.0), x.nan_to_num(7.0, 8.0, 9.0))
        assert torch.equal(w_fed.to(torch.bfloat16).to(torch.float32), w_rounded)
        self.volume, self.n_tgt, self.n_src, self.c_dst, self.form = volume, n_tgt, n_src, c_dst, form
        self.col_order_host = np.arange(n_tgt) if col_order is None else np.asarray(col_order)
        self.out_order_host = np.arange(n_tgt) if out_order is None else np.asarray(out_order)
        # ---- the oracle, per tile POSITION p: sum_k x[tbl[k][col_order[p]]] @ W[k] in float64 ----
        x64, w64 = x.numpy().astype(np.float64), w_rounded.numpy().astype(np.float64)
        cols = tbl[:, self.col_order_host]
        ref_pos, mag = np.zeros((n_tgt, c_dst)), np.zeros((n_tgt, c_dst))
        with np.errstate(invalid="ignore"):
            for k in range(volume):
                m = cols[k] >= 0
                ref_pos[m] += x64[cols[k][m]] @ w64[k]
                mag[m] += np.abs(np.nan_to_num(x64[cols[k][m]], nan=0.0, posinf=0.0, neginf=0.0)) @ np.abs(w64[k])
        self.ref_pos, self.mag = ref_pos, mag
        self.ref = np.empty_like(ref_pos)
        self.ref[self.out_order_host] = ref_pos          # by output row
        # ---- device buffers: views into the middle of larger tensors ----
        nan = float("nan")
        self.src_big, self.src = _middle(n_src * 8, torch.bfloat16, device, nan)
        self.src.copy_(x.to(torch.bfloat16).reshape(-1))
        is_f32, transposed = form
        w_dev = (w_fed if is_f32 else w_rounded.to(torch.bfloat16))
        w_dev = (w_dev.permute(0, 2, 1) if transposed else w_dev).contiguous().reshape(-1)
        self.w_big, self.w = _middle(w_dev.numel(), w_dev.dtype, device, nan)
        self.w.copy_(w_dev)
        # a stray table read gives source row n_src: the NaN after the features; a stray col_order read gives column
        # volume * n_tgt: the table's surroundings again, under every offset; a stray out_order read gives output row n_tgt:
        # the pattern after dst (PAD is wider than a row)
        self.tbl_big, self.tbl = _middle(volume * n_tgt, torch.int32, device, n_src, pad=PAD + 2 * volume * n_tgt)
        self.tbl.copy_(torch.from_numpy(np.ascontiguousarray(tbl)).reshape(-1))
        self.index_tensors = [self.tbl_big]
        self.col_order = self.out_order = None
        if col_order is not None:
            big, self.col_order = _middle(n_tgt, torch.int32, device, volume * n_tgt)
            self.col_order.copy_(torch.from_numpy(self.col_order_host.astype(np.int32)))
            self.index_tensors.append(big)
        if out_order is not None:
            big, self.out_order = _middle(n_tgt, torch.int32, device, n_tgt)
            self.out_order.copy_(torch.from_numpy(self.out_order_host.astype(np.int32)))
            self.index_tensors.append(big)
        # the output and the partials as bit patterns: a position-dependent pattern around them, NaN inside before a launch
        n_out = n_tgt * c_dst
        self.dst_big = _pattern(2 * PAD + DST_SHIFT + n_out, torch.int16, device, 0x4000)
        self.dst = self.dst_big[PAD + DST_SHIFT:PAD + DST_SHIFT + n_out]
        self.n_part = -(-n_tgt // 64) * c_dst               # tiles of G = 1; a larger G fills a prefix
        self.part_big = [_pattern(2 * PAD + self.n_part, torch.int32, device, 0x40000000 + 1000 * i) for i in range(2)]
        self.part = [b[PAD:PAD + self.n_part] for b in self.part_big]
        self.guarded = [(self.dst_big, PAD + DST_SHIFT, n_out)] + [(b, PAD, self.n_part) for b in self.part_big]
        self.guards = [(b[:lo].clone(), b[lo + n:].clone()) for b, lo, n in self.guarded]
        self.inputs = [self.src_big, self.w_big] + self.index_tensors
        self.inputs_before = [t.clone() for t in self.inputs]
        assert self.src.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 8
        torch.cuda.synchronize()

    def exact(self):
        """dst must equal the bf16 rounding of the fp64 sum bit for bit: every fp32 partial sum is a multiple of 2^-6 below
        2^18 — exact in any order.  Returns the expected bits by output row."""
        finite = np.isfinite(self.ref)
        assert (self.mag * 64 < 2.0 ** 24).all(), "exact data: sum|products| * 2^6 must stay below 2^24"
        assert (np.where(finite, self.ref, 0.0) * 64 % 1 == 0).all()
        return _bits(torch.from_numpy(self.ref).to(torch.bfloat16))

    def call(self, groups, tiles_per_wg, partials=True, **over):
        """one call of me_conv_stem_bf16 (dst and the partials NaN before); returns the return code"""
        lib = self.lib
        self.dst.fill_(NAN_BITS16)
        for p in self.part:
            p.fill_(0x7fc00001)
        lib.me_debug_set_stem(1, groups)
        lib.me_debug_set_stem_tiles_per_wg(tiles_per_wg)
        ptr = lambda t: None if t is None else t.data_ptr()    # noqa: E731
        a = dict(src=ptr(self.src), n_src=self.n_src, c_src=8, w=ptr(self.w), volume=self.volume, c_dst=self.c_dst,
                 dst=ptr(self.dst), n_tgt=self.n_tgt, mean=ptr(self.part[0]) if partials else None,
                 m2=ptr(self.part[1]) if partials else None)
        a.update(over)
        rc = lib.me_conv_stem_bf16(a["src"], a["n_src"], a["c_src"], a["w"], self.form[0], self.form[1], a["volume"],
                                   a["c_dst"], ptr(self.tbl), ptr(self.col_order), ptr(self.out_order), a["dst"],
                                   a["n_tgt"], a["mean"], a["m2"], None)
        torch.cuda.synchronize()
        return rc

    def launch(self, groups, tiles_per_wg, partials=True, what=""):
        """-> (dst bf16 [n_tgt, c_dst], (mean, m2) fp32 [tiles, c_dst] or None); guards and unwritten partials checked"""
        self.check(self.call(groups, tiles_per_wg, partials))
        assert self.guards_intact(), f"{what}: the kernel wrote outside dst or the partials"
        out = self.dst.clone().view(torch.bfloat16).reshape(self.n_tgt, self.c_dst)
        used = -(-self.n_tgt // int(self.lib.me_conv_stem_tile_rows())) * self.c_dst if partials else 0
        for p in self.part:
            assert bool((p[used:] == 0x7fc00001).all()), f"{what}: partials written beyond the tiles (or without being asked)"
        parts = tuple(p[:used].clone().view(torch.float32).reshape(-1, self.c_dst) for p in self.part) if partials else None
        return out, parts

    def untouched(self):
        """dst and the partials still hold their NaN fill, the guards their pattern"""
        return (self.guards_intact() and bool((self.dst == NAN_BITS16).all()) and
                all(bool((p == 0x7fc00001).all()) for p in self.part))

    def guards_intact(self):
        return all(torch.equal(b[:lo], g[0]) and torch.equal(b[lo + n:], g[1])
                   for (b, lo, n), g in zip(self.guarded, self.guards))

    def inputs_intact(self):
        return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(self.inputs, self.inputs_before))

    # ---- the partials against float64 statistics of the STORED dst ----
    def check_partials(self, out, parts, what):
        """per tile of T tile positions, from the stored bf16 values: |mean - ref| <= c 2^-24 (|shift| + max|d|) and
        |M2 - ref| <= c 2^-22 sum d^2 with d about the tile's first row (the kernel's shift) and c = rows + 4 — fp32
        summation of at most c terms (d, d^2, the division, the shift added back; b - a m, each below sum d^2)"""
        T = int(self.lib.me_conv_stem_tile_rows())
        n = self.n_tgt
        tiles = -(-n // T)
        d_pos = out.double().cpu().numpy()[self.out_order_host]
        mean, m2 = (p.double().cpu().numpy() for p in parts)
        assert mean.shape == (tiles, self.c_dst) and m2.shape == mean.shape
        assert np.isfinite(mean).all() and np.isfinite(m2).all() and (m2 >= 0).all(), what
        counts, tol_mean = np.zeros(tiles), np.zeros_like(mean)
        for t in range(tiles):
            rows = d_pos[t * T:min((t + 1) * T, n)]
            c = len(rows) + 4
            d = rows - rows[0]
            ref_mean = rows.mean(0)
            ref_m2 = ((rows - ref_mean) ** 2).sum(0)
            counts[t] = len(rows)
            tol_mean[t] = c * 2.0 ** -24 * (np.abs(rows[0]) + np.abs(d).max(0))
            tol_m2 = c * 2.0 ** -22 * (d * d).sum(0)
            em, e2 = np.abs(mean[t] - ref_mean), np.abs(m2[t] - ref_m2)
            assert (em <= tol_mean[t]).all(), f"{what}: tile {t} ({len(rows)} rows) mean off by {em.max():.3g}"
            assert (e2 <= tol_m2).all(), f"{what}: tile {t} ({len(rows)} rows) M2 off by {e2.max():.3g}"
            assert (m2[t][(d == 0).all(0)] == 0).all(), f"{what}: tile {t}: M2 of a constant column is not exactly 0"
        # all tiles merged (Chan, in float64): the column variance of dst.  M2 = sum M2_t + sum n_t (mean_t - mu)^2: the
        # first sum within the tiles' own bounds, the second within sum n_t (4 |mean_t - mu| E + 4 E^2) for means off by
        # at most E each (mu moves by at most E as well)
        mu = (counts[:, None] * mean).sum(0) / n
        merged = m2.sum(0) + (counts[:, None] * (mean - mu) ** 2).sum(0)
        col = d_pos
        ref_total = ((col - col.mean(0)) ** 2).sum(0)
        E = tol_mean.max(0)
        tol = sum((min(T, n - t * T) + 4) * 2.0 ** -22 * ((d_pos[t * T:(t + 1) * T] - d_pos[t * T]) ** 2).sum(0)
                  for t in range(tiles))
        tol = tol + (counts[:, None] * (4 * np.abs(mean - mu) * E + 4 * E * E)).sum(0)
        ev = np.abs(merged - ref_total)
        assert (ev <= tol).all(), f"{what}: merged variance off by {(ev / n).max():.3g}"


def _equal_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run_settings(case, expect_bits=None, settings=SETTINGS, what="", partials=True):
    """the case under every (G, tiles per workgroup): dst against the oracle (bit for bit on exact data), bitwise the same
    under every setting, the partials within their bound; returns dst"""
    first = None
    for groups, tpw in settings:
        w = f"{what} G={groups} tiles/wg={tpw}"
        out, parts = case.launch(groups, tpw, partials, w)
        if first is None:
            first = out
            if expect_bits is not None:
                bad = (_bits(out).cpu() != expect_bits)
                assert not bool(bad.any()), f"{w}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result"
            else:
                assert bool(torch.isfinite(out.float()).all()), f"{w}: rows not written, or computed from the surroundings"
                assert_bf16_close(out.float().cpu().numpy(), case.ref, w)
        else:
            assert _equal_bits(out, first), f"{w}: bits differ from G={settings[0][0]} tiles/wg={settings[0][1]}"
        if partials:
            case.check_partials(out, parts, w)
    assert case.inputs_intact(), f"{what}: an input buffer or its surroundings changed"
    return first


def _exact_case(device, seed, kind, volume, c_dst, n_tgt, n_src=None, form=(1, 0), col_order=None, out_order=None,
                tile_rows=256, first_row=0):
    rng = np.random.default_rng(seed)
    n_src = max(2, n_tgt // 2) if n_src is None else n_src
    tbl = make_table(rng, kind, volume, n_tgt, n_src, tile_rows, first_row)
    w_fed, w_r = exact_weights(rng, volume, c_dst)
    return _Case(device, tbl, exact_features(rng, n_src), w_fed, w_r, form, col_order, out_order)


def _random_case(device, seed, kind, volume, c_dst, n_tgt, n_src=None, form=(1, 0), col_order=None, out_order=None,
                 tile_rows=256):
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    n_src = max(2, n_tgt // 2) if n_src is None else n_src
    tbl = make_table(rng, kind, volume, n_tgt, n_src, tile_rows)
    w_fed, w_r = random_weights(g, volume, c_dst)
    return _Case(device, tbl, random_features(g, n_src), w_fed, w_r, form, col_order, out_order)


# ---- offset counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_dst", [16, 32])
@pytest.mark.parametrize("volume", [1, 2, 3, 4, 5, 15, 16, 17, 27, 125])
def test_offset_counts_on_the_quad_and_unroll_edges(device, stem, volume, c_dst):
    """one quad with one to four live slots, the first slot of a second quad, one below / on / above the unroll of four
    quads, 27 and 125; 300 rows (five tiles of G = 1, a partial last tile under every G)"""
    assert stem.me_conv_stem_use_bf16(300, volume, 8, c_dst) == 1
    case = _exact_case(device, 100 * volume + c_dst, "random", volume, c_dst, 300)
    _run_settings(case, case.exact(), what=f"exact K={volume} C={c_dst}")
    case = _random_case(device, 100 * volume + c_dst + 1, "random", volume, c_dst, 300)
    _run_settings(case, None, SETTINGS[:2], what=f"random K={volume} C={c_dst}")


def _largest_volume(lib, n_tgt, c_dst):
    """the largest volume the policy takes in mode 1, by probing; every volume below it is taken, none above"""
    taken = [v for v in range(1, 1100) if lib.me_conv_stem_use_bf16(n_tgt, v, 8, c_dst) == 1]
    assert taken and taken == list(range(1, taken[-1] + 1)), taken[-5:]
    return taken[-1]


@pytest.mark.parametrize("c_dst", [16, 32, 64])
def test_largest_volume_the_lds_admits_and_one_more(device, stem, c_dst):
    n_tgt = 200
    volume = _largest_volume(stem, n_tgt, c_dst)
    assert volume % 16 == 0 and volume >= 64, volume        # (the LDS holds whole groups of four quads)
    case = _exact_case(device, 7000 + c_dst, "random", volume, c_dst, n_tgt)
    _run_settings(case, case.exact(), what=f"exact K={volume} C={c_dst}")
    case = _random_case(device, 7001 + c_dst, "dense", volume, c_dst, n_tgt)
    _run_settings(case, None, SETTINGS[:2], what=f"random dense K={volume} C={c_dst}")
    # one offset more: refused by the policy, an error from the entry point, dst untouched
    assert stem.me_conv_stem_use_bf16(n_tgt, volume + 1, 8, c_dst) == 0
    case = _random_case(device, 7002 + c_dst, "random", volume + 1, c_dst, n_tgt)
    for groups in (1, 2, 4):
        assert case.call(groups, 0) != 0
        assert case.untouched() and case.inputs_intact()


# ---- weight forms -------------------------------------------------------------------------------------------------------
def _form_cases():
    """a cross, not the product: every form on every c_dst, the volume alternating between 27 (padded slots) and 16 (none)
    so that every form meets both"""
    return [(form, c_dst, (27, 16)[(i + j) % 2]) for i, form in enumerate(WEIGHT_FORMS) for j, c_dst in enumerate((16, 32, 64))]


FORM_CASES = _form_cases()


def test_weight_form_cross_holds_every_form_on_both_volumes_and_every_width():
    for form in WEIGHT_FORMS:
        assert {v for f, _, v in FORM_CASES if f == form} == {16, 27}
        assert {c for f, c, _ in FORM_CASES if f == form} == {16, 32, 64}


@pytest.mark.parametrize("form,c_dst,volume", FORM_CASES,
                         ids=[f"{'f32' if f[0] else 'bf16'}-{'transposed' if f[1] else 'plain'}-c{c}-k{v}"
                              for f, c, v in FORM_CASES])
def test_weight_forms(device, stem, form, c_dst, volume):
    """fp32 / bf16 weights as [K, 8, C] and as [K, C, 8]: the same bits from all four forms of the same (exact) weights — the
    fp32 forms are rounded by the kernel, the bf16 forms hold torch's rounding"""
    seed = 9000 + volume + c_dst
    case = _exact_case(device, seed, "random", volume, c_dst, 300, form=form)
    out = _run_settings(case, case.exact(), SETTINGS[:2], what=f"exact form={form} K={volume} C={c_dst}")
    if form != (1, 0):
        plain = _exact_case(device, seed, "random", volume, c_dst, 300)
        assert _equal_bits(out, plain.launch(4, 0)[0])
    case = _random_case(device, seed, "random", volume, c_dst, 300, form=form)
    _run_settings(case, None, SETTINGS[:1], what=f"random form={form} K={volume} C={c_dst}")


# ---- the tile walk ------------------------------------------------------------------------------------------------------
WALK_G = (1, 2, 4)
WALK_TPW = (1, 2, 3, 5)
WALK_ROWS = sorted({n for g in WALK_G for n in (1, 64 * g - 1, 64 * g, 64 * g + 1, 7 * 64 * g + 5)})


def test_tile_walk_list_leaves_some_workgroups_a_tile_short():
    """(host only) the row counts are 1, T - 1, T, T + 1 and 7 T + 5 of every G's tile; some (rows, G, tiles per workgroup)
    gives workgroups of unequal length"""
    _, lib = _lib()
    try:
        for g in WALK_G:
            lib.me_debug_set_stem(-1, g)
            T = int(lib.me_conv_stem_tile_rows())
            assert T == 64 * g and {1, T - 1, T, T + 1, 7 * T + 5} <= set(WALK_ROWS)
    finally:
        lib.me_debug_set_stem(-1, 0)
    assert max(WALK_ROWS) == 1797
    tiles = lambda n, g: -(-n // (64 * g))                      # noqa: E731
    uneven = [(n, g, r) for n in WALK_ROWS for g in WALK_G for r in WALK_TPW if tiles(n, g) % -(-tiles(n, g) // r)]
    assert (453, 1, 3) in uneven and len(uneven) >= 6, uneven       # 8 tiles on 3 workgroups: 3, 3, 2


@pytest.mark.parametrize("n_tgt", WALK_ROWS)
def test_tile_walk_is_bitwise_the_same_under_every_tile_and_workgroup_shape(device, stem, n_tgt):
    """several tiles per workgroup: the rings start over, the statistics buffers alternate, the last workgroups walk a tile
    less; with partials and without.  dst: the same bits under every (G, tiles per workgroup); the partials: under every
    tiles per workgroup at a fixed G"""
    case = _exact_case(device, 4000 + n_tgt, "random", 27, 32, n_tgt)
    expect = case.exact()
    rnd = _random_case(device, 5000 + n_tgt, "random", 27, 32, n_tgt)
    for c, exp in ((case, expect), (rnd, None)):
        first = None
        for groups in WALK_G:
            parts_g = None
            for tpw in WALK_TPW:
                what = f"n={n_tgt} G={groups} tiles/wg={tpw} {'exact' if exp is not None else 'random'}"
                out, parts = c.launch(groups, tpw, True, what)
                if first is None:
                    first = out
                    if exp is not None:
                        assert torch.equal(_bits(out).cpu(), exp), what
                    else:
                        assert_bf16_close(out.float().cpu().numpy(), c.ref, what)
                else:
                    assert _equal_bits(out, first), f"{what}: dst differs from G=1 tiles/wg=1"
                if parts_g is None:
                    parts_g = parts
                    c.check_partials(out, parts, what)
                    if n_tgt % (64 * groups) > 1:        # the partial tile's count matters once its rows differ
                        T = 64 * groups
                        tail = out.float().cpu().numpy()[n_tgt // T * T:]
                        assert (tail != tail[0]).any(), "the partial tile must hold different rows"
                else:
                    assert all(_equal_bits(a, b) for a, b in zip(parts, parts_g)), f"{what}: partials differ from tiles/wg=1"
                out, parts = c.launch(groups, tpw, False, what + " no partials")
                assert parts is None and _equal_bits(out, first), f"{what}: dst differs without partials"
        assert c.inputs_intact()


# ---- orders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orders", ["none", "col", "out", "both"])
def test_col_order_and_out_order(device, stem, orders):
    """tbl[k][col_order[p]] feeds tile position p, the result goes to row out_order[p]; the partials belong to the tile
    POSITIONS (the oracle groups rows that way)"""
    n_tgt, rng = 453, np.random.default_rng(11)
    col = rng.permutation(n_tgt) if orders in ("col", "both") else None
    out = rng.permutation(n_tgt) if orders in ("out", "both") else None
    if orders == "both":
        assert (col != out).any()
    for volume in (27, 16):
        case = _exact_case(device, 600 + volume, "random", volume, 32, n_tgt, col_order=col, out_order=out)
        got = _run_settings(case, case.exact(), what=f"exact orders={orders} K={volume}")
        if orders != "none":
            # the same table without the orders: the rows are the same rows, elsewhere
            plain = _exact_case(device, 600 + volume, "random", volume, 32, n_tgt)
            base = plain.launch(4, 0)[0]
            assert not _equal_bits(got, base)
            moved = torch.empty_like(base)
            moved[torch.from_numpy(case.out_order_host).to(device)] = base[torch.from_numpy(case.col_order_host).to(device)]
            assert _equal_bits(got, moved)
    case = _random_case(device, 601, "random", 27, 16, n_tgt, col_order=col, out_order=out)
    _run_settings(case, None, SETTINGS[:2], what=f"random orders={orders}")


# ---- occupancy of the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_src", [("absent", 1), ("dense", None), ("random", None), ("last_offset", None),
                                        ("random", 1), ("tail_last_col", None)],
                         ids=["absent", "dense", "random", "last-offset-only", "row0-only", "tail-last-column"])
def test_table_occupancy(device, stem, kind, n_src):
    """n_src = 1 with a fully absent table still launches (only n_src = 0 is answered by a memset) and must give zeros;
    "row0-only": every present entry is source row 0, the row the absent entries load as well; "tail-last-column": the
    lanes beyond n_tgt are clamped to table column n_tgt - 1, the only present one of the partial tile — what they
    compute must reach neither dst nor the partials"""
    n_tgt = 300
    for volume, c_dst in ((27, 32), (16, 16), (5, 64)):
        for groups in (4, 1) if kind == "tail_last_col" else (4,):
            settings = [(groups, 0), (groups, 2)] if kind == "tail_last_col" else SETTINGS
            case = _exact_case(device, 800 + volume, kind, volume, c_dst, n_tgt, n_src=n_src, tile_rows=64 * groups)
            out = _run_settings(case, case.exact(), settings, what=f"exact {kind} K={volume} C={c_dst}")
            if kind == "absent":
                assert not bool(_bits(out).any()), "no neighbour anywhere: +0 everywhere"
            else:
                assert bool((out.float() != 0).any())
    case = _random_case(device, 801, kind, 27, 32, n_tgt, n_src=n_src)
    _run_settings(case, None, SETTINGS[:2], what=f"random {kind}")


# ---- the "no neighbour" mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", [27, 16])
def test_poisoned_row_0_behind_the_mask(device, stem, volume):
    """absent neighbours load source row 0 and are masked: with no table entry on row 0 the output must not depend on it —
    NaN or +Inf there, bit for bit the result of zeros (0 x finite = 0 would hide a broken mask)"""
    n_tgt, n_src = 300, 150
    rng = np.random.default_rng(volume)
    tbl = make_table(rng, "random", volume, n_tgt, n_src, first_row=1)
    assert tbl.max() > 0 and not (tbl == 0).any() and (tbl == -1).mean() > 0.5
    w_fed, w_r = exact_weights(rng, volume, 32)
    x = exact_features(rng, n_src)
    outs = {}
    for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
        xr = x.clone()
        xr[0] = fill
        case = _Case(device, tbl, xr, w_fed, w_r)
        assert np.isfinite(case.ref).all()
        outs[name] = _run_settings(case, case.exact(), what=f"row 0 = {name} K={volume}")
    assert _equal_bits(outs["nan"], outs["zero"]) and _equal_bits(outs["inf"], outs["zero"])


@pytest.mark.parametrize("volume", [27, 16])
def test_non_finite_rows_propagate_exactly(device, stem, volume):
    """one source row with +Inf in a channel, one with -Inf, one with NaN, each the neighbour of a few targets at several
    offsets — the last one, volume - 1, among them: that is the neighbour the padded slots beyond `volume` load (K = 27:
    five of them; K = 16: none).  Where the float64 oracle gives NaN / +Inf / -Inf so does the kernel, everywhere else the
    output is finite and exact: every element is compared.  (Before the padded slots were masked, K = 27 gave NaN in 148
    elements whose sum is +-Inf: 0 x Inf from the zero weight fragments of the slots beyond `volume`.)"""
    n_tgt, n_src = 300, 150
    rng = np.random.default_rng(50 + volume)
    tbl = make_table(rng, "random", volume, n_tgt, n_src, first_row=4)
    x = exact_features(rng, n_src)
    x[1, 2], x[2, 5], x[3, 0] = float("inf"), float("-inf"), float("nan")
    offsets = (0, volume // 2, volume - 1)
    targets = rng.permutation(n_tgt)[:27].reshape(3, 3, 3)       # [special row][offset][target]: all distinct
    for r in range(3):
        for o, k in enumerate(offsets):
            tbl[k, targets[r, o]] = r + 1
    t_both = targets[0, 2, 0]                                    # +Inf at the last offset and -Inf at the first
    tbl[0, t_both] = 2
    t_last_only = targets[0, 2, 1]                               # the +Inf row at the last offset and nothing else
    tbl[:volume - 1, t_last_only] = -1
    w_fed, w_r = exact_weights(rng, volume, 32)
    w_fed[:, :, :4] = w_fed[:, :, :4].abs() + 0.25               # columns that keep the sign of the Inf (+-Inf, not NaN) ...
    w_fed[:, :, 4:8] = 0.0                                       # ... and columns of 0 x Inf = NaN
    w_r = w_fed.to(torch.bfloat16).to(torch.float32)
    case = _Case(device, tbl, x, w_fed, w_r)
    ref = case.ref
    assert np.isposinf(ref[t_last_only, :4]).all() and np.isnan(ref[t_last_only, 4:8]).all()
    assert np.isnan(ref[targets[2].reshape(-1)]).all()
    assert np.isposinf(ref).any() and np.isneginf(ref).any() and np.isnan(ref).any()
    assert np.isfinite(ref).mean() > 0.8
    expect = case.exact()
    first = None
    for groups, tpw in SETTINGS:
        what = f"K={volume} G={groups} tiles/wg={tpw}"
        out, _ = case.launch(groups, tpw, False, what)
        got = out.double().cpu().numpy()
        for name, sel in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf), ("finite", np.isfinite)):
            bad = sel(ref) != sel(got)
            at = tuple(np.argwhere(bad)[0]) if bad.any() else None
            assert at is None, (f"{what}: {int(bad.sum())} elements are {name} on one side only, e.g. {at}: "
                                f"{got[at]} for {ref[at]}")
        fin = torch.from_numpy(np.isfinite(ref))
        assert torch.equal(_bits(out).cpu()[fin], expect[fin]), f"{what}: finite elements differ from the exact result"
        if first is None:
            first = out
        assert torch.equal(torch.isnan(out), torch.isnan(first)) and \
            _equal_bits(out.nan_to_num(0.0), first.nan_to_num(0.0)), what
    assert case.inputs_intact()


# ---- the partials -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 4])
def test_partials_constant_tile_and_first_row_maximum(device, stem, groups):
    """tile 1 holds one value per column (every row sees the same neighbour: M2 == 0 exactly, mean == the value); tile 2
    starts with its column-0 maximum (col_order swaps that row to the front: every d <= 0).  T + 1 and 7 T + 5 rows: the
    last tile counts 1 and 5 rows"""
    T = 64 * groups
    for n_tgt in (T + 1, 7 * T + 5):
        rng = np.random.default_rng(n_tgt)
        n_src = 200
        tbl = make_table(rng, "random", 27, n_tgt, n_src)
        if n_tgt > 2 * T:
            tbl[:, T:2 * T] = -1
            tbl[3, T:2 * T] = 17
        g = torch.Generator().manual_seed(n_tgt)
        w_fed, w_r = random_weights(g, 27, 32)
        x = random_features(g, n_src)
        probe = _Case(device, tbl, x, w_fed, w_r)
        col = np.arange(n_tgt)
        if n_tgt > 3 * T:
            top = 2 * T + int(np.argmax(probe.ref[2 * T:3 * T, 0]))
            col[[2 * T, top]] = col[[top, 2 * T]]
        case = _Case(device, tbl, x, w_fed, w_r, col_order=col)
        for tpw in (0, 2, 3):
            what = f"n={n_tgt} G={groups} tiles/wg={tpw}"
            out, (mean, m2) = case.launch(groups, tpw, True, what)
            assert_bf16_close(out.float().cpu().numpy(), case.ref, what)
            case.check_partials(out, (mean, m2), what)
            o = out.float()
            last = n_tgt // T * T
            assert mean.shape[0] == n_tgt // T + 1 and n_tgt - last in (1, 5)
            if n_tgt - last == 1:
                assert torch.equal(mean[-1], o[-1]) and not bool(m2[-1].any()), f"{what}: a tile of one row"
            if n_tgt > 3 * T:
                assert bool((o[T:2 * T] == o[T]).all()) and bool((o[T] != 0).any())
                assert torch.equal(mean[1], o[T]) and not bool(m2[1].any()), f"{what}: a constant tile"
                assert float(o[2 * T, 0]) == float(o[2 * T:3 * T, 0].max()) > float(o[2 * T:3 * T, 0].min())


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_argument_checks_leave_dst_untouched(device, stem):
    case = _random_case(device, 1, "random", 27, 32, 300)
    good = dict(src=case.src.data_ptr(), dst=case.dst.data_ptr(), mean=case.part[0].data_ptr(), m2=case.part[1].data_ptr())
    bad = {
        "c_src != 8": dict(c_src=16),
        "c_dst = 24": dict(c_dst=24),
        "source pointer off by 2 bytes": dict(src=good["src"] + 2),
        "dst pointer off by 2 bytes": dict(dst=good["dst"] + 2),
        "part_m2 NULL alone": dict(m2=None),
        "part_mean NULL alone": dict(mean=None),
    }
    for name, over in bad.items():
        assert case.call(4, 0, True, **over) != 0, name
        assert case.untouched(), f"{name}: refused, yet something was written"
        assert stem.me_last_error(), name
    # no target rows: nothing to do, nothing touched
    assert case.call(4, 0, True, n_tgt=0) == 0
    assert case.untouched() and case.inputs_intact()
    # ... and the same arguments, unchanged, run
    out, parts = case.launch(4, 0, True, "good arguments")
    assert_bf16_close(out.float().cpu().numpy(), case.ref, "good arguments")
