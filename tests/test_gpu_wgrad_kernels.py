"""The weight-gradient launches themselves (csrc/conv.hip k_wgrad_bf16, k_wgrad_f32x3, k_wgrad_f32, k_wgrad_reduce and the
reduce tail of csrc/wgrad_reduce.hpp) on synthetic pair lists, through the C ABI:
    grad_w[k] = sum over the pairs e of offset k of x[in[e]]^T (outer) dy[out[e]]
from me_conv_wgrad_bf16, me_conv_wgrad_f32 under me_debug_set_wgrad_config(-4, 0) (the split kernel) and (-3, 0) (the
fp32-MFMA kernel), and the two-launch order me_conv_wgrad_partials_f32 + me_conv_dgrad_reduce_tail_f32x3.

The layer tests feed these kernels the pair lists of uniform random clouds.  Here: offsets without pairs (first, last, a
run of them), pair counts around the kernels' steps (4 pairs: k_wgrad_f32; 32: k_wgrad_f32x3; 64: k_wgrad_bf16), totals
below one step, range boundaries (the list is cut into n_pairs r / n_ranges, whatever the offsets) on, before and behind
an offset boundary, repeated pairs, one row named by all pairs, volumes 1 / 27 / 125, every block shape of the dispatch,
poisoned rows that no pair names (row 0; the guard rows behind the last pair's rows, which the clamp of the index loads
to n_pairs - 1 must keep out), non-finite rows that are named, the launch order switch, the workspace check.
The host gives every range at least 64 pairs (wgrad_geom: ranges <= n_pairs / 64), so a range is never empty; lists
shorter than 64 pairs run as one range.

Oracle: numpy float64.  EXACT data: integer x and dy in [-8, 8] — every product and partial sum is an integer below 2^24
(asserted), so grad_w must equal the float64 sum exactly from every kernel, and the two-launch grad_w must be bit-identical
to me_conv_wgrad_f32's.  RANDOM data: |err| <= 2e-6 sum|x||dy| per element (test_gpu_conv.py::
test_wgrad_range_order_and_split_kernel), for the bf16 kernel on bf16-rounded operands.  Buffers as in
test_gpu_conv_tile_kernels.py: views into the middle of guard tensors, NaN inside grad_w and the workspace before a launch."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import Guarded, int_view, middle
from test_gpu_bf16 import bf16_round
from test_gpu_conv_tile_kernels import Case as ConvCase, Plan

pytestmark = pytest.mark.gpu

KERNELS = {"bf16": (0, 0), "split": (-4, 0), "mfma": (-3, 0)}      # me_debug_set_wgrad_config of each launch
# (c_in, c_out): 64-channel blocks whole and partial, c_out <= 64 / <= 128 / above 256 (the 1-, 2- and 4-block waves of
# k_wgrad_f32), 128 x 128 blocks of k_wgrad_bf16 (c_in >= 192, c_out > 64), rows that are no whole 16-byte pieces
# ((12, 20): the split kernel and k_wgrad_bf16 hand them to k_wgrad_f32; (10, 6): its scalar loads)
CHANNELS = [(32, 32), (64, 128), (40, 24), (72, 136), (192, 128), (128, 320), (64, 256), (12, 20), (10, 6), (8, 8)]


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _restore(lib):
    lib.me_debug_set_wgrad_config(0, 0)
    lib.me_debug_set_wgrad_order(0)
    lib.me_debug_set_wgrad_mb(0)
    lib.me_debug_set_dgrad_reduce_tail(0)
    lib.me_debug_set_conv_variant(0)


@pytest.fixture
def lib():
    _, lib = _lib()
    _restore(lib)
    try:
        yield lib
    finally:
        _restore(lib)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ranges_staged(n_pairs, c_in, c_out, wpc, mb=4):
    """wgrad_geom_staged of csrc/conv.hip: (ranges, floats per slot) of k_wgrad_f32x3 (wpc 3) / k_wgrad_bf16 (wpc 2)"""
    nb = 1 if c_out <= 64 else 2
    n_cib, n_cob = -(-c_in // (16 * mb)), -(-c_out // (16 * nb))
    gz = -(-n_cob // 4)
    r = -(-_cus() * (3 if n_cib == 3 else wpc) // (n_cib * gz))
    return max(1, min(r, n_pairs // 64)), n_cib * n_cob * mb * nb * 4 * 64


def ranges_direct(n_pairs, c_in, c_out):
    """wgrad_geom: k_wgrad_f32"""
    nb = 1 if c_out <= 64 else 2 if c_out <= 128 else 4
    n_cib, n_cob = -(-c_in // 64), -(-c_out // (16 * nb))
    gz = -(-n_cob // min(n_cob, 4))
    r = -(-_cus() * 3 // (n_cib * gz))
    return max(1, min(r, n_pairs // 64)), n_cib * n_cob * 4 * nb * 4 * 64


class WCase:
    """x, dy and the pair lists of one problem on the device, and the float64 oracle"""

    def __init__(self, device, dtype, counts, x, dy, in_pairs, out_pairs):
        L, self.lib = _lib()
        self.check, self.device, self.dtype = L.check, device, dtype
        self.volume = len(counts)
        self.n_in, self.c_in = x.shape
        self.n_out, self.c_out = dy.shape
        koffs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_pairs = int(koffs[-1])
        assert len(in_pairs) == len(out_pairs) == self.n_pairs
        assert self.n_pairs == 0 or (0 <= in_pairs.min() and in_pairs.max() < self.n_in and 0 <= out_pairs.min() and
                                     out_pairs.max() < self.n_out)
        if dtype == torch.bfloat16:
            for t in (x, dy):
                assert torch.equal(bf16_round(t).nan_to_num(7.0, 8.0, 9.0), t.nan_to_num(7.0, 8.0, 9.0))
        self.koffs_host_np, self.x_host, self.dy_host, self.in_host, self.out_host = koffs, x, dy, in_pairs, out_pairs
        x64, dy64 = x.numpy().astype(np.float64), dy.numpy().astype(np.float64)
        clean = lambda a: np.abs(np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0))   # noqa: E731
        self.ref = np.zeros((self.volume, self.c_in, self.c_out))
        self.mag = np.zeros_like(self.ref)
        with np.errstate(invalid="ignore"):
            for k in range(self.volume):
                e = slice(koffs[k], koffs[k + 1])
                if koffs[k + 1] > koffs[k]:
                    self.ref[k] = x64[in_pairs[e]].T @ dy64[out_pairs[e]]
                    self.mag[k] = clean(x64[in_pairs[e]]).T @ clean(dy64[out_pairs[e]])
        nan = float("nan")
        self.x_big, self.x = middle(x.numel(), dtype, device, nan)
        self.x.copy_(x.to(dtype).reshape(-1))
        self.dy_big, self.dy = middle(dy.numel(), dtype, device, nan)
        self.dy.copy_(dy.to(dtype).reshape(-1))
        # index loads beyond the list give the rows behind x and dy: NaN
        self.in_big, self.in_pairs = middle(self.n_pairs, torch.int32, device, self.n_in)
        self.in_pairs.copy_(torch.from_numpy(in_pairs.astype(np.int32)))
        self.out_big, self.out_pairs = middle(self.n_pairs, torch.int32, device, self.n_out)
        self.out_pairs.copy_(torch.from_numpy(out_pairs.astype(np.int32)))
        self.koffs_host = (ctypes.c_int64 * (self.volume + 1))(*koffs.tolist())
        self.koffs_big, self.koffs = middle(self.volume + 1, torch.int64, device, self.n_pairs)
        self.koffs.copy_(torch.from_numpy(koffs))
        self.grad_w = Guarded(self.ref.size, 4, device)
        fn = self.lib.me_conv_wgrad_workspace_bytes_bf16 if dtype == torch.bfloat16 else self.lib.me_conv_wgrad_workspace_bytes
        self.ws_bytes = int(fn(self.koffs_host, self.volume, self.c_in, self.c_out))
        self.ws = Guarded(self.ws_bytes // 4, 4, device, base=500)
        self.inputs = [self.x_big, self.dy_big, self.in_big, self.out_big, self.koffs_big]
        self.inputs_before = [t.clone() for t in self.inputs]
        torch.cuda.synchronize()

    def exact_precondition(self):
        assert (self.mag < 2.0 ** 24).all(), "exact data: sum|x||dy| must stay below 2^24"

    def args(self, **over):
        a = dict(x=self.x.data_ptr(), dy=self.dy.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        return a

    def call(self, kind, **over):
        """one launch of the kernel `kind`; grad_w and the workspace hold NaN before it.  Returns the return code."""
        lib = self.lib
        assert (kind == "bf16") == (self.dtype == torch.bfloat16)
        lib.me_debug_set_wgrad_config(*KERNELS[kind])
        self.grad_w.fill()
        self.ws.fill()
        a = self.args(**over)
        fn = lib.me_conv_wgrad_bf16 if kind == "bf16" else lib.me_conv_wgrad_f32
        rc = fn(a["x"], self.n_in, self.c_in, a["dy"], self.n_out, self.c_out, self.in_pairs.data_ptr(),
                self.out_pairs.data_ptr(), self.koffs_host, self.koffs.data_ptr(), self.volume, self.grad_w.ptr(),
                self.ws.ptr(), a["ws_bytes"], None)
        torch.cuda.synchronize()
        return rc

    def intact(self):
        return (all(torch.equal(int_view(a) if a.element_size() < 8 else a, int_view(b) if b.element_size() < 8 else b)
                    for a, b in zip(self.inputs, self.inputs_before)) and self.grad_w.intact() and self.ws.intact())

    def run(self, kind, what=""):
        self.check(self.call(kind))
        assert self.intact(), f"{what}: the launch wrote outside grad_w / the workspace, or into an input"
        return self.grad_w.as_dtype(torch.float32, self.ref.shape)


def make_pairs(rng, counts, n_in, n_out, first=0):
    n = int(np.sum(counts))
    return rng.integers(first, n_in, n), rng.integers(first, n_out, n)


def exact_rows(rng, n, c):
    return torch.from_numpy(rng.integers(-8, 9, size=(n, c)).astype(np.float32))


def random_rows(g, n, c, dtype):
    t = torch.rand(n, c, generator=g) - 0.3
    return bf16_round(t) if dtype == torch.bfloat16 else t


def _dtype(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def check_lists(device, kind, counts, c_in, c_out, seed, what, pairs=None, n_in=90, n_out=70, random=True):
    """the pair lists on exact data (grad_w == the float64 sum, offsets without pairs exact zeros) and on random data"""
    rng = np.random.default_rng(seed)
    in_pairs, out_pairs = make_pairs(rng, counts, n_in, n_out) if pairs is None else pairs
    dt = _dtype(kind)
    case = WCase(device, dt, counts, exact_rows(rng, n_in, c_in), exact_rows(rng, n_out, c_out), in_pairs, out_pairs)
    case.exact_precondition()
    got = case.run(kind, what).double().cpu().numpy()
    bad = got != case.ref
    assert not bad.any(), (f"{what} {kind} exact: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {case.ref[bad][0]}")
    for k in np.flatnonzero(np.asarray(counts) == 0):
        assert not int_view(case.grad_w.as_dtype(torch.float32, case.ref.shape)[k]).any(), f"{what}: offset {k} has no pairs: +0"
    if random:
        g = torch.Generator().manual_seed(seed)
        case = WCase(device, dt, counts, random_rows(g, n_in, c_in, dt), random_rows(g, n_out, c_out, dt), in_pairs, out_pairs)
        got = case.run(kind, what).double().cpu().numpy()
        assert np.isfinite(got).all(), f"{what} {kind}: elements not written, or computed from the surroundings"
        excess = np.abs(got - case.ref) - 2e-6 * case.mag
        assert (excess <= 0).all(), f"{what} {kind} random: error {np.abs(got - case.ref).max():.3g} above 2e-6 sum|x||dy|"
    return case


# offsets without pairs first, last and in a run; counts around the steps of 4 (k_wgrad_f32), 32 (k_wgrad_f32x3) and 64
# (k_wgrad_bf16) pairs and their doubles
STEP_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 0, 0, 0, 3, 4, 5, 127, 128, 129, 95, 96, 97, 7, 8, 9, 0]


@pytest.mark.parametrize("c_in,c_out", CHANNELS)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_pair_counts_on_the_step_edges(device, lib, kind, c_in, c_out):
    assert lib.me_conv_wgrad_is_split_f32(32, 32) == 1 and lib.me_conv_wgrad_is_split_f32(12, 20) == 0
    lib.me_debug_set_wgrad_config(*KERNELS[kind])
    if kind != "bf16":
        assert lib.me_conv_wgrad_is_split_f32(c_in, c_out) == int(kind == "split" and c_in % 8 == 0 and c_out % 8 == 0)
    check_lists(device, kind, STEP_COUNTS, c_in, c_out, c_in + c_out, "step edges")


@pytest.mark.parametrize("kind", list(KERNELS))
def test_short_lists_and_one_offset(device, lib, kind):
    """fewer pairs than one step; fewer than the 64 a range gets (one range); no pair at all (grad_w is still written:
    zeros); all pairs in one offset of 27"""
    for c_in, c_out in ((32, 32), (64, 128)):
        for name, counts in (("5 pairs", [0, 2, 0, 3]), ("63 pairs", [20, 0, 43]), ("no pair", [0, 0, 0]),
                             ("one pair", [0, 1]), ("one offset", [0] * 13 + [700] + [0] * 13)):
            check_lists(device, kind, counts, c_in, c_out, len(counts), name, random=(name == "one offset"))


@pytest.mark.parametrize("kind", list(KERNELS))
def test_range_boundaries_on_before_and_behind_offset_boundaries(device, lib, kind):
    """640 pairs are cut into 10 ranges of 64 (range r begins at 640 r / 10, computed as the kernel does and checked
    against the workspace size the library asks for): offsets end at 64 (on a range boundary), 127 (one before), 193
    (one behind), 320 twice (an empty offset on a boundary), 321, 639 (one pair in the last offset)"""
    c_in, c_out, n_pairs = 32, 64, 640
    bounds = [0, 64, 127, 193, 320, 320, 321, 639, 640]
    counts = np.diff(bounds).tolist()
    case = check_lists(device, kind, counts, c_in, c_out, 3, "range boundaries")
    if kind == "bf16":
        (r4, s4), (r8, s8) = ranges_staged(n_pairs, c_in, c_out, 2, 4), ranges_staged(n_pairs, c_in, c_out, 2, 8)
        ranges, need = r4, max(-(-(r4 + 8) * s4 * 4 // 256) * 256, -(-(r8 + 8) * s8 * 4 // 256) * 256)
    else:
        ranges = (ranges_staged(n_pairs, c_in, c_out, 3) if kind == "split" else ranges_direct(n_pairs, c_in, c_out))[0]
        need = 0
    (rd, sd), (rs, ss) = ranges_direct(n_pairs, c_in, c_out), ranges_staged(n_pairs, c_in, c_out, 3)
    need = max(need, -(-max((rd + 8) * sd, (rs + 8) * ss) * 4 // 256) * 256)
    assert case.ws_bytes == need, "the test's copy of the launch geometry is out of date"
    begins = [n_pairs * r // ranges for r in range(ranges)]
    assert ranges == 10 and {64, 128, 192, 320} <= set(begins)
    assert 64 in bounds and 127 in bounds and 193 in bounds and bounds.count(320) == 2


@pytest.mark.parametrize("kind", list(KERNELS))
def test_repeated_pairs_and_one_row(device, lib, kind):
    rng = np.random.default_rng(5)
    counts = [70, 0, 33, 130]
    n = sum(counts)
    same_pair = (np.full(n, 7), np.full(n, 11))
    one_in_row = (np.full(n, 3), rng.integers(0, 70, n))
    one_out_row = (rng.integers(0, 90, n), np.full(n, 69))
    for name, pairs in (("one pair repeated", same_pair), ("one x row", one_in_row), ("one dy row", one_out_row)):
        check_lists(device, kind, counts, 64, 128, 8, name, pairs=pairs)
    check_lists(device, kind, counts, 32, 32, 9, "one row each", pairs=(np.zeros(n, int), np.zeros(n, int)), n_in=1, n_out=1)


@pytest.mark.parametrize("volume", [1, 27, 125])
@pytest.mark.parametrize("kind", list(KERNELS))
def test_volumes(device, lib, kind, volume):
    rng = np.random.default_rng(volume)
    counts = rng.integers(0, 40, volume)
    counts[rng.random(volume) < 0.2] = 0
    counts[volume // 2] = 300
    check_lists(device, kind, counts.tolist(), 32, 64, volume, f"K={volume}")


@pytest.mark.parametrize("kind", list(KERNELS))
def test_launch_order_switch_gives_the_same_bits(device, lib, kind):
    """me_debug_set_wgrad_order 0 (ranges of the same list fraction to the same XCD: active from 64 ranges on, one workgroup
    per range) and -1 (launch order)"""
    c_in, c_out, counts = 32, 32, [400, 0, 900, 2500, 37, 1300]
    n_pairs = sum(counts)
    ranges = ranges_staged(n_pairs, c_in, c_out, 3 if kind == "split" else 2)[0] if kind != "mfma" else ranges_direct(n_pairs, c_in, c_out)[0]
    assert ranges >= 64
    rng = np.random.default_rng(2)
    g = torch.Generator().manual_seed(2)
    dt = _dtype(kind)
    case = WCase(device, dt, counts, random_rows(g, 90, c_in, dt), random_rows(g, 70, c_out, dt), *make_pairs(rng, counts, 90, 70))
    outs = []
    for mode in (0, -1, 0):
        lib.me_debug_set_wgrad_order(mode)
        outs.append(case.run(kind, f"order {mode}"))
    lib.me_debug_set_wgrad_order(0)
    assert torch.equal(int_view(outs[0]), int_view(outs[1])) and torch.equal(int_view(outs[0]), int_view(outs[2]))
    got = outs[0].double().cpu().numpy()
    assert (np.abs(got - case.ref) <= 2e-6 * case.mag).all()


# ---- poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KERNELS))
def test_poisoned_rows_that_no_pair_names(device, lib, kind):
    """x row 0 and dy row 0 NaN / +Inf with no pair naming them (index loads of masked pairs must not bring them in), the
    last pair naming the LAST rows of x and dy (finite; what follows them is the NaN of the guards, and the pair lists are
    surrounded by indices of those guard rows: the clamp to n_pairs - 1 keeps them out): grad_w finite, exact, bit for bit
    what zeros in row 0 give"""
    n_in, n_out = 90, 70
    for c_in, c_out in ((64, 128), (40, 24)):
        rng = np.random.default_rng(c_in)
        in_pairs, out_pairs = make_pairs(rng, STEP_COUNTS, n_in, n_out, first=1)
        in_pairs[-1], out_pairs[-1] = n_in - 1, n_out - 1
        x, dy = exact_rows(rng, n_in, c_in), exact_rows(rng, n_out, c_out)
        outs = {}
        for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
            xp, dyp = x.clone(), dy.clone()
            xp[0], dyp[0] = fill, fill
            case = WCase(device, _dtype(kind), STEP_COUNTS, xp, dyp, in_pairs, out_pairs)
            case.exact_precondition()
            outs[name] = case.run(kind, name)
            got = outs[name].double().cpu().numpy()
            assert np.array_equal(got, case.ref), f"{kind} {c_in}->{c_out} row 0 = {name}: {int((got != case.ref).sum())} elements differ"
        assert torch.equal(int_view(outs["nan"]), int_view(outs["zero"])) and torch.equal(int_view(outs["inf"]), int_view(outs["zero"]))


@pytest.mark.parametrize("kind", list(KERNELS))
def test_non_finite_rows_that_are_named(device, lib, kind):
    """x (the row side of the split) and dy (the weight side) with +Inf / -Inf / NaN in single elements of rows that pairs
    name, among them the first and the last pair of the list and of an offset: grad_w is non-finite wherever the float64
    reference is (and nowhere else: a masked pair or another channel block must not pick it up), and exact elsewhere"""
    n_in, n_out, inf = 90, 70, float("inf")
    for c_in, c_out in ((64, 128), (32, 32), (72, 136)):
        rng = np.random.default_rng(c_out)
        in_pairs, out_pairs = make_pairs(rng, STEP_COUNTS, n_in, n_out, first=4)
        koffs = np.concatenate([[0], np.cumsum(STEP_COUNTS)])
        in_pairs[0], in_pairs[-1], in_pairs[koffs[5]], in_pairs[koffs[15] - 1] = 1, 2, 3, 1
        out_pairs[koffs[2]], out_pairs[koffs[17] + 40] = 1, 2
        x, dy = exact_rows(rng, n_in, c_in), exact_rows(rng, n_out, c_out)
        x[1, 2], x[2, c_in - 1], x[3, 17] = inf, -inf, float("nan")
        dy[1, 3], dy[2, c_out - 1] = inf, float("nan")
        case = WCase(device, _dtype(kind), STEP_COUNTS, x, dy, in_pairs, out_pairs)
        case.exact_precondition()
        got = case.run(kind, "non-finite").double().cpu().numpy()
        bad = ~np.isfinite(case.ref)
        assert bad.any() and bad.mean() < 0.2
        wrong = ~np.isfinite(got) != bad
        assert not wrong.any(), (f"{kind} {c_in}->{c_out}: non-finite positions differ at {int(wrong.sum())} elements, first "
                                 f"{tuple(np.argwhere(wrong)[0])}: {got[wrong][0]} for {case.ref[wrong][0]}")
        assert np.array_equal(got[~bad], case.ref[~bad]), f"{kind} {c_in}->{c_out}: finite elements differ"


# ---- argument checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KERNELS))
def test_argument_checks_leave_grad_w_untouched(device, lib, kind):
    rng = np.random.default_rng(1)
    counts = [100, 0, 200]
    dt = _dtype(kind)
    case = WCase(device, dt, counts, exact_rows(rng, 90, 64), exact_rows(rng, 70, 128), *make_pairs(rng, counts, 90, 70))
    assert case.ws_bytes > 256
    for name, over in {"workspace one byte short": dict(ws_bytes=case.ws_bytes - 1), "workspace of 0 bytes": dict(ws_bytes=0),
                       "x off by 4 bytes": dict(x=case.x.data_ptr() + 4), "dy off by 8 bytes": dict(dy=case.dy.data_ptr() + 8)}.items():
        assert case.call(kind, **over) != 0, name
        assert case.grad_w.untouched() and case.ws.untouched() and case.intact() and lib.me_last_error(), name
    got = case.run(kind, "good arguments").double().cpu().numpy()
    assert np.array_equal(got, case.ref)


# ---- the two-launch order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in,c_out", [(64, 128), (128, 64), (40, 72), (256, 128)])
def test_two_launch_order_is_bit_identical_to_wgrad_f32(device, lib, c_in, c_out):
    """me_conv_wgrad_partials_f32, then me_conv_dgrad_reduce_tail_f32x3 on a plan of the transposed table: dx against the
    oracle of the tile kernels, grad_w bit for bit me_conv_wgrad_f32's (and exact on exact data).  The pair lists come from
    the table (in row r, out row tbl[k][r]); offsets 0, 4 and 5 hold no pair; T = 39 and a permuted order give partial and
    short tiles in front of the tail workgroups."""
    from test_gpu_conv_tile_kernels import make_table
    n_in, n_out, volume = 2 * 64 + 21, 100, 8
    rng = np.random.default_rng(c_in)
    tbl = make_table(rng, "random", volume, n_in, n_out)          # [volume, n_in]: out row of (offset, in row)
    tbl[[0, 4, 5]] = -1
    counts = (tbl >= 0).sum(1).tolist()
    ks, rs = np.nonzero(tbl >= 0)                                  # (offsets ascending: the pair list's layout)
    in_pairs, out_pairs = rs, tbl[ks, rs]
    lib.me_debug_set_wgrad_config(-4, 0)
    lib.me_debug_set_dgrad_reduce_tail(2)
    assert lib.me_conv_wgrad_is_split_f32(c_in, c_out) == 1
    assert lib.me_conv_dgrad_reduce_tail_supported(c_in, c_out, volume, len(rs)) == 1
    g = torch.Generator().manual_seed(c_out)
    for exact in (True, False):
        x = exact_rows(rng, n_in, c_in) if exact else random_rows(g, n_in, c_in, torch.float32)
        dy = exact_rows(rng, n_out, c_out) if exact else random_rows(g, n_out, c_out, torch.float32)
        w = torch.from_numpy(rng.integers(-128, 129, size=(volume, c_in, c_out)).astype(np.float32) / 64)
        case = WCase(device, torch.float32, counts, x, dy, in_pairs, out_pairs)
        want = case.run("split", "three launches")
        if exact:
            case.exact_precondition()
            assert np.array_equal(want.double().cpu().numpy(), case.ref)
        # the input gradient: source dy, weights W[k]^T — the forward kernel packed with transposed = 1
        wt = w.permute(0, 2, 1).contiguous()
        dgrad = ConvCase(device, tbl, dy, wt, wt, "f32")
        assert torch.equal(dgrad.wt.cpu(), w.reshape(-1))          # pack(1) reads the forward kernel [K, c_in, c_out]
        for T, order in ((64, None), (39, rng.permutation(n_in))):
            plan = Plan(dgrad, T, 4, order)
            wp = dgrad.pack(1)
            case.grad_w.fill()
            case.ws.fill()
            dgrad.dst.fill()
            lib.me_debug_set_wgrad_config(-4, 0)
            case.check(lib.me_conv_wgrad_partials_f32(case.x.data_ptr(), n_in, c_in, case.dy.data_ptr(), n_out, c_out,
                                                      case.in_pairs.data_ptr(), case.out_pairs.data_ptr(), case.koffs_host,
                                                      case.koffs.data_ptr(), volume, case.ws.ptr(), case.ws_bytes, None))
            assert case.grad_w.untouched()
            case.check(lib.me_conv_dgrad_reduce_tail_f32x3(dgrad.src.data_ptr(), n_out, c_out, wp.ptr(), volume, c_in,
                                                           *plan.ptrs(), dgrad.dst.ptr(), n_in, T, 4, case.koffs_host,
                                                           case.koffs.data_ptr(), case.ws.ptr(), case.ws_bytes,
                                                           case.grad_w.ptr(), None))
            torch.cuda.synchronize()
            assert case.intact() and dgrad.intact() and plan.intact(), "the two launches wrote outside their outputs"
            got = case.grad_w.as_dtype(torch.float32, case.ref.shape)
            assert torch.equal(int_view(got), int_view(want)), f"T={T}: grad_w differs from me_conv_wgrad_f32's"
            dx = dgrad.dst.as_dtype(torch.float32, (n_in, c_in)).double().cpu().numpy()
            if exact:
                dgrad.exact_precondition()
                assert np.array_equal(dx, dgrad.ref), f"T={T}: dx differs from the exact sum"
            else:
                assert (np.abs(dx - dgrad.ref) <= 2e-6 * dgrad.mag).all(), f"T={T}: dx"
        # a workspace smaller than me_conv_wgrad_workspace_bytes is refused by both launches
        case.grad_w.fill()
        assert lib.me_conv_wgrad_partials_f32(case.x.data_ptr(), n_in, c_in, case.dy.data_ptr(), n_out, c_out,
                                              case.in_pairs.data_ptr(), case.out_pairs.data_ptr(), case.koffs_host,
                                              case.koffs.data_ptr(), volume, case.ws.ptr(), case.ws_bytes - 1, None) != 0
        dgrad.dst.fill()
        assert lib.me_conv_dgrad_reduce_tail_f32x3(dgrad.src.data_ptr(), n_out, c_out, wp.ptr(), volume, c_in, *plan.ptrs(),
                                                   dgrad.dst.ptr(), n_in, T, 4, case.koffs_host, case.koffs.data_ptr(),
                                                   case.ws.ptr(), case.ws_bytes - 1, case.grad_w.ptr(), None) != 0
        torch.cuda.synchronize()
        assert case.grad_w.untouched() and dgrad.dst.untouched()
