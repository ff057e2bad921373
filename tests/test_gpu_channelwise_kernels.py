"""The channelwise-convolution launches themselves (csrc/conv_channelwise.hip: k_cw_forward, k_cw_backward_partial,
k_cw_backward_final and the float64 kernels) on synthetic neighbour tables, through the C ABI:
me_cwconv_forward_{f32,bf16,f64}, me_cwconv_backward_workspace_bytes, me_cwconv_backward_{f32,bf16,f64}.  The tables
tbl [volume, n_tgt] and tbl_t [volume, n_src] (int32, -1: none) are built with numpy; no coordinate manager is involved.

tests/test_gpu_channelwise.py drives these kernels through the module on uniform random clouds.  Here the claims of the
kernel file's header are the subject: the batches of KB = 8 offsets and the clamped last batch; the k-groups of 16 / 32
offsets, the fused dx and the separate dx pass with the same bits; every vector width, reached by the ADDRESS of an
operand; the (pieces x row lanes) split of a workgroup with idle threads, more than 256 pieces, fewer rows than lanes;
the chunks of source rows up to and beyond the cap of 512; n_src and n_tgt that differ or are 0; row 0 behind an
absent entry; non-finite rows that are named; the workspace size and the argument checks; bitwise reproducibility.

Oracle: numpy float64 on the operands as the kernel sees them (bf16 features rounded to bf16 first, fp32 weights and
bias), the header's formulas restated over the table (src[tbl] with a mask):
    dst[t] = bias + sum_k w[k] src[tbl[k, t]]      dx[i] = sum_k w[k] dy[tbl_t[k, i]]
    dW[k] = sum_i x[i] dy[tbl_t[k, i]]             db = sum_t dy[t]                  over present entries only.
EXACT data — integer features and gradients in [-8, 8] with 1 for 0, weights and bias multiples of 2^-6 in [-2, 2] —
under the asserted precondition 2^6 sum|terms| < 2^24 per output element: every term and every partial sum is a
multiple of 2^-6 below 2^18, hence an fp32 number, so the fp32 sum is exact in any order, with or without fma: fp32
results must EQUAL the float64 sum, bf16 results its one RNE rounding (np.array_equal: +0 == -0).
RANDOM data — uniform in [-0.5, 0.5] — under the bound |got - ref| <= E = 1.01 (m + 1) 2^-24 S per element, m the
number of terms and S the sum of their magnitudes (|bias| included): each partial sum of a summation tree over m terms
(products rounded once: fmaf, or exact products of bf16 x bf16) is off by at most 2^-24 of its magnitude <= S, there are
at most m of them on the way to an element (the zeros of idle lanes and absent chunks add exactly), and 1.01 covers
the second-order terms (1 + 2^-24)^m - 1 - m 2^-24 for m < 2^17.  A bf16 result adds its own rounding, 2^-8 (|ref| + E);
the float64 entry points take 2^-53 for 2^-24.  No bound is taken from the kernels' output.

Every input is a view into the middle of a NaN tensor (tables: of an out-of-range index), every output a Guarded
buffer holding a NaN pattern before the launch that must be gone from every element after it, the workspace a
GuardedBytes buffer of exactly the bytes the library asks for, filled with a NaN word."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import GUARD_PAD, Guarded, GuardedBytes, middle, same_nonfinite_class
from test_gpu_conv_tile_kernels import make_table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# csrc/conv_channelwise.hip: `constexpr int KB = 8;`, `constexpr int kCwRowsPerChunk = 256;`, `constexpr int
# kCwMaxChunks = 512;`, `cw_backward_v<T, 4, 16>` and `cw_backward_v<T, 1, 32>` (channels per thread, offsets per k-group)
KB = 8
K_ROWS_PER_CHUNK = 256
K_MAX_CHUNKS = 512
KG = {4: 16, 1: 32}
MAX_VOLUME = 65535

ELEM = {"f32": 4, "bf16": 2, "f64": 8}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
WEIGHT = {"f32": torch.float32, "bf16": torch.float32, "f64": torch.float64}
GRAD = {"f32": "f32", "bf16": "f32", "f64": "f64"}         # type of dW and db
UNIT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -24, "f64": 2.0 ** -53}
NAN_WORD, NAN64_WORD = 0x7fc00001, 0x7ff80001

TABLE_KINDS = ("dense", "absent", "first_offset", "last_offset", "one_row", "random")
FWD_VOLUMES = (1, 7, 8, 9, 16, 17, 27, 125)                # the KB = 8 batch edges
FWD_CHANNELS = (16, 12, 7)                                 # fp32: widths 4, 4, 1; bf16: 8, 4, 1
FWD_N_TGT, FWD_N_SRC = 130, 97
# (c, byte offsets of the operands from a 16-byte boundary) -> the width cw_launch_forward takes
FWD_PLACEMENTS = {
    "f32": [(8, {}, 4), (8, {"src": 8}, 1), (8, {"dst": 8}, 1), (8, {"w": 4}, 1), (8, {"bias": 4}, 1), (6, {}, 1), (7, {}, 1)],
    "bf16": [(16, {}, 8), (16, {"src": 8}, 4), (12, {}, 4), (16, {"src": 2}, 1), (16, {"w": 4}, 1), (7, {}, 1)],
}
BWD_VOLUMES = {4: (1, 8, 15, 16, 17, 32, 33), 1: (31, 32, 33, 65)}     # channels per thread -> volumes (KG 16 / 32)
BWD_CHANNELS = {4: 8, 1: 3}
# (c, byte offsets) -> channels per thread of cw_backward
BWD_PLACEMENTS = {
    "f32": [(8, {}, 4), (8, {"x": 4}, 1), (8, {"dy": 4}, 1), (8, {"dx": 4}, 1), (8, {"w": 4}, 1), (6, {}, 1)],
    "bf16": [(8, {}, 4), (8, {"dy": 2}, 1)],
}
BWD_PIECE_CHANNELS = (4, 12, 256, 255, 1024, 1028, 257)
BWD_ROWS = (1, 5, 255, 256, 257, 513)
BWD_ROWS_CAPPED = K_ROWS_PER_CHUNK * K_MAX_CHUNKS + 1      # 131073: 512 chunks of 256 or 257 rows
BWD_N_SRC, BWD_N_TGT = 300, 200


# ---- Python mirrors of the launch rules (piece.hpp, cw_launch_forward, cw_backward) -----------------------------------------
def _al(offsets, b):
    return all(o is None or o % b == 0 for o in offsets)


def forward_width(e, c, src=0, dst=0, w=0, bias=0):
    """channels per thread of k_cw_forward for e-byte features: operands given as byte offsets from a 16-byte boundary"""
    if not _al([w, bias], 16):
        return 1
    a = 16 if _al([src, dst], 16) else 8 if _al([src, dst], 8) else 1
    if c % (16 // e) == 0 and a == 16:
        return 16 // e
    if e == 2 and c % 4 == 0 and a >= 8:
        return 4
    return 1


def backward_plan(e, c, volume, need_dx, x=0, dy=0, dx=0, w=0):
    v = 4 if c % 4 == 0 and _al([x, dy, dx if need_dx else None], 4 * e) and _al([w], 16) else 1
    kgroups = -(-volume // KG[v])
    P = c // v
    return dict(v=v, kg=KG[v], kgroups=kgroups, fused=bool(need_dx) and kgroups == 1, P=P, R=256 // min(P, 256))


def n_chunks(n):
    return min(-(-max(n, 1) // K_ROWS_PER_CHUNK), K_MAX_CHUNKS)


def chunk_bounds(n):
    g = n_chunks(n)
    return [i * n // g for i in range(g + 1)]


# ---- data -----------------------------------------------------------------------------------------------------------------
def _as_seen(a, dt):
    """float64 of the values after the conversion to the feature type"""
    if dt == "f64":
        return a.astype(np.float64)
    t = torch.from_numpy(a.astype(np.float32))
    return (t.bfloat16() if dt == "bf16" else t).double().numpy()


def features(rng, data, shape, dt, hi=8):
    if data == "exact":
        a = rng.integers(-hi, hi + 1, size=shape).astype(np.float64)
        a[a == 0] = 1.0
        return a
    return _as_seen(rng.uniform(-0.5, 0.5, size=shape), dt)


def weights(rng, data, shape, dt):
    if data == "exact":
        return rng.integers(-128, 129, size=shape) / 64.0
    return _as_seen(rng.uniform(-0.5, 0.5, size=shape), "f64" if dt == "f64" else "f32")


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def oracle_forward(src, w, bias, tbl, mutant=None):
    """(ref, S, m) [n_tgt, c]: the float64 result, the sum of the magnitudes of its terms and their number.  `mutant`
    restates a WRONG kernel (test_inputs_*): "row0" adds row 0 for an absent entry, "drop_last" loses the last offset,
    "drop_tail" the offsets behind the last full batch of KB, "no_bias" the bias."""
    volume, n_tgt = tbl.shape
    c = w.shape[1]
    if mutant == "drop_last":
        tbl = tbl.copy()
        tbl[volume - 1] = -1
    if mutant == "drop_tail":
        tbl = tbl.copy()
        tbl[volume // KB * KB:] = -1
    mask = tbl >= 0
    with np.errstate(invalid="ignore"):
        if src.shape[0] == 0:
            terms = np.zeros((volume, n_tgt, c))
        else:
            terms = w[:, None, :] * src[np.where(mask, tbl, 0)]
            if mutant != "row0":
                terms = np.where(mask[:, :, None], terms, 0.0)
        ref, S = terms.sum(0), np.abs(terms).sum(0)
    m = np.repeat(mask.sum(0)[:, None], c, 1)
    if bias is not None and mutant != "no_bias":
        ref, S, m = ref + bias, S + np.abs(bias), m + 1
    return ref, S, m


def oracle_backward(x, dy, w, tbl_t, mutant=None, plan=None):
    """{"dx", "dw", "db"} -> (ref, S, m).  Mutants: "chunk_last_row" loses the last source row of every chunk in dW,
    "last_lane" the rows of the last row lane (plan["R"]), "db_n_src" sums db over n_src rows of dy (NaN behind its end),
    "no_second_kgroup" leaves dW of offsets [KG, 2 KG) at 0."""
    volume, n_src = tbl_t.shape
    n_tgt, c = dy.shape
    mask = tbl_t >= 0
    m3 = mask[:, :, None]
    with np.errstate(invalid="ignore"):
        g = np.zeros((volume, n_src, c)) if n_tgt == 0 else dy[np.where(mask, tbl_t, 0)]
        tdx = np.where(m3, w[:, None, :] * g, 0.0)
        tdw = np.where(m3, x[None, :, :] * g, 0.0)
        keep = np.ones(n_src, bool)
        b = chunk_bounds(n_src)
        if mutant == "chunk_last_row":
            keep[[r - 1 for r in b[1:] if r > 0]] = False
        if mutant == "last_lane":
            for r0, r1 in zip(b[:-1], b[1:]):
                keep[r0 + plan["R"] - 1:r1:plan["R"]] = False
        tdw, mdw = tdw[:, keep], mask[:, keep].sum(1)
        dw, sdw = tdw.sum(1), np.abs(tdw).sum(1)
        if mutant == "no_second_kgroup":
            dw[plan["kg"]:2 * plan["kg"]] = 0.0
        rows = dy
        if mutant == "db_n_src":
            rows = np.concatenate([dy, np.full((max(n_src - n_tgt, 0), c), np.nan)])[:n_src]
        db, sdb = rows.sum(0), np.abs(rows).sum(0)
    return {"dx": (tdx.sum(0), np.abs(tdx).sum(0), np.repeat(mask.sum(0)[:, None], c, 1)),
            "dw": (dw, sdw, np.repeat(mdw[:, None], c, 1)),
            "db": (db, sdb, np.full(c, rows.shape[0]))}


def _wide(dt, *arrays):
    """the operands of a float64 entry point in extended precision: the oracle of a 2^-53 bound has to be finer than
    2^-53 (x87 long double, 2^-64: its own summation error is then 2^-11 of the bound, inside the factor 1.01)"""
    if dt != "f64":
        return arrays
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    return tuple(None if a is None else a.astype(np.longdouble) for a in arrays)


def exact_holds(S):
    """the precondition of EXACT data: 2^6 sum|terms| < 2^24 for every output element"""
    return bool((64.0 * S < 2.0 ** 24).all())


def compare(got, ref, S, m, dt, data, what):
    """EXACT: equality with the float64 sum (bf16: with its RNE rounding).  Otherwise the bound of the file's docstring on
    the finite elements and the same non-finite class everywhere."""
    got = got.double().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if data == "exact":
        assert np.isfinite(ref).all() and exact_holds(S), f"{what}: exact data: 2^6 sum|terms| must stay below 2^24"
        want = torch.from_numpy(ref).float().bfloat16().double().numpy() if dt == "bf16" else ref
        if not np.array_equal(got, want):
            at = tuple(np.argwhere(got != want)[0])
            raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} elements differ, e.g. {at}: "
                                 f"{got[at]!r} for {want[at]!r}")
        return
    assert int(m.max(initial=0)) < 2 ** 17
    same_nonfinite_class(got, ref, what)
    fin = np.isfinite(ref)
    E = 1.01 * (m + 1) * UNIT[dt] * np.where(fin, S, 0.0)
    if dt == "bf16":
        E = E + 2.0 ** -8 * (np.abs(np.where(fin, ref, 0.0)) + E)
    err = np.where(fin, np.abs(got - np.where(fin, ref, 0.0)), 0.0)
    if not (err <= E).all():
        at = np.unravel_index(np.argmax(err - E), err.shape)
        raise AssertionError(f"{what}: element {at}: {got[at]!r} for {ref[at]!r}, off by {err[at]:.3e} > {E[at]:.3e} "
                             f"({int(m[at])} terms, sum of magnitudes {S[at]:.3e})")


# ---- device buffers ------------------------------------------------------------------------------------------------------
def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _put(keep, t, device, off=0, fill=float("nan")):
    """the address of a copy of t in the middle of a tensor of `fill`, `off` bytes behind a 16-byte boundary"""
    flat = t.reshape(-1)
    e = flat.element_size()
    assert off % e == 0
    big, mid = middle(flat.numel() + off // e, flat.dtype, device, fill)
    if flat.numel():
        mid[off // e:].copy_(flat)
    addr = big.data_ptr() + GUARD_PAD * e + off           # (data_ptr() of an empty view is NULL)
    assert (addr - off) % 16 == 0
    keep.append(big)
    return addr


class Out:
    """An output of n elements of type dt, `off` bytes behind a 16-byte boundary, in a guard pattern; `spare` more elements
    behind it that no launch may touch (an output of no rows still has an address)."""

    def __init__(self, n, dt, device, off=0, spare=0):
        self.n, self.dt, self.total = n, dt, n + spare
        if dt == "f64":
            assert off == 0
            self.g = GuardedBytes(8 * self.total, device)
        else:
            self.g = Guarded(self.total, ELEM[dt], device, shift=off // ELEM[dt])
        assert self.total > 0
        self.fill()

    def fill(self):
        self.g.fill(NAN64_WORD) if self.dt == "f64" else self.g.fill()

    def ptr(self):
        return self.g.ptr()

    def _bits(self):
        return self.g.view(torch.int64) if self.dt == "f64" else self.g.bits

    def _nan(self):
        return (NAN64_WORD << 32) | NAN64_WORD if self.dt == "f64" else self.g.nan

    def untouched(self):
        return bool((self._bits() == self._nan()).all())

    def written(self):
        """every element inside holds something else than the pattern, every spare element still the pattern"""
        b = self._bits()
        return bool((b[:self.n] != self._nan()).all()) and bool((b[self.n:] == self._nan()).all())

    def intact(self):
        return self.g.intact()

    def bits(self):
        return self._bits()[:self.n].clone().cpu()

    def values(self, shape):
        return self._bits()[:self.n].clone().view(TORCH[self.dt]).reshape(shape).cpu()


def launch_forward(device, dt, src, w, bias, tbl, n_src, c, place=None, src_null=False):
    """me_cwconv_forward_<dt>(src, w, bias or NULL, tbl) into a fresh guarded dst, which it returns"""
    L, lib = _lib()
    place = place or {}
    volume, n_tgt = tbl.shape
    keep = []
    a_src = None if src_null else _put(keep, src, device, place.get("src", 0))
    a_w = _put(keep, w, device, place.get("w", 0))
    a_b = None if bias is None else _put(keep, bias, device, place.get("bias", 0))
    a_tbl = _put(keep, torch.from_numpy(np.ascontiguousarray(tbl)), device, 0, n_src)   # a stray read: the NaN behind src
    dst = Out(n_tgt * c, dt, device, place.get("dst", 0), spare=c if n_tgt == 0 else 0)
    L.check(getattr(lib, "me_cwconv_forward_" + dt)(a_src, c, a_w, a_b, a_tbl, n_src, n_tgt, volume, dst.ptr(), None))
    torch.cuda.synchronize()
    assert dst.intact(), "the forward wrote outside dst"
    assert dst.written(), "the forward left elements of dst unwritten (or wrote behind its rows)"
    return dst


def launch_backward(device, dt, x, dy, w, tbl_t, c, need_dx=1, dbias=True, place=None):
    """me_cwconv_backward_<dt> with a workspace of exactly the bytes asked for -> {"dx", "dw", "db"} of guarded outputs"""
    L, lib = _lib()
    place = place or {}
    volume, n_src = tbl_t.shape
    n_tgt = dy.shape[0]
    keep = []
    a_x = _put(keep, x, device, place.get("x", 0))
    a_dy = _put(keep, dy, device, place.get("dy", 0))
    a_w = _put(keep, w, device, place.get("w", 0))
    a_tbl = _put(keep, torch.from_numpy(np.ascontiguousarray(tbl_t)), device, 0, n_tgt)
    out = {"dx": Out(n_src * c, dt, device, place.get("dx", 0), spare=c if n_src == 0 else 0),
           "dw": Out(volume * c, GRAD[dt], device), "db": Out(c, GRAD[dt], device)}
    ws, a_ws, ws_bytes = None, None, 0
    if dt != "f64" and (n_src or n_tgt):                    # float64 and the empty problem need none
        ws_bytes = int(lib.me_cwconv_backward_workspace_bytes(n_src, volume, c))
        ws = GuardedBytes(ws_bytes, device)
        ws.fill(NAN_WORD)
        a_ws = ws.ptr()
    L.check(getattr(lib, "me_cwconv_backward_" + dt)(a_x, a_dy, c, a_w, a_tbl, n_src, n_tgt, volume, need_dx,
                                                     out["dx"].ptr() if need_dx else None, out["dw"].ptr(),
                                                     out["db"].ptr() if dbias else None, a_ws, ws_bytes, None))
    torch.cuda.synchronize()
    assert all(o.intact() for o in out.values()) and (ws is None or ws.intact()), "the backward wrote outside a buffer"
    assert out["dw"].written(), "elements of dW were left unwritten"
    assert out["dx"].written() if need_dx else out["dx"].untouched(), "dx: unwritten elements, or written without need_dx"
    assert out["db"].written() if dbias else out["db"].untouched()
    return out


class Fwd:
    """one forward problem: host operands as float64 (the values the kernel sees), their oracle, the launch.  Source
    rows that no entry names hold NaN."""

    def __init__(self, dt, data, tbl, c, n_src, rng, bias=True, hi=8, poison=True):
        self.dt, self.data, self.tbl, self.c, self.n_src = dt, data, tbl, c, n_src
        volume, self.n_tgt = tbl.shape
        assert tbl.dtype == np.int32 and tbl.min(initial=-1) >= -1 and tbl.max(initial=-1) < max(n_src, 0)
        self.src = features(rng, data, (n_src, c), dt, hi)
        self.w = weights(rng, data, (volume, c), dt)
        self.bias = weights(rng, data, (c,), dt) if bias else None
        self.named = np.zeros(n_src, bool)
        self.named[tbl[tbl >= 0]] = True
        if poison:
            self.src[~self.named] = np.nan
        self.ref, self.S, self.m = oracle_forward(*_wide(dt, self.src, self.w, self.bias), tbl)

    def run(self, device, place=None, src_null=False):
        t = lambda a, d: None if a is None else torch.from_numpy(a).to(d)      # noqa: E731
        return launch_forward(device, self.dt, t(self.src, TORCH[self.dt]), t(self.w, WEIGHT[self.dt]),
                              t(self.bias, WEIGHT[self.dt]), self.tbl, self.n_src, self.c, place, src_null)

    def check(self, dst, what):
        compare(dst.values((self.n_tgt, self.c)), self.ref, self.S, self.m, self.dt, self.data, f"{what}: dst")


class Bwd:
    """one backward problem.  Rows of x whose every entry is -1 hold NaN; with poison_dy the rows of dy that no entry
    names do too (then db, the sum of all of them, is not asked for)."""

    def __init__(self, dt, data, tbl_t, c, n_tgt, rng, hi_x=8, hi_dy=8, poison_dy=False):
        self.dt, self.data, self.tbl_t, self.c, self.n_tgt, self.poison_dy = dt, data, tbl_t, c, n_tgt, poison_dy
        volume, self.n_src = tbl_t.shape
        assert tbl_t.dtype == np.int32 and tbl_t.min(initial=-1) >= -1 and tbl_t.max(initial=-1) < max(n_tgt, 0)
        self.x = features(rng, data, (self.n_src, c), dt, hi_x)
        self.dy = features(rng, data, (n_tgt, c), dt, hi_dy)
        self.w = weights(rng, data, (volume, c), dt)
        self.x[(tbl_t < 0).all(0)] = np.nan
        self.named = np.zeros(n_tgt, bool)
        self.named[tbl_t[tbl_t >= 0]] = True
        if poison_dy:
            self.dy[~self.named] = np.nan
        self.ref = oracle_backward(*_wide(dt, self.x, self.dy, self.w), tbl_t)

    def tensors(self):
        return (torch.from_numpy(self.x).to(TORCH[self.dt]), torch.from_numpy(self.dy).to(TORCH[self.dt]),
                torch.from_numpy(self.w).to(WEIGHT[self.dt]))

    def run(self, device, need_dx=1, dbias=True, place=None):
        assert not (dbias and self.poison_dy)
        x, dy, w = self.tensors()
        return launch_backward(device, self.dt, x, dy, w, self.tbl_t, self.c, need_dx, dbias, place)

    def check(self, out, need_dx, dbias, what):
        shapes = {"dx": (self.n_src, self.c), "dw": (self.tbl_t.shape[0], self.c), "db": (self.c,)}
        for name in ("dx",) * bool(need_dx) + ("dw",) + ("db",) * bool(dbias):
            dt = self.dt if name == "dx" else GRAD[self.dt]
            compare(out[name].values(shapes[name]), *self.ref[name], dt, self.data, f"{what}: {name}")

    def dx_by_forward(self, device, place=None):
        """dx as me_cwconv_forward_<dt>(dy, w, bias = NULL, tbl_t) gives it"""
        _, dy, w = self.tensors()
        place = {"src": place.get("dy", 0), "dst": place.get("dx", 0), "w": place.get("w", 0)} if place else None
        return launch_forward(device, self.dt, dy, w, None, self.tbl_t, self.n_tgt, self.c, place)


def _rng(*key):
    return np.random.default_rng([7] + [int(k) for k in key])


def fwd_case(dt, data, kind, volume, c, bias=True, n_tgt=FWD_N_TGT, n_src=FWD_N_SRC, first_row=0, poison=True):
    rng = _rng(1, TABLE_KINDS.index(kind), volume, c, n_tgt, n_src)
    tbl = make_table(rng, kind, volume, n_tgt, n_src, first_row=first_row)
    return Fwd(dt, data, tbl, c, n_src, rng, bias=bias, poison=poison)


def bwd_case(dt, data, kind, volume, c, n_src=BWD_N_SRC, n_tgt=BWD_N_TGT, first_row=0, poison_dy=False, hi_x=8, hi_dy=8):
    rng = _rng(2, TABLE_KINDS.index(kind), volume, c, n_src, n_tgt)
    tbl_t = make_table(rng, kind, volume, n_src, n_tgt, first_row=first_row)
    return Bwd(dt, data, tbl_t, c, n_tgt, rng, hi_x=hi_x, hi_dy=hi_dy, poison_dy=poison_dy)


def sparse_wide_table(rng, n_rows, n_named, volume=MAX_VOLUME, density=0.02):
    """[volume, n_rows] with few entries, the first offset and the last KB + 1 offsets present in row 1"""
    tbl = np.where(rng.random((volume, n_rows)) < density, rng.integers(0, n_named, (volume, n_rows)), -1).astype(np.int32)
    tbl[0, 1] = 0
    tbl[volume - KB - 1:, 1] = n_named - 1
    return tbl


# =====================================================================================================================
# CPU-side checks of the inputs (no GPU)
# =====================================================================================================================
def test_inputs_constants_match_the_source():
    src = open(os.path.join(HERE, "..", "minkowskiengine_amd", "csrc", "conv_channelwise.hip")).read()
    assert int(re.search(r"constexpr int KB = (\d+);", src).group(1)) == KB
    assert int(re.search(r"constexpr int kCwRowsPerChunk = (\d+);", src).group(1)) == K_ROWS_PER_CHUNK
    assert int(re.search(r"constexpr int kCwMaxChunks = (\d+);", src).group(1)) == K_MAX_CHUNKS
    assert int(re.search(r"constexpr int kCwMaxVolume = (\d+);", src).group(1)) == MAX_VOLUME
    kg = {int(v): int(k) for v, k in re.findall(r"cw_backward_v<T, (\d+), (\d+)>\(", src)}
    assert kg == KG


def test_inputs_placements_reach_every_width_and_both_backward_kernels():
    for dt, widths in (("f32", {4, 1}), ("bf16", {8, 4, 1})):
        got = [forward_width(ELEM[dt], c, **place) for c, place, _ in FWD_PLACEMENTS[dt]]
        assert got == [v for _, _, v in FWD_PLACEMENTS[dt]] and set(got) == widths, (dt, got)
        assert {forward_width(ELEM[dt], c) for c in FWD_CHANNELS} == widths
        plans = [backward_plan(ELEM[dt], c, 16, 1, **place) for c, place, _ in BWD_PLACEMENTS[dt]]
        assert [p["v"] for p in plans] == [v for _, _, v in BWD_PLACEMENTS[dt]] and {p["v"] for p in plans} == {4, 1}
        # a dx that is not asked for does not count
        assert backward_plan(ELEM[dt], 8, 16, 0, dx=ELEM[dt])["v"] == 4 and backward_plan(ELEM[dt], 8, 16, 1, dx=ELEM[dt])["v"] == 1
        # fused and unfused, one and several k-groups, at both widths; bf16 fused at 4 channels per thread (volume <= 16)
        for v, c in BWD_CHANNELS.items():
            p = [backward_plan(ELEM[dt], c, vol, 1) for vol in BWD_VOLUMES[v]]
            assert all(q["v"] == v for q in p) and {q["fused"] for q in p} == {True, False}
            assert {q["kgroups"] for q in p} >= {1, 2, 3}
            assert not any(backward_plan(ELEM[dt], c, vol, 0)["fused"] for vol in BWD_VOLUMES[v])
        assert backward_plan(2, 8, 8, 1)["fused"] and backward_plan(2, 8, 16, 1)["fused"] and not backward_plan(2, 8, 17, 1)["fused"]
    assert backward_plan(4, 4, MAX_VOLUME, 1)["kgroups"] == 4096
    # pieces per row and row lanes; the idle threads
    pr = {c: backward_plan(4, c, 3, 1) for c in BWD_PIECE_CHANNELS}
    assert [(pr[c]["v"], pr[c]["P"], pr[c]["R"]) for c in BWD_PIECE_CHANNELS] == \
        [(4, 1, 256), (4, 3, 85), (4, 64, 4), (1, 255, 1), (4, 256, 1), (4, 257, 1), (1, 257, 1)]
    assert 85 * 3 == 255 and 255 * 1 == 255               # thread 255 has no (row lane, piece)


def test_inputs_chunk_list():
    counts = {n: n_chunks(n) for n in BWD_ROWS + (BWD_ROWS_CAPPED,)}
    assert counts == {1: 1, 5: 1, 255: 1, 256: 1, 257: 2, 513: 3, BWD_ROWS_CAPPED: 512}
    assert np.diff(chunk_bounds(257)).tolist() == [128, 129]
    assert np.diff(chunk_bounds(513)).tolist() == [171, 171, 171]
    d = np.diff(chunk_bounds(BWD_ROWS_CAPPED))
    assert set(d.tolist()) == {256, 257} and (d == 257).sum() == 1 and d.sum() == BWD_ROWS_CAPPED
    assert 5 < backward_plan(4, 8, 2, 1)["R"]             # fewer rows than row lanes
    assert n_chunks(0) == 1 and chunk_bounds(0) == [0, 0]


def _capped_case(dt):
    # x in [-2, 2], dy = +-1: sum|x dy| over 131073 rows is about 1.4 * 131073, times 2^6 below 2^24 (asserted)
    return bwd_case(dt, "exact", "dense", 2, 4, n_src=BWD_ROWS_CAPPED, n_tgt=777, hi_x=2, hi_dy=1)


def _wide_fwd(dt):
    rng = _rng(3)
    return Fwd(dt, "exact", sparse_wide_table(rng, 3, 11), 4, 11, rng, hi=2)


def _wide_bwd(dt):
    rng = _rng(4)
    return Bwd(dt, "exact", sparse_wide_table(rng, 3, 5), 4, 5, rng, hi_x=2, hi_dy=2)


def test_inputs_exact_cases_meet_the_precondition():
    for kind in TABLE_KINDS:
        for volume in FWD_VOLUMES:
            for c in FWD_CHANNELS:
                assert exact_holds(fwd_case("f32", "exact", kind, volume, c).S), (kind, volume, c)
    for v, c in BWD_CHANNELS.items():
        for volume in BWD_VOLUMES[v]:
            for kind in ("dense", "random", "last_offset"):
                p = bwd_case("f32", "exact", kind, volume, c)
                assert all(exact_holds(p.ref[k][1]) for k in ("dx", "dw", "db")), (kind, volume, c)
    for c in BWD_PIECE_CHANNELS:
        p = bwd_case("f32", "exact", "dense", 3, c)
        assert all(exact_holds(p.ref[k][1]) for k in ("dx", "dw", "db")), c
    for n in BWD_ROWS:
        for c in (8, 3):
            for volume in (3, 17):
                for kind in ("dense", "random"):
                    p = bwd_case("f32", "exact", kind, volume, c, n_src=n, n_tgt=max(n, 2))
                    assert all(exact_holds(p.ref[k][1]) for k in ("dx", "dw", "db")), (n, c, volume, kind)
    for p in (_capped_case("f32"), _wide_bwd("f32")):
        assert all(exact_holds(p.ref[k][1]) for k in ("dx", "dw", "db"))
    assert exact_holds(_wide_fwd("f32").S)


def _differs(a, b):
    return not np.array_equal(a, b, equal_nan=True)


def forward_mutant_must_coincide(mutant, kind, volume, tbl):
    """the tables on which a wrong kernel is right by construction — the ONLY cases in which a mutant may equal the oracle"""
    if mutant == "row0":                                    # no absent entry to replace
        return kind == "dense"
    if mutant == "drop_last":                               # nothing at the last offset
        return kind == "absent" or (kind == "first_offset" and volume > 1)
    if mutant == "drop_tail":                               # no partial batch, or nothing in it
        return volume % KB == 0 or kind == "absent" or (kind == "first_offset" and volume > KB)
    return False                                            # the bias is never 0 everywhere


@pytest.mark.parametrize("poison", [False, True])
def test_inputs_forward_mutants_differ_from_the_oracle(poison):
    for kind in TABLE_KINDS:
        for volume in FWD_VOLUMES:
            p = fwd_case("f32", "exact", kind, volume, 7, poison=poison)
            for mutant in ("row0", "drop_last", "drop_tail", "no_bias"):
                wrong = oracle_forward(p.src, p.w, p.bias, p.tbl, mutant)[0]
                assert _differs(wrong, p.ref) == (not forward_mutant_must_coincide(mutant, kind, volume, p.tbl)), \
                    (mutant, kind, volume)


def test_inputs_backward_mutants_differ_from_the_oracle():
    seen = set()
    for c, volumes in ((8, (3, 17, 33)), (3, (3, 33, 65)), (255, (3,))):
        for n_src in BWD_ROWS + (BWD_N_SRC,):
            for volume in volumes:
                for n_tgt in (n_src, 3 * n_src, max(n_src // 3, 1)):
                    p = bwd_case("f32", "exact", "dense", volume, c, n_src=n_src, n_tgt=n_tgt)
                    plan = backward_plan(4, c, volume, 1)
                    b = chunk_bounds(n_src)
                    must = {
                        "chunk_last_row": False,
                        # no row in the last lane of any chunk: fewer rows than lanes
                        "last_lane": all(r1 - r0 < plan["R"] for r0, r1 in zip(b[:-1], b[1:])),
                        "db_n_src": n_tgt == n_src,
                        "no_second_kgroup": volume <= plan["kg"],
                    }
                    for mutant, coincide in must.items():
                        wrong = oracle_backward(p.x, p.dy, p.w, p.tbl_t, mutant, plan)
                        name = "db" if mutant == "db_n_src" else "dw"
                        assert _differs(wrong[name][0], p.ref[name][0]) == (not coincide), (mutant, c, n_src, volume, n_tgt)
                        seen.add((mutant, coincide))
    assert seen == {(m, f) for m in ("last_lane", "db_n_src", "no_second_kgroup") for f in (False, True)} | \
        {("chunk_last_row", False)}


# =====================================================================================================================
# forward
# =====================================================================================================================
@pytest.mark.parametrize("volume", FWD_VOLUMES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_batch_edges_and_table_kinds(device, dt, volume):
    """every table kind at every width, with and without bias; unnamed source rows hold NaN (row 0 among them whenever
    the table does not name it), so a value taken from behind an absent entry shows"""
    for kind in TABLE_KINDS:
        for c in FWD_CHANNELS:
            for bias in (True, False):
                p = fwd_case(dt, "exact", kind, volume, c, bias=bias)
                dst = p.run(device)
                assert np.isfinite(dst.values((p.n_tgt, c)).double().numpy()).all()
                p.check(dst, f"{dt} {kind} volume {volume} c {c} bias {bias}")
                if kind == "absent":
                    want = torch.from_numpy(p.bias if bias else np.zeros(c)).expand(p.n_tgt, c)
                    assert torch.equal(dst.values((p.n_tgt, c)).double(), want)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_widths_by_address(device, dt):
    """one table and one set of values per c: the oracle at every placement, and the same bits of dst at all of them"""
    for data in ("exact", "random"):
        for volume in (9, 27):
            bits = {}
            for c, place, v in FWD_PLACEMENTS[dt]:
                assert forward_width(ELEM[dt], c, **place) == v
                p = fwd_case(dt, data, "random", volume, c)
                dst = p.run(device, place)
                p.check(dst, f"{dt} {data} volume {volume} c {c} at {place} (width {v})")
                assert torch.equal(bits.setdefault(c, dst.bits()), dst.bits()), \
                    f"{dt} {data} volume {volume} c {c}: dst at {place} (width {v}) differs in bits from the aligned one"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_random_data_at_every_width_and_volume(device, dt):
    for volume in FWD_VOLUMES:
        for c in FWD_CHANNELS:
            p = fwd_case(dt, "random", "random", volume, c)
            p.check(p.run(device), f"{dt} random volume {volume} c {c}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_work_items_on_the_block_edge(device, dt):
    """n_tgt (c / V) = 255, 256, 257 threads with work (and 258 for three pieces per row), one target row"""
    for c, rows in ((4, (1, 255, 256, 257)), (1, (1, 255, 256, 257)), (3, (85, 86)), (16, (1, 64, 65))):
        for n_tgt in rows:
            for data in ("exact", "random"):
                p = fwd_case(dt, data, "random", 9, c, n_tgt=n_tgt)
                p.check(p.run(device), f"{dt} {data} c {c} n_tgt {n_tgt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_rows_0_and_last_named_or_poisoned(device, dt):
    for c in FWD_CHANNELS:
        for volume in (7, 9):
            # rows 0 and n_src - 1 are named, and only they and a few more
            rng = _rng(5, c, volume)
            tbl = make_table(rng, "random", volume, FWD_N_TGT, FWD_N_SRC)
            tbl[tbl >= 0] = rng.choice([0, FWD_N_SRC - 1, 13], size=int((tbl >= 0).sum()))
            p = Fwd(dt, "exact", tbl, c, FWD_N_SRC, rng)
            assert p.named[0] and p.named[-1] and p.named.sum() == 3 and np.isnan(p.src[1]).all()
            p.check(p.run(device), f"{dt} c {c} volume {volume}: rows 0 and n_src - 1 named")
            # row 0 is not named and holds NaN, behind every absent entry
            q = fwd_case(dt, "exact", "random", volume, c, first_row=1)
            assert not q.named[0] and np.isnan(q.src[0]).all() and (q.tbl < 0).any()
            dst = q.run(device)
            assert np.isfinite(dst.values((q.n_tgt, c)).double().numpy()).all(), "a poisoned row reached the output"
            q.check(dst, f"{dt} c {c} volume {volume}: NaN in row 0")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_named_non_finite_rows(device, dt):
    """named rows of +Inf, -Inf and NaN; a zero weight meets an Inf (0 Inf = NaN, in the kernel as in the oracle); every
    finite element stays within the bound"""
    for c in FWD_CHANNELS:
        for data in ("exact", "random"):
            p = fwd_case(dt, data, "random", 9, c, poison=False)
            rows = np.flatnonzero(p.named)[:4]
            p.src[rows[0]], p.src[rows[1]], p.src[rows[2]] = np.inf, -np.inf, np.nan
            p.src[rows[3], ::2] = np.inf
            k, t = np.argwhere(p.tbl == rows[3])[0]
            p.w[k, 0] = 0.0
            p.ref, p.S, p.m = oracle_forward(p.src, p.w, p.bias, p.tbl)
            assert np.isnan(p.ref[t, 0]) and np.isinf(p.ref).any() and np.isfinite(p.ref).any()
            dst = p.run(device)
            compare(dst.values((p.n_tgt, c)), p.ref, p.S, p.m, dt, "bound", f"{dt} {data} c {c}: non-finite rows")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_forward_without_source_rows_or_target_rows(device, dt):
    L, lib = _lib()
    for c in (8, 7):
        for bias in (True, False):
            for src_null in (False, True):
                p = fwd_case(dt, "exact", "absent", 9, c, bias=bias, n_src=0)
                dst = p.run(device, src_null=src_null)
                want = torch.from_numpy(p.bias if bias else np.zeros(c)).expand(p.n_tgt, c)
                assert torch.equal(dst.values((p.n_tgt, c)).double(), want), (c, bias, src_null)
        # no target rows: nothing is launched, nothing written
        p = fwd_case(dt, "exact", "absent", 9, c, n_tgt=0)
        keep = []
        dst = Out(0, dt, device, spare=c)
        rc = getattr(lib, "me_cwconv_forward_" + dt)(
            _put(keep, torch.from_numpy(np.nan_to_num(p.src)).to(TORCH[dt]), device), c,
            _put(keep, torch.from_numpy(p.w).to(WEIGHT[dt]), device), None,
            _put(keep, torch.zeros(1, dtype=torch.int32), device, 0, 0), p.n_src, 0, 9, dst.ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0 and dst.untouched() and dst.intact()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_volume_65535(device, dt):
    p = _wide_fwd(dt)
    assert p.tbl.shape == (MAX_VOLUME, 3) and (p.tbl[-KB - 1:, 1] >= 0).all() and MAX_VOLUME % KB
    p.check(p.run(device), f"{dt} volume {MAX_VOLUME}")


# =====================================================================================================================
# backward
# =====================================================================================================================
def _same_bits(a, b, what):
    for name in a:
        assert torch.equal(a[name].bits(), b[name].bits()), f"{what}: {name} differs in bits"


@pytest.mark.parametrize("v", [4, 1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_k_group_edges(device, dt, v):
    """volumes on the edges of the k-groups (16 offsets at 4 channels per thread, 32 at one): the fused dx up to one
    k-group, the separate pass beyond; need_dx and dbias on and off; dx bit for bit what the forward launch gives on
    (dy, w, NULL, tbl_t); a second launch on a freshly poisoned workspace bit for bit the first"""
    c = BWD_CHANNELS[v]
    for volume in BWD_VOLUMES[v]:
        for kind in ("dense", "random", "last_offset"):
            p = bwd_case(dt, "exact", kind, volume, c)
            assert backward_plan(ELEM[dt], c, volume, 1)["v"] == v
            first = None
            for need_dx in (1, 0):
                for dbias in (True, False):
                    what = f"{dt} {kind} volume {volume} c {c} need_dx {need_dx} dbias {dbias}"
                    out = p.run(device, need_dx, dbias)
                    p.check(out, need_dx, dbias, what)
                    first = first or out
            _same_bits(first, p.run(device, 1, True), f"{dt} {kind} volume {volume} c {c}: two launches")
            assert torch.equal(first["dx"].bits(), p.dx_by_forward(device).bits()), \
                f"{dt} {kind} volume {volume} c {c}: dx of the backward and of the forward launch on tbl_t differ in bits"
        q = bwd_case(dt, "random", "random", volume, c)
        q.check(q.run(device, 1, True), 1, True, f"{dt} random volume {volume} c {c}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_widths_by_address(device, dt):
    """4 channels per thread or one by the addresses of x, dy, dx and w: dx in the same bits at every placement (each
    channel is summed in the same k order), dW and db within the oracle's terms (their lane order changes)"""
    for data in ("exact", "random"):
        for volume in (16, 17):                             # fused at 4 channels per thread, and not
            bits = {}
            for c, place, v in BWD_PLACEMENTS[dt]:
                assert backward_plan(ELEM[dt], c, volume, 1, **place)["v"] == v
                p = bwd_case(dt, data, "random", volume, c)
                out = p.run(device, 1, True, place)
                what = f"{dt} {data} volume {volume} c {c} at {place} ({v} per thread)"
                p.check(out, 1, True, what)
                assert torch.equal(bits.setdefault(c, out["dx"].bits()), out["dx"].bits()), f"{what}: dx differs in bits"
                assert torch.equal(out["dx"].bits(), p.dx_by_forward(device, place).bits()), f"{what}: dx by the forward launch"
                if "dx" in place:                           # without dx its address does not count
                    q = p.run(device, 0, True, place)
                    p.check(q, 0, True, what + " need_dx 0")


def test_backward_bf16_fused_at_four_channels(device):
    for volume in (8, 16):
        assert backward_plan(2, 8, volume, 1) == dict(v=4, kg=16, kgroups=1, fused=True, P=2, R=128)
        for data in ("exact", "random"):
            for kind in ("dense", "random"):
                p = bwd_case("bf16", data, kind, volume, 8)
                out = p.run(device, 1, True)
                p.check(out, 1, True, f"bf16 fused {data} {kind} volume {volume}")
                assert torch.equal(out["dx"].bits(), p.dx_by_forward(device).bits())


@pytest.mark.parametrize("c", BWD_PIECE_CHANNELS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_pieces_per_row(device, dt, c):
    """P pieces x R row lanes of a workgroup: idle threads (P = 3, 255), one lane (P >= 255), a second block of pieces
    (P = 257 at either width)"""
    for volume in (2, 3):
        for data in ("exact", "random"):
            p = bwd_case(dt, data, "dense" if volume == 3 else "random", volume, c)
            for need_dx in (1, 0):
                out = p.run(device, need_dx, True)
                p.check(out, need_dx, True, f"{dt} {data} c {c} volume {volume} need_dx {need_dx}")


@pytest.mark.parametrize("n_src", BWD_ROWS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_rows_and_chunks(device, dt, n_src):
    for c in (8, 3):
        for volume in (3, 17):
            for data in ("exact", "random"):
                for kind in ("dense", "random"):
                    p = bwd_case(dt, data, kind, volume, c, n_src=n_src, n_tgt=max(n_src, 2))
                    out = p.run(device, 1, True)
                    p.check(out, 1, True, f"{dt} {data} {kind} n_src {n_src} c {c} volume {volume}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_chunk_cap(device, dt):
    """131073 source rows: 512 chunks of 256 or 257 rows by chunk_begin"""
    p = _capped_case(dt)
    out = p.run(device, 1, True)
    p.check(out, 1, True, f"{dt} n_src {BWD_ROWS_CAPPED}")
    _same_bits(out, p.run(device, 1, True), f"{dt} n_src {BWD_ROWS_CAPPED}: two launches")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_volume_65535(device, dt):
    p = _wide_bwd(dt)
    assert backward_plan(ELEM[dt], 4, MAX_VOLUME, 1)["kgroups"] == 4096
    for need_dx in (1, 0):
        p.check(p.run(device, need_dx, True), need_dx, True, f"{dt} volume {MAX_VOLUME} need_dx {need_dx}")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_backward_n_tgt_against_n_src(device, dt):
    """db is a sum over n_tgt rows split by the chunk count of n_src; either side may be empty"""
    for c in (8, 3):
        for n_src, n_tgt in ((100, 300), (300, 900), (300, 100), (513, 171), (257, 2)):
            for volume in (3, 17):
                p = bwd_case(dt, "exact", "random", volume, c, n_src=n_src, n_tgt=n_tgt)
                for need_dx in (1, 0):
                    p.check(p.run(device, need_dx, True), need_dx, True, f"{dt} c {c} n_src {n_src} n_tgt {n_tgt} volume {volume}")
        for volume in (3, 17, 33):
            # no source rows: dW = 0, db = sum dy, no dx
            p = bwd_case(dt, "exact", "absent", volume, c, n_src=0, n_tgt=300)
            for need_dx in (1, 0):
                out = p.run(device, need_dx, True)
                assert not out["dw"].values((volume, c)).any() and out["dx"].untouched()
                compare(out["db"].values((c,)), *p.ref["db"], GRAD[dt], "exact", f"{dt} n_src 0: db")
            # no target rows: dW = db = 0, dx = 0
            p = bwd_case(dt, "exact", "absent", volume, c, n_src=300, n_tgt=0)
            assert np.isnan(p.x).all()                      # (no row of x is used)
            for need_dx in (1, 0):
                out = p.run(device, need_dx, True)
                assert not out["dw"].values((volume, c)).any() and not out["db"].values((c,)).any()
                assert not need_dx or not out["dx"].values((300, c)).any()
            # neither: zero fill, no workspace
            p = bwd_case(dt, "exact", "absent", volume, c, n_src=0, n_tgt=0)
            for dbias in (True, False):
                out = p.run(device, 1, dbias)
                assert not out["dw"].values((volume, c)).any() and out["dx"].untouched()
                assert not dbias or not out["db"].values((c,)).any()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_poisoned_rows(device, dt):
    """NaN in the rows of x without any entry, and (dbias NULL) in the rows of dy that no entry names, row 0 among them:
    it is what an absent entry reads"""
    for c in (8, 3):
        for volume in (3, 16, 17, 33):
            for kind in ("random", "one_row", "last_offset"):
                p = bwd_case(dt, "exact", kind, volume, c, first_row=1, poison_dy=True)
                assert not p.named[0] and np.isnan(p.dy[0]).all() and (p.tbl_t < 0).any()
                assert kind == "random" or np.isnan(p.x).any()
                out = p.run(device, 1, False)
                for name, shape in (("dx", (p.n_src, c)), ("dw", (volume, c))):
                    assert np.isfinite(out[name].values(shape).double().numpy()).all(), f"{name}: a poisoned row was used"
                p.check(out, 1, False, f"{dt} poisoned {kind} volume {volume} c {c}")


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_transposed_pair(device, dt):
    """tbl with at most one target per (offset, source row) and tbl_t derived from it: on EXACT data
    <dy, dst - bias> == <x, dx> exactly (float64 of the stored values; fp32 and float64 store the sums themselves), and
    dW[k] is the derivative of that sum by w[k]"""
    for c in (8, 3):
        for volume in (9, 17, 33):
            rng = _rng(6, c, volume)
            n_src, n_tgt = 211, 160
            tbl = np.full((volume, n_tgt), -1, np.int32)
            tbl_t = np.full((volume, n_src), -1, np.int32)
            for k in range(volume):
                t = rng.choice(n_tgt, n_tgt // 2, replace=False)
                s = rng.choice(n_src, n_tgt // 2, replace=False)
                tbl[k, t], tbl_t[k, s] = s, t
            b = Bwd(dt, "exact", tbl_t, c, n_tgt, rng)
            f = Fwd(dt, "exact", tbl, c, n_src, rng, bias=False, poison=False)
            f.src, f.w = np.nan_to_num(b.x, nan=1.0), b.w
            f.ref, f.S, f.m = oracle_forward(f.src, f.w, None, tbl)
            b.x = f.src
            b.ref = oracle_backward(b.x, b.dy, b.w, tbl_t)
            dst = f.run(device)
            out = b.run(device, 1, True)
            f.check(dst, f"{dt} pair c {c} volume {volume}")
            b.check(out, 1, True, f"{dt} pair c {c} volume {volume}")
            if dt != "bf16":                                # (bf16 rounds dst and dx at the store)
                lhs = (b.dy * dst.values((n_tgt, c)).double().numpy()).sum()
                rhs = (b.x * out["dx"].values((n_src, c)).double().numpy()).sum()
                assert lhs == rhs, (lhs, rhs)
            # d/dw[k, ch] of sum_t dy[t] dst[t] = sum_t dy[t, ch] src[tbl[k, t], ch]
            g = np.where((tbl >= 0)[:, :, None], b.dy[None] * f.src[np.where(tbl >= 0, tbl, 0)], 0.0).sum(1)
            assert np.array_equal(out["dw"].values((volume, c)).double().numpy(), g)


# =====================================================================================================================
# float64 entry points
# =====================================================================================================================
@pytest.mark.parametrize("volume", [1, 9, 33])
def test_f64_entry_points(device, volume):
    for c in (1, 3, 8):
        for kind in TABLE_KINDS:
            for data in ("exact", "random"):
                p = fwd_case("f64", data, kind, volume, c, bias=kind != "one_row")
                p.check(p.run(device), f"f64 {data} {kind} volume {volume} c {c}")
                q = bwd_case("f64", data, kind, volume, c, n_src=150, n_tgt=97)
                for need_dx, dbias in ((1, True), (0, True), (1, False)):
                    q.check(q.run(device, need_dx, dbias), need_dx, dbias,
                            f"f64 {data} {kind} volume {volume} c {c} need_dx {need_dx} dbias {dbias}")


# =====================================================================================================================
# workspace and arguments
# =====================================================================================================================
def test_workspace_bytes(device):
    _, lib = _lib()
    for n in (0,) + BWD_ROWS + (BWD_N_SRC, 131072, BWD_ROWS_CAPPED, 10 ** 6):
        for volume, c in ((1, 1), (3, 8), (27, 17), (125, 96), (MAX_VOLUME, 4)):
            want = -(-(n_chunks(n) * (volume * c + c) * 4) // 256) * 256
            assert int(lib.me_cwconv_backward_workspace_bytes(n, volume, c)) == want, (n, volume, c)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_argument_checks_leave_the_outputs_untouched(device, dt):
    """refused in the library's own checks, before any launch: non-zero, a message, nothing written"""
    L, lib = _lib()
    c, volume = 8, 9
    f = fwd_case(dt, "exact", "random", volume, c, poison=False)
    b = bwd_case(dt, "exact", "random", volume, c)
    keep = []
    x, dy, w = b.tensors()
    a = dict(src=_put(keep, torch.from_numpy(f.src).to(TORCH[dt]), device), w=_put(keep, w, device),
             fw=_put(keep, torch.from_numpy(f.w).to(WEIGHT[dt]), device),
             bias=_put(keep, torch.from_numpy(f.bias).to(WEIGHT[dt]), device),
             tbl=_put(keep, torch.from_numpy(f.tbl), device, 0, f.n_src),
             x=_put(keep, x, device), dy=_put(keep, dy, device), tbl_t=_put(keep, torch.from_numpy(b.tbl_t), device, 0, b.n_tgt))
    dst = Out(f.n_tgt * c, dt, device)
    outs = {"dx": Out(b.n_src * c, dt, device), "dw": Out(volume * c, GRAD[dt], device), "db": Out(c, GRAD[dt], device)}
    ws_bytes = int(lib.me_cwconv_backward_workspace_bytes(b.n_src, volume, c))
    ws = GuardedBytes(ws_bytes, device)
    ws.fill(NAN_WORD)

    def forward(c=c, volume=volume):
        return getattr(lib, "me_cwconv_forward_" + dt)(a["src"], c, a["fw"], a["bias"], a["tbl"], f.n_src, f.n_tgt, volume,
                                                       dst.ptr(), None)

    def backward(c=c, volume=volume, need_dx=1, dx=outs["dx"].ptr(), dw=outs["dw"].ptr(), wsp=ws.ptr(), wsb=ws_bytes):
        return getattr(lib, "me_cwconv_backward_" + dt)(a["x"], a["dy"], c, a["w"], a["tbl_t"], b.n_src, b.n_tgt, volume,
                                                        need_dx, dx, dw, outs["db"].ptr(), wsp, wsb, None)

    def nothing_written(name):
        torch.cuda.synchronize()
        assert dst.untouched() and all(o.untouched() for o in outs.values()) and ws.holds(NAN_WORD), \
            f"{name}: refused, yet something was written"
        assert dst.intact() and all(o.intact() for o in outs.values()) and ws.intact()
        assert lib.me_last_error(), name

    for name, over in (("c = 0", dict(c=0)), ("volume = 0", dict(volume=0)), ("volume = 65536", dict(volume=MAX_VOLUME + 1))):
        assert forward(**over) != 0, name
        nothing_written("forward " + name)
    bad = [("c = 0", dict(c=0)), ("volume = 0", dict(volume=0)), ("volume = 65536", dict(volume=MAX_VOLUME + 1)),
           ("need_dx without dx", dict(dx=None)), ("dweight NULL", dict(dw=None))]
    if dt != "f64":                                         # (float64 takes no workspace)
        bad += [("workspace NULL", dict(wsp=None)), ("workspace one byte short", dict(wsb=ws_bytes - 1))]
    for name, over in bad:
        assert backward(**over) != 0, name
        nothing_written("backward " + name)
    # ... and the same arguments, unchanged, run
    L.check(forward())
    L.check(backward())
    torch.cuda.synchronize()
    f.check(dst, f"{dt} good arguments")
    b.check(outs, 1, True, f"{dt} good arguments")
    assert dst.intact() and all(o.intact() for o in outs.values()) and ws.intact()
