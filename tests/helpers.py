"""Shared input generators and comparison helpers for the tests (SURVEY.md §8d inputs)."""
import glob
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_cloud(n, extent, D=3, seed=0, batch=1, dup=0, negative=False):
    """Unique, unsorted int32 voxels drawn uniformly from [0, extent)^D (optionally centred on 0),
    batch index prepended; `dup` extra duplicated rows shuffled in."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for b in range(batch):
        lo = -(extent // 2) if negative else 0
        pts = torch.randint(lo, lo + extent, (int(1.6 * n) + 16, D), generator=g)
        pts = torch.unique(pts, dim=0)
        pts = pts[torch.randperm(pts.shape[0], generator=g)][:n]
        parts.append(torch.cat([torch.full((pts.shape[0], 1), b, dtype=torch.long), pts], 1))
    c = torch.cat(parts, 0)
    if dup:
        c = torch.cat([c, c[torch.randint(0, c.shape[0], (dup,), generator=g)]], 0)
        c = c[torch.randperm(c.shape[0], generator=g)]
    return c.int().contiguous()


def golden_cases(pattern="ref_*d_k*.npz"):
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, pattern)))


def golden_kmap(z):
    """npz -> {k: int32 [2, n_k]}"""
    out, s = {}, 0
    for k, n in zip(z["kmap_k"].tolist(), z["kmap_n"].tolist()):
        out[int(k)] = z["kmap_pairs"][:, s:s + n]
        s += n
    return out


def rel_err(a, b):
    """max |a - b| normalised by the largest reference magnitude (a coarse, GLOBAL figure: used only for
    oracle-vs-reference sanity checks; the GPU parity tests use assert_close, which is per element)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def close_excess(a, b, atol=1e-4, rtol=1e-4):
    """max over elements of |a - b| / (atol + rtol * |b|): <= 1 means every element is within tolerance."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, f"shape mismatch {a.shape} vs {b.shape}"
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


def assert_close(a, b, atol=1e-4, rtol=1e-4, what=""):
    """PER-ELEMENT parity check |a - b| <= atol + rtol * |b| — the fp32 bar of BASELINE.json's north_star
    (1e-4 absolute + relative), not a max-normalised figure."""
    if hasattr(a, "detach"):
        a = a.detach().float().cpu().numpy()
    if hasattr(b, "detach"):
        b = b.detach().float().cpu().numpy()
    ex = close_excess(a, b, atol, rtol)
    if not ex <= 1.0:
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        i = np.unravel_index(np.argmax(np.abs(a64 - b64) / (atol + rtol * np.abs(b64))), a64.shape)
        raise AssertionError(f"{what} element {i}: got {a64[i]!r} want {b64[i]!r} "
                             f"(|diff| {abs(a64[i] - b64[i]):.3e} = {ex:.2f} x tolerance {atol}+{rtol}|b|)")


# ---- entry-point tests on synthetic tables (test_gpu_conv_tile_kernels.py, test_gpu_wgrad_kernels.py) ---------------------
GUARD_PAD = 4096       # elements around every buffer (16-byte alignment kept; wider than any row of those tests)
DEBUG_BUILD_ONLY = "only in a -DME_DEBUG_VARIANTS build (scripts/build_debug.sh)"


def int_view(t):
    """the bits of a 2- or 4-byte tensor"""
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def middle(n, dtype, device, fill, pad=GUARD_PAD):
    """(big, view): n elements in the MIDDLE of a tensor of pad + n + pad, all of it `fill` (NaN around an input; for an
    index array the index of a guard row)"""
    big = torch.full((pad + n + pad,), fill, dtype=dtype, device=device)
    return big, big[pad:pad + n]


class Guarded:
    """An output buffer of n 2- or 4-byte elements in the middle of a position-dependent bit pattern.  fill() puts a NaN
    bit pattern inside before a launch; intact() says whether the surroundings still hold the pattern.  `shift` elements
    move the inside off its 16-byte boundary (a kernel whose vector width follows the address)."""
    NAN = {2: 0x7fc1, 4: 0x7fc00001}

    def __init__(self, n, elem_bytes, device, base=0, pad=GUARD_PAD, shift=0):
        idt = {2: torch.int16, 4: torch.int32}[elem_bytes]
        start = {2: 0x4000, 4: 0x40000000}[elem_bytes]
        self.big = ((torch.arange(2 * pad + shift + n, device=device) % 251) + start + base).to(idt)
        self.bits = self.big[pad + shift:pad + shift + n]
        self.before, self.after = self.big[:pad + shift].clone(), self.big[pad + shift + n:].clone()
        self.nan = self.NAN[elem_bytes]
        self.pad, self.n = pad + shift, n
        assert (self.big.data_ptr() + pad * elem_bytes) % 16 == 0

    def ptr(self):
        return self.bits.data_ptr()

    def fill(self):
        self.bits.fill_(self.nan)

    def untouched(self):
        return bool((self.bits == self.nan).all())

    def intact(self):
        return torch.equal(self.big[:self.pad], self.before) and torch.equal(self.big[self.pad + self.n:], self.after)

    def as_dtype(self, dtype, shape):
        return self.bits.clone().view(dtype).reshape(shape)


class GuardedBytes:
    """The byte-typed sibling of Guarded, for 8-byte arrays, byte flags and workspaces: `nbytes` bytes in the middle of a
    position-dependent byte pattern (`pad` bytes on either side; the start keeps the allocation's alignment).  fill(word) repeats
    a 32-bit word over the inside, holds(word) says whether it still does, view() reinterprets the inside."""

    def __init__(self, nbytes, device, pad=GUARD_PAD):
        assert pad % 256 == 0
        band = ((torch.arange(pad, device=device) % 251) + 1).to(torch.uint8)
        self.big = torch.zeros(2 * pad + nbytes, dtype=torch.uint8, device=device)
        self.big[:pad] = band
        self.big[pad + nbytes:] = band.flip(0)
        self.bytes = self.big[pad:pad + nbytes]
        self.before, self.after = self.big[:pad].clone(), self.big[pad + nbytes:].clone()
        self.pad, self.n = pad, nbytes
        assert self.bytes.data_ptr() % 16 == 0

    def ptr(self):
        return self.bytes.data_ptr()

    def _pattern(self, word):
        return torch.tensor(list(int(word).to_bytes(4, "little")), dtype=torch.uint8, device=self.big.device)

    def fill(self, word):
        whole = self.n // 4 * 4
        self.bytes[:whole].view(torch.int32).fill_(int(word) - (1 << 32) if int(word) >= 1 << 31 else int(word))
        if whole < self.n:
            self.bytes[whole:] = self._pattern(word)[:self.n - whole]

    def holds(self, word):
        whole = self.n // 4 * 4
        w = int(word) - (1 << 32) if int(word) >= 1 << 31 else int(word)
        return bool((self.bytes[:whole].view(torch.int32) == w).all()) and \
            torch.equal(self.bytes[whole:], self._pattern(word)[:self.n - whole])

    def intact(self):
        return torch.equal(self.big[:self.pad], self.before) and torch.equal(self.big[self.pad + self.n:], self.after)

    def view(self, dtype, shape=(-1,)):
        return self.bytes.view(dtype).reshape(shape)


def exact_weights_bf16(rng, shape):
    """fp32 weights that round (RNE) to multiples of 2^-6 in [-2, 2]: such a value plus a perturbation below a quarter of
    a bf16 ulp, and a few exact ties (value + half an ulp away from zero, which round back to the even value).
    Returns (fed, rounded) as torch tensors."""
    m = rng.integers(-128, 129, size=shape)
    w = (m / 64.0).astype(np.float32)
    _, e = np.frexp(np.abs(w))
    ulp = np.where(m != 0, np.ldexp(1.0, e - 8), 0.0)
    pert = rng.uniform(-0.24, 0.24, size=w.shape) * ulp
    ties = np.zeros(w.shape, bool)
    nz = np.flatnonzero(m)
    ties.reshape(-1)[rng.choice(nz, min(len(nz), max(3, w.size // 50)), replace=False)] = True
    pert[ties] = (np.sign(w) * 0.5 * ulp)[ties]
    fed = torch.from_numpy((w.astype(np.float64) + pert).astype(np.float32))
    rounded = fed.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(rounded, torch.from_numpy(w)), "the perturbed weights must round to the multiples of 2^-6"
    return fed, rounded


def same_nonfinite_class(got, ref, what):
    """NaN / +Inf / -Inf / finite at the same elements of both arrays"""
    for name, sel in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf), ("finite", np.isfinite)):
        bad = sel(ref) != sel(got)
        at = tuple(np.argwhere(bad)[0]) if bad.any() else None
        assert at is None, (f"{what}: {int(bad.sum())} elements are {name} on one side only, e.g. {at}: "
                            f"{got[at]} for {ref[at]}")


def assert_tile_partials(stored, tile_rows, mean, m2, what):
    """Batch-norm partials of a kernel that forms them as the tile kernels do — per tile and column, over the rows in tile
    order (`stored`: float64 [n, c], the values actually stored), d = y - (the tile's first row), a = sum d, b = sum d^2 in
    fp32, mean = shift + a / rows, M2 = max(b - a (a / rows), 0) — against the float64 mean and M2 of the same values:
      |mean - ref| <= c 2^-24 (|shift| + max|d|)      |M2 - ref| <= c 2^-22 sum d^2      with c = rows + 4:
    each d is exact (bf16 differences fit fp32), a sum of `rows` terms in any order is off by at most rows 2^-24 times the
    sum of the magnitudes (<= rows max|d|, and a / rows brings that back to max|d|), the division and the shift added
    back are two more roundings; b and a m are each at most sum d^2 (Cauchy-Schwarz) with the same relative error, and
    their difference keeps the absolute one: four such terms -> 2^-22.  A tile of equal rows gives M2 == 0 exactly."""
    n, c = stored.shape
    tiles = -(-n // tile_rows)
    assert mean.shape == (tiles, c) and m2.shape == (tiles, c), (what, mean.shape, (tiles, c))
    assert np.isfinite(mean).all() and np.isfinite(m2).all() and (m2 >= 0).all(), f"{what}: partials not finite"
    for t in range(tiles):
        rows = stored[t * tile_rows:min((t + 1) * tile_rows, n)]
        cnt = len(rows) + 4
        d = rows - rows[0]
        ref_mean = rows.mean(0)
        ref_m2 = ((rows - ref_mean) ** 2).sum(0)
        em, e2 = np.abs(mean[t] - ref_mean), np.abs(m2[t] - ref_m2)
        tol_mean = cnt * 2.0 ** -24 * (np.abs(rows[0]) + np.abs(d).max(0))
        tol_m2 = cnt * 2.0 ** -22 * (d * d).sum(0)
        assert (em <= tol_mean).all(), f"{what}: tile {t} ({len(rows)} rows) mean off by {em.max():.3g}"
        assert (e2 <= tol_m2).all(), f"{what}: tile {t} ({len(rows)} rows) M2 off by {e2.max():.3g}"
        assert (m2[t][(d == 0).all(0)] == 0).all(), f"{what}: tile {t}: M2 of a constant column is not exactly 0"


def row_mapping(coords_a, coords_b):
    """m with coords_b[m[i]] == coords_a[i] (same coordinate sets, different row order)."""
    from oracle import me_oracle as O
    ca, cb = np.asarray(coords_a), np.asarray(coords_b)
    assert ca.shape == cb.shape, f"coordinate sets differ in size: {ca.shape} vs {cb.shape}"
    ra, rb = O.coordinate_rank(ca), O.coordinate_rank(cb)
    assert np.array_equal(ca[ra], cb[rb]), "coordinate sets differ"
    m = np.empty(len(ra), np.int64)
    m[ra] = rb
    return m


def placed(t, how):
    """A copy of the contiguous tensor t at a chosen address: "alloc" from the allocator (aligned far beyond 16 bytes),
    "8" a contiguous view that starts 8 bytes into its storage and ends at the storage's end, "1" one that starts one
    element into its storage.  The vector width of a HIP kernel follows the address; its result must not."""
    if how == "alloc":
        return t.clone()
    pad = 8 // t.element_size() if how == "8" else 1
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=t.device)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + pad * t.element_size()
    return v
