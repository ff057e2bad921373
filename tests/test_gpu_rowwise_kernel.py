"""The row-wise kernel itself (csrc/conv_rowwise.hip, k_conv_rowwise_bf16) on synthetic pair lists, through the C ABI:
dst[tgt_rows[e]] = src[src_rows[e]] @ W[k(e)].

tests/test_gpu_rowwise.py drives the kernel through whole layers, where a workgroup walks one item and an offset holds
thousands of pairs.  Here the control flow around the items is the subject: several items per workgroup (W[k] staged again
when a run of items crosses an offset, the x-row ring and the indices running ahead into the next item and the next
offset), per-offset pair counts on the item boundaries (items are 64 G pairs), empty first / last offsets, up to the 64
offsets of the wave scan, a pair bound above the pair count, both item shapes (G) at small sizes, partial 32-channel steps,
padding steps of the ring, output widths that are no multiple of 16 and a last column slab narrower than the others.

Oracle: numpy float64 on the bf16-rounded operands; tolerance: assert_bf16_close (one rounding of an fp32 sum).  Besides
the values, every case checks that the output is BITWISE the same under every (G, items per workgroup, pair bound) — the
per-row sum does not depend on the item shape — and that nothing around the buffers was touched: every buffer is a view
into the MIDDLE of a larger tensor, NaN around the features and the weights, a pattern around the output (compared bit for
bit afterwards), the output itself NaN before every launch.  The surroundings of the index arrays hold indices of those
guard rows, so a stray index read shows as a NaN or a damaged guard, never as an access outside the tensors."""
import itertools

import numpy as np
import pytest
import torch

from test_gpu_bf16 import assert_bf16_close, bf16_round

PAD = 4096            # elements around every buffer: 8 KB of bf16 (16-byte alignment kept; wider than any row here)
CYCLE = (0, 1, 17, 64, 65)


def _cycling(volume, shift):
    return [CYCLE[(i + shift) % len(CYCLE)] for i in range(volume)]


COUNTS = {
    "v1_n1": [1], "v1_n63": [63], "v1_n64": [64], "v1_n65": [65], "v1_n129": [129],
    "v8_edges": [0, 1, 63, 64, 65, 0, 128, 129],
    "v8_skew": [5, 0, 0, 0, 0, 0, 0, 700],
    "v27_first_empty": _cycling(27, 0),       # 0, 1, 17, ... last 1
    "v27_last_empty": _cycling(27, 4),        # 65, 0, 1, ... last 0
    "v64_first_empty": _cycling(64, 0),       # 0, 1, 17, ... last 64
    "v64_last_empty": _cycling(64, 2),        # 17, 64, 65, 0, ... last 0
}
LARGEST = "largest"    # resolved by _largest_supported_shape()
SHAPES = [(8, 8), (16, 24), (24, 40), (32, 32), (40, 72), (72, 104), (96, 24), (128, 96), (64, 136), (128, 256),
          (192, 40),   # six steps: above four and no multiple of the ring depth (two padding steps)
          (136, 24),   # eight steps of which three lie wholly beyond the row, the fifth partial (chunks of 128)
          LARGEST]
SETTINGS = [(g, ipw, extra) for g in (1, 2) for ipw in (1, 2, 3, 7) for extra in (0, 1000)]


def _cases():
    """a cross of the two lists, not their product: every shape on the item-boundary list and on one more list (rotating),
    every list on a one-step shape with partial channels and on 32 -> 32"""
    names = list(COUNTS)
    cases = []
    for i, shape in enumerate(SHAPES):
        cases += [("v8_edges", shape), (names[(3 * i + 1) % len(names)], shape)]
    for name in names:
        cases += [(name, (24, 40)), (name, (32, 32))]
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CASES = _cases()


def _lib():
    from minkowskiengine_amd import _lib as L
    return L, L.load()


def _largest_supported_shape(lib, volume=8):
    """the largest (c_src x c_dst, then c_src) shape of up to 512 channels a side that the kernel takes"""
    best = None
    for c_src, c_dst in itertools.product(range(8, 513, 8), repeat=2):
        if lib.me_conv_rowwise_supported_bf16(volume, c_src, c_dst):
            key = (c_src * c_dst, c_src, c_dst)
            best = key if best is None or key > best else best
    return best[1], best[2]


def _steps(lib, c_src, c_dst):
    kc = lib.me_conv_pack_chunk_bf16(c_src, c_dst)
    return -(-c_src // kc) * (kc // 32)


def test_shape_list_reaches_every_path_of_the_kernel():
    """(host only) every shape of the matrix is one the kernel takes — for every volume of the matrix — and the list holds
    step counts 1, 2, one that is no multiple of 4 and one above 4 (both ring depths, padding steps), partial 32-channel
    steps, widths that are no multiple of 16, and a second column slab narrower than the first"""
    _, lib = _lib()
    shapes = [_largest_supported_shape(lib) if s == LARGEST else s for s in SHAPES]
    assert shapes[-1] == (256, 512), shapes[-1]       # 8 steps x 8 blocks x 1 KB = the 64 KB policy limit, four slabs
    for c_src, c_dst in shapes:
        for volume in (1, 8, 27, 64):
            assert lib.me_conv_rowwise_supported_bf16(volume, c_src, c_dst) == 1, (volume, c_src, c_dst)
    steps = [_steps(lib, *s) for s in shapes]
    assert 1 in steps and 2 in steps
    assert any(s % 4 for s in steps if s > 2), steps          # ring depth 4 with padding steps
    assert any(s > 4 for s in steps) and any(s > 4 and s % 4 for s in steps), steps
    assert {8, 16, 24} <= {s[0] for s in shapes}
    assert any(s[1] % 16 for s in shapes)
    assert any(128 < s[1] <= 256 and s[1] % 128 for s in shapes)
    assert lib.me_conv_rowwise_supported_bf16(8, 384, 256) == 0     # (12 x 8 KB: beyond the LDS policy)


def _middle(n, dtype, device, fill):
    """a view of n elements into the middle of a tensor of PAD + n + PAD, everything set to `fill`"""
    big = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=device)
    return big, big[PAD:PAD + n]


class _Case:
    """inputs of one (count list, shape) on the device, and the float64 oracle — built once, launched many times"""

    def __init__(self, device, counts, c_src, c_dst, seed):
        L, lib = _lib()
        self.lib, self.check = lib, L.check
        rng = np.random.default_rng(seed)
        volume, n = len(counts), int(sum(counts))
        n_src = max(1, n // 2 + 1)
        src_rows = rng.integers(0, n_src, size=n).astype(np.int32)
        if n >= 2:
            a, b = rng.choice(n, size=2, replace=False)
            src_rows[a], src_rows[b] = 0, n_src - 1
        else:
            src_rows[:] = 0
        assert src_rows.min() == 0 and src_rows.max() == n_src - 1
        tgt_rows = rng.permutation(n).astype(np.int32)
        koffs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        g = torch.Generator().manual_seed(seed)
        x = bf16_round(torch.rand(n_src, c_src, generator=g) - 0.4)
        w = bf16_round(torch.rand(volume, c_src, c_dst, generator=g) - 0.5)
        self.volume, self.n, self.n_src, self.c_src, self.c_dst = volume, n, n_src, c_src, c_dst
        # ---- the oracle: out[tgt[e]] = x[src[e]] @ W[k(e)] in float64 ----
        x64, w64 = x.numpy().astype(np.float64), w.numpy().astype(np.float64)
        ref = np.full((n, c_dst), np.nan)
        for k in range(volume):
            e = slice(koffs[k], koffs[k + 1])
            ref[tgt_rows[e]] = x64[src_rows[e]] @ w64[k]
        assert np.isfinite(ref).all()
        self.ref = ref
        # ---- device buffers: views into the middle of larger tensors ----
        nan = float("nan")
        self.src_big, self.src = _middle(n_src * c_src, torch.bfloat16, device, nan)
        self.src.copy_(x.to(torch.bfloat16).reshape(-1))
        elems = int(lib.me_conv_packed_weight_elems_bf16(volume, c_src, c_dst))
        self.wp_big, self.wp = _middle(elems, torch.bfloat16, device, nan)
        w_dev = w.to(device)
        self.check(lib.me_conv_pack_weights_bf16(w_dev.data_ptr(), 1, volume, c_src, c_dst, 0, self.wp.data_ptr(), None))
        # a stray index read lands on a guard ROW: NaN features after the last source row / the pattern after the last
        # output row (PAD is wider than a row) — seen by the checks below, inside the tensors
        assert c_src <= PAD and c_dst <= PAD
        self.srows_big, self.srows = _middle(n, torch.int32, device, n_src)
        self.srows.copy_(torch.from_numpy(src_rows))
        self.trows_big, self.trows = _middle(n, torch.int32, device, n)
        self.trows.copy_(torch.from_numpy(tgt_rows))
        self.koffs_big, self.koffs = _middle(volume + 1, torch.int64, device, 0)
        self.koffs_big[PAD + volume + 1:] = n           # (offsets read beyond the list would be empty)
        self.koffs.copy_(torch.from_numpy(koffs))
        # the output as bit patterns: a position-dependent pattern around it, NaN (0x7fc1) inside before every launch
        self.dst_big = ((torch.arange(2 * PAD + n * c_dst, device=device) % 251) + 0x4000).to(torch.int16)
        self.dst = self.dst_big[PAD:PAD + n * c_dst]
        self.dst_guards = (self.dst_big[:PAD].clone(), self.dst_big[PAD + n * c_dst:].clone())
        self.inputs = [t.clone() for t in (self.src_big, self.wp_big, self.srows_big, self.trows_big, self.koffs_big)]
        for t in (self.src, self.wp, self.dst):
            assert t.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def launch(self, groups, items_per_wg, extra_bound):
        lib = self.lib
        self.dst.fill_(0x7fc1)
        lib.me_debug_set_rowwise_groups(groups)
        lib.me_debug_set_rowwise_items_per_wg(items_per_wg)
        try:
            self.check(lib.me_conv_rowwise_bf16(self.src.data_ptr(), self.n_src, self.c_src, self.wp.data_ptr(), self.volume,
                                                self.c_dst, self.srows.data_ptr(), self.trows.data_ptr(),
                                                self.koffs.data_ptr(), self.n + extra_bound, self.dst.data_ptr(), self.n,
                                                None))
            torch.cuda.synchronize()
        finally:
            lib.me_debug_set_rowwise_groups(0)
            lib.me_debug_set_rowwise_items_per_wg(0)
        return self.dst.clone().view(torch.bfloat16).reshape(self.n, self.c_dst)

    def guards_intact(self):
        n = self.n * self.c_dst
        return (torch.equal(self.dst_big[:PAD], self.dst_guards[0]) and
                torch.equal(self.dst_big[PAD + n:], self.dst_guards[1]))

    def inputs_intact(self):
        # (bit patterns: NaN != NaN)
        bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t    # noqa: E731
        return all(torch.equal(bits(a), bits(b)) for a, b in
                   zip((self.src_big, self.wp_big, self.srows_big, self.trows_big, self.koffs_big), self.inputs))


@pytest.mark.gpu
@pytest.mark.parametrize("counts_name,shape", CASES, ids=[f"{n}-{s if s == LARGEST else '%dx%d' % s}" for n, s in CASES])
def test_rowwise_kernel_vs_oracle_bitwise_across_item_shapes(device, counts_name, shape):
    _, lib = _lib()
    c_src, c_dst = _largest_supported_shape(lib) if shape == LARGEST else shape
    counts = COUNTS[counts_name]
    assert lib.me_conv_rowwise_supported_bf16(len(counts), c_src, c_dst) == 1
    case = _Case(device, counts, c_src, c_dst, seed=1000 * len(counts) + sum(counts) + c_src + c_dst)
    first = None
    for groups, ipw, extra in SETTINGS:
        what = f"{counts_name} {c_src}->{c_dst} G={groups} ipw={ipw} bound=+{extra}"
        out = case.launch(groups, ipw, extra)
        assert case.guards_intact(), f"{what}: the kernel wrote outside the output"
        assert bool(torch.isfinite(out.float()).all()), f"{what}: rows not written, or computed from memory around the inputs"
        if first is None:
            first = out
            assert_bf16_close(out.float().cpu().numpy(), case.ref, what)
        else:
            assert torch.equal(out.view(torch.int16), first.view(torch.int16)), \
                f"{what}: bits differ from G={SETTINGS[0][0]} ipw={SETTINGS[0][1]}"
    assert case.inputs_intact(), "an input buffer or its surroundings changed"
