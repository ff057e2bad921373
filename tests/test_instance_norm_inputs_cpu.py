"""What tests/test_gpu_instance_norm_kernels.py relies on, checked without a GPU: the launch geometry its case tables
claim (piece width V, pieces per row P, row lanes R, chunk counts, reduce branch, LDS bytes — recomputed from the rules of
in_piece / bn_chunks / bn_reduce_lanes / bn_partial_lds_bytes, whose constants are read from the sources), the segment
patterns (mixed chunks, absent instances), and that the fp32 bar is not tight for the inputs: a naive float32 restatement
stays within half of it."""
import os
import re

import numpy as np
import pytest

import test_gpu_instance_norm_kernels as K
from helpers import close_excess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "minkowskiengine_amd", "csrc")


def test_constants_are_the_sources():
    common = open(os.path.join(CSRC, "norm_common.hpp")).read()
    assert int(re.search(r"constexpr int kBnMaxChunks = (\d+);", common).group(1)) == K.K_MAX_CHUNKS
    assert int(re.search(r"constexpr int kBnRowsPerThread = (\d+);", common).group(1)) == K.K_ROWS_PER_THREAD


@pytest.mark.parametrize("dtype,c,aligned,v,p,r,branch,g", [
    ("f32", 1, True, 1, 1, 256, "grouped", 128), ("f32", 3, True, 1, 3, 85, "grouped", 42),
    ("f32", 4, True, 4, 1, 256, "grouped", 32), ("f32", 12, True, 4, 3, 85, "grouped", 10),
    ("f32", 64, True, 4, 16, 16, "grouped", 2), ("f32", 65, True, 1, 65, 3, "direct", None),
    ("f32", 68, True, 4, 17, 15, "direct", None), ("f32", 96, True, 4, 24, 10, "direct", None),
    ("f32", 1024, True, 4, 256, 1, "direct", None), ("f32", 257, True, 1, 257, 1, "direct", None),
    ("f32", 1028, True, 4, 257, 1, "direct", None), ("bf16", 2056, True, 8, 257, 1, "direct", None),
    ("bf16", 4, True, 4, 1, 256, "grouped", 32), ("bf16", 12, True, 4, 3, 85, "grouped", 10),
    ("bf16", 8, True, 8, 1, 256, "grouped", 16), ("bf16", 24, True, 8, 3, 85, "grouped", 5),
    ("bf16", 64, True, 8, 8, 32, "grouped", 2), ("bf16", 3, True, 1, 3, 85, "grouped", 42),
    ("f32", 8, True, 4, 2, 128, "grouped", 16), ("f32", 8, False, 1, 8, 32, "grouped", 16),
    ("bf16", 16, True, 8, 2, 128, "grouped", 8), ("bf16", 16, False, 1, 16, 16, "grouped", 8),
    ("f32", 3224, True, 4, 806, 1, "direct", None), ("f32", 3225, True, 1, 3225, 1, "direct", None)])
def test_geometry_of_the_cases(dtype, c, aligned, v, p, r, branch, g):
    geo = K.geometry(dtype, c, 1, aligned)
    assert (geo["V"], geo["P"], geo["R"], geo["branch"], geo["G"]) == (v, p, r, branch, g)
    assert geo["lds"] <= K.K_LDS_LIMIT
    if branch == "grouped" and c in (3, 12):
        assert r % g != 0                       # the lane ranges l = g R / G .. (g + 1) R / G are uneven
    used = {(d, cc) for (d, cc, _, _) in K.SHAPE_CASES + K.PATTERN_CASES + K.UNALIGNED_CASES}
    assert (dtype, c) in used


def test_chunk_counts_of_the_cases():
    chunks = {case: K.geometry(case[0], case[1], len(K.segments(case[3], case[2])[0])) for case in K.SHAPE_CASES}
    for c in (1, 3, 4, 12, 64):
        got = [chunks[("f32", c, n, "sorted3")]["chunks"] for n in K._edge_ns(c)]
        assert got == [1, 1, 2, 6], (c, got)
    for c in (65, 68, 96):
        assert chunks[("f32", c, K._several("f32", c), "sorted3")]["chunks"] == 6
    assert chunks[("f32", 1024, 40, "sorted3")]["chunks"] == 5 and chunks[("f32", 1024, 40, "sorted3")]["bwd_chunks"] == 10
    capped = chunks[("f32", 1024, 5000, "sorted3")]
    assert capped["chunks"] == capped["bwd_chunks"] == 512 and 5000 > 512 * 8       # more than one batch of rows each
    assert {(g + 1) * 5000 // 512 - g * 5000 // 512 for g in range(512)} == {9, 10}  # chunk_begin: uneven chunks
    narrow = chunks[("f32", 64, 70000, "sorted35")]
    assert narrow["R"] == 16 and narrow["chunks"] == narrow["bwd_chunks"] == 512 and 70000 > 512 * 128
    for case in (("f32", 257, 40, "sorted3"), ("f32", 1028, 40, "sorted3"), ("bf16", 2056, 40, "sorted3")):
        assert chunks[case]["P"] == 257 and chunks[case]["chunks"] == 5
    for case in K.PATTERN_CASES:
        n = len(K.segments(case[3], case[2])[0])
        geo = K.geometry(case[0], case[1], n)
        assert geo["bwd_chunks"] >= 2, case
        if not case[3].startswith("many300"):
            assert geo["chunks"] >= 4, case
    for d, c, n, _ in K.UNALIGNED_CASES:
        assert K.geometry(d, c, n, True)["chunks"] >= 3 and K.geometry(d, c, n, False)["chunks"] >= 3
        assert K.geometry(d, c, n, True)["V"] > 1 and K.geometry(d, c, n, False)["V"] == 1


def test_the_lds_limit_is_at_3225_channels():
    assert K.geometry("f32", 3225, 24)["lds"] <= K.K_LDS_LIMIT < K.geometry("f32", 3226, 24)["lds"]
    assert K.geometry("f32", 4096, 24)["lds"] > K.K_LDS_LIMIT
    assert K.geometry("f32", 3224, 24)["V"] == 4 and K.geometry("f32", 3225, 24)["V"] == 1


def _indices_per_chunk(br, chunks):
    n = len(br)
    return [len(np.unique(br[g * n // chunks:(g + 1) * n // chunks])) for g in range(chunks)]


def test_patterns_mix_the_chunks_and_leave_the_stated_gaps():
    for d, c, n in K.PATTERN_SHAPES:
        for pattern, least in (("rr3", 3), ("rr7", 7), ("perm3", 3), ("many300", 100), ("many300_shuffled", 100)):
            br, nb = K.segments(pattern, n)
            assert br.dtype == np.int32 and br.min() >= 0 and br.max() < nb
            geo = K.geometry(d, c, len(br))
            if pattern.startswith("many300") and c != 4:
                least = 3
            assert max(_indices_per_chunk(br, geo["chunks"])) >= least, (d, c, pattern)
            assert max(_indices_per_chunk(br, geo["bwd_chunks"])) >= min(least, 3), (d, c, pattern)
        br, nb = K.segments("sorted3", n)          # instance boundaries fall inside chunks, not between them
        geo = K.geometry(d, c, n)
        assert sorted(_indices_per_chunk(br, geo["chunks"]))[-2:] == [2, 2]
        br, nb = K.segments("gapped", n)
        cnt = np.bincount(br, minlength=nb)
        assert nb == 9 and tuple(np.nonzero(cnt == 0)[0]) == K.GAPPED_ABSENT
        assert cnt[[1, 2, 4, 7]].tolist() == [1, 2, 1, 3] and cnt.sum() == n
        assert max(_indices_per_chunk(br, geo["chunks"])) >= 3
        br, nb = K.segments("only37", n)
        assert nb == 64 and set(br.tolist()) == {37}
        assert K.segments("one", n)[1] == 1
    br, nb = K.segments("many300", 0)
    cnt = np.bincount(br, minlength=300)
    assert nb == 300 and cnt.min() == 1 and cnt.max() == 8 and len(br) <= 2000
    assert sorted(K.segments("many300_shuffled", 0)[0].tolist()) == br.tolist()
    assert np.count_nonzero(np.diff(K.segments("many300_shuffled", 0)[0])) > 1000


def test_constant_instance_inputs():
    for c, layout in K.CONST_CASES:
        inp = K.const_inputs(c, layout)
        rows = inp["batch_row"] == 1
        assert rows.sum() == K.CONST_ROWS and np.all(inp["x"][rows] == np.float32(K.CONST_VALUE))
        assert np.float32(K.CONST_VALUE) == K.CONST_VALUE
        assert K.geometry("f32", c, K.CONST_ROWS)["chunks"] >= 4
        if layout == "interleaved":
            assert np.count_nonzero(np.diff(inp["batch_row"])) > 1000
        ref = K.reference(inp)
        assert np.all(ref["mean"][1] == K.CONST_VALUE) and np.all(ref["out"][rows] == inp["beta"].astype(np.float64))


def test_reference_is_the_formula_row_by_row():
    """the vectorised reference against a loop over the instances on a small case with absent instances"""
    inp = K.inputs("f32", 5, 200, "gapped")
    ref = K.reference(inp)
    x, dy, br = inp["x"].astype(np.float64), inp["dy"].astype(np.float64), inp["batch_row"]
    gg, gb = np.zeros(5), np.zeros(5)
    for b in range(inp["n_batch"]):
        m = br == b
        if not m.any():
            assert np.all(ref["mean"][b] == 0) and np.allclose(ref["rstd"][b], 1 / np.sqrt(K.EPS), rtol=1e-15)
            continue
        mu, var = x[m].mean(0), x[m].var(0)
        rs = 1 / np.sqrt(var + K.EPS)
        xh = (x[m] - mu) * rs
        assert np.abs(ref["mean"][b] - mu).max() <= 1e-13 and np.abs(ref["rstd"][b] / rs - 1).max() <= 1e-12
        assert np.abs(ref["out"][m] - (xh * inp["gamma"] + inp["beta"])).max() <= 1e-9
        want = inp["gamma"] * rs * (dy[m] - dy[m].mean(0) - xh * (dy[m] * xh).mean(0))
        assert np.abs(ref["dx"][m] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        gg += (dy[m] * xh).sum(0)
        gb += dy[m].sum(0)
    assert np.abs(ref["grad_gamma"] - gg).max() <= 1e-9 and np.abs(ref["grad_beta"] - gb).max() <= 1e-12


def _fp32_cases():
    seen, out = set(), []
    for case in K.SHAPE_CASES + K.PATTERN_CASES + K.UNALIGNED_CASES + K.ISOLATION_CASES + K.REPRO_CASES + K.ARG_CASES:
        if case[0] == "f32" and case not in seen:
            seen.add(case)
            out.append(case)
    return out


def _assert_half_bar(inp, tag, eps=K.EPS):
    ref, naive = K.reference(inp, eps=eps), K.naive_f32(inp, eps=eps)
    for name in K.OUTPUTS:
        ex = close_excess(naive[name], ref[name], atol=0.5e-4, rtol=0.5e-4)
        assert ex <= 1.0, f"{tag} {name}: naive float32 is {ex:.2f} x half the fp32 bar from float64"


@pytest.mark.parametrize("case", _fp32_cases(), ids=K._id)
def test_naive_float32_meets_half_the_bar(case):
    _assert_half_bar(K.inputs(*case), K._id(case))


@pytest.mark.parametrize("c,layout", K.CONST_CASES)
def test_naive_float32_meets_half_the_bar_constant_instance(c, layout):
    _assert_half_bar(K.const_inputs(c, layout), f"const {c} {layout}", K.CONST_EPS)


def test_bf16_inputs_are_bf16_values():
    import torch
    inp = K.inputs("bf16", 24, K._several("bf16", 24), "gapped")
    for k in ("x", "dy"):
        assert np.array_equal(torch.tensor(inp[k]).bfloat16().float().numpy(), inp[k])
