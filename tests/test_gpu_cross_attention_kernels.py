"""Entry-point tests of cross-attention's kernels (csrc/attention.hip, ABI 1.20) through the C ABI: the context row lists
(me_attn_context_lists) against a numpy construction, and the dK / dV pass split over the queries (me_attn_backward_split)
against the float64 twin on the same lists.

Error bound (the rule of tests/test_gpu_attention_kernels.py): per tensor E_kernel <= FACTOR * E_torch, both against the
float64 twin me_attn_backward_split_f64; E_torch is the error of torch's math-backend attention in the dtype of the case on
the same rows (imported from that module, which also supplies a float64 yardstick written out with torch that the twin is
held to).  Every figure is printed before it is asserted (pytest -s).  Measured maxima: DESIGN 8.14.
Bitwise cases compare two runs of the kernels."""
import math

import numpy as np
import pytest
import torch

from minkowskiengine_amd import _lib
from test_gpu_attention_kernels import FACTOR, reference, torch_attention

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16)
HEADS = 2
SIZES = (1, 70, 200)                       # query rows of the three instances, interleaved in shuffled order
TOKENS = 77
LENGTHS = (None, (77, 1, 0), (0, 1, 77))   # the second one backwards too: the 200-row instance with a full context
SPLITS = (1, 2, 3, 8)                      # 8 leaves empty slices: the instances have 1, 3 and 7 query blocks


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _i32(x, dev):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(dev)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- the lists ----------------------------------------------------------------------------------------------------------------
def numpy_context_lists(n_batch, tokens, lengths):
    lens = [tokens] * n_batch if lengths is None else [min(max(int(x), 0), tokens) for x in lengths]
    seg_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    seg_rows = np.array([b * tokens + t for b in range(n_batch) for t in range(lens[b])], dtype=np.int32)
    n_entries = -(-n_batch * tokens // 64) + n_batch
    tab = np.full((n_entries, 2), -1, dtype=np.int32)
    e = 0
    for b in range(n_batch):
        for first in range(0, lens[b], 64):
            tab[e] = (b, first)
            e += 1
    return seg_ptr, seg_rows, tab


def context_lists(n_batch, tokens, lengths, dev):
    lib = _lib.load()
    n = n_batch * tokens
    seg_ptr = torch.full((n_batch + 1,), -7, dtype=torch.int32, device=dev)
    seg_rows = torch.full((n,), -7, dtype=torch.int32, device=dev)
    blk_tab = torch.full((2 * (-(-n // 64) + n_batch),), -7, dtype=torch.int32, device=dev)
    len_dev = None if lengths is None else _i32(lengths, dev)
    _lib.check(lib.me_attn_context_lists(n_batch, tokens, _ptr(len_dev), _ptr(seg_ptr), _ptr(seg_rows), _ptr(blk_tab),
                                         _stream(dev)))
    return seg_ptr, seg_rows, blk_tab


@pytest.mark.parametrize("n_batch,tokens,lengths", [
    (3, 77, None), (3, 77, (77, 1, 0)), (3, 77, (0, 1, 77)), (3, 77, (100, -3, 64)), (2, 65, (65, 64)), (1, 1, None),
    (5, 128, (0, 0, 129, 128, 1)), (300, 3, None)])
def test_context_lists_equal_the_numpy_construction(device, n_batch, tokens, lengths):
    """seg_ptr, the listed part of seg_rows and the whole block table (unused entries hold -1); lengths above `tokens` and
    below 0 are clamped on the device; seg_rows past seg_ptr[B] is left alone"""
    seg_ptr, seg_rows, blk_tab = (t.cpu().numpy() for t in context_lists(n_batch, tokens, lengths, device))
    want_ptr, want_rows, want_tab = numpy_context_lists(n_batch, tokens, lengths)
    assert np.array_equal(seg_ptr, want_ptr)
    total = int(want_ptr[-1])
    assert np.array_equal(seg_rows[:total], want_rows) and (seg_rows[total:] == -7).all()
    assert np.array_equal(blk_tab.reshape(-1, 2), want_tab)


# ---- a case: queries in shuffled order, a context, the forward pass ----------------------------------------------------------
class Case:
    def __init__(self, dev, dtype, d, sizes, tokens, lengths, seed, poison=None):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.dtype, self.d, self.c, self.tokens = dev, dtype, d, HEADS * d, tokens
        self.n_batch, self.n_q, self.n_kv = len(sizes), sum(sizes), len(sizes) * tokens
        bq = torch.cat([torch.full((n,), b) for b, n in enumerate(sizes)])
        self.bq = bq[torch.randperm(self.n_q, generator=g)].to(dev)
        lens = [tokens] * self.n_batch if lengths is None else list(lengths)
        self.bk = torch.cat([torch.where(torch.arange(tokens) < lens[b], b, -1) for b in range(self.n_batch)]).to(dev)
        order = torch.sort(self.bq, stable=True).indices                        # rows ascending inside an instance
        self.seg_q = (_i32(np.concatenate([[0], np.cumsum(sizes)]), dev), order.to(torch.int32))
        self.seg_kv = context_lists(self.n_batch, tokens, lengths, dev)
        self.q, self.dout = (torch.randn(self.n_q, self.c, generator=g).to(dtype).to(dev) for _ in range(2))
        self.k, self.v = (torch.randn(self.n_kv, self.c, generator=g).to(dtype).to(dev) for _ in range(2))
        if poison is not None:
            poison(self)
        self.scale = 1.0 / math.sqrt(d)
        self.out = torch.empty_like(self.q)
        self.lse = torch.empty(self.n_q, HEADS, dtype=torch.float32, device=dev)
        lib = _lib.load()
        _lib.check(lib.me_attn_forward_tab(
            _ptr(self.q), _ptr(self.k), _ptr(self.v), int(dtype == torch.bfloat16), self.c, self.c, self.c,
            *map(_ptr, self.seg_q), _ptr(self.seg_kv[0]), _ptr(self.seg_kv[1]), None, _ptr(self.seg_kv[2]), self.n_q,
            self.n_kv, self.n_batch, self.c, HEADS, self.scale, _ptr(self.out), self.c, _ptr(self.lse), _stream(dev)))

    def _grads(self, want, dtype, fill):
        shapes = dict(dq=(self.n_q, self.c), dk=(self.n_kv, self.c), dv=(self.n_kv, self.c))
        return {n: torch.full(shapes[n], fill, dtype=dtype, device=self.dev) if n in want else None
                for n in ("dq", "dk", "dv")}

    def backward(self, splits, want=("dq", "dk", "dv"), fill=math.nan, tab_entry=False):
        """me_attn_backward_split (tab_entry: me_attn_backward_tab) into buffers pre-filled with `fill`"""
        lib = _lib.load()
        g = self._grads(want, self.dtype, fill)
        args = [_ptr(self.q), _ptr(self.k), _ptr(self.v), _ptr(self.out), _ptr(self.lse), _ptr(self.dout),
                int(self.dtype == torch.bfloat16), self.c, self.c, self.c, self.c, self.c, *map(_ptr, self.seg_q),
                _ptr(self.seg_kv[0]), _ptr(self.seg_kv[1]), None, _ptr(self.seg_kv[2]), self.n_q, self.n_kv, self.n_batch,
                self.c, HEADS, self.scale, _ptr(g["dq"]), self.c, _ptr(g["dk"]), self.c, _ptr(g["dv"]), self.c]
        if tab_entry:
            ws = torch.empty(lib.me_attn_workspace_bytes(self.n_q, self.n_kv, self.n_batch, HEADS), dtype=torch.uint8,
                             device=self.dev)
            _lib.check(lib.me_attn_backward_tab(*args, _ptr(ws), ws.numel(), _stream(self.dev)))
        else:
            ws = torch.empty(lib.me_attn_split_workspace_bytes(self.n_q, self.n_kv, self.n_batch, self.c, HEADS, splits),
                             dtype=torch.uint8, device=self.dev)
            _lib.check(lib.me_attn_backward_split(*args, _ptr(ws), ws.numel(), splits, _stream(self.dev)))
        return g

    def twin(self):
        """forward and backward of the float64 twin on the same values and lists; rows on no list stay zero"""
        lib = _lib.load()
        q, k, v, dout = (t.double() for t in (self.q, self.k, self.v, self.dout))
        out = torch.zeros_like(q)
        lse = torch.zeros(self.n_q, HEADS, dtype=torch.float64, device=self.dev)
        lists = [*map(_ptr, self.seg_q), _ptr(self.seg_kv[0]), _ptr(self.seg_kv[1]), None, _ptr(self.seg_kv[2])]
        _lib.check(lib.me_attn_forward_tab_f64(_ptr(q), _ptr(k), _ptr(v), self.c, self.c, self.c, *lists, self.n_q,
                                               self.n_kv, self.n_batch, self.c, HEADS, self.scale, _ptr(out), self.c,
                                               _ptr(lse), _stream(self.dev)))
        g = self._grads(("dq", "dk", "dv"), torch.float64, 0.0)
        _lib.check(lib.me_attn_backward_split_f64(
            _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(dout), self.c, self.c, self.c, self.c, self.c, *lists,
            self.n_q, self.n_kv, self.n_batch, self.c, HEADS, self.scale, _ptr(g["dq"]), self.c, _ptr(g["dk"]), self.c,
            _ptr(g["dv"]), self.c, 5, _stream(self.dev)))
        g["out"] = out
        return g

    def yardsticks(self):
        """(the float64 twin, torch's attention in the dtype of the case); the twin is held to torch's float64 here"""
        twin = self.twin()
        ref = reference(self.q, self.k, self.v, self.dout, self.bq, self.bk, HEADS, self.scale)
        for name in ("out", "dq", "dk", "dv"):
            assert float((twin[name] - ref[name]).abs().max()) <= 1e-11 * max(1.0, float(ref[name].abs().max())), name
        return twin, torch_attention(self.q, self.k, self.v, self.dout, self.bq, self.bk, HEADS, self.scale)


def within_bound(ours, twin, theirs, what, names=("dq", "dk", "dv"), listed=None):
    bad = []
    for name in names:
        a = ours[name] if listed is None or name == "dq" else ours[name][listed]
        t = twin[name] if listed is None or name == "dq" else twin[name][listed]
        o = theirs[name] if listed is None or name == "dq" else theirs[name][listed]
        assert torch.isfinite(a.float()).all(), f"{what} {name}: not finite"
        e, et = float((a.double() - t).abs().max()), float((o.double() - t).abs().max())
        print(f"{what} {name}: E_kernel {e:.3e}  E_torch {et:.3e}  ratio {e / et if et > 0 else float('inf') if e > 0 else 0:.2f}")
        if not e <= FACTOR * et:
            bad.append((name, e, et))
    assert not bad, f"{what}: beyond {FACTOR} x E_torch: {bad}"


# ---- the split against the twin, and its bitwise properties ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("lengths", LENGTHS, ids=["full", "77_1_0", "0_1_77"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_split_gradients(device, d, lengths, dtype):
    """for every S: dq / dk / dv within the bound of the float64 twin; two runs bitwise equal; the dK-only and dV-only
    calls bitwise equal to the halves of the full call; S = 1 bitwise equal to me_attn_backward_tab.  With one slice the
    key rows on no list are not written (the operators zero them), with more they are written as zeros."""
    case = Case(device, dtype, d, SIZES, TOKENS, lengths, seed=d)
    twin, theirs = case.yardsticks()
    listed = case.bk >= 0
    out_e = float((case.out.double() - twin["out"]).abs().max())
    out_et = float((theirs["out"].double() - twin["out"]).abs().max())
    print(f"d={d} {lengths} {dtype} out: E_kernel {out_e:.3e}  E_torch {out_et:.3e}")
    assert out_e <= FACTOR * out_et
    tab = case.backward(1, tab_entry=True)
    for s in SPLITS:
        g = case.backward(s)
        within_bound(g, twin, theirs, f"S={s} d={d} {lengths} {dtype}", listed=listed)
        again = case.backward(s)
        only_k, only_v = case.backward(s, want=("dk",)), case.backward(s, want=("dv",))
        for name in ("dq", "dk", "dv"):
            assert _same(g[name], again[name]), (s, name)
        assert _same(g["dk"], only_k["dk"]) and _same(g["dv"], only_v["dv"]), s
        assert only_k["dq"] is None and only_k["dv"] is None and only_v["dk"] is None
        for name in ("dk", "dv"):
            rest = g[name][~listed]
            if s == 1:
                assert bool(torch.isnan(rest).all()), (s, name)                 # the fill: not written
            else:
                assert _same(rest, torch.zeros_like(rest)), (s, name)           # written as +0
        if s == 1:
            for name in ("dq", "dk", "dv"):
                assert _same(g[name], tab[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_partial_blocks_on_both_sides(device, dtype):
    """a 33-row instance (one query past a block of 32) under 65 tokens (one key past a block of 64), next to a 5-row one"""
    case = Case(device, dtype, 64, (33, 5), 65, None, seed=3)
    twin, theirs = case.yardsticks()
    for s in (1, 2, 3):
        within_bound(case.backward(s), twin, theirs, f"33 rows x 65 tokens S={s} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("splits", [1, 3])
def test_masked_tokens_and_neighbours_are_never_read(device, splits, dtype):
    """lengths (33, 77, 5).  Run two fills the tokens beyond every length, and ALL rows of instance 1 (its queries, their
    dout and its context), with NaN and Inf: every output of instances 0 and 2 stays bit for bit, and (S > 1) the gradients
    of the masked tokens are exactly 0"""
    lengths, d = (33, 77, 5), 64

    def poison(case):
        bad = torch.full((case.c,), math.inf, dtype=case.dtype, device=case.dev)
        bad[::2] = math.nan
        bad[1::4] = -math.inf
        ctx_inst = torch.arange(case.n_kv, device=case.dev) // case.tokens
        for t in (case.k, case.v):
            t[(case.bk < 0) | (ctx_inst == 1)] = bad
        for t in (case.q, case.dout):
            t[case.bq == 1] = bad
    clean = Case(device, dtype, d, SIZES, TOKENS, lengths, seed=11)
    dirty = Case(device, dtype, d, SIZES, TOKENS, lengths, seed=11, poison=poison)
    keep_q = clean.bq != 1
    keep_kv = (clean.bk >= 0) & (clean.bk != 1)
    assert int(keep_kv.sum()) == 38 and not torch.isfinite(dirty.k.float()[clean.bk < 0]).any()
    assert _same(clean.out[keep_q], dirty.out[keep_q]) and _same(clean.lse[keep_q], dirty.lse[keep_q])
    a, b = clean.backward(splits, fill=0.0), dirty.backward(splits, fill=0.0)
    assert torch.isfinite(a["dq"].float()).all() and torch.isfinite(a["dk"].float()).all()
    assert _same(a["dq"][keep_q], b["dq"][keep_q])
    for name in ("dk", "dv"):
        assert _same(a[name][keep_kv], b[name][keep_kv]), name
        masked = b[name][clean.bk < 0]
        assert _same(masked, torch.zeros_like(masked)), name
