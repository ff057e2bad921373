"""Generate the direct max pooling fixtures (direct_pool_*.npz) with the reference's own CPU extension.

The reference's operators (compiled unmodified into oracle/_ref/_C.so by oracle/build_ref.py, through oracle.ref) give
    direct_max_pool_fw(in_map, out_map, in_feat, out_nrows, is_sorted)   -> out_feat, max_index
    direct_max_pool_bw(grad_out_feat, max_index, in_nrows)               -> grad_in

The reference's CPU kernel (src/pooling_max_kernel.hpp:47-64 over the zero-initialised buffers of
src/direct_max_pool.cpp:83-86) computes max(0, .) and leaves mask 0 where nothing is positive; it equals the rule of
its GPU kernel (src/pooling_max_kernel.cu:55-96), which the product follows, only when
    1. every output row in [0, out_nrows) has at least one entry,
    2. every feature is strictly positive,
    3. no two entries of one output row tie in any channel.
Every case is asserted to satisfy the three before its file is written.  Features are (permutation + 1) / (n + 1)
scaled into [0.05, 1) per column: distinct per column, and spaced by more than a bf16 ulp (n <= 100 rows per case with
such a check, see bf16_distinct below), so that rounding to bf16 creates no tie either.

Run where the reference's source tree is available:
    python tests/golden/make_golden_direct_pool.py
The .npz files are committed; tests never need the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref  # noqa: E402


def features(n, c, g, dtype):
    """[n, c]: every column a scaled permutation in [0.05, 1): strictly positive, distinct per column"""
    cols = [(torch.randperm(n, generator=g).double() + 1) / (n + 1) * 0.95 + 0.05 * (1 - 1 / (n + 1)) for _ in range(c)]
    return torch.stack(cols, 1).to(dtype).contiguous()


def check_conditions(in_map, out_map, feats, out_nrows):
    im, om, f = in_map.long().numpy(), out_map.long().numpy(), feats.double().numpy()
    assert set(om.tolist()) == set(range(out_nrows)), "condition 1: every output row needs an entry"
    assert (f > 0).all() and (f >= 0.05).all() and (f < 1).all(), "condition 2: strictly positive features"
    for o in range(out_nrows):
        v = f[im[om == o]]
        for ch in range(v.shape[1]):
            assert len(np.unique(v[:, ch])) == v.shape[0], "condition 3: no ties inside an output row"


def bf16_distinct(in_map, out_map, feats, out_nrows):
    im, om = in_map.long().numpy(), out_map.long().numpy()
    f = feats.to(torch.bfloat16).double().numpy()
    for o in range(out_nrows):
        v = f[im[om == o]]
        for ch in range(v.shape[1]):
            if len(np.unique(v[:, ch])) != v.shape[0]:
                return False
    return True


def write(name, in_map, out_map, feats, out_nrows, is_sorted, g, extra=None):
    C = ref.load()
    check_conditions(in_map, out_map, feats, out_nrows)
    assert bf16_distinct(in_map, out_map, feats, out_nrows), "rounding to bf16 must not create a tie"
    im, om = in_map.clone(), out_map.clone()             # (the reference may sort its arguments in place)
    out_feat, max_index = C.direct_max_pool_fw(im, om, feats, out_nrows, is_sorted)
    assert max_index.dtype == in_map.dtype
    grad_out = features(out_nrows, feats.shape[1], g, feats.dtype)
    grad_in = C.direct_max_pool_bw(grad_out, max_index, feats.shape[0])
    # the reference's result obeys the rule the product implements (numpy restatement)
    f = feats.numpy()
    for o in range(out_nrows):
        rows = in_map.long().numpy()[out_map.long().numpy() == o]
        assert np.array_equal(out_feat.numpy()[o], f[rows].max(0))
        assert np.array_equal(max_index.numpy()[o], rows[f[rows].argmax(0)] * f.shape[1] + np.arange(f.shape[1]))
    out = os.path.join(HERE, f"direct_pool_{name}.npz")
    data = dict(in_map=in_map.numpy(), out_map=out_map.numpy(), in_feat=feats.numpy(), out_nrows=out_nrows,
                is_sorted=int(is_sorted), out_feat=out_feat.numpy(), max_index=max_index.numpy(),
                grad_out=grad_out.numpy(), grad_in=grad_in.numpy())
    data.update(extra or {})
    np.savez_compressed(out, **data)
    assert os.path.getsize(out) < (1 << 20)
    print(f"{out}: nmap {len(in_map)}, in rows {feats.shape[0]}, out rows {out_nrows}, C {feats.shape[1]}, "
          f"{os.path.getsize(out)} bytes")


def random_case(name, n_in, out_nrows, c, itype, ftype, is_sorted, seed, shared=0):
    """every input row under one output row (+ `shared` rows listed under a second one)"""
    g = torch.Generator().manual_seed(seed)
    out_of = torch.cat([torch.arange(out_nrows), torch.randint(0, out_nrows, (n_in - out_nrows,), generator=g)])
    in_map = torch.randperm(n_in, generator=g)
    out_map = out_of[in_map]
    if shared:
        extra_in = torch.randperm(n_in, generator=g)[:shared]
        extra_out = (out_of[extra_in] + 1 + torch.randint(0, out_nrows - 1, (shared,), generator=g)) % out_nrows
        in_map, out_map = torch.cat([in_map, extra_in]), torch.cat([out_map, extra_out])
        perm = torch.randperm(len(in_map), generator=g)
        in_map, out_map = in_map[perm], out_map[perm]
    if is_sorted:
        order = torch.argsort(out_map, stable=True)
        in_map, out_map = in_map[order], out_map[order]
    write(name, in_map.to(itype).contiguous(), out_map.to(itype).contiguous(), features(n_in, c, g, ftype), out_nrows,
          is_sorted, g)


def field_case(name, n, c, seed):
    """maps of a real field_to_sparse_insert_and_map of the reference's manager: arange(N) -> inverse_mapping"""
    g = torch.Generator().manual_seed(seed)
    C = ref.load()
    b = torch.randint(0, 2, (n, 1), generator=g).float()
    x = (torch.rand(n, 3, generator=g) - 0.5) * 6.0
    coords = torch.cat([b, x], 1).float().contiguous()
    mgr = C.CoordinateMapManagerCPU(C.MinkowskiAlgorithm.DEFAULT, 1)
    fkey = mgr.insert_field(coords, [1, 1, 1], "")
    skey, (unique_map, inverse_map) = mgr.field_to_sparse_insert_and_map(fkey, [1, 1, 1], "")
    n_vox = mgr.get_coordinates(skey).shape[0]
    write(name, torch.arange(n, dtype=torch.int64), inverse_map.long().contiguous(), features(n, c, g, torch.float32),
          n_vox, False, g, extra=dict(field_coords=coords.numpy(), sparse_coords=mgr.get_coordinates(skey).int().numpy()))


if __name__ == "__main__":
    random_case("i32_f32_c1", 90, 20, 1, torch.int32, torch.float32, False, 1)
    random_case("i64_f32_c3", 100, 25, 3, torch.int64, torch.float32, False, 2, shared=15)
    random_case("i32_f64_c16", 96, 30, 16, torch.int32, torch.float64, False, 3)
    random_case("i64_f64_c17_sorted", 100, 28, 17, torch.int64, torch.float64, True, 4, shared=10)
    random_case("i32_f32_c16_sorted", 80, 16, 16, torch.int32, torch.float32, True, 5)
    random_case("i64_f32_c17", 100, 40, 17, torch.int64, torch.float32, False, 6)
    field_case("field_3d", 100, 3, 7)
