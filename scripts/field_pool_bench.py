"""Direct max pooling (csrc/direct_pool.hip) and global pooling of fields: time per call on field_bench's scene (~250k
points voxelised to ~200k voxels), against a byte model and against the same result computed with torch on the same GPU.

    python scripts/field_pool_bench.py [--iters 30] [--json out.jsonl]

Direct max pool: forward and forward + backward, with the sort (maps in field order) and without it (is_sorted on maps
sorted beforehand), C = 20 and 96, fp32 and bf16.  The call includes the map check and its 4-byte read-back.  torch:
scatter_reduce_("amax") plus an argmax recovery (amin of the entry index over the entries that reach the max), and
index_add_ of the gradient at the winners for the backward.
Byte model of the forward: e*C*(n_vox + n_points) + 8*C*n_vox (int64 mask) + 4*nmap; fraction of 6.3 TB/s.
Global pooling: MinkowskiGlobalMaxPooling / AvgPooling forward of a 250k-point field with 2 and 16 clouds (row table
cached), torch: scatter_reduce_ amax / index_add_ by cloud."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import minkowskiengine_amd as ME
from field_bench import HBM, scene, timed


def torch_max(im, om, x, n_out):
    c = x.shape[1]
    src = x[im]
    out = torch.full((n_out, c), float("-inf"), device=x.device, dtype=x.dtype)
    out.scatter_reduce_(0, om[:, None].expand(-1, c), src, "amax", include_self=True)
    e = torch.arange(len(im), device=x.device)[:, None].expand(-1, c)
    first = torch.full((n_out, c), len(im), device=x.device, dtype=torch.long)
    first.scatter_reduce_(0, om[:, None].expand(-1, c), torch.where(src == out[om], e, len(im)), "amin")
    idx = im[first.clamp_max(len(im) - 1)] * c + torch.arange(c, device=x.device)
    return out, idx


def torch_bwd(go, idx, n_in):
    return torch.zeros(n_in * go.shape[1], device=go.device, dtype=go.dtype).index_add_(0, idx.reshape(-1), go.reshape(-1))


def direct_case(coords, inv, n_vox, C, dtype, iters, dev, rows):
    e = 2 if dtype == torch.bfloat16 else 4
    n_p = coords.shape[0]
    x = torch.rand(n_p, C, device=dev).to(dtype)
    go = torch.rand(n_vox, C, device=dev).to(dtype)
    B = ME.host.backend()
    im = torch.arange(n_p, device=dev)
    order = torch.argsort(inv, stable=True)
    im_s, om_s = im[order].contiguous(), inv[order].contiguous()
    nbytes = e * C * (n_vox + n_p) + 8 * C * n_vox + 4 * n_p

    def rec(op, t, nb, t_torch):
        r = dict(op=op, C=C, dtype=str(dtype).split(".")[-1], us=round(t * 1e6, 1),
                 hbm_frac=round(nb / t / HBM, 3) if nb else None, torch_us=round(t_torch * 1e6, 1) if t_torch else None)
        rows.append(r)
        print(json.dumps(r), flush=True)

    def fb(a, b, s):
        o, idx = B.direct_max_pool_fw(a, b, x, n_vox, s)
        return B.direct_max_pool_bw(go, idx, n_p)

    def torch_fb():
        o, idx = torch_max(im, inv, x, n_vox)
        return torch_bwd(go, idx, n_p)

    o, idx = B.direct_max_pool_fw(im, inv, x, n_vox, False)
    to, tidx = torch_max(im, inv, x, n_vox)
    assert torch.equal(o, to) and torch.equal(idx, tidx), "torch and the kernel disagree"
    assert torch.equal(B.direct_max_pool_bw(go, idx, n_p).reshape(-1), torch_bwd(go, tidx, n_p))
    t_t = timed(lambda: torch_max(im, inv, x, n_vox), iters)
    rec("direct_max_fwd(sort)", timed(lambda: B.direct_max_pool_fw(im, inv, x, n_vox, False), iters), nbytes, t_t)
    rec("direct_max_fwd(is_sorted)", timed(lambda: B.direct_max_pool_fw(im_s, om_s, x, n_vox, True), iters), nbytes, t_t)
    t_t = timed(torch_fb, max(3, iters // 3))
    rec("direct_max_fwd+bwd(sort)", timed(lambda: fb(im, inv, False), max(3, iters // 3)), 0, t_t)
    rec("direct_max_fwd+bwd(is_sorted)", timed(lambda: fb(im_s, om_s, True), max(3, iters // 3)), 0, t_t)


def global_case(coords, clouds, C, dtype, iters, dev, rows):
    e = 2 if dtype == torch.bfloat16 else 4
    n_p = coords.shape[0]
    c2 = coords.clone()
    c2[:, 0] = torch.randint(0, clouds, (n_p,), device=dev).float()
    x = torch.rand(n_p, C, device=dev).to(dtype)
    tf = ME.TensorField(x, coordinates=c2)
    b = c2[:, 0].long()
    for name, mod, tfn in (
            ("global_max", ME.MinkowskiGlobalMaxPooling(),
             lambda: torch.full((clouds, C), float("-inf"), device=dev, dtype=dtype).scatter_reduce_(
                 0, b[:, None].expand(-1, C), x, "amax")),
            ("global_avg", ME.MinkowskiGlobalAvgPooling(),
             lambda: torch.zeros(clouds, C, device=dev, dtype=dtype).index_add_(0, b, x) /
             torch.bincount(b, minlength=clouds)[:, None])):
        t = timed(lambda: mod(tf), iters)
        r = dict(op=f"{name}(field, {clouds} clouds)", C=C, dtype=str(dtype).split(".")[-1], us=round(t * 1e6, 1),
                 hbm_frac=round((e * C * n_p + 4 * n_p) / t / HBM, 3), torch_us=round(timed(tfn, iters) * 1e6, 1))
        rows.append(r)
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    coords = scene(dev)
    tf = ME.TensorField(torch.zeros(coords.shape[0], 1, device=dev), coordinates=coords)
    key, (_, inv) = tf.coordinate_manager.field_to_sparse_insert_and_map(tf.coordinate_field_map_key, [1, 1, 1])
    n_vox = tf.coordinate_manager.size(key)
    print(json.dumps(dict(points=coords.shape[0], voxels=n_vox, host=ME.get_host())), flush=True)
    rows = []
    for C in (20, 96):
        for dt in (torch.float32, torch.bfloat16):
            direct_case(coords, inv, n_vox, C, dt, a.iters, dev, rows)
    for clouds in (2, 16):
        for C in (20, 96):
            for dt in (torch.float32, torch.bfloat16):
                global_case(coords, clouds, C, dt, a.iters, dev, rows)
    if a.json:
        with open(a.json, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
