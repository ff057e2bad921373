"""GPU tests of the trilinear interpolation map and MinkowskiInterpolation (csrc/field.hip, both host layers): the map
against a float64 restatement of the reference's interpolation_kernel (order, rows, weights), forward / backward values,
gradcheck, splat / interpolate, missing corners and bf16."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-3)
HERE = os.path.dirname(os.path.abspath(__file__))
FIELD_CASES = sorted(glob.glob(os.path.join(HERE, "golden", "field_*.npz")))


def _me():
    import minkowskiengine_amd as ME
    return ME


def _voxels(D, n, extent, batch, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-extent, extent, (n, D), generator=g)
    b = torch.randint(0, batch, (n, 1), generator=g)
    return torch.unique(torch.cat([b, v], 1), dim=0).int().to(device)


def _expected_map(coords, samples, ts):
    """the reference's interpolation_kernel in numpy: (in row, sample, weight) for every present corner, (p, v) order"""
    table = {tuple(r): i for i, r in enumerate(coords.tolist())}
    D = samples.shape[1] - 1
    out = []
    for p, x in enumerate(samples.tolist()):
        base = [int(np.floor(x[j + 1] / ts[j]) * ts[j]) for j in range(D)]
        for v in range(1 << D):
            c = [int(np.rint(x[0]))] + [base[j] + (ts[j] if (v >> (D - 1 - j)) & 1 else 0) for j in range(D)]
            r = table.get(tuple(c))
            if r is not None:
                w = 1.0
                for j in range(D):
                    w *= 1 - abs(x[j + 1] - c[j + 1]) / ts[j]
                out.append((r, p, w))
    return out


@pytest.mark.parametrize("D,ts", [(2, [1, 1]), (3, [1, 1, 1]), (3, [2, 2, 2]), (3, [2, 4, 1]), (4, [1, 1, 1, 1])])
def test_interpolation_map_and_values(host_layer, device, D, ts):
    ME = _me()
    vox = _voxels(D, 400, 4, 2, device)
    vox[:, 1:] *= torch.tensor(ts, dtype=torch.int32, device=device)
    f = torch.rand(vox.shape[0], 6, device=device, dtype=torch.float64)
    s = ME.SparseTensor(f, coordinates=vox, tensor_stride=ts)
    g = torch.Generator().manual_seed(1)
    q = torch.cat([torch.randint(0, 2, (300, 1), generator=g).double(),
                   (torch.rand(300, D, generator=g, dtype=torch.float64) - 0.5) * 10 * max(ts)], 1)
    q[:20, 1:] = torch.round(q[:20, 1:])                          # on voxel boundaries
    q[20:25, 1:] = 1000.0                                         # no corner present
    q = q.to(device)
    in_map, out_map, w = s.coordinate_manager.interpolation_map_weight(s.coordinate_map_key, q)
    want = _expected_map(s.C.cpu().numpy(), q.cpu().numpy(), ts)
    assert in_map.dtype == torch.int32 and w.dtype == torch.float64
    assert [(int(a), int(b)) for a, b in zip(in_map.tolist(), out_map.tolist())] == [(r, p) for r, p, _ in want]
    np.testing.assert_allclose(w.cpu().numpy(), [x for _, _, x in want], rtol=1e-12)
    # weights of one sample sum to at most 1 (exactly 1 with all corners present)
    tot = torch.zeros(q.shape[0], dtype=torch.float64, device=device).index_add_(0, out_map.long(), w)
    assert float(tot.max()) <= 1 + 1e-12
    # forward / backward against the float64 restatement
    ff = s.F.clone().requires_grad_(True)
    out = ME.MinkowskiInterpolationFunction.apply(ff, q, s.coordinate_map_key, s.coordinate_manager)[0]
    ref = torch.zeros(q.shape[0], 6, dtype=torch.float64, device=device).index_add(
        0, out_map.long(), ff[in_map.long()] * w[:, None])
    torch.testing.assert_close(out, ref, rtol=1e-10, atol=1e-12)
    assert torch.equal(out[20:25], torch.zeros_like(out[20:25]))
    gy = torch.rand_like(out)
    (g1,) = torch.autograd.grad(out, ff, gy)
    (g2,) = torch.autograd.grad(ref, ff, gy)
    torch.testing.assert_close(g1, g2, rtol=1e-10, atol=1e-12)
    # fp32 map of the same samples: the same entries; the weights differ from the float64 ones only by the rounding of
    # the samples to fp32 (|x| <= 20: half an ulp is 1e-6 per factor, D factors).  The 1e-6 relative bar of fp32
    # weights is checked against the reference's own fp32 weights (test_reference_fixture).
    i32_, o32_, w32 = s.coordinate_manager.interpolation_map_weight(s.coordinate_map_key, q.float())
    assert torch.equal(i32_, in_map) and torch.equal(o32_, out_map)
    np.testing.assert_allclose(w32.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=D * 2e-6)


def test_gradcheck_interpolation_and_splat(host_layer, device):
    ME = _me()
    vox = _voxels(3, 60, 2, 1, device)
    f = torch.rand(vox.shape[0], 2, device=device, dtype=torch.float64, requires_grad=True)
    s = ME.SparseTensor(f.detach(), coordinates=vox)
    q = torch.cat([torch.zeros(40, 1, dtype=torch.float64), torch.rand(40, 3, dtype=torch.float64) * 3 - 1.5], 1).to(device)
    fn = lambda x: ME.MinkowskiInterpolationFunction.apply(x, q, s.coordinate_map_key, s.coordinate_manager)[0]
    assert torch.autograd.gradcheck(fn, (f,), **GC)
    pf = torch.rand(40, 2, device=device, dtype=torch.float64, requires_grad=True)

    def splat(x):
        tf = ME.TensorField(x, coordinates=q)
        return tf.splat().F

    assert torch.autograd.gradcheck(splat, (pf,), **GC)


def test_module_splat_interpolate_bf16(host_layer, device):
    ME = _me()
    vox = _voxels(3, 2000, 8, 2, device)
    f = torch.rand(vox.shape[0], 20, device=device)
    s = ME.SparseTensor(f, coordinates=vox)
    q = torch.cat([torch.randint(0, 2, (500, 1)).float(), torch.rand(500, 3) * 16 - 8], 1).to(device)
    m = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)
    out, (im, om), w = m(s, q)
    assert out.shape == (500, 20)
    sb = ME.SparseTensor(f.bfloat16(), coordinates=vox)
    ob = ME.MinkowskiInterpolation()(sb, q)
    assert ob.dtype == torch.bfloat16
    torch.testing.assert_close(ob.float(), out, rtol=2e-2, atol=2e-2)
    tf = ME.TensorField(torch.rand(500, 20, device=device), coordinates=q)
    sp = tf.splat()
    back = sp.interpolate(tf)
    assert back.F.shape == (500, 20)


@pytest.mark.parametrize("path", FIELD_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixture(host_layer, device, path):
    """tests/golden/make_golden_field.py: the reference's CPU manager's maps and float64 restatements over them"""
    from helpers import row_mapping
    ME = _me()
    z = np.load(path)
    ts = [int(t) for t in z["tensor_stride"]]
    coords = torch.from_numpy(z["field_coords"]).to(device)
    feats = torch.from_numpy(z["field_feats"]).double().to(device).requires_grad_(True)
    tf = ME.TensorField(feats, coordinates=coords)
    s = tf.sparse(tensor_stride=ts)
    # field_to_sparse_insert_and_map: the same voxels; unique_index / inverse_mapping after relabelling
    ours = s.C.cpu().numpy()
    m = np.asarray(row_mapping(z["sparse_coords"], ours))          # ours[m[i]] == reference row i
    um, im = tf.coordinate_manager.get_field_to_sparse_map(tf.coordinate_field_map_key, s.coordinate_map_key)
    assert np.array_equal(um.cpu().numpy()[m], z["unique_map"])
    assert np.array_equal(im.cpu().numpy(), m[z["inverse_map"]])
    # UNWEIGHTED_AVERAGE sparse(): values and gradient against the float64 restatement
    np.testing.assert_allclose(s.F.detach().cpu().numpy()[m], z["avg_feats"], rtol=1e-10, atol=1e-12)
    gy = torch.zeros(len(ours), z["grad_sparse"].shape[1], dtype=torch.float64)
    gy[torch.from_numpy(m)] = torch.from_numpy(z["grad_sparse"]).double()
    (g,) = torch.autograd.grad(s.F, feats, gy.to(device))
    np.testing.assert_allclose(g.cpu().numpy(), z["avg_grad"], rtol=1e-10, atol=1e-12)
    # the interpolation map: the reference's (in, out) pairs after relabelling, ordered by (point, corner) — corner order
    # is the lexicographic order of the corner coordinates — and its fp32 weights within 1e-6 relative
    q = torch.from_numpy(z["queries"]).to(device)
    in_map, out_map, w = tf.coordinate_manager.interpolation_map_weight(s.coordinate_map_key, q)
    rin, rout, rw = m[z["ref_in"]], z["ref_out"], z["ref_w"]
    c = ours[rin]
    order = np.lexsort(tuple(c[:, j] for j in range(c.shape[1] - 1, 0, -1)) + (rout,))
    assert np.array_equal(in_map.cpu().numpy(), rin[order])
    assert np.array_equal(out_map.cpu().numpy(), rout[order])
    assert w.dtype == torch.float32
    np.testing.assert_allclose(w.cpu().numpy(), rw[order], rtol=1e-6, atol=1e-7)
    # interpolation forward / backward against the float64 restatement
    x = torch.zeros(len(ours), z["sparse_feats"].shape[1], dtype=torch.float64)
    x[torch.from_numpy(m)] = torch.from_numpy(z["sparse_feats"]).double()
    x = x.to(device).requires_grad_(True)
    sd = ME.SparseTensor(x.detach(), coordinate_map_key=s.coordinate_map_key, coordinate_manager=s.coordinate_manager)
    out = ME.MinkowskiInterpolationFunction.apply(x, q, sd.coordinate_map_key, sd.coordinate_manager)[0]
    np.testing.assert_allclose(out.detach().cpu().numpy(), z["interp_out"], rtol=1e-5, atol=1e-6)
    (gx,) = torch.autograd.grad(out, x, torch.from_numpy(z["grad_queries"]).double().to(device))
    np.testing.assert_allclose(gx.cpu().numpy()[m], z["interp_grad"], rtol=1e-5, atol=1e-6)
